// The chunked device pipeline of the point routes (zkey_scale.hip, ptau_scale.hip, ptau_points.hip; host code only).
// n items of a host buffer run through the device in chunks over two buffer sets and two streams: the copies of chunk
// c + 1 (up) and c - 1 (down) go over the copy stream while chunk c computes, and the device never holds more than two
// chunks (one buffer set when there is a single chunk).  Per chunk c, with b = c & 1:
//   copy stream     [c >= 2: wait ev_k[b] -- the kernels of chunk c - 2 have read in[b]]   upload c -> ev_up[b]
//   compute stream  wait ev_up[b]   [c >= 2: wait ev_down[b] -- out[b], out2[b] of chunk c - 2 have been copied out]
//                   launch(stream, in[b], out[b], out2[b], cnt, lo) -> ev_k[b]
//   copy stream     wait ev_k[b]   download c -> ev_down[b]
// and the upload of chunk c + 1 is enqueued ahead of the kernels of chunk c.  Both streams are drained before run()
// returns and before anything is freed.  What a stage needs beyond the buffers (tables, digits, a result word) stays
// with its caller: a DeviceBuf each, declared AHEAD of the pipeline (device_job.h: the pipeline owns the streams),
// written and read over stream() before and after run().
// Two options, both off unless asked for (zkey_cshash.hip asks for both, ptau_points.hip's to-be stage for the sink):
//   second(off)  every item has a partner `off` items further on in the host buffer: the upload side takes TWO copies
//                per chunk, items [lo, lo + cnt) to the head of in[b] and [lo + off, lo + off + cnt) to its second half,
//                which starts chunk * in_sz bytes in, whatever cnt is;
//   a sink       run(.., sink): sink(lo, cnt) is called on the calling thread, chunk by chunk in order, once the copies
//                down of that chunk have landed in the host buffer -- while the next chunk computes and copies.
#pragma once
#include <algorithm>
#include <functional>

#include "internal.h"

namespace g16 {

// Chunk size and grid of a run over n items, both overridable so that a small test runs several chunks and grid-stride
// passes: chunk = G16_<..>_CHUNK or 2^18 items; lanes = G16_<..>_LANES rounded up to whole wavefronts (workgroups of 64
// when that is no multiple of 256), else lanes_cap, else -- lanes_cap = 0 -- one lane per item of a chunk.
struct ChunkPlan {
  uint32_t chunk = 0, block = 256, lanes = 0;   // lanes: whole workgroups, no more than a full chunk asks for
  uint32_t grid(uint32_t cnt) const { return std::min(lanes / block, (cnt + block - 1) / block); }
};
inline ChunkPlan chunk_plan(const char* chunk_env, const char* lanes_env, uint64_t n, uint32_t lanes_cap) {
  ChunkPlan p;
  p.chunk = env_u32(chunk_env);
  if (!p.chunk) p.chunk = 1u << 18;
  p.chunk = (uint32_t)std::min<uint64_t>(p.chunk, n);
  p.lanes = lanes_cap ? lanes_cap : 0xffffff00u;
  if (const uint32_t forced = env_u32(lanes_env)) {
    p.lanes = std::min((forced + 63) / 64 * 64, p.lanes);
    if (p.lanes % p.block) p.block = 64;
  }
  p.lanes = std::min(p.lanes, (p.chunk + p.block - 1) / p.block * p.block);
  return p;
}

class ChunkPipeline : public DeviceJob {   // fail(): also for the caller's own calls
 public:
  explicit ChunkPipeline(const char* route) : DeviceJob(route) {}
  ChunkPipeline(const ChunkPipeline&) = delete;
  ChunkPipeline& operator=(const ChunkPipeline&) = delete;
  ~ChunkPipeline() {
    drain();
    for (int b = 0; b < 2; b++) {
      for (hipEvent_t e : {ev_up_[b], ev_k_[b], ev_down_[b]}) if (e) (void)hipEventDestroy(e);
      for (uint8_t* p : {in_[b], out_[b], out2_[b]}) if (p) (void)hipFree(p);
    }
    for (hipEvent_t e : te_) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {xst_, cst_}) if (s) (void)hipStreamDestroy(s);
  }
  hipStream_t stream() const { return cst_; }   // the compute stream
  void second(uint64_t off_items) { in2_off_ = off_items; }   // before open()
  // streams, events and buffers: n > 0 items of in_sz bytes, out_sz bytes out each and -- when out2_sz -- as many into out2
  bool open(uint64_t n, uint32_t chunk, size_t in_sz, size_t out_sz, size_t out2_sz) {
    n_ = n; chunk_ = chunk; in_sz_ = in_sz; out_sz_ = out_sz; out2_sz_ = out2_sz;
    nchunks_ = (n + chunk - 1) / chunk;
    if (fail(hipStreamCreateWithFlags(&cst_, hipStreamNonBlocking)) || fail(hipStreamCreateWithFlags(&xst_, hipStreamNonBlocking))) return false;
    for (int b = 0; b < 2; b++)
      for (hipEvent_t* e : {&ev_up_[b], &ev_k_[b], &ev_down_[b]})
        if (fail(hipEventCreateWithFlags(e, hipEventDisableTiming))) return false;
    te_.assign(6 * nchunks_, nullptr);
    for (auto& e : te_) if (fail(hipEventCreate(&e))) return false;
    for (int b = 0; b < (nchunks_ > 1 ? 2 : 1); b++) {
      if (fail(hipMalloc(&in_[b], (size_t)chunk * in_sz * (in2_off_ ? 2 : 1))) || fail(hipMalloc(&out_[b], (size_t)chunk * out_sz))) return false;
      if (out2_sz && fail(hipMalloc(&out2_[b], (size_t)chunk * out2_sz))) return false;
    }
    return true;
  }
  // every chunk through launch(stream, d_in, d_out, d_out2, cnt, lo) (lo = the chunk's first item), in -> out, out2
  using Sink = std::function<void(uint64_t lo, uint32_t cnt)>;
  template <class Launch>
  int run(const uint8_t* in, uint8_t* out, uint8_t* out2, ChunkStats* st, Launch launch, const Sink* sink = nullptr) {
    bool ok = upload(in, 0);
    for (uint64_t c = 0; ok && c < nchunks_; c++) {
      ok = (c + 1 == nchunks_ || upload(in, c + 1)) && chunk(c, out, out2, launch);
      if (ok && sink && c >= 1) ok = landed(c - 1, *sink);
    }
    if (ok && sink) ok = landed(nchunks_ - 1, *sink);
    if (ok) ok = !fail(hipStreamSynchronize(xst_)) && !fail(hipStreamSynchronize(cst_));
    if (!ok) { drain(); return rc; }
    for (uint64_t c = 0; st && c < nchunks_; c++) {
      float ms = 0.f;
      for (int h = 0; h < 3; h++)
        if (hipEventElapsedTime(&ms, te_[6 * c + 2 * h], te_[6 * c + 2 * h + 1]) == hipSuccess) (h ? st->xfer_ms : st->kern_ms) += ms;
    }
    if (st) st->points = n_;
    return G16_OK;
  }

 private:
  void drain() { for (hipStream_t s : {xst_, cst_}) if (s) (void)hipStreamSynchronize(s); }
  bool upload(const uint8_t* in, uint64_t c) {
    const int b = (int)(c & 1);
    const uint64_t lo = c * chunk_, cnt = std::min<uint64_t>(chunk_, n_ - lo);
    return !(c >= 2 && fail(hipStreamWaitEvent(xst_, ev_k_[b], 0))) && !fail(hipEventRecord(te_[6 * c + 2], xst_)) &&
           !fail(hipMemcpyAsync(in_[b], in + lo * in_sz_, cnt * in_sz_, hipMemcpyHostToDevice, xst_)) &&
           !(in2_off_ && fail(hipMemcpyAsync(in_[b] + (size_t)chunk_ * in_sz_, in + (lo + in2_off_) * in_sz_, cnt * in_sz_,
                                             hipMemcpyHostToDevice, xst_))) &&
           !fail(hipEventRecord(te_[6 * c + 3], xst_)) && !fail(hipEventRecord(ev_up_[b], xst_));
  }
  template <class Launch> bool chunk(uint64_t c, uint8_t* out, uint8_t* out2, Launch& launch) {
    const int b = (int)(c & 1);
    const uint64_t lo = c * chunk_;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk_, n_ - lo);
    if (fail(hipStreamWaitEvent(cst_, ev_up_[b], 0)) || (c >= 2 && fail(hipStreamWaitEvent(cst_, ev_down_[b], 0)))) return false;
    if (fail(hipEventRecord(te_[6 * c], cst_))) return false;
    launch(cst_, in_[b], out_[b], out2_[b], cnt, lo);
    if (fail(hipGetLastError()) || fail(hipEventRecord(te_[6 * c + 1], cst_)) || fail(hipEventRecord(ev_k_[b], cst_))) return false;
    if (fail(hipStreamWaitEvent(xst_, ev_k_[b], 0)) || fail(hipEventRecord(te_[6 * c + 4], xst_))) return false;
    if (fail(hipMemcpyAsync(out + lo * out_sz_, out_[b], (size_t)cnt * out_sz_, hipMemcpyDeviceToHost, xst_))) return false;
    if (out2 && fail(hipMemcpyAsync(out2 + lo * out2_sz_, out2_[b], (size_t)cnt * out2_sz_, hipMemcpyDeviceToHost, xst_))) return false;
    return !fail(hipEventRecord(te_[6 * c + 5], xst_)) && !fail(hipEventRecord(ev_down_[b], xst_));
  }

  // chunk c's copies down have landed (ev_down[c & 1] is recorded again only by chunk c + 2, which is not enqueued yet)
  bool landed(uint64_t c, const Sink& sink) {
    if (fail(hipEventSynchronize(ev_down_[c & 1]))) return false;
    const uint64_t lo = c * chunk_;
    sink(lo, (uint32_t)std::min<uint64_t>(chunk_, n_ - lo));
    return true;
  }

  uint64_t n_ = 0, nchunks_ = 0, in2_off_ = 0;
  uint32_t chunk_ = 0;
  size_t in_sz_ = 0, out_sz_ = 0, out2_sz_ = 0;
  hipStream_t cst_ = nullptr, xst_ = nullptr;   // compute, copies
  hipEvent_t ev_up_[2] = {}, ev_k_[2] = {}, ev_down_[2] = {};
  std::vector<hipEvent_t> te_;   // timing, six per chunk: begin and end of its kernels, its upload, its download
  uint8_t *in_[2] = {}, *out_[2] = {}, *out2_[2] = {};
};

}  // namespace g16
