// Witness calculation on the device (g16_wtns_calc): a witness program (witness_program.h) evaluated level by level.
//
// The program -- ops, terms, coefficient table, targets, level index -- stays resident.  ONE workgroup of kWcalcThreads
// threads computes one witness: its threads stride over the ops of a level (wtns_calc_eval.cuh: the same code the host
// route runs -- the 8 x 32 Montgomery arithmetic of fp.cuh, with two measured shortcuts for small values: a table of the
// inverses of small integers and a 64 x 64 product for a small wire times an integer coefficient), then
// meet at a barrier, because the next level reads what this one wrote.  The loop bounds are the level index alone, which is the same for every thread whatever the data, so
// every thread meets every barrier.  No workgroup waits for another; nothing spins on memory.
//
// Wire values live in global memory (32 bytes per wire: the canonical standard-form words of a .wtns body), written and
// read by the one workgroup that owns the witness.  A workgroup runs on one CU, whose L1 serves all its waves, so the
// stores of a level are visible to the loads of the next once every wave has drained them and passed the barrier:
// __syncthreads() is that (workgroup-scope release, s_barrier, acquire).
//
// Status: the lowest violated check of a witness, atomicMin on one word per witness (0xffffffff: none).
//
// Chunks for a prover on the same device (g16_fullprove_batch, g16_plonk_fullprove_batch): wcalc_chunk_launch computes
// up to `chunk` witnesses into one of TWO chunk buffers on the calculator's own stream and records an event once the
// chunk's status words and its public signals (gathered side by side by one small kernel) are in pinned host memory; the
// witnesses stay where they are and the prover reads them there.  Two buffers, so that chunk k + 1 is computed while the
// proofs of chunk k run; each holds what the 4 GiB rule (or G16_WTNS_CALC_CHUNK) allows, so a batched fullprove takes at
// most 2 x 4 GiB of device memory for witnesses (buffer 0 is the one g16_wtns_calc uses; both grow with the chunks
// that arrive).  wcalc_chunk_launch_from is the routine; what fills d_in is its caller's: a copy of host words
// (wcalc_chunk_launch), or a kernel that forms them on the device (pass_prove.hip).
#include <memory>

#include "witness_program.h"

namespace g16 {

static constexpr int kWcalcThreads = 256;

__global__ __launch_bounds__(kWcalcThreads) void wtns_calc_kernel(WpView p, const uint32_t* __restrict__ levels, uint32_t n_levels,
                                                                  const Fr* __restrict__ inputs, uint32_t n_inputs, Fr* w,
                                                                  uint32_t n_wires, uint32_t* __restrict__ status) {
  const uint32_t y = blockIdx.x;
  w += (size_t)y * n_wires;
  inputs += (size_t)y * n_inputs;
  if (threadIdx.x == 0) w[0] = wp_small(1);
  __syncthreads();
  uint32_t lo = levels[0];
  for (uint32_t l = 1; l <= n_levels; l++) {   // (uniform: the header's counts only)
    const uint32_t hi = levels[l];
    uint32_t worst = kWpNoCheck;
    for (uint32_t k = lo + threadIdx.x; k < hi; k += kWcalcThreads) {
      const uint32_t c = wp_eval_op(p, k, inputs, w);
      worst = c < worst ? c : worst;
    }
    if (worst != kWpNoCheck) atomicMin(status + y, worst);
    lo = hi;
    __syncthreads();
  }
}

// the public signals of `cnt` witnesses -- words 1 .. n_public of each -- side by side; total = cnt * n_public
__global__ __launch_bounds__(256) void wtns_gather_pub_kernel(const Fr* __restrict__ w, uint32_t n_wires, uint32_t n_public,
                                                              uint32_t total, Fr* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const uint32_t y = i / n_public, j = i - y * n_public;
  out[i] = w[(size_t)y * n_wires + 1 + j];
}

// One set of batch buffers.  Set 0 serves g16_wtns_calc and g16_stage_inputs; the chunks of a batched fullprove
// alternate between the two.
struct WcalcBuf {
  uint32_t cap = 0, cap_pub = 0;   // witnesses the buffers hold; ... the public-signal buffers
  DeviceBuf<Fr> d_w, d_in;         // cap * n_wires words; cap * n_inputs words
  DeviceBuf<uint32_t> d_status;    // cap words
  PinnedBuf<uint32_t> h_status;    // ... pinned
  DeviceBuf<Fr> d_pub;             // cap_pub * n_public words
  PinnedBuf<uint8_t> h_pub;        // ... pinned
  DeviceEvent ready;               // the last chunk's status words and public signals are on the host
};

struct WcalcDevice {
  int device = 0;
  uint32_t n_wires = 0, n_inputs = 0, n_public = 0, n_levels = 0, chunk = 1;
  WcalcBuf buf[2];
  DeviceBuf<WpOp> ops;
  DeviceBuf<WpEvalTerm> terms;
  DeviceBuf<Fr> coefs;
  DeviceBuf<int64_t> icoefs;
  DeviceBuf<Fr> inv_small;
  DeviceBuf<uint32_t> targets, levels;
  PhaseEvents<3> ev;
  DeviceStream st;   // (device_job.h: after everything its work touches)
  ~WcalcDevice() { (void)hipSetDevice(device); }
};

void wcalc_device_destroy(WcalcDevice* d) { delete d; }

int wcalc_device_id(const WcalcDevice* d) { return d->device; }

// the batch buffers hold `cap` witnesses; they grow to the largest chunk asked for (at most d->chunk)
static int wcalc_reserve(WcalcDevice* d, WcalcBuf& b, uint32_t cnt) {
  if (cnt <= b.cap) return G16_OK;
  b.cap = 0;
  G16_HIP(b.d_w.alloc((size_t)cnt * d->n_wires + 1));
  G16_HIP(b.d_in.alloc((size_t)cnt * d->n_inputs + 1));
  G16_HIP(b.d_status.alloc(cnt));
  G16_HIP(b.h_status.alloc(cnt));
  b.cap = cnt;
  return G16_OK;
}
// ... and the public signals of a chunk, for the callers that ask for them
static int wcalc_reserve_pub(WcalcDevice* d, WcalcBuf& b, uint32_t cnt) {
  if (cnt <= b.cap_pub) return G16_OK;
  b.cap_pub = 0;
  G16_HIP(b.d_pub.alloc((size_t)cnt * d->n_public + 1));
  G16_HIP(b.h_pub.alloc(((size_t)cnt * d->n_public + 1) * sizeof(Fr)));
  b.cap_pub = cnt;
  return G16_OK;
}

static int wcalc_device_fill(WcalcDevice* d, const WitnessProgram& p) {
  G16_HIP(hipSetDevice(d->device));
  G16_HIP(d->st.create());
  G16_HIP(d->ev.create());
  G16_HIP(upload(d->ops, p.ops));
  G16_HIP(upload(d->terms, p.eterms));
  G16_HIP(upload(d->coefs, p.coefs));
  G16_HIP(upload(d->icoefs, p.icoefs));
  G16_HIP(upload(d->inv_small, p.inv_small));
  G16_HIP(upload(d->targets, p.targets));
  G16_HIP(upload(d->levels, p.levels));
  for (WcalcBuf& b : d->buf) G16_HIP(b.ready.create());
  return wcalc_reserve(d, d->buf[0], 1);
}

int wcalc_device_create(int device, const WitnessProgram& p, uint32_t chunk, WcalcDevice** out) {
  if (const int rc = require_hip_device(device, "wtns calc: no HIP device (device = -1 is the host route)", "wtns calc: bad device ordinal"))
    return rc;
  std::unique_ptr<WcalcDevice> d(new WcalcDevice);
  d->device = device;
  d->n_wires = p.n_wires;
  d->n_inputs = p.n_inputs;
  d->n_public = p.n_public;
  d->n_levels = (uint32_t)p.levels.size() - 1;
  d->chunk = chunk < 1 ? 1 : chunk;
  if (const int rc = wcalc_device_fill(d.get(), p)) return rc;
  *out = d.release();
  return G16_OK;
}

// cnt witnesses whose inputs are at d_in, into d_w, on st (enqueue only)
static int wcalc_launch(WcalcDevice* d, const Fr* d_in, Fr* d_w, uint32_t* d_status, uint32_t cnt, hipStream_t st) {
  G16_HIP(hipMemsetAsync(d_status, 0xff, (size_t)cnt * 4, st));
  const WpView v{d->ops.p, d->terms.p, d->coefs.p, d->icoefs.p, d->targets.p, d->inv_small.p};
  wtns_calc_kernel<<<cnt, kWcalcThreads, 0, st>>>(v, d->levels.p, d->n_levels, d_in, d->n_inputs, d_w, d->n_wires, d_status);
  G16_HIP(hipGetLastError());
  return G16_OK;
}

int wcalc_device_run(WcalcDevice* d, const uint8_t* inputs, size_t count, uint8_t* out_bodies, uint32_t* status, float ms[3]) {
  G16_HIP(hipSetDevice(d->device));
  if (ms) ms[0] = ms[1] = ms[2] = 0.f;
  hipStream_t st = d->st;
  StreamDrain drain(st);   // (inputs and out_bodies are the caller's)
  for (size_t at = 0; at < count; at += d->chunk) {
    const uint32_t cnt = (uint32_t)(count - at < d->chunk ? count - at : d->chunk);
    WcalcBuf& b = d->buf[0];
    if (const int rc = wcalc_reserve(d, b, cnt)) return rc;
    G16_HIP(d->ev.record(0, st));
    if (d->n_inputs)
      G16_HIP(hipMemcpyAsync(b.d_in.p, inputs + at * d->n_inputs * 32, (size_t)cnt * d->n_inputs * 32, hipMemcpyHostToDevice, st));
    G16_HIP(d->ev.record(1, st));
    if (const int rc = wcalc_launch(d, b.d_in.p, b.d_w.p, b.d_status.p, cnt, st)) return rc;
    G16_HIP(d->ev.record(2, st));
    G16_HIP(hipMemcpyAsync(b.h_status.p, b.d_status.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    if (out_bodies)
      G16_HIP(hipMemcpyAsync(out_bodies + at * d->n_wires * 32, b.d_w.p, (size_t)cnt * d->n_wires * 32, hipMemcpyDeviceToHost, st));
    G16_HIP(d->ev.record(3, st));
    G16_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < cnt; i++) status[at + i] = b.h_status.p[i];
    if (ms)
      for (int k = 0; k < 3; k++) ms[k] += d->ev.ms(k);
  }
  drain.dismiss();
  return G16_OK;
}

int wcalc_device_run_into(WcalcDevice* d, const uint8_t* inputs, Fr* d_out, hipStream_t st, uint32_t* status) {
  G16_HIP(hipSetDevice(d->device));
  // (the calculator's own stream is idle between calls: every run ends with a wait)
  WcalcBuf& b = d->buf[0];
  StreamDrain drain(st);   // (inputs and d_out are the caller's)
  if (d->n_inputs) G16_HIP(hipMemcpyAsync(b.d_in.p, inputs, (size_t)d->n_inputs * 32, hipMemcpyHostToDevice, st));
  if (const int rc = wcalc_launch(d, b.d_in.p, d_out, b.d_status.p, 1, st)) return rc;
  G16_HIP(hipMemcpyAsync(b.h_status.p, b.d_status.p, 4, hipMemcpyDeviceToHost, st));
  G16_HIP(hipStreamSynchronize(st));
  drain.dismiss();
  *status = b.h_status.p[0];
  return G16_OK;
}

uint32_t wcalc_chunk_size(const WcalcDevice* d) { return d->chunk; }

int wcalc_chunk_release(WcalcDevice* d, hipEvent_t ev) {
  G16_HIP(hipSetDevice(d->device));
  G16_HIP(hipStreamWaitEvent(d->st, ev, 0));
  return G16_OK;
}

int wcalc_chunk_launch_from(WcalcDevice* d, int which, const WcalcFill& fill, uint32_t cnt, bool want_pub, WcalcChunk* out) {
  if (cnt < 1 || cnt > d->chunk || (which & ~1)) { set_error("wtns calc: bad chunk"); return G16_E_ARG; }
  G16_HIP(hipSetDevice(d->device));
  WcalcBuf& b = d->buf[which];
  want_pub = want_pub && d->n_public;
  if (d->n_public >= d->n_wires || (uint64_t)cnt * d->n_public > 0x7fffffffull) { set_error("wtns calc: bad chunk"); return G16_E_ARG; }
  // (a buffer that grows is freed first: the caller has released it, and hipFree waits for the device)
  int rc = wcalc_reserve(d, b, cnt);
  if (!rc && want_pub) rc = wcalc_reserve_pub(d, b, cnt);
  if (rc) return rc;
  StreamDrain drain(d->st);   // (what the fill reads is promised to `ready`, which a failing launch does not record)
  if (d->n_inputs && (rc = fill(b.d_in.p, cnt, d->st))) return rc;
  if ((rc = wcalc_launch(d, b.d_in.p, b.d_w.p, b.d_status.p, cnt, d->st))) return rc;
  G16_HIP(hipMemcpyAsync(b.h_status.p, b.d_status.p, (size_t)cnt * 4, hipMemcpyDeviceToHost, d->st));
  if (want_pub) {
    const uint32_t total = cnt * d->n_public;   // (below cnt * n_wires <= 2^27: the 4 GiB rule)
    wtns_gather_pub_kernel<<<(total + 255) / 256, 256, 0, d->st>>>(b.d_w.p, d->n_wires, d->n_public, total, b.d_pub.p);
    G16_HIP(hipGetLastError());
    G16_HIP(hipMemcpyAsync(b.h_pub.p, b.d_pub.p, (size_t)total * 32, hipMemcpyDeviceToHost, d->st));
  }
  G16_HIP(b.ready.record(d->st));
  drain.dismiss();
  out->d_w = b.d_w.p;
  out->status = b.h_status.p;
  out->pub = want_pub ? b.h_pub.p : nullptr;
  out->ready = b.ready.e;
  return G16_OK;
}

int wcalc_chunk_launch(WcalcDevice* d, int which, const uint8_t* inputs, uint32_t cnt, bool want_pub, WcalcChunk* out) {
  const size_t bytes = (size_t)cnt * d->n_inputs * 32;
  return wcalc_chunk_launch_from(d, which, [&](Fr* d_in, uint32_t, hipStream_t st) -> int {
    G16_HIP(hipMemcpyAsync(d_in, inputs, bytes, hipMemcpyHostToDevice, st));
    return G16_OK;
  }, cnt, want_pub, out);
}

void wcalc_chunk_drain(WcalcDevice* d) {
  (void)hipSetDevice(d->device);
  (void)hipStreamSynchronize(d->st);
}

}  // namespace g16
