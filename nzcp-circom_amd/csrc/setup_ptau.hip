// Sparse point combination on the device: the Groth16 setup from a prepared powers-of-tau file
// (setup_groth16.cpp::g16_groth16_setup_ptau, `snarkjs groth16 setup c.r1cs pot.ptau c_0000.zkey`).
//
// Every point section of that key is a sparse matrix times a vector of ceremony points, one sum per wire:
//   out[o] = sum over the terms t of output o of  coef_t * bases[base_t]
// with the bases the Lagrange points [L_c(tau)]G1 / [alpha L_c]G1 / [beta L_c]G1 (or [L_c]G2) of the domain and the
// coefficients those of the R1CS.  The circom mix is mostly +-1, small integers and powers of two, with few full-width
// field elements, so the host gives each term a signed class and the device runs one kernel per class:
//   +-1     : no product -- the reduce reads the affine base and adds or subtracts it (mixed addition);
//   short   : min(cf, r - cf) < 2^64: sp_short_kernel, double-and-add over the 64-bit magnitude (terms sorted by bit
//             length, so a wave runs one loop count);
//   full    : sp_full_kernel, a signed 3-bit fixed window (digits -3..4) over the 254-bit scalar, the table [1..4]P of
//             each lane in LDS.
// The products land in XYZZ; sp_reduce_kernel then sums each output's terms: the output-sorted term list is cut into
// fixed chunks of kChunk entries, one lane per chunk.  A segment that starts and ends inside a chunk is written to its
// output; a segment that crosses a chunk border leaves a partial (head or tail slot of the chunk, two per chunk).  The
// partials are again a key-sorted list, reduced by the same kernel, level after level (each one kChunk / 2 times
// shorter) until one chunk holds them all.  Column lengths run from 0 to hundreds of thousands (wire 0, the constant
// one, is in a large share of the rows); every lane still adds exactly kChunk entries.
// A slot whose segment was complete carries a dummy entry (bit 31 of the key, value infinity) so the list stays
// sorted; a segment made of dummies alone is dropped.
// Last, setup_to_affine_kernel (setup_affine.cuh) converts the outputs.  Exact canonical arithmetic (fp.cuh / ec.cuh,
// complete XYZZ formulas) as in setup_gpu.hip: the affine result is unique, so the bytes equal the oracle's whatever
// the order of summation.
//
// Terms are processed in pieces of at most kPieceTerms (cut at output borders) so the device arrays stay bounded:
// 16 M terms = 64 MB of keys / refs and at most 2 / 4 GB of G1 / G2 products.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "ec.cuh"
#include "internal.h"
#include "setup_affine.cuh"

namespace g16 {
namespace {

constexpr uint32_t kChunk = 32;                   // entries per lane of the reduce
constexpr uint32_t kDummy = 0x80000000u;          // key bit: slot without a value
constexpr uint32_t kProd = 0x80000000u;           // ref bit: the entry is product [ref & 0x7fffffff]
constexpr uint32_t kNeg = 0x40000000u;            // ref bit (no kProd): subtract base [ref & 0x3fffffff]
constexpr uint64_t kPieceTerms = (uint64_t)1 << 24;
constexpr int kFullWin = 3, kFullTbl = 1 << (kFullWin - 1), kFullDigits = (254 + kFullWin - 1) / kFullWin;
constexpr int kFullBlock = 64;

template <class FC> __device__ __forceinline__ Affine<FC> load_base(const Affine<FC>* bases, uint32_t b, bool neg) {
  Affine<FC> q = bases[b];
  if (neg && !aff_is_inf(q)) aff_neg(q);
  return q;
}

// prod[i] = [mag_i] (+-bases[base_i]), mag < 2^64 (bit 31 of sbase: negative)
template <class FC>
__global__ __launch_bounds__(256) void sp_short_kernel(const Affine<FC>* __restrict__ bases, const uint32_t* __restrict__ sbase,
                                                       const uint64_t* __restrict__ smag, uint32_t n,
                                                       XYZZ<FC>* __restrict__ prod) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = sbase[i];
  const Affine<FC> q = load_base(bases, b & 0x7fffffffu, (b >> 31) != 0);
  const uint64_t k = smag[i];
  XYZZ<FC> acc;
  xyzz_set_inf(acc);
  if (!aff_is_inf(q) && k) {
    for (int bit = 63 - __builtin_clzll(k); bit >= 0; bit--) {
      xyzz_dbl(acc);
      if ((k >> bit) & 1) xyzz_madd(acc, q);
    }
  }
  prod[i] = acc;
}

// prod[i] = [k_i] bases[base_i], k standard form < r: signed 3-bit digits, table [1..4]P in LDS (one wave per block)
template <class FC>
__global__ __launch_bounds__(kFullBlock) void sp_full_kernel(const Affine<FC>* __restrict__ bases, const uint32_t* __restrict__ fbase,
                                                             const Fr* __restrict__ fk, uint32_t n, XYZZ<FC>* __restrict__ prod) {
  __shared__ XYZZ<FC> tbl[kFullTbl][kFullBlock];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int l = threadIdx.x;
  const Affine<FC> q = bases[fbase[i]];
  XYZZ<FC> acc;
  xyzz_set_inf(acc);
  if (!aff_is_inf(q)) {
    XYZZ<FC> t;
    xyzz_from_affine(t, q);
    tbl[0][l] = t;
    xyzz_dbl_affine(t, q);
    tbl[1][l] = t;
    for (int e = 2; e < kFullTbl; e++) {
      xyzz_madd(t, q);
      tbl[e][l] = t;
    }
    const uint32_t* k = fk[i].v;   // (read from memory where indexed: a private copy would go to scratch)
    // signed digits d_j in [-3, 4], k = sum d_j 2^(3j): a window above 4 becomes window - 8 and carries one into the
    // next; k < 2^254, so the top window (bits 252-254) takes its carry without producing one
    auto window = [&](int j) -> uint32_t {
      const int pos = j * kFullWin;
      uint64_t v = k[pos >> 5];
      if ((pos >> 5) + 1 < 8) v |= (uint64_t)k[(pos >> 5) + 1] << 32;
      return (uint32_t)(v >> (pos & 31)) & ((1u << kFullWin) - 1);
    };
    // the carries run from the bottom: a bit mask of them first (kFullDigits = 85 < 128)
    uint64_t carry_lo = 0, carry_hi = 0;
    {
      uint32_t c = 0;
      for (int j = 0; j < kFullDigits; j++) {
        const uint32_t d = window(j) + c;
        c = d > (uint32_t)kFullTbl ? 1u : 0u;
        if (c) {
          if (j < 64) carry_lo |= 1ull << j;
          else carry_hi |= 1ull << (j - 64);
        }
      }
    }
    auto carry = [&](int j) -> uint32_t {
      if (j < 0) return 0;
      return (uint32_t)((j < 64 ? carry_lo >> j : carry_hi >> (j - 64)) & 1);
    };
    for (int j = kFullDigits - 1; j >= 0; j--) {
      if (j != kFullDigits - 1)
        for (int s = 0; s < kFullWin; s++) xyzz_dbl(acc);
      const int d = (int)(window(j) + carry(j - 1)) - (int)(carry(j) << kFullWin);
      if (d) {
        XYZZ<FC> e = tbl[(d < 0 ? -d : d) - 1][l];
        if (d < 0) xyzz_neg(e);
        xyzz_add(acc, e);
      }
    }
  }
  prod[i] = acc;
}

template <class FC, bool kLevel0>
__device__ __forceinline__ void sp_entry_add(XYZZ<FC>& acc, uint32_t i, const uint32_t* refs, const Affine<FC>* bases,
                                             const XYZZ<FC>* vals) {
  if (kLevel0) {
    const uint32_t r = refs[i];
    if (r & kProd) {
      xyzz_add(acc, vals[r & 0x7fffffffu]);
    } else {
      const Affine<FC> q = load_base(bases, r & 0x3fffffffu, (r & kNeg) != 0);
      if (!aff_is_inf(q)) xyzz_madd(acc, q);
    }
  } else {
    xyzz_add(acc, vals[i]);
  }
}

// One lane per chunk of kChunk key-sorted entries (see the file header).  Level 0: entry i is refs[i] (a signed base
// or a product in vals); later levels: entry i is vals[i], keys may carry kDummy.  Complete segments go to out[key];
// partials to the chunk's slots pkeys/pvals[2c] (first segment, open at the chunk's start) and [2c + 1] (last
// segment, open at its end).
template <class FC, bool kLevel0>
__global__ __launch_bounds__(256) void sp_reduce_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ refs,
                                                        const Affine<FC>* __restrict__ bases, const XYZZ<FC>* __restrict__ vals,
                                                        uint32_t n, XYZZ<FC>* __restrict__ out, uint32_t* __restrict__ pkeys,
                                                        XYZZ<FC>* __restrict__ pvals) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lo = c * kChunk;
  if (lo >= n) return;
  const uint32_t hi = n - lo < kChunk ? n : lo + kChunk;
  constexpr uint32_t M = ~kDummy;
  uint32_t cur = keys[lo] & M;
  const bool open_lo = lo > 0 && (keys[lo - 1] & M) == cur;
  bool first = true, valid = false, head_written = false;
  XYZZ<FC> acc;
  xyzz_set_inf(acc);
  XYZZ<FC> inf;
  xyzz_set_inf(inf);
  const uint32_t k_first = cur;
  for (uint32_t i = lo; i < hi; i++) {
    const uint32_t k = keys[i];
    if ((k & M) != cur) {
      // the segment `cur` ends inside the chunk
      if (first && open_lo) {
        pkeys[2 * c] = cur | (valid ? 0u : kDummy);
        pvals[2 * c] = acc;
        head_written = true;
      } else if (valid) {
        out[cur] = acc;
      }
      first = false;
      cur = k & M;
      valid = false;
      xyzz_set_inf(acc);
    }
    if (!(k & kDummy)) {
      valid = true;
      sp_entry_add<FC, kLevel0>(acc, i, refs, bases, vals);
    }
  }
  const bool open_hi = hi < n && (keys[hi] & M) == cur;
  if (first && open_lo) {            // one segment, open at the start (and perhaps at the end)
    pkeys[2 * c] = cur | (valid ? 0u : kDummy);
    pvals[2 * c] = acc;
    pkeys[2 * c + 1] = cur | kDummy;
    pvals[2 * c + 1] = inf;
    return;
  }
  if (!head_written) {               // the first segment was complete: a dummy keeps the list sorted
    pkeys[2 * c] = k_first | kDummy;
    pvals[2 * c] = inf;
  }
  if (open_hi) {
    pkeys[2 * c + 1] = cur | (valid ? 0u : kDummy);
    pvals[2 * c + 1] = acc;
  } else {
    if (valid) out[cur] = acc;
    pkeys[2 * c + 1] = cur | kDummy;
    pvals[2 * c + 1] = inf;
  }
}

bool is_u64(const Fr& x) {
  for (int i = 2; i < 8; i++)
    if (x.v[i]) return false;
  return true;
}
uint64_t lo64(const Fr& x) { return (uint64_t)x.v[0] | ((uint64_t)x.v[1] << 32); }
Fr r_minus(const Fr& x) {   // r - x for 0 < x < r
  static const uint32_t R[8] = G16_FR_P;
  Fr o;
  int64_t br = 0;
  for (int i = 0; i < 8; i++) {
    br += (int64_t)R[i] - (int64_t)x.v[i];
    o.v[i] = (uint32_t)br;
    br >>= 32;
  }
  return o;
}

// one piece of the term list: outputs [o_lo, o_hi), terms [t_lo, t_hi)
struct HostPiece {
  std::vector<uint32_t> keys, refs;     // level-0 entries, output-sorted
  std::vector<uint32_t> sbase;          // short products (sorted by magnitude bit length), bit 31 = negative
  std::vector<uint64_t> smag;
  std::vector<uint32_t> fbase;          // full products
  std::vector<Fr> fk;
};

bool build_piece(const SparseTerms& t, uint64_t o_lo, uint64_t o_hi, uint64_t nbases, HostPiece& hp, SparseStats& st) {
  const uint64_t t_lo = t.start[o_lo], t_hi = t.start[o_hi];
  hp.keys.clear(); hp.refs.clear(); hp.sbase.clear(); hp.smag.clear(); hp.fbase.clear(); hp.fk.clear();
  hp.keys.reserve(t_hi - t_lo);
  hp.refs.reserve(t_hi - t_lo);
  // short terms by bit length: counting sort over 64 bins, the product index fixed once all are known
  std::vector<uint32_t> sterm;   // index into keys of each short term (pre-sort order)
  std::vector<uint8_t> sbits;
  std::vector<uint32_t> fterm;
  for (uint64_t o = o_lo; o < o_hi; o++) {
    for (uint64_t j = t.start[o]; j < t.start[o + 1]; j++) {
      const Fr& cf = t.coef[j];
      const uint32_t b = t.base[j];
      if (b >= nbases) return false;
      bool zero = true;
      for (int i = 0; i < 8; i++) zero = zero && cf.v[i] == 0;
      if (zero) { st.zero++; continue; }
      const Fr ncf = r_minus(cf);
      const bool pos_small = is_u64(cf), neg_small = is_u64(ncf);
      const uint32_t e = (uint32_t)hp.keys.size();
      hp.keys.push_back((uint32_t)o);
      if (pos_small && lo64(cf) == 1) { hp.refs.push_back(b); st.pm1++; continue; }
      if (neg_small && lo64(ncf) == 1) { hp.refs.push_back(b | kNeg); st.pm1++; continue; }
      hp.refs.push_back(0);   // product index set below
      if (pos_small || neg_small) {
        const uint64_t mag = pos_small ? lo64(cf) : lo64(ncf);
        sterm.push_back(e);
        sbits.push_back((uint8_t)(63 - __builtin_clzll(mag)));
        hp.sbase.push_back(b | (pos_small ? 0u : 0x80000000u));
        hp.smag.push_back(mag);
        st.shorts++;
      } else {
        fterm.push_back(e);
        hp.fbase.push_back(b);
        hp.fk.push_back(cf);
        st.full++;
      }
    }
  }
  const size_t ns = sterm.size();
  uint32_t cnt[65] = {0};
  for (size_t i = 0; i < ns; i++) cnt[sbits[i] + 1]++;
  for (int i = 0; i < 64; i++) cnt[i + 1] += cnt[i];
  std::vector<uint32_t> sb2(ns);
  std::vector<uint64_t> sm2(ns);
  for (size_t i = 0; i < ns; i++) {
    const uint32_t d = cnt[sbits[i]]++;
    sb2[d] = hp.sbase[i];
    sm2[d] = hp.smag[i];
    hp.refs[sterm[i]] = kProd | d;
  }
  hp.sbase.swap(sb2);
  hp.smag.swap(sm2);
  for (size_t i = 0; i < fterm.size(); i++) hp.refs[fterm[i]] = kProd | (uint32_t)(ns + i);
  return true;
}

template <class FC>
int sparse_device(int device, const uint8_t* const* seg, const size_t* seg_n, int nseg, const SparseTerms& t,
                  uint8_t* out, SparseStats* stats) {
  const uint64_t nout = t.start.size() - 1;
  if (const int rc = require_hip_device("groth16 setup", device)) return rc;
  if (nout == 0) return G16_OK;
  G16_HIP(hipSetDevice(device));
  uint64_t nbases = 0;
  for (int s = 0; s < nseg; s++) nbases += seg_n[s];
  // pieces: cut at output borders once kPieceTerms are reached (an output with more terms is a piece of its own)
  uint64_t piece_terms = kPieceTerms;
  if (const char* e = getenv("G16_SETUP_PIECE_TERMS")) {   // (tests: force several pieces on a small circuit)
    const long long v = atoll(e);
    if (v > 0) piece_terms = (uint64_t)v;
  }
  std::vector<uint64_t> cuts{0};
  {
    uint64_t o = 0;
    while (o < nout) {
      uint64_t e = o + 1;
      while (e < nout && t.start[e + 1] - t.start[o] <= piece_terms) e++;
      cuts.push_back(e);
      o = e;
    }
  }
  uint64_t max_terms = 0;
  for (size_t k = 0; k + 1 < cuts.size(); k++) max_terms = std::max(max_terms, t.start[cuts[k + 1]] - t.start[cuts[k]]);
  if (max_terms >= 0x40000000ull || nbases >= 0x40000000ull || nout >= 0x80000000ull) {
    set_error("groth16 setup: too many terms for one output or too many points");
    return G16_E_ARG;
  }
  const uint64_t max_slots = 2 * ((max_terms + kChunk - 1) / kChunk) + 2;
  DeviceJob job("groth16 setup");
  DeviceBuf<Affine<FC>> d_bases, d_aff;
  DeviceBuf<uint32_t> d_keys, d_refs, d_sb, d_fb, d_pk[2];
  DeviceBuf<uint64_t> d_sm;
  DeviceBuf<Fr> d_fk;
  DeviceBuf<XYZZ<FC>> d_prod, d_out, d_pv[2];
  DeviceTimer timer;
  DeviceStream st;
  float kern_ms = 0.f;
  HostPiece hp;
  SparseStats local;
  if (job.fail(st.create()) || job.fail(timer.create()) || job.fail(d_bases.alloc(nbases)) || job.fail(d_keys.alloc(max_terms)) ||
      job.fail(d_refs.alloc(max_terms)) || job.fail(d_sb.alloc(max_terms)) || job.fail(d_sm.alloc(max_terms)) ||
      job.fail(d_prod.alloc(max_terms)))
    return job.rc;
  for (int k = 0; k < 2; k++)
    if (job.fail(d_pk[k].alloc(max_slots)) || job.fail(d_pv[k].alloc(max_slots))) return job.rc;
  if (job.fail(d_out.alloc(nout)) || job.fail(d_aff.alloc(nout)) ||
      job.fail(hipMemsetAsync(d_out.p, 0, nout * sizeof(XYZZ<FC>), st)))   // zz = 0: infinity (empty sums)
    return job.rc;
  {
    uint64_t off = 0;
    for (int s = 0; s < nseg; s++) {
      if (seg_n[s] && job.fail(hipMemcpyAsync(d_bases.p + off, seg[s], seg_n[s] * sizeof(Affine<FC>), hipMemcpyHostToDevice, st)))
        return job.rc;
      off += seg_n[s];
    }
  }
  size_t fcap = 0;
  for (size_t k = 0; k + 1 < cuts.size(); k++) {
    if (!build_piece(t, cuts[k], cuts[k + 1], nbases, hp, local)) {
      set_error("groth16 setup: term refers to a point outside the uploaded blocks");
      return G16_E_ARG;
    }
    const uint32_t n = (uint32_t)hp.keys.size();
    const uint32_t ns = (uint32_t)hp.sbase.size(), nf = (uint32_t)hp.fbase.size();
    if (n == 0) continue;
    if (nf > fcap) {   // (the stream is idle: every piece ends with a wait)
      d_fb.reset();
      d_fk.reset();
      fcap = nf;
      if (job.fail(d_fb.alloc(fcap)) || job.fail(d_fk.alloc(fcap))) return job.rc;
    }
    if (job.fail(hipMemcpyAsync(d_keys.p, hp.keys.data(), (size_t)n * 4, hipMemcpyHostToDevice, st)) ||
        job.fail(hipMemcpyAsync(d_refs.p, hp.refs.data(), (size_t)n * 4, hipMemcpyHostToDevice, st)))
      return job.rc;
    if (ns && (job.fail(hipMemcpyAsync(d_sb.p, hp.sbase.data(), (size_t)ns * 4, hipMemcpyHostToDevice, st)) ||
               job.fail(hipMemcpyAsync(d_sm.p, hp.smag.data(), (size_t)ns * 8, hipMemcpyHostToDevice, st))))
      return job.rc;
    if (nf && (job.fail(hipMemcpyAsync(d_fb.p, hp.fbase.data(), (size_t)nf * 4, hipMemcpyHostToDevice, st)) ||
               job.fail(hipMemcpyAsync(d_fk.p, hp.fk.data(), (size_t)nf * sizeof(Fr), hipMemcpyHostToDevice, st))))
      return job.rc;
    if (job.fail(timer.start(st))) return job.rc;
    if (ns) sp_short_kernel<FC><<<(ns + 255) / 256, 256, 0, st>>>(d_bases.p, d_sb.p, d_sm.p, ns, d_prod.p);
    if (nf) sp_full_kernel<FC><<<(nf + kFullBlock - 1) / kFullBlock, kFullBlock, 0, st>>>(d_bases.p, d_fb.p, d_fk.p, nf, d_prod.p + ns);
    // level 0, then the partials until one chunk holds them all
    uint32_t chunks = (n + kChunk - 1) / kChunk;
    sp_reduce_kernel<FC, true><<<(chunks + 255) / 256, 256, 0, st>>>(d_keys.p, d_refs.p, d_bases.p, d_prod.p, n, d_out.p, d_pk[0].p,
                                                                     d_pv[0].p);
    int cur = 0;
    while (chunks > 1) {
      const uint32_t m = 2 * chunks;
      chunks = (m + kChunk - 1) / kChunk;
      sp_reduce_kernel<FC, false><<<(chunks + 255) / 256, 256, 0, st>>>(d_pk[cur].p, nullptr, d_bases.p, d_pv[cur].p, m, d_out.p,
                                                                        d_pk[cur ^ 1].p, d_pv[cur ^ 1].p);
      cur ^= 1;
    }
    if (job.fail(hipGetLastError()) || job.fail(timer.stop(st)) || job.fail(hipStreamSynchronize(st))) return job.rc;
    kern_ms += timer.ms();
  }
  if (job.fail(timer.start(st))) return job.rc;
  const uint64_t nb = (nout + kBatch - 1) / kBatch;
  setup_to_affine_kernel<FC><<<(unsigned)((nb + 255) / 256), 256, 0, st>>>(d_out.p, d_aff.p, (uint32_t)nout);
  if (job.fail(hipGetLastError()) || job.fail(timer.stop(st)) ||
      job.fail(hipMemcpyAsync(out, d_aff.p, nout * sizeof(Affine<FC>), hipMemcpyDeviceToHost, st)) ||
      job.fail(hipStreamSynchronize(st)))
    return job.rc;
  kern_ms += timer.ms();
  if (stats) {
    stats->pm1 += local.pm1;
    stats->shorts += local.shorts;
    stats->full += local.full;
    stats->zero += local.zero;
    stats->kern_ms += kern_ms;
  }
  return G16_OK;
}

}  // namespace

int setup_sparse_g1(int device, const uint8_t* const* seg, const size_t* seg_n, int nseg, const SparseTerms& t,
                    uint8_t* out, SparseStats* st) {
  return sparse_device<FqOps>(device, seg, seg_n, nseg, t, out, st);
}
int setup_sparse_g2(int device, const uint8_t* const* seg, const size_t* seg_n, int nseg, const SparseTerms& t,
                    uint8_t* out, SparseStats* st) {
  return sparse_device<Fq2Ops>(device, seg, seg_n, nseg, t, out, st);
}

}  // namespace g16
