/*
 * g16_prover.h -- C ABI of libg16hip.so, the MI355X (gfx950) Groth16 prover for snarkjs-format
 * proving keys.  This is the drop-in boundary: plain pointers and sizes,
 * no C++ or torch types, no exceptions across the boundary.
 *
 * What each entry point replaces.  The reference repo has no prover source; the path lives in
 * the npm packages it pins (never vendored):
 *     snarkjs 0.4.12        /root/reference/yarn.lock:987-1001   (package.json:12)
 *     ffjavascript 0.2.48   /root/reference/yarn.lock:408-416
 *     wasmcurves 0.1.0      /root/reference/yarn.lock:1132-1138
 *     @iden3/binfileutils   /root/reference/yarn.lock:10-16
 * and the only snarkjs call sites in the reference are the CLI lines /root/reference/Makefile:30-33.
 * The [EXT] names below are the published functions of those packages.
 *
 * Conventions
 *   - return 0 on success, negative G16_E_* on failure; g16_last_error() gives the text
 *     (thread-local; for input errors the text is snarkjs's own Error message).
 *   - the caller owns every buffer it passes; the library copies what it keeps.
 *   - field elements are 32 bytes little-endian.  Proof points come out affine in STANDARD
 *     (non-Montgomery) form: that is what snarkjs `G1.toObject` stringifies.
 *   - one in-flight call per g16_prover handle; different handles may be used concurrently.
 */
#ifndef G16_PROVER_H
#define G16_PROVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G16_OK 0
#define G16_E_ARG (-1)    /* bad argument */
#define G16_E_FORMAT (-2) /* malformed zkey/wtns (message = snarkjs's) */
#define G16_E_HIP (-3)    /* HIP runtime error */
#define G16_E_NOGPU (-4)  /* no gfx950 device / extension cannot run: never falls back to CPU */
#define G16_E_STATE (-5)

typedef struct g16_prover g16_prover;

typedef struct g16_opts {
  int32_t device;       /* HIP device ordinal */
  int32_t shard_rank;   /* this handle owns point range [rank*n/count, (rank+1)*n/count) of every */
  int32_t shard_count;  /* base section; 0/1 = whole key                               */
  int32_t window_bits;  /* Pippenger window c (0 = auto)                                           */
  int32_t task_len;     /* max sorted entries per bucket-accumulation task (0 = auto)              */
  uint32_t flags;       /* bits 8..15: MSM window-precomputation factor (0 = default, see G16_OPT_PRECOMP); other bits 0 */
} g16_opts;
/* flags value asking for a base table with 2^(c*W*k)*P for k < factor (more HBM, fewer bucket rows) */
#define G16_OPT_PRECOMP(factor) (((uint32_t)(factor) & 0xffu) << 8)

typedef struct g16_proof {
  uint8_t a[64];  /* pi_a: x | y                      */
  uint8_t b[128]; /* pi_b: x.c0 | x.c1 | y.c0 | y.c1  */
  uint8_t c[64];  /* pi_c: x | y                      */
} g16_proof;      /* infinity = all-zero bytes        */

typedef struct g16_info {
  uint32_t n_vars, n_public, domain_size, n_coefs;
  uint32_t n_a, n_b1, n_b2, n_c, n_h; /* non-infinity bases resident per MSM (this shard) */
  uint32_t window_bits[5];            /* c chosen for A, B1, B2, C, H */
} g16_info;

/* Per-phase device timings of the last g16_prove* on this handle, milliseconds (HIP events on the
 * prover's streams).  The witness MSMs A, B1, C share one front end and one G1 bucket-accumulate launch, B2 rides
 * on B1's buckets as the G2 lane: msm_ms[0] = that group's main chain, msm_ms[2] = until the G2 lane ends (traced
 * runs only), msm_ms[4] = the H-MSM, [1] and [3] are 0.  *_kernel_ms are the bucket-accumulate kernels alone
 * (the roofline kernel of bench.py): [0] = G1 over A+B1+C, [2] = G2 (B2), [4] = H. */
typedef struct g16_timings {
  float upload_ms, qap_ms, ntt_ms, msm_ms[5], tail_ms, total_ms;
  float msm_accum_kernel_ms[5];
} g16_timings;

/* [EXT] snarkjs groth16_prove.js: readBinFile(zkey,"zkey",2) + zkey_utils.readHeader + the
 * section reads 4..9 of groth16.prove.  Parses and validates, regroups section 4 into CSR,
 * uploads coefficients and (this shard's) bases to HBM once, builds NTT tables.
 * Errors: "<name>: Invalid File format", "Version not supported", "zkey file is not groth16". */
int g16_create(const uint8_t* zkey, size_t zkey_len, const g16_opts* opts, g16_prover** out);

/* [EXT] snarkjs groth16.prove(zkey, wtns): buildABC1 -> 3x(Fr.ifft, batchApplyKey, Fr.fft) ->
 * joinABC -> 5x multiExpAffine -> blinding -> toAffine.  r, s: 32-byte LE scalars < r, or NULL
 * for the OS CSPRNG (snarkjs: Fr.random()).  pub receives n_public * 32 bytes (w[1..p]).
 * Errors: "Curve of the witness does not match the curve of the proving key",
 *         "Invalid witness length. Circuit: N, witness: M". */
int g16_prove(g16_prover* p, const uint8_t* wtns, size_t wtns_len, const uint8_t r[32],
              const uint8_t s[32], g16_proof* out, uint8_t* pub);

/* Batch of independent witnesses against the resident key (BASELINE config 3).  rs: count*64
 * bytes (r|s per proof) or NULL; pub: count*n_public*32 bytes or NULL. */
int g16_prove_batch(g16_prover* p, const uint8_t* const* wtns, const size_t* wtns_lens, size_t count,
                    const uint8_t* rs, g16_proof* out, uint8_t* pub);

/* HBM-resident witness slots: g16_stage_witness parses + uploads (the PCIe leg), g16_prove_staged
 * runs the device pipeline on a staged slot -- bench.py times the latter ("inputs already
 * resident in HBM").  Slots are created on demand; staging the same slot again overwrites it. */
int g16_stage_witness(g16_prover* p, uint32_t slot, const uint8_t* wtns, size_t wtns_len);
int g16_prove_staged(g16_prover* p, uint32_t slot, const uint8_t r[32], const uint8_t s[32],
                     g16_proof* out, uint8_t* pub);

/* Multi-GPU: a sharded handle computes its partial MSM sums; the host exchanges the
 * G16_PARTIAL_BYTES blobs (RCCL all-gather of bytes) and any rank finishes the proof.
 * partials = count blobs back to back, one per shard rank. */
#define G16_PARTIAL_BYTES (128 * 4 + 256) /* XYZZ sums A,B1,C,H (G1) + B2 (G2), Montgomery */
int g16_prove_partial(g16_prover* p, uint32_t slot, uint8_t partial[G16_PARTIAL_BYTES]);
int g16_prove_finish(g16_prover* p, uint32_t slot, const uint8_t* partials, uint32_t count,
                     const uint8_t r[32], const uint8_t s[32], g16_proof* out, uint8_t* pub);

/* Multi-GPU with the H-polynomial pipeline sharded as well (SURVEY 8e "later: split A/B/C across GPUs"): instead
 * of every shard repeating QAP + 6 NTTs, shard v mod count evaluates vector v (0 = A, 1 = B, 2 = C) on the odd
 * coset and the shards exchange slices, so that each joins and multi-exponentiates only its own range of P:
 *   g16_shard_begin  starts this shard's witness MSMs (they keep running) and, for every bit v of vec_mask,
 *                    computes the coset evaluations of vector v and copies all domain_size elements to
 *                    out_vecs[v] -- any memory the device can address (device, peer device, pinned or plain host);
 *                    returns when the copies are complete.  Elements are G16_LAZY_FR_BYTES each (the kernels'
 *                    9 x 29-bit lazy Montgomery image: opaque, only to be handed to g16_shard_end).
 *   (exchange)       shard r needs elements [lo, hi) = g16_shard_range(domain_size, r, count) of all three vectors:
 *                    an RCCL scatter / all-to-all between processes, peer copies inside one process.
 *   g16_shard_end    takes the three slices ((hi - lo) elements each), joins P = A.B - C on the slice, runs the
 *                    H-MSM over its bases and returns the partial sums exactly like g16_prove_partial.
 * Between the two, the handle's proof context runs the begun witness MSMs: g16_get_info, g16_get_timings and
 * g16_prove_finish (host only) are allowed; every other call on the handle -- g16_prove, g16_prove_batch,
 * g16_stage_witness, g16_prove_staged, g16_prove_partial, g16_qap_eval, a second g16_shard_begin -- fails with
 * G16_E_STATE ("g16_shard_begin in progress: call g16_shard_end first") and changes nothing. */
#define G16_LAZY_FR_BYTES 40
int g16_shard_begin(g16_prover* p, uint32_t slot, uint32_t vec_mask, void* const out_vecs[3]);
int g16_shard_end(g16_prover* p, uint32_t slot, const void* const slices[3], uint8_t partial[G16_PARTIAL_BYTES]);

/* One PROCESS, several GPUs (the Node.js host of BASELINE config 4): a g16_multi owns one sharded handle per
 * entry of `devices` (an ordinal may repeat: several shards on one GPU) and g16_multi_prove runs the sharded
 * pipeline above on one host thread per shard, moving the slices between devices with peer copies and adding the
 * partial sums on the host.  Same results and error texts as g16_prove.  opts: device / shard_* are ignored. */
typedef struct g16_multi g16_multi;
int g16_multi_create(const uint8_t* zkey, size_t zkey_len, const int32_t* devices, uint32_t ndev,
                     const g16_opts* opts, g16_multi** out);
int g16_multi_prove(g16_multi* m, const uint8_t* wtns, size_t wtns_len, const uint8_t r[32], const uint8_t s[32],
                    g16_proof* out, uint8_t* pub);
int g16_multi_get_info(const g16_multi* m, g16_info* out, uint32_t* n_shards);
void g16_multi_destroy(g16_multi* m);

/* Host-only assembly from gathered partials (no GPU handle needed; reads only the zkey header),
 * and the shard -> point-range map used by g16_create. */
int g16_finish_host(const uint8_t* zkey, size_t zkey_len, const uint8_t* partials, uint32_t count,
                    const uint8_t r[32], const uint8_t s[32], g16_proof* out);
void g16_shard_range(uint32_t total, int32_t rank, int32_t count, uint32_t* lo, uint32_t* hi);

int g16_get_info(const g16_prover* p, g16_info* out);
/* Device-side phase times of the last proof this handle completed: a g16_prove, g16_prove_staged, g16_prove_partial
 * or g16_shard_end that succeeded (after g16_prove_batch: the last proof of the batch it collected).  A proof that
 * failed, a refused call and a g16_shard_begin still in progress leave them unchanged, and two reads with nothing
 * completed in between return the same struct.  Read from that proof's HIP events when called (a proof itself does
 * not pay for them; the events are kept apart from those of the next launch, so a read never waits for work still
 * in flight); upload_ms is the last staging's (g16_stage_witness, or the upload of a successful g16_prove).
 * Serialised with the handle's other entry points. */
int g16_get_timings(const g16_prover* p, g16_timings* out);
void g16_destroy(g16_prover* p);
const char* g16_last_error(void);

/* Operator-level entry points, the device twins of ffjavascript's public curve API [EXT]:
 *   g16_fr_fft / g16_fr_ifft          Fr.fft / Fr.ifft   (n Montgomery residues, natural order,
 *                                     in place; ifft includes 1/n)
 *   g16_g1_multiexp / g16_g2_multiexp G1/G2.multiExpAffine(bases LEM affine, scalars standard LE)
 *                                     -> affine STANDARD-form point (64 / 128 bytes)
 *   g16_fr_batch_mul                  Montgomery products out[i] = a[i]*b[i]  (frm_mul)        */
int g16_fr_fft(int device, uint8_t* buf, size_t n);
int g16_fr_ifft(int device, uint8_t* buf, size_t n);
int g16_fr_batch_mul(int device, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n, int field /*0 Fr, 1 Fq*/);
/* Layer tests: elementwise field op (op: 0 mul, 1 add, 2 sub, 3 toMontgomery, 4 fromMontgomery,
 * 5 neg; field 0 = Fr, 1 = Fq; raw 32-byte images in and out) and elementwise affine point addition
 * a[i]+b[i] on the device (curve 1 = G1, 2 = G2; LEM affine in, STANDARD affine out). */
int g16_field_op(int device, int field, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);
int g16_ec_add(int device, int curve, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);
/* Layer tests of the arithmetic the kernels actually run (fq29.cuh / fr29.cuh / ec29.cuh: 9 x 29-bit limbs,
 * lazy reduction, Montgomery radix 2^261), the device twins of wasmcurves' f1m_mul / f1m_square / curve add [EXT].
 * Elements are RAW limb images: 9 little-endian u32 limbs + 1 pad word = 40 bytes, value = sum l[i] 2^(29 i)
 * (limbs 0..7 below 2^29; the value may exceed p: the format is lazy), so tests can place inputs at the bounds
 * the kernels rely on.  field 0 = Fr, 1 = Fq.  op: 0 mul(a,b)  1 sqr(a)  2 a*b + c*d (one reduction)
 * 3 a^2 + c*d  4 a+b  5 a+2p-b  6 a+6p-b  7 a+4p-b-2c  8 2p-a  9 mul (row-wise variant)  10 weak_reduce (Fr)
 * 11 zero tests: limb 0 = (a == 0 mod p), limb 1 = the low-limb filter f29_maybe_zero<7>.  b/c/d may be NULL
 * when the op ignores them. */
int g16_f29_op(int device, int field, int op, const uint8_t* a, const uint8_t* b, const uint8_t* c,
               const uint8_t* d, uint8_t* out, size_t n);
/* XYZZ point formulas over that field.  curve 1 = G1 (coordinate = 40 B), 2 = G2 (80 B: a | b of a + b u).
 * acc / out: n XYZZ images (x | y | zz | zzz); q: n affine images (x | y) for op 0, 1, 4, n XYZZ images for op 2.
 * op 0 = x29_madd_fast, the exception-free hot-loop formula (flags[i] = 1 when it asks for the redo pass),
 * 1 = x29_madd (complete), 2 = x29_add, 3 = x29_dbl, 4 = x29_madd after a pack/unpack round trip of q (the
 * resident 64/128-byte base format). */
int g16_x29_op(int device, int curve, int op, const uint8_t* acc, const uint8_t* q, uint8_t* out, uint8_t* flags,
               size_t n);
/* [EXT] snarkjs groth16_prove.js buildABC1 on a staged witness: A_T, B_T, C_T = A_T o B_T as canonical
 * Montgomery(2^256) residues, domain_size * 32 bytes each. */
int g16_qap_eval(g16_prover* p, uint32_t slot, uint8_t* a, uint8_t* b, uint8_t* c);
int g16_g1_multiexp(int device, const uint8_t* bases, const uint8_t* scalars, size_t n,
                    int window_bits, uint8_t out[64]);
int g16_g2_multiexp(int device, const uint8_t* bases, const uint8_t* scalars, size_t n,
                    int window_bits, uint8_t out[128]);

/* Test-only trapdoor setup over a shape-matched synthetic R1CS (the real nzcp_live
 * R1CS cannot be produced offline).  Host-only (no GPU needed).  Emits a snarkjs-layout .zkey and
 * .wtns plus the verification key points (alpha1 | beta2 | gamma2 | delta2 | IC[0..p], affine
 * Montgomery LE, 64/128 bytes each).  Buffers are malloc'd; release with g16_free.
 * Generator spec: oracle/synth.py docstring (both sides follow the same draw order). */
int g16_synth_setup(uint32_t n_vars, uint32_t n_public, uint32_t n_constraints, uint64_t seed,
                    int threads, uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                    uint8_t** vkey, size_t* vkey_len);
/* A fresh satisfying witness for the same synthetic circuit (batch mode, BASELINE config 3): the
 * free wires are redrawn from `wseed`, the slack wires re-solved; the circuit stays that of `seed`.
 * g16_synth_setup uses wseed = seed.  Returns a .wtns image. */
int g16_synth_witness(uint32_t n_vars, uint32_t n_public, uint32_t n_constraints, uint64_t seed,
                      uint64_t wseed, uint8_t** wtns, size_t* wtns_len);
/* Test-only trapdoor setup of a REAL circuit: iden3 .r1cs v1 in (what `circom --r1cs`
 * writes; nPublic = nPubOut + nPubIn), snarkjs-layout .zkey and the verification-key points out (same
 * layout as g16_synth_setup).  Trapdoor from `seed`.  Lets anyone with circom fabricate a key for the
 * real nzcp_live R1CS and benchmark its true shape; NOT a ceremony -- the trapdoor is known. */
int g16_r1cs_setup(const uint8_t* r1cs, size_t r1cs_len, uint64_t seed, int threads, uint8_t** zkey,
                   size_t* zkey_len, uint8_t** vkey, size_t* vkey_len);
/* Where the fixed-base multiplications of every *_setup entry point run ("trapdoor setup at scale on
 * GPU (fixed-base MSM kernel)"; stands in for `snarkjs groth16 setup`, /root/reference/Makefile:30-31 records the PLONK
 * twin): device >= 0 = that HIP device (csrc/setup_gpu.hip: one lane per scalar over a small L2-resident window table,
 * batched conversion to affine), -1 = host threads (the default).  Process-wide; the zkey bytes are the same either way.
 * A setup with the device path selected and no GPU present returns G16_E_NOGPU. */
int g16_setup_device(int device);

/* Test-only: a REAL constraint system for BASELINE config 5 -- `blocks` chained SHA-256 compressions
 * d_{i+1} = SHA-256(d_i) over a 32-byte private message, bit-level R1CS in the style of the circomlib sha256
 * gadgets nzcptpl.circom includes (/root/reference/circuits/nzcptpl.circom:3-6 include list), ~27 k
 * constraints per block; public signals = the 256 digest bits, MSB-first (the NZCP circuit's bit order,
 * /root/reference/test/nzcp.js:41-47).  Trapdoor zkey as g16_synth_setup; r1cs = iden3 .r1cs v1 image.
 * Any output pair may be NULL. */
int g16_sha256_chain_setup(uint32_t blocks, const uint8_t msg[32], uint64_t seed, int threads,
                           uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                           uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len);

/* Test-only: plain SHA-256 of a `len`-byte private message (len fixed at circuit-build time, FIPS 180-4
 * padding, multi-block), same gadgets and wire layout: public signals = the 256 digest bits MSB-first, i.e.
 * the `toBeSignedSha256` slice of the NZCP circuit's public.json when msg = the pass's ToBeSigned
 * (/root/reference/circuits/nzcptpl.circom:447-500, /root/reference/test/nzcp.js:41-47). */
int g16_sha256_message_setup(const uint8_t* msg, uint32_t len, uint64_t seed, int threads,
                             uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                             uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len);

/* Test-only: the NZCP circuit's public interface on a FIXED pass layout -- public signals [0..255] =
 * SHA-256("given,family,dob") bits, [256..511] = SHA-256(ToBeSigned) bits, [512] = exp, exactly the layout and
 * bit order of /root/reference/test/nzcp.js:41-47 -- with the byte offsets of the three strings and of the
 * 4 exp bytes inside ToBeSigned given as circuit constants (the reference finds them by in-circuit CBOR parsing,
 * /root/reference/circuits/cbortpl.circom; not restated).  The credential string reuses the ToBeSigned bit
 * wires, so the three outputs are bound to one ToBeSigned. */
int g16_nzcp_fixed_layout_setup(const uint8_t* tbs, uint32_t len, const uint32_t seg_off[3], const uint32_t seg_len[3],
                                uint32_t exp_off, uint64_t seed, int threads,
                                uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len,
                                uint8_t** vkey, size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len);
/* Test-only: the NZCP circuit library as native R1CS gadgets (csrc/nzcp_gadgets.h), the twins of the reference's
 * per-template test circuits /root/reference/circuits/ *_test.circom.  Builds ONE template over the given private
 * inputs, checks every emitted row on the computed witness and returns the template's output signals (in the
 * order the reference declares them).  name: getType getX quinSelector getV decodeUint23 decodeUint readType
 * skipValueScalar skipValue stringEquals readStringLength readMapLength copyString findVCAndExp findCredSubj
 * readCredSubj concatCredSubj sha256Var; params / inputs: the template parameters / input signals in declaration
 * order (arrays flattened).  G16_E_STATE with "constraint not satisfied: ..." where circom's witness generator
 * would throw.  *nout: capacity in, count out. */
int g16_nzcp_gadget(const char* name, const uint32_t* params, uint32_t nparams, const uint64_t* inputs, uint32_t nin,
                    uint64_t* outputs, uint32_t* nout, uint32_t* n_constraints);
/* Test-only: NZCPPubIdentity(params[0..6]) (/root/reference/circuits/nzcptpl.circom:433) with the CBOR search in
 * the circuit -- nzcp_exampleTest.circom = {0, 314, 0, 4, 2, 4, 5}, nzcp_liveTest.circom = {1, 355, 0, 4, 2, 4, 6} --
 * built natively for the given ToBeSigned bytes: R1CS, witness, trapdoor key.  Public signals as
 * /root/reference/test/nzcp.js:41-47.  Any output pair may be NULL. */
int g16_nzcp_circuit_setup(const uint32_t params[7], const uint8_t* tbs, uint32_t len, uint64_t seed, int threads,
                           uint8_t** zkey, size_t* zkey_len, uint8_t** wtns, size_t* wtns_len, uint8_t** vkey,
                           size_t* vkey_len, uint8_t** r1cs, size_t* r1cs_len, uint32_t* n_constraints);
void g16_free(void* p);

/* ---------------------------------------------------------------------------------------------------------------
 * Groth16 batch verifier on the device (the acceptance check of SURVEY 3.4).
 * [EXT] snarkjs groth16_verify.js `groth16.verify(vk, publicSignals, proof)`: cpub = IC[0] + sum pub_i IC[i+1], then
 * curve.pairingEq(-pi_a, pi_b, cpub, vk_gamma_2, pi_c, vk_delta_2, vk_alpha_1, vk_beta_2)  (pins
 * /root/reference/yarn.lock:987-1001; verification_key.json layout SURVEY App. A.5).  One handle = one verification
 * key resident on one GPU; a batch call returns one verdict per proof (the verdicts of one-at-a-time verification).
 *
 * vkey: alpha1 (64 B) | beta2 (128) | gamma2 (128) | delta2 (128) | IC[0..n_public] (64 each), affine little-endian,
 *       G2 as x.c0 | x.c1 | y.c0 | y.c1; montgomery = 1: Montgomery residues (what the *_setup entry points return),
 *       0: standard integers (what verification_key.json holds).  Rejected with G16_E_FORMAT: wrong length, a
 *       coordinate >= q, a point off its curve.
 * proofs: g16_proof as g16_prove writes them (standard form).  pubs: count * n_public * 32 bytes, standard LE
 *       (any 256-bit value: snarkjs reduces modulo r, so does the scalar multiplication here).
 * ok[i] = 1 accepted, 0 rejected (pairing product != 1, or a proof coordinate >= q, or a proof point off its curve).
 * No CPU path: G16_E_NOGPU without a HIP device. */
typedef struct g16_verifier g16_verifier;
int g16_verifier_create(const uint8_t* vkey, size_t vkey_len, uint32_t n_public, int montgomery, int device,
                        g16_verifier** out);
int g16_verify_batch(g16_verifier* v, const g16_proof* proofs, const uint8_t* pubs, size_t count, uint8_t* ok);
/* device time of the last batch, ms: [0] vk_x (public-signal MSMs), [1] Miller loops, [2] final exponentiations */
int g16_verifier_timings(const g16_verifier* v, float ms[3]);
void g16_verifier_destroy(g16_verifier* v);
/* Layer-test operator: `count` pairs (P in G1, Q in G2; six standard-form 32-byte words each: px py qx.c0 qx.c1 qy.c0
 * qy.c1, both on their curves, neither infinity) -> twelve standard-form words per pair: the pairing value the verifier
 * kernels compute, as the coefficients (c0, c1) of W^0..W^5 in the tower Fq12 = Fq2[W]/(W^6 - (9+u)). */
int g16_pairing_op(int device, const uint8_t* in, uint32_t count, uint8_t* out);
/* Layer tests of the point conversions of the challenge / response exchange (csrc/ptau_points.hip; the formats are
 * described at g16_ptau_export_challenge).  group 1 = G1, 2 = G2; n points; host buffers.  *first_bad (optional) = the
 * smallest index whose image is not a point, else -1 (the outputs are then not to be used); kernel_ms (optional) = the
 * device time of the kernels.  G16_PTAU_CHUNK / G16_PTAU_LANES size the chunks and the grid as in ptau_scale.hip.
 *   from_be:     uncompressed big-endian (64 / 128 bytes) -> the file form (affine little-endian Montgomery); bad: a
 *                coordinate >= q, a point off its curve, bit 0x80, bit 0x40 with anything else set;
 *   compress:    the file form -> x and the flags (32 / 64 bytes); first_bad is always -1;
 *   decompress:  the inverse, and -- out_be, optional -- the uncompressed big-endian image of every point; bad: x >= q,
 *                x^3 + b without a root, bit 0x40 with anything else set.
 * g16_fq_sqrt_batch: square roots of n raw field elements in standard little-endian form (ext 0 = Fq, 32 bytes; 1 = Fq2,
 * c0 | c1, 64 bytes; every word below q, else G16_E_ARG) by the decompression's routine: out[i] = a root of in[i] and
 * has_root[i] = 1, or zeros and 0.  It reaches the Fq2 cases a curve point cannot (c1 = 0, a non-residue c0). */
int g16_ptau_points_from_be(int group, const uint8_t* in, size_t n, int device, uint8_t* out, int64_t* first_bad, float* kernel_ms);
int g16_ptau_points_compress(int group, const uint8_t* in, size_t n, int device, uint8_t* out, int64_t* first_bad, float* kernel_ms);
int g16_ptau_points_decompress(int group, const uint8_t* in, size_t n, int device, uint8_t* out, uint8_t* out_be /* or NULL */,
                               int64_t* first_bad, float* kernel_ms);
int g16_fq_sqrt_batch(int ext, const uint8_t* in, size_t n, int device, uint8_t* out, uint8_t* has_root);

/* ---------------------------------------------------------------------------------------------------------------
 * PLONK prover on the device.  [EXT] snarkjs 0.4.12 plonk_prove.js `plonk.prove(zkey, wtns)` -- the
 * protocol whose setup the reference scripts (/root/reference/Makefile:30-33: `snarkjs plonk setup`, `zkey export
 * verificationkey`, `zkey export solidityverifier`).  zkey: a PLONK .zkey as `snarkjs plonk setup` writes it (protocol
 * id 2; the Lagrange section 13 is not read).  Errors carry snarkjs's texts: "zkey file is not plonk" (snarkjs's own
 * text says "groth16" there), "Invalid witness length. Circuit: N, witness: M, A", "Copy constraints does not match",
 * "T Polynomial is not divisible", "Polinomial does not divide".
 * blinding: nine 32-byte LE scalars b1..b9 below r (snarkjs: Fr.random() each), or NULL for the OS CSPRNG -- with the
 * same nine scalars the proof is reproducible byte for byte.
 * proof: points affine in standard form (x | y, infinity = zeros), evaluations as standard-form integers: the fields of
 * snarkjs's proof.json in its key order.  pub receives n_public * 32 bytes.  No CPU path (G16_E_NOGPU). */
typedef struct g16_plonk g16_plonk;
typedef struct g16_plonk_proof {
  uint8_t A[64], B[64], C[64], Z[64], T1[64], T2[64], T3[64];
  uint8_t eval_a[32], eval_b[32], eval_c[32], eval_s1[32], eval_s2[32], eval_zw[32], eval_r[32];
  uint8_t Wxi[64], Wxiw[64];
} g16_plonk_proof;
int g16_plonk_create(const uint8_t* zkey, size_t zkey_len, int device, g16_plonk** out);
int g16_plonk_prove(g16_plonk* p, const uint8_t* wtns, size_t wtns_len, const uint8_t* blinding /* 9 * 32 or NULL */,
                    g16_plonk_proof* out, uint8_t* pub);
/* info: nVars (with the addition signals), nPublic, domainSize, nAdditions, nConstraints, addition dependency levels */
int g16_plonk_get_info(const g16_plonk* p, uint32_t info[6]);
/* host wall time of the last proof, ms: [0] witness + round 1, [1] round 2, [2] round 3, [3] round 4, [4] round 5, [5] total */
int g16_plonk_timings(const g16_plonk* p, float ms[6]);
void g16_plonk_destroy(g16_plonk* p);
/* Test-only stand-in for `snarkjs plonk setup c.r1cs pot.ptau c.zkey` (/root/reference/Makefile:31) with a KNOWN tau
 * (derived from seed): iden3 .r1cs v1 in, snarkjs-layout PLONK .zkey out (g16_free).  R1CS -> gates as plonk_setup.js
 * does it; the selector / sigma transforms run on `device` (required), the N + 6 powers of tau through the fixed-base
 * kernel.  with_lagrange = 0 writes an EMPTY section 13 (a prover that derives the public-input polynomial by NTT does
 * not read it; snarkjs does). */
int g16_plonk_setup(const uint8_t* r1cs, size_t r1cs_len, uint64_t seed, int device, int with_lagrange, uint8_t** zkey,
                    size_t* zkey_len);
/* `snarkjs plonk setup c.r1cs pot.ptau c.zkey` itself (/root/reference/Makefile:31: powersOfTau28_hez_final_22.ptau):
 * the powers come from a .ptau v1 image ([EXT] snarkjs powersoftau_utils.js; sections 1-3 are read), the eight
 * selector / sigma commitments are MSMs over them on the device.  "circuit too big for this power of tau ceremony.
 * G > 2**P" when the gates do not fit. */
int g16_plonk_setup_ptau(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                         int with_lagrange, uint8_t** zkey, size_t* zkey_len);
/* the same from / to files (inputs mapped read-only): for hosts whose buffers end at 2 GB (Node.js) -- a 2^22 ceremony
 * file is 4.6 GB, the key it yields 5.8 GB without the Lagrange section */
int g16_plonk_setup_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device, int with_lagrange);

/* `snarkjs groth16 setup c.r1cs pot.ptau c_0000.zkey` (alias `zkey new`): a Groth16 .zkey from an iden3 .r1cs v1 and a
 * PREPARED .ptau v1 image (`powersoftau prepare phase2`; the Hermez _final_ files are prepared).  Sections 4-6 give
 * alpha1, beta1, beta2; the Lagrange sections 12-15 (blocks k of 2^k points from point 2^k - 1; the block count is
 * taken from each section's length) give every point section, as sums of the R1CS coefficients times the ceremony's
 * points on `device` (there is no CPU path: G16_E_NOGPU).  Only blocks L (13-15) and L + 1 (12) are uploaded, 2^L the
 * smallest domain with 2^L >= m + p + 1.  The key is a fresh _0000 key: gamma = delta = 1 and section 10 (the
 * circuit hash, csHash) is 64 zero bytes and no contributions -- the LEGACY form, kept because keys of this entry are
 * compared byte for byte; g16_zkey_new below writes the same key with the real csHash.  Correct, but NOT safe to deploy
 * until a phase-2 contribution changes delta (`zkey contribute`: g16_zkey_contribute below).
 * Every input is checked before the device is touched: the r1cs as g16_r1cs_setup reads it; "Powers of tau is not
 * prepared." (no section 12); "ptau: Invalid File format" (a section that is not whole blocks or has more than the
 * power allows); "circuit too big for this power of tau ceremony. M > 2**P" when block L or L + 1 is missing. */
int g16_groth16_setup_ptau(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                           uint8_t** zkey, size_t* zkey_len);
/* the same from / to files: the inputs are mapped read-only and the key is written in chunks (ceremony files are GBs) */
int g16_groth16_setup_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device);
/* `snarkjs zkey new c.r1cs pot.ptau c_0000.zkey` WITH the circuit hash: the key of g16_groth16_setup_ptau, byte for byte
 * in sections 1-9 and in section order, and section 10 = csHash (64) | u32 0.  snarkjs 0.4.12 zkey_new.js, as far as it
 * can be restated without the package:
 *   csHash = Blake2b-512( alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2
 *                         | u32be p+1 | IC | u32be N-1 | H | u32be n-p-1 | L | u32be n | A | u32be n | B1 | u32be n | B2 )
 * every point uncompressed big-endian standard form: the MPCParams image of the fresh key (g16_zkey_export_bellman
 * below) up to its csHash field.  H is taken from section 2 of the ceremony file, not from section 9 of the key:
 * H_k = P_(k+N) - P_k, k < N - 1, P_j = point j of section 2 (snarkjs hashHPoints), a batched affine subtraction on
 * `device` (csrc/zkey_cshash.hip); the other runs go through the conversions of the export; every chunk is hashed on the
 * calling thread as it comes down.  g16_zkey_export_bellman derives the same H from section 9 by its basis change, so
 * Blake2b-512 of an exported initial key's image up to csHash IS this hash: two device routes with no code in common.
 * cs_hash (optional) receives the 64 bytes.  With this hash a ceremony's transcripts are bound to the circuit and to the
 * phase-1 file: every contribution, beacon, export and import chains from and compares whatever section 10 holds.
 * NOT CLAIMED: that the value is the one snarkjs computes for the same inputs (the package is not at hand).
 * Checked before the device is touched: everything g16_groth16_setup_ptau checks, with its texts and first (the ptau
 * must be prepared; "circuit too big for this power of tau ceremony..."); a domain above 2^24: G16_E_ARG; section 2 of
 * the ptau present with at least 2N - 1 points, each with coordinates below q and on the curve, else "ptau: Invalid
 * File format".  No CPU path: G16_E_NOGPU. */
int g16_zkey_new(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device, uint8_t** zkey,
                 size_t* zkey_len, uint8_t cs_hash[64] /* or NULL */);
int g16_zkey_new_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device,
                       uint8_t cs_hash[64] /* or NULL */);
/* The hash g16_zkey_new stores, for an INITIAL key that is already there: out <- csHash of `zkey` over `ptau` (prepared
 * or not: only section 2 is read).  Defined for initial keys only: delta1 / delta2 other than the generators, or a
 * section 10 with records, is G16_E_ARG "zkey cs hash: not an initial key".  The 64 bytes section 10 already holds are
 * not read: this is how the owner of a legacy zero-hash key checks or upgrades it.  Checked before the device is
 * touched: the key as g16_zkey_contribute reads it; the ptau's container, header and curve with the texts of
 * g16_zkey_verify_from_init_ptau; a power below log2 N: G16_E_ARG "zkey new: the ptau is too small for this key"; section
 * 2 as above.  No CPU path: G16_E_NOGPU. */
int g16_zkey_cs_hash(const uint8_t* zkey, size_t zkey_len, const uint8_t* ptau, size_t ptau_len, int device, uint8_t out[64]);
int g16_zkey_cs_hash_files(const char* zkey_path, const char* ptau_path, int device, uint8_t out[64]);
/* `snarkjs powersoftau prepare phase2 in.ptau out.ptau` (alias `pt2`): the .ptau v1 image (g16_free) that holds
 * sections 1-7 of the input, byte for byte and in that order, then the sections 12-15 the setups above read, computed
 * on `device` (there is no CPU path: G16_E_NOGPU).  Section 12 comes from section 2, 13 / 14 / 15 from 3 / 4 / 5: block
 * k (2^k points from point 2^k - 1) is the inverse Fourier transform of size 2^k over group elements of the source's
 * first 2^k points, point j = (1 / 2^k) sum_i w_k^(-ij) P_i -- for a ceremony of trapdoor tau the Lagrange basis
 * [L_j(tau)] of the size-2^k domain.  Sections 13-15 run through block `power`; section 12 through block power + 1,
 * whose missing last input (section 2 holds 2^(power+1) - 1 points) is the point at infinity, as in snarkjs: that one
 * block is [L_j(tau) - w^j tau^(M-1) / M]G1, M = 2^(power+1), which Groth16's H basis (its odd points) cannot tell from
 * the Lagrange basis.  Sections 12-15 of an already prepared input are ignored and recomputed; other section ids are
 * not carried over; a missing section 7 is written as "no contributions".  Points keep the file's format (affine,
 * little-endian Montgomery, infinity = zero bytes); infinity inputs and outputs are handled.
 * Checked before the device is touched: "ptau: Invalid File format..." as above for the header, the section table and
 * the curve; sections 2-6 present with exactly the sizes the header's power implies, else "ptau: Invalid File format";
 * a power above 24: G16_E_ARG, the text names the limit. */
int g16_ptau_prepare(const uint8_t* ptau, size_t ptau_len, int device, uint8_t** out, size_t* out_len);
/* the same from / to files: the input is mapped read-only and the output written in chunks (a power-22 output is
 * several GB) */
int g16_ptau_prepare_files(const char* in_path, const char* out_path, int device);
/* TEST-ONLY.  g16_r1cs_setup with the caller's trapdoor td = tau | alpha | beta | gamma | delta (standard-form 32-byte
 * LE scalars below r; gamma, delta non-zero) instead of the seed stream; where its multiplications run follows
 * g16_setup_device.  A key anyone holding td can forge proofs for. */
int g16_r1cs_setup_trapdoor(const uint8_t* r1cs, size_t r1cs_len, const uint8_t td[5 * 32], int threads, uint8_t** zkey,
                            size_t* zkey_len, uint8_t** vkey, size_t* vkey_len);
/* TEST-ONLY.  A .ptau v1 image (g16_free) for a KNOWN tau | alpha | beta (standard-form LE scalars): sections 1-7 as
 * snarkjs lays them out (2 = [tau^i]G1, i < 2^(power+1) - 1; 3 = [tau^i]G2, 4 = [alpha tau^i]G1, 5 = [beta tau^i]G1,
 * i < 2^power; 6 = [beta]G2; 7 = no contributions) and, when `prepared`, sections 12-15 in the block layout above
 * (12 through block power + 1, 13-15 through block power).  power <= 24; device -1 = host threads. */
int g16_ptau_synth(uint32_t power, const uint8_t tau_alpha_beta[3 * 32], int prepared, int device, uint8_t** ptau,
                   size_t* ptau_len);

/* `snarkjs powersoftau new bn128 <power> pot_0000.ptau`: the .ptau v1 image (g16_free) of a ceremony nobody has
 * contributed to: sections 1-7, every point of sections 2-6 the generator of its group (2: 2^(power+1) - 1 points of
 * G1; 3: 2^power of G2; 4, 5: 2^power of G1; 6: one of G2), section 7 "no contributions" (four zero bytes).  Host only.
 * The bytes are g16_ptau_synth(power, 1 | 1 | 1, prepared = 0)'s.  A power above 24: G16_E_ARG, the text names the limit. */
int g16_ptau_new(uint32_t power, uint8_t** out, size_t* out_len);
int g16_ptau_new_file(uint32_t power, const char* path);
/* `snarkjs powersoftau contribute old.ptau new.ptau --name=.. -e=..`: one phase-1 contribution (g16_free).
 * secret = tau | alpha | beta | s_tau | s_alpha | s_beta, six standard-form 32-byte LE scalars in [1, r) (anything else:
 * G16_E_ARG), or NULL for the OS CSPRNG; the same inputs give the same bytes.  On `device` (there is no CPU path:
 * G16_E_NOGPU; csrc/ptau_scale.hip, every lane forms its own scalar): point i of sections 2 and 3 <- [tau^i] point i,
 * of section 4 <- [alpha tau^i], of section 5 <- [beta tau^i], section 6 <- [beta].  Section 1 byte for byte; section 7 =
 * the old records and the new one; sections 12-15 of a prepared input are DROPPED (a contribution invalidates them),
 * other section ids are not carried; the output order is 1..7.
 * Section 7, snarkjs's powersoftau_utils.js layout as far as it can be restated without the package: u32 n, then n
 * records, every point in the file's form (affine little-endian Montgomery):
 *   tauG1 (64) | tauG2 (128) | alphaG1 (64) | betaG1 (64) | betaG2 (128) |
 *   tau.g1_s | tau.g1_sx | alpha.g1_s | alpha.g1_sx | beta.g1_s | beta.g1_sx (64 each) |
 *   tau.g2_spx | alpha.g2_spx | beta.g2_spx (128 each) |
 *   partialHash (216) | nextChallenge (64) | u32 type = 0 | u32 paramsLen | params
 * params as in g16_zkey_contribute (byte 1, byte len, the name cut to 64 characters and 255 bytes, or nothing).  tauG1,
 * tauG2 = point 1 of the new sections 2, 3 (a power-0 file holds no point 1: there they are [tau] times the last
 * record's, or times the generators); alphaG1, betaG1, betaG2 = point 0 of the new sections 4, 5, 6.
 * Hashes.  challengeHash(state, prev) = Blake2b-512(prev | every point of sections 2, 3, 4, 5, 6 in that order,
 * uncompressed big-endian standard form as in g16_zkey_contribute).  The challenge a contribution answers is the last
 * record's nextChallenge, or -- no records -- challengeHash(the input file, Blake2b-512("")).  For key x (tau = 0,
 * alpha = 1, beta = 2): g1_s = [s_x]G1, g1_sx = [x]g1_s, g2_sp = g16_zkey_hash_to_g2(Blake2b-512(challenge | byte x |
 * g1_s | g1_sx uncompressed)), g2_spx = [x]g2_sp.  responseHash = Blake2b-512(challenge | the nine key points
 * uncompressed, in record order) = contribution_hash (optional), what the CLI prints as "Contribution Hash";
 * nextChallenge = challengeHash(new state, responseHash).
 * DEPARTURES from snarkjs: it hashes a response file of COMPRESSED points and stores a hasher snapshot in partialHash;
 * here the new points enter through nextChallenge only and partialHash is 216 zero bytes that nothing reads.  The layout
 * and the powers are snarkjs's; its `powersoftau verify` is NOT claimed to accept this transcript.  `powersoftau beacon`
 * is g16_ptau_beacon, the challenge / response file exchange g16_ptau_export_challenge and its neighbours, all below.
 * The G2 derivation is NOT cross-checked against snarkjs.
 * Checked before the device is touched: the container, curve and power texts of g16_ptau_prepare ("ptau: Invalid File
 * format...", a power above 24: G16_E_ARG naming the limit); sections 2-6 present with exactly the sizes the power
 * implies and a section 7 that parses (not shorter than its records say, no trailing bytes, every record point a valid
 * image), else "ptau: Invalid File format"; "ptau contribute: the secret scalars must be in [1, r)". */
int g16_ptau_contribute(const uint8_t* ptau, size_t ptau_len, const char* name /* or NULL */,
                        const uint8_t secret[192] /* or NULL = OS CSPRNG */, int device, uint8_t** out, size_t* out_len,
                        uint8_t contribution_hash[64]);
/* the same from / to files: the input is mapped read-only and the output written in chunks */
int g16_ptau_contribute_files(const char* in_path, const char* out_path, const char* name, const uint8_t secret[192],
                              int device, uint8_t contribution_hash[64]);
/* The secret scalars of a BEACON contribution: what closes a ceremony, a last contribution whose secret anyone can
 * recompute from a public random value and a delay function, so that the last contributor's secret is no longer what
 * the ceremony rests on.  beacon = the beacon hash, 1 to 255 bytes; num_iterations_exp = e, 10 <= e <= 63 (snarkjs's
 * range).  seed = SHA-256 applied 2^e times (the first application hashes the raw beacon bytes, every later one 32
 * bytes).  The scalars are draws of the ChaCha20 word stream of g16_zkey_hash_to_g2, keyed with the seed as eight
 * big-endian 32-bit words from counter 0: four 64-bit words each (low word first), masked to 254 bits, redrawn until
 * below r, a zero draw mapped to 1.  count = 6: tau, alpha, beta, s_tau, s_alpha, s_beta in the order of secret[192];
 * count = 2: d, s -- the first two of the same stream.  out <- count standard-form little-endian scalars of 32 bytes.
 * Like the `-e` rule (g16_ptau_secret_from_text) this derivation is THIS LIBRARY'S, not snarkjs's: ffjavascript's
 * fromRng is not available to restate, so a beacon record made by snarkjs does not pass the verifiers' beacon check
 * here, and one made here not snarkjs's.  Host only, one thread: the 2^e applications depend on each other, and the call
 * takes that long (e = 63 does not end).  G16_E_ARG, before any hashing: "beacon: the beacon hash must be 1 to 255
 * bytes", "beacon: numIterationsExp must be between 10 and 63", "beacon: count must be 2 or 6". */
int g16_beacon_scalars(const uint8_t* beacon, size_t beacon_len, uint32_t num_iterations_exp, int count, uint8_t* out);
/* `snarkjs powersoftau beacon old.ptau new.ptau <beaconHash(hex)> <numIterationsExp> --name=..`: g16_ptau_contribute with
 * secret = g16_beacon_scalars(beacon, e, 6), byte for byte and with the same contribution hash, except that the new
 * record has type = 1 and its params state the beacon, ids ascending as snarkjs's readers demand: the name's params if
 * any (byte 1, len, bytes), then byte 2, byte e, then byte 3, byte beacon_len, the beacon bytes.  type and params enter
 * no hash.  Every check, error and output rule of g16_ptau_contribute applies (texts led by "ptau beacon: "; no CPU path:
 * G16_E_NOGPU; sections 12-15 dropped; any power 0-24); after the file's checks come the argument errors of
 * g16_beacon_scalars, then the chain on the calling thread, and only then is the device touched. */
int g16_ptau_beacon(const uint8_t* ptau, size_t ptau_len, const char* name /* or NULL */, const uint8_t* beacon,
                    size_t beacon_len, uint32_t num_iterations_exp, int device, uint8_t** out, size_t* out_len,
                    uint8_t contribution_hash[64]);
int g16_ptau_beacon_files(const char* in_path, const char* out_path, const char* name, const uint8_t* beacon, size_t beacon_len,
                          uint32_t num_iterations_exp, int device, uint8_t contribution_hash[64]);
/* `snarkjs powersoftau verify pot.ptau`: is the file the generator file plus a chain of honest contributions (of THIS
 * library's transcript, see above)?  G16_OK with *ok = 1 / 0; for 0 g16_last_error() holds the reason, one fixed text
 * per check, each led by "ptau verify: ", in this order:
 *   1. "the first point of section 2 or 3 is not the generator";
 *   2. per record, from the generators on: "a contribution holds the point at infinity"; "a contribution's public key
 *      is not consistent" (e(g1_s, g2_spx) != e(g1_sx, g2_sp) for one of its three keys); "a contribution's tauG1 /
 *      alphaG1 / betaG1 does not continue the chain" (not the record before's by the ratio of its key); "a contribution's
 *      tauG2 does not match its tauG1" (e(tauG1, G2) != e(G1, tauG2)), "... betaG2 does not match its betaG1".  g2_sp is
 *      recomputed from the record's challenge: the generator file's for the first record, the nextChallenge of the
 *      record before for every other.  nextChallenge itself can be recomputed only where the state it hashes is at hand,
 *      that is for the last record (check 4); the first record's challenge is that of the generator file of this power.
 *      A record of type 1 (a beacon) must also BE its beacon's: its params are walked by snarkjs's rule (ids 1, 2, 3
 *      ascending, nothing else, nothing cut short); without both id 2 (e, in 10 .. 63) and id 3 (the beacon hash, not
 *      empty) "a beacon contribution does not state its beacon"; else g16_beacon_scalars is recomputed and every key
 *      must have g1_s = [s_x]G1 and g1_sx = [x]g1_s, else "a beacon contribution's key is not the beacon's" (g2_spx is
 *      tied to these by the consistency pairing).  Reported after the pairing checks of the records and instead of
 *      checks 3 to 5.  This costs 2^e hashes per beacon record on one host thread: a record that states a large e makes
 *      verification that slow.  A record of any other type is not touched by this;
 *   3. "the file's points are not the last contribution's" (point 1 of sections 2 and 3 -- power >= 1 --, point 0 of
 *      sections 4, 5, 6), or, without records, "a file without contributions is not the generator file";
 *   4. "the last contribution's challenge hash does not match the file" (skipped without records);
 *   5. the powers, with fresh random rho_i (ChaCha20 keyed from the OS CSPRNG): S1 = sum rho_i P_i, S2 = sum rho_i
 *      P_(i+1), e(S1, tauG2) != e(S2, G2): "section 2 is not the powers of tau", "section 4 is not alpha times the powers
 *      of tau", "section 5 is not beta times the powers of tau"; the G2 sums of section 3 against (G1, tauG1): "section 3
 *      is not the powers of tau"; "the combination of section N is the point at infinity";
 *   6. a prepared file: "the prepared sections 12 to 15 are not all present"; "the prepared sections are not the
 *      transform of sections 2 to 5" (g16_ptau_prepare is run and compared byte for byte).
 * A malformed file is G16_E_FORMAT, not a verdict: the container, the sizes, section 7, and a coordinate >= q or a point
 * off its curve anywhere in sections 2-6.  A power above 24: G16_E_ARG.  The sums are MSMs (g16_g1_multiexp /
 * g16_g2_multiexp), the pairings ONE g16_pairing_op call on `device` (G16_E_NOGPU). */
int g16_ptau_verify(const uint8_t* ptau, size_t ptau_len, int device, int* ok);
int g16_ptau_verify_file(const char* path, int device, int* ok);
/* The challenge / response file exchange of phase 1: how somebody who does not hold the .ptau contributes.  The
 * coordinator exports a challenge, the contributor answers it with a response, the coordinator imports the response.
 * File formats, snarkjs 0.4.12's (powersoftau_export_challenge.js, powersoftau_challenge_contribute.js,
 * powersoftau_import.js) as far as they can be restated without ffjavascript, which is not available here; n = 2^power:
 *   challenge file, 384 n + 128 bytes: prev (64) | the 2n - 1 points of section 2, the n of 3, of 4, of 5, the one of 6,
 *     each uncompressed big-endian standard form (G1: x | y; G2: x.c1 | x.c0 | y.c1 | y.c0; infinity: zeros with bit 0x40
 *     of byte 0).  prev = Blake2b-512("") for a file without records, else the last record's responseHash (not stored:
 *     recomputed from the record's key points and the challenge it answered -- the nextChallenge of the record before,
 *     or the generator file's challenge).  Blake2b-512(challenge file) = challengeHash(state, prev) of
 *     g16_ptau_contribute: the challenge the next contribution answers.
 *   response file, 192 n + 864 bytes: that challenge hash (64) | the same five runs of points COMPRESSED | the nine key
 *     points uncompressed in record order (768: tau.g1_s, tau.g1_sx, alpha.g1_s, alpha.g1_sx, beta.g1_s, beta.g1_sx,
 *     tau.g2_spx, alpha.g2_spx, beta.g2_spx).
 *   compressed point: the big-endian x alone (G1: 32 bytes; G2: c1 | c0, 64); infinity: zeros with bit 0x40 of byte 0;
 *     bit 0x80 of byte 0 set when y is "negative": in Fq y > (q - 1) / 2, in Fq2 that of c1, or of c0 when c1 = 0 (the
 *     rule g16_zkey_hash_to_g2 uses).  q < 2^254 leaves both bits free.
 * For the same old file, name and secret, import_response(old, challenge_contribute(export_challenge(old), secret),
 * name) is g16_ptau_contribute(old, name, secret) byte for byte, with the same hash.
 * DEPARTURES from snarkjs: the hash printed and returned by challenge contribute and import response is THIS library's
 * responseHash = Blake2b-512(challenge | the nine key points), i.e. over the response's first 64 and last 768 bytes, not
 * snarkjs's Blake2b-512 of the whole response file; partialHash stays zero.  An imported record has type 0.
 *
 * `snarkjs powersoftau export challenge pot.ptau challenge` (alias `ptec`): the challenge file (g16_free) and --
 * optionally -- its Blake2b-512.  Host only (never G16_E_NOGPU); any power 0-24; the checks of g16_ptau_contribute on the
 * input.  With records the hash must be the last record's nextChallenge, else G16_E_FORMAT "ptau export challenge: the
 * file's points are not the last contribution's challenge". */
int g16_ptau_export_challenge(const uint8_t* ptau, size_t ptau_len, uint8_t** out, size_t* out_len, uint8_t challenge_hash[64]);
int g16_ptau_export_challenge_files(const char* ptau_path, const char* challenge_path, uint8_t challenge_hash[64]);
/* `snarkjs powersoftau challenge contribute bn128 challenge response -e=..` (alias `ptcc`): the response file (g16_free)
 * to a challenge file; secret as in g16_ptau_contribute.  The power comes from the size: (size - 128) / 384 must be a
 * power of two up to 2^24, else G16_E_FORMAT "ptau challenge: Invalid File format"; a power-0 challenge (512 bytes) is
 * G16_E_ARG, the text says so: its response would hold no point 1 for the import to take tauG1 from.  On `device` (no
 * CPU path: G16_E_NOGPU; csrc/ptau_points.hip): every point from big-endian to the file form -- a coordinate >= q, a
 * point off its curve, a set 0x80 bit or a 0x40 bit with anything else set is G16_E_FORMAT "ptau challenge contribute:
 * point I of section S is not a point of the curve" for the first such point of the first such section --, scaled as
 * g16_ptau_contribute scales the sections, compressed.  challenge = Blake2b-512(the input file); the keys are formed from
 * it as in g16_ptau_contribute; contribution_hash (optional) = responseHash. */
int g16_ptau_challenge_contribute(const uint8_t* challenge, size_t challenge_len, const uint8_t secret[192] /* or NULL */,
                                  int device, uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]);
int g16_ptau_challenge_contribute_files(const char* challenge_path, const char* response_path, const uint8_t secret[192],
                                        int device, uint8_t contribution_hash[64]);
/* `snarkjs powersoftau import response old.ptau response new.ptau --name=..` (alias `ptir`): old.ptau with the
 * response's points and one record more (g16_free): sections 1..7, sections 12-15 of a prepared input dropped.
 * Checked before the device is touched: everything g16_ptau_contribute checks on old.ptau; power >= 1 (power 0:
 * G16_E_ARG); the response's size for that power (G16_E_FORMAT "ptau import response: Invalid File format"); its first
 * 64 bytes = old.ptau's challenge (the last nextChallenge, or the first challenge computed on the host) -- otherwise the
 * VERDICT "ptau import response: the response does not answer this file's challenge"; the nine key points valid images
 * (G16_E_FORMAT "ptau import response: a key point is not a valid image").  On `device` (G16_E_NOGPU) every point is
 * decompressed, y = sqrt(x^3 + b) with the sign the flag asks for: a 0x40 bit with any other bit set, x >= q or no root
 * is G16_E_FORMAT "ptau import response: point I of section S is not a point of the curve"; the big-endian images for
 * nextChallenge come from the same pass.  The record is built as g16_ptau_contribute builds it (tauG1 / tauG2 = point 1
 * of the new sections 2 / 3, alphaG1 / betaG1 / betaG2 = point 0 of 4 / 5 / 6, the key points from the response,
 * partialHash zero, nextChallenge = challengeHash(new state, responseHash), type 0, params from the name).  Before
 * anything is written, check 2 of g16_ptau_verify is applied to the new record against the record before it (or the
 * generators), its pairings in ONE g16_pairing_op call.  A failing check is a verdict as in g16_ptau_verify: G16_OK with
 * *ok = 0, *out = NULL, nothing written, g16_last_error() = the text of that check led by "ptau import response: ".
 * *ok = 1: the output is there and contribution_hash (optional) = responseHash.  The powers themselves (check 5) are
 * left to g16_ptau_verify, as in snarkjs. */
int g16_ptau_import_response(const uint8_t* ptau, size_t ptau_len, const uint8_t* response, size_t response_len,
                             const char* name /* or NULL */, int device, uint8_t** out, size_t* out_len,
                             uint8_t contribution_hash[64], int* ok);
int g16_ptau_import_response_files(const char* ptau_path, const char* response_path, const char* out_path, const char* name,
                                   int device, uint8_t contribution_hash[64], int* ok);
/* The CLI's rule for `-e=<text>` (NOT snarkjs's): h_j = Blake2b-512(text | byte j), j = 0, 1, 2; the first 32 bytes of
 * h_j (little-endian, reduced mod r, zero mapped to 1) are key j (tau, alpha, beta), the last 32 bytes s_j.  The scalars
 * of a beacon (g16_beacon_scalars) are this library's rule in the same way, and not snarkjs's either. */
int g16_ptau_secret_from_text(const char* text, uint8_t secret[192]);

/* `snarkjs zkey contribute old.zkey new.zkey --name=.. -e=..`: one phase-2 contribution to a Groth16 .zkey (g16_free).
 * secret = d | s, two standard-form 32-byte LE scalars in [1, r) (anything else: G16_E_ARG), or NULL for the OS CSPRNG;
 * like g16_prove's explicit r, s the same inputs give the same bytes.  g1_s = [s]G1, g1_sx = [d]g1_s; transcript =
 * Blake2b-512(csHash | hashPubKey of every earlier record | g1_s | g1_sx); g2_sp = the transcript's point on G2
 * (g16_zkey_hash_to_g2), g2_spx = [d]g2_sp; delta1, delta2 of the header <- [d]delta; sections 8 and 9 <- [1/d] section,
 * on `device` (there is no CPU path: G16_E_NOGPU); sections 1, 3-7 byte for byte; section 10 = the old csHash, the old
 * records and the new one (deltaAfter | g1_s | g1_sx | g2_spx | transcript | u32 type = 0 | u32 paramsLen | params;
 * params = byte 1, byte len, the name's UTF-8 bytes cut to 64 characters and 255 bytes, or nothing without a name).
 * Section order and ids as in the input.  contribution_hash (optional) = Blake2b-512(hashPubKey(new record)), what
 * snarkjs prints as "Contribution Hash".  hashPubKey feeds deltaAfter, g1_s, g1_sx, g2_spx in uncompressed big-endian
 * standard form (G1: x | y; G2: x.c1 | x.c0 | y.c1 | y.c0; infinity: zeros with bit 0x40 of byte 0), then the transcript.
 * Every input is checked before the device is touched: "zkey file is not groth16", "zkey: Invalid File format" (the
 * container, the header, section sizes, a section 10 shorter than its records say or with trailing bytes, a point
 * coordinate >= q or a point off its curve).  A beacon record (type 1) in the input is carried and hashed like any other,
 * its params untouched.  `zkey beacon` is g16_zkey_beacon below.
 * The chain is hashed from whatever csHash section 10 holds: the circuit hash of g16_zkey_new above, or the 64 zero
 * bytes of g16_groth16_setup_ptau's legacy keys (then nothing in the transcripts binds them to the circuit).  That the
 * csHash built here equals snarkjs's own value is NOT claimed, so neither is `snarkjs zkey verify` of these keys: the
 * file layout and the proofs are snarkjs's.  The G2 derivation is NOT cross-checked against snarkjs. */
int g16_zkey_contribute(const uint8_t* zkey, size_t zkey_len, const char* name /* or NULL */,
                        const uint8_t secret[64] /* d | s, or NULL = OS CSPRNG */, int device,
                        uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]);
/* the same from / to files: the input is mapped read-only and the key is written in chunks */
int g16_zkey_contribute_files(const char* in_path, const char* out_path, const char* name,
                              const uint8_t secret[64], int device, uint8_t contribution_hash[64]);
/* `snarkjs zkey beacon old.zkey new.zkey <beaconHash(hex)> <numIterationsExp> --name=..`: g16_zkey_contribute with secret =
 * g16_beacon_scalars(beacon, e, 2) = d | s, byte for byte and with the same contribution hash, except that the new
 * record has type = 1 and params = the name's if any | byte 2, byte e | byte 3, byte beacon_len, the beacon bytes (as in
 * g16_ptau_beacon; type and params enter no hash).  Every check, error and output rule of g16_zkey_contribute applies
 * (no CPU path: G16_E_NOGPU); after the key's checks come the argument errors of g16_beacon_scalars, then the chain on
 * the calling thread, and only then is the device touched.  The derivation is this library's, not snarkjs's. */
int g16_zkey_beacon(const uint8_t* zkey, size_t zkey_len, const char* name /* or NULL */, const uint8_t* beacon,
                    size_t beacon_len, uint32_t num_iterations_exp, int device, uint8_t** out, size_t* out_len,
                    uint8_t contribution_hash[64]);
int g16_zkey_beacon_files(const char* in_path, const char* out_path, const char* name, const uint8_t* beacon, size_t beacon_len,
                          uint32_t num_iterations_exp, int device, uint8_t contribution_hash[64]);
/* `snarkjs zkey verify frominit init.zkey pot.ptau circuit.zkey` without the ptau leg (section 9 is not checked against
 * a ceremony file; g16_zkey_verify_from_init_ptau below is the route with it): is `zkey` the key `init` plus a chain of honest contributions?  G16_OK with *ok = 1 / 0; for 0
 * g16_last_error() holds the reason, one fixed text per check, each led by "zkey verify: ":
 *   "the header differs from the initial key's (sizes, alpha, beta or gamma)", "sections 3 to 7 differ from the initial
 *   key's", "the circuit hash differs from the initial key's", "the contributions do not begin with the initial key's",
 *   "section 8 or 9 has not the initial key's length", "a contribution's transcript hash does not match", "a
 *   contribution holds the point at infinity", "a contribution's public key is not consistent" (e(g1_s, g2_spx) !=
 *   e(g1_sx, g2_sp)), "a contribution's delta does not continue the chain" (e(cur, g2_spx) != e(deltaAfter, g2_sp)),
 *   "delta1 of the header is not the last contribution's", "delta2 does not match delta1", "sections 8 and 9 are not the
 *   initial key's scaled by 1 / delta" (S = sum rho_i new_i, T = sum rho_i init_i over both sections together, e(S,
 *   delta2) != e(T, delta2 of init); section 8: fresh random rho_i, and its infinity points must be the initial key's;
 *   section 9: rho_i = (1 / N) sum_k u_k w^((2i+1) k) with fresh random u_0 .. u_(N-2) and u_(N-1) = 0, formed on the
 *   device as in g16_zkey_h_scalars -- the combinations of quotients of degree <= N - 2, which are what a prover forms
 *   and what `zkey import bellman` preserves, so an imported key passes; a tampered point still moves the sum), "the
 *   combination of sections 8 and 9 is the point at infinity".
 * Every further record of type 1 (a beacon) must also BE its beacon's, as in check 2 of g16_ptau_verify: "a beacon
 * contribution does not state its beacon" (params without ids 2 and 3 by snarkjs's sorted-id rule, or e outside 10 ..
 * 63), "a beacon contribution's key is not the beacon's" (g1_s != [s]G1 or g1_sx != [d]g1_s for d, s =
 * g16_beacon_scalars); reported after every pairing check; 2^e hashes per beacon record on one host thread.
 * A key with no records beyond init's (init against itself) is accepted.  A malformed file is G16_E_FORMAT, not a
 * verdict.  The two sums are MSMs and the pairings Miller loops + final exponentiations on `device` (G16_E_NOGPU). */
int g16_zkey_verify_from_init(const uint8_t* init, size_t init_len, const uint8_t* zkey, size_t zkey_len,
                              int device, int* ok);
int g16_zkey_verify_from_init_files(const char* init_path, const char* zkey_path, int device, int* ok);
/* `snarkjs zkey verify frominit init.zkey pot.ptau circuit.zkey` WITH the ptau leg (snarkjs sectionHasSameRatioH): every
 * check above, then section 9 of `zkey` against the ceremony file.  N = the key's domain, P_j = point j of the ptau's
 * section 2, H_i = point i of the key's section 9, w = the primitive 2N-th root.  Drawn: u_0 .. u_(N-2) in Fr (ChaCha20
 * keyed from the OS CSPRNG), u_(N-1) = 0.  rho_i = 2 sum_k u_k w^((2i+1) k), S = sum rho_i H_i, T = sum_(k <= N-2) u_k
 * (P_k - P_(k+N)); accepted iff e(S, delta2 of zkey) = e(T, G2 generator), or S and T are both the point at infinity (the
 * tau = 1 ceremony of g16_ptau_new: every P_j is the generator, so T is infinity, and the H points are infinity or sum to
 * it); exactly one of them at infinity is a rejection.  The
 * combination lies on the hyperplane sum rho_i w^(2i+1) = 0 -- the one the prover's scalars lie on -- where the two
 * forms of the H basis agree: the full Lagrange block, and the block `prepare phase2` computes from the 2N - 1 points
 * section 2 holds at N = 2^power.  The device forms rho / 2N (g16_zkey_h_scalars) and the host multiplies S by 2N.
 * The ptau may be prepared or not: ONLY section 2 is read (its first 2N - 1 points).  The leg ties the key to those
 * points; whether the file is a sound ceremony is g16_ptau_verify's question.
 * Checked before the device is touched, after the two keys: the ptau's container, header and curve ("ptau: Invalid
 * File format (bn128 powers of tau expected)" / "ptau: Invalid File format", G16_E_FORMAT); a power below log2 N is the
 * verdict "zkey verify: the ptau is too small for this key"; a section 2 with fewer than 2N - 1 points, a coordinate
 * >= q or a point off the curve among them is "ptau: Invalid File format".  The leg's verdict, after the checks above:
 * "zkey verify: section 9 is not the ceremony's H basis scaled by 1 / delta".  One NTT of size N and two MSMs (N and
 * 2N - 1 points, the ptau's read where they lie) on `device`; its pair joins the one pairing call. */
int g16_zkey_verify_from_init_ptau(const uint8_t* init, size_t init_len, const uint8_t* ptau, size_t ptau_len,
                                   const uint8_t* zkey, size_t zkey_len, int device, int* ok);
int g16_zkey_verify_from_init_ptau_files(const char* init_path, const char* ptau_path, const char* zkey_path, int device,
                                         int* ok);
/* `snarkjs zkey verify circuit.r1cs pot.ptau circuit.zkey`: g16_groth16_setup_ptau(r1cs, ptau) in memory (its errors and
 * texts; the ptau must be prepared; no temporary file), then g16_zkey_verify_from_init_ptau against that key.  Which
 * csHash the in-memory initial key gets follows the key under test: 64 zero bytes there -- the legacy initial key, as
 * before; anything else -- the real csHash of g16_zkey_new (one g16_zkey_cs_hash more on `device`).  Every input that
 * was accepted or rejected before gets the same verdict and text; only keys that carry the true hash change, from
 * rejected ("the circuit hash differs from the initial key's") to accepted.  g16_zkey_verify_from_init(_ptau) compare
 * the two section 10s as they are. */
int g16_zkey_verify_r1cs(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, const uint8_t* zkey,
                         size_t zkey_len, int device, int* ok);
int g16_zkey_verify_r1cs_files(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device, int* ok);
/* Layer operator of the ptau leg (beside g16_fr_fft): both scalar vectors as the device forms them from one upload of u.
 * u = N = 2^log_n standard-form LE scalars below r (not checked) with u[N-1] = 0 (else G16_E_ARG); log_n in [1, 27].
 *   rho_out[i] = (1 / N) sum_k u[k] w^((2i+1) k)   (N x 32 bytes: the check's rho_i / 2N -- the NTT's coset table carries
 *                                                   the 1 / N, the host multiplies the point S by 2N instead)
 *   t_out      = u[0..N-2] | 0 | -u[0..N-2] mod r  ((2N - 1) x 32 bytes)
 * so that 2N sum rho_out[i] H_i = sum t_out[j] P_j.  Standard form out. */
int g16_zkey_h_scalars(int device, const uint8_t* u, uint32_t log_n, uint8_t* rho_out, uint8_t* t_out);
/* The MPCParams file exchange of phase 2: how somebody who does not hold the .zkey contributes (the twin of the
 * challenge / response exchange of phase 1).  File format, snarkjs 0.4.12's zkey_export_bellman.js as far as it can be
 * restated without the package; every G1 is 64 bytes (x | y), every G2 128 bytes (x.c1 | x.c0 | y.c1 | y.c0), big-endian
 * standard form, infinity = byte 0 = 0x40 and the rest zero; counts are u32 big-endian; n = nVars, p = nPublic, N = the
 * domain:
 *   alpha1 | beta1 | beta2 | gamma2 | delta1 | delta2
 *   u32 p+1 | IC (section 3)    u32 N-1 | H    u32 n-p-1 | L (section 8)
 *   u32 n | A (section 5)       u32 n | B1 (section 6)    u32 n | B2 (section 7, G2)
 *   csHash (64) | u32 c | c x ( deltaAfter | delta.g1_s | delta.g1_sx | delta.g2_spx (G2) | transcript (64) )
 * H is the MONOMIAL basis H_k = [tau^k (tau^N - 1) / delta] G, k < N - 1; section 9 of a key is the odd-coset Lagrange
 * basis S9[i] = [L^{2N}_{2i+1}(tau) / delta] G.  With w the primitive 2N-th root of unity, T[k] = [-2 w^k] sum_i w^(2ik)
 * S9[i] = H_k for every k < N (T[N-1] is not infinity); the file holds T[0 .. N-2].  The import puts infinity at k = N - 1,
 * multiplies point k by -(1/2) w^(-k) and applies the inverse transform with its 1 / N.  So import(export(key)) is the
 * PROJECTION of section 9 onto the quotients of degree <= N - 2, not the identity: sum e_i S9[i] is unchanged for every
 * such quotient (every proof of a satisfying witness), the bytes of section 9 generally change, and the projection is
 * idempotent.  g16_zkey_verify_from_init accepts such keys (its section-9 combination lies on the same subspace).
 * The transform runs on `device` (csrc/zkey_bellman.hip: L N/2 + N scalar products at N = 2^L; no CPU path: G16_E_NOGPU),
 * as do the conversions between the file form and the big-endian images (csrc/ptau_points.hip).  Domains up to 2^24.
 * NOT CLAIMED: an exchange with a snarkjs or bellman contributor.  The files are restated from snarkjs's description
 * without the package at hand; csHash is carried as section 10 holds it (g16_zkey_new's circuit hash, or the 64 zero
 * bytes of a legacy _0000 key), and its agreement with snarkjs's own value is not claimed either.
 *
 * `snarkjs zkey export bellman circuit.zkey circuit.mpcparams` (alias `zkeb`): the MPCParams image of a Groth16 key
 * (g16_free).  The checks of g16_zkey_contribute on the input, then the device.  A record's type and params are not
 * carried: the format has no room for them. */
int g16_zkey_export_bellman(const uint8_t* zkey, size_t zkey_len, int device, uint8_t** out, size_t* out_len);
int g16_zkey_export_bellman_files(const char* zkey_path, const char* mpcparams_path, int device);
/* `snarkjs zkey bellman contribute bn128 challenge response -e=..` (alias `zkbc`): the response (g16_free) to an MPCParams
 * file.  secret = d | s as in g16_zkey_contribute (NULL: OS CSPRNG).  Everything but delta1, delta2, H and L is copied;
 * delta <- d delta; H and L: from big-endian (every point checked: on its curve), times 1 / d, back to big-endian, on
 * `device`; one record more, formed exactly as g16_zkey_contribute forms it (the transcript over csHash, every earlier
 * record as the file holds it -- a record IS its hashPubKey feed --, g1_s and g1_sx), so for the same (d, s)
 * contribution_hash (optional) and the record equal those of g16_zkey_contribute on the key the file was exported from.
 * Checked before the device is touched: the length the file's own counts ask for, every flag (a clean 0x40 or none) and
 * every coordinate below q, delta1 and delta2 on their curves and not infinity -- G16_E_FORMAT "mpcparams: Invalid File
 * format", as is a point of H or L off its curve. */
int g16_zkey_bellman_contribute(const uint8_t* challenge, size_t challenge_len, const uint8_t secret[64] /* d | s, or NULL */,
                                int device, uint8_t** out, size_t* out_len, uint8_t contribution_hash[64]);
int g16_zkey_bellman_contribute_files(const char* challenge_path, const char* response_path, const uint8_t secret[64],
                                      int device, uint8_t contribution_hash[64]);
/* `snarkjs zkey import bellman old.zkey response new.zkey --name=..` (alias `zkib`): the new key (g16_free) with the old
 * key's sections in the old key's order.  From the old key: sections 1, 3-7 and the header up to delta1; from the file:
 * delta1, delta2, section 8 (from big-endian), section 9 (the inverse transform, see above); section 10 = the old
 * records as they are, then the file's new ones (there may be several) with type 0 and params from the name each.
 * G16_E_FORMAT "mpcparams: Invalid File format": a length that is not what the file's counts ask for, a bad flag, a
 * coordinate >= q, a point off its curve.  Refused as a VERDICT -- G16_OK with *ok = 0, *out = NULL, nothing written,
 * g16_last_error() = one fixed text per check, each led by "zkey import bellman: ":
 *   "a count is not the key's", "alpha, beta, gamma, IC, A, B1 or B2 differ from the key's", "the circuit hash differs
 *   from the key's", "the response holds no new contribution", "the contributions do not begin with the key's", "delta1
 *   or delta2 is the point at infinity".
 * Counts, alpha / beta / gamma, csHash, the records and the infinity flags are checked on the host before the device is
 * touched; IC, A, B1 and B2 are converted and compared on `device` (G16_E_NOGPU).  The import does not judge the
 * contribution itself: that is g16_zkey_verify_from_init's job, as in snarkjs. */
int g16_zkey_import_bellman(const uint8_t* zkey, size_t zkey_len, const uint8_t* response, size_t response_len,
                            const char* name /* or NULL */, int device, uint8_t** out, size_t* out_len, int* ok);
int g16_zkey_import_bellman_files(const char* zkey_path, const char* response_path, const char* out_path, const char* name,
                                  int device, int* ok);
/* TEST-ONLY layer operator of the exchange: the basis change alone.  points = N = 2^log_n affine LE Montgomery G1 points
 * (zero bytes = infinity; not checked), out as many; log_n in [0, 24].  inverse = 0: out[k] = [-2 w^k] sum_i w^(2ik)
 * points[i], ALL N values (T[N-1] included); inverse != 0: out[i] = (1 / N) sum_k w^(-2ik) [-(1/2) w^(-k)] points[k]. */
int g16_zkey_h_basis(int device, const uint8_t* points, uint32_t log_n, int inverse, uint8_t* out);
/* Layer operators of the two routes above, host only.  Blake2b-512 (RFC 7693, unkeyed); the transcript's point on G2
 * (ChaCha20 keyed with the first 32 bytes, x drawn as the Montgomery image, cofactor 2q - r; affine LE Montgomery). */
int g16_blake2b512(const uint8_t* data, size_t len, uint8_t out[64]);
int g16_zkey_hash_to_g2(const uint8_t transcript[64], uint8_t out[128] /* affine LE Montgomery */);
/* TEST-ONLY layer entries of g16_zkey_new's circuit hash.
 * The difference kernel alone: points = 2N - 1 affine LE Montgomery G1 points, N = 2^log_n (zero bytes = infinity; not
 * checked); out = (N - 1) x 64 bytes, out[k] = the uncompressed big-endian image of points[k + N] - points[k] (infinity =
 * 0x40 and zeros).  log_n in [0, 24]; log_n = 0 writes nothing and returns G16_OK.  G16_CSHASH_CHUNK / G16_CSHASH_LANES
 * set the chunk (points) and the grid (threads) of the run.
 * The streaming hasher (host only): Blake2b-512 of data fed in the parts the ascending offsets cuts[0 .. n_cuts) split
 * it into (equal offsets, 0 and len give empty parts); G16_E_ARG for offsets that descend or pass len. */
int g16_zkey_h_monomial(int device, const uint8_t* points, uint32_t log_n, uint8_t* out);
int g16_blake2b512_parts(const uint8_t* data, size_t len, const size_t* cuts, size_t n_cuts, uint8_t out[64]);

/* PLONK batch verifier on the device: [EXT] snarkjs 0.4.12 plonk_verify.js `plonk.verify(vk, publicSignals, proof)` for
 * many proofs against one key, one verdict per proof (transcript and scalar arithmetic on host threads, the twenty
 * scalar multiplications, two Miller loops and the final exponentiation of every proof on the device).
 * vkey (712 bytes, what verification_key.json holds, standard-form little-endian): power u32 | nPublic u32 | k1 (32) |
 * k2 (32) | Qm Ql Qr Qo Qc S1 S2 S3 (64 each: x | y) | X_2 (128: x.c0 | x.c1 | y.c0 | y.c1).
 * proofs: g16_plonk_proof as g16_plonk_prove writes them; pubs: count * nPublic * 32 bytes.  ok[i] = 1 / 0. */
typedef struct g16_plonk_verifier g16_plonk_verifier;
int g16_plonk_verifier_create(const uint8_t* vkey, size_t vkey_len, int device, g16_plonk_verifier** out);
int g16_plonk_verify_batch(g16_plonk_verifier* v, const g16_plonk_proof* proofs, const uint8_t* pubs, size_t count, uint8_t* ok);
void g16_plonk_verifier_destroy(g16_plonk_verifier* v);

/* `snarkjs wtns check <circuit.r1cs> <witness.wtns>` of later snarkjs releases (the pinned 0.4.12 has none, so nothing here
 * is compared with snarkjs; the oracle is big-integer arithmetic over the R1CS): does the witness w satisfy
 * (A_i.w)(B_i.w) = C_i.w in Fr for every constraint row i, and if not, where does it break?  bn128 only.
 * One checker = one .r1cs (iden3 v1, what g16_r1cs_setup reads; here a file with 0 constraints is accepted and every
 * witness of the right length passes), its three matrices resident on `device` (csrc/wtns_check.hip: one launch forms the
 * three sparse row sums of every row and writes only the verdict), or device = -1: host threads (at most 16), the route
 * that needs no GPU.  A device >= 0 without one: G16_E_NOGPU.  Not thread-safe: one call at a time per checker.
 * AN UNSATISFIED WITNESS IS A VERDICT, NOT AN ERROR: G16_OK, constraint = the lowest failing row, n_failed = how many rows
 * fail, a, b, c = the standard-form little-endian values A.w, B.w, C.w of that row, and g16_last_error() =
 * "wtns check: constraint I is not satisfied (N in all)" (the convention of g16_ptau_verify).  Every failing row a device
 * run reports is recomputed on the host, which fills a, b, c; should the host find that row satisfied the call returns
 * G16_E_STATE and says so: a device verdict is never reported unconfirmed.
 * A MALFORMED INPUT IS AN ERROR (G16_E_FORMAT), checked before the device is touched: for the .r1cs the texts of
 * g16_r1cs_setup ("r1cs: ..."); for the witness those of g16_prove -- "wtns: Invalid File format", "Version not
 * supported", "wtns: Missing section N", "Curve of the witness does not match the curve of the proving key", "Invalid
 * witness length. Circuit: X, witness: Y", "wtns: signal K is not reduced modulo the scalar field" -- and "wtns check:
 * signal 0 is not 1".
 * g16_wtns_check_batch: `count` witnesses of one circuit, one verdict each.  A malformed witness fails the whole call, its
 * text led by "witness K: " (the lowest such K); with unsatisfied witnesses g16_last_error() is the verdict text of the
 * first of them, led the same way.  On the device the batch runs in chunks of several witnesses per launch; a witness
 * takes 72 bytes per wire there (its 32-byte words and their 40-byte Montgomery images), a chunk as many witnesses as
 * 256 MB hold, at least one and at most 1024 -- the device memory of a checker does not grow with `count`.
 * G16_WTNS_CHECK_CHUNK=<witnesses> (read at create) overrides the chunk size.
 * g16_wtns_check_files: both files mapped read-only, a checker made for the one call.
 * g16_r1cs_checker_timings: device time of the last call's uploads and of its kernels, all chunks (zero on the host route). */
typedef struct g16_r1cs_checker g16_r1cs_checker;
typedef struct {
  int64_t constraint;           /* -1: every constraint holds */
  uint32_t n_failed;
  uint8_t a[32], b[32], c[32];  /* standard-form LE values of row `constraint`; zero when it is -1 */
} g16_wtns_verdict;
int g16_r1cs_checker_create(const uint8_t* r1cs, size_t len, int device /* -1 = host threads */, g16_r1cs_checker** out);
int g16_wtns_check(g16_r1cs_checker* k, const uint8_t* wtns, size_t len, g16_wtns_verdict* out);
int g16_wtns_check_batch(g16_r1cs_checker* k, const uint8_t* const* wtns, const size_t* lens, size_t count,
                         g16_wtns_verdict* out);
int g16_wtns_check_files(const char* r1cs_path, const char* wtns_path, int device, g16_wtns_verdict* out);
int g16_r1cs_checker_timings(const g16_r1cs_checker* k, float ms[2]);
void g16_r1cs_checker_destroy(g16_r1cs_checker* k);

/* ---- wtns calculate / groth16 fullprove: the witness computed from a recorded PROGRAM (csrc/witness_program.h) -------------
 * A witness program is a tape of how every wire of a natively built circuit follows from earlier wires -- six kinds of op
 * (INPUT, QUAD, BITS, INV0, ISZ, CHECK) sorted by dependency level -- recorded once by the native builders, independent
 * of any input; it takes the place of circom's .wasm calculator for these circuits and runs no .wasm.
 * g16_nzcp_witness_program: the program of NZCPPubIdentity(params) (the parameter checks of g16_nzcp_circuit_setup); its
 * inputs are toBeSigned (8 * MaxToBeSignedBytes words, a bit each, MSB first per byte, zero beyond the length) and
 * toBeSignedLen, which g16_nzcp_inputs fills from the ToBeSigned bytes (out_words: 8 * max_bytes + 1 words).  The
 * calculator trusts the toBeSigned words to be bits, as the builder's bytes are; other values give a witness that
 * g16_wtns_check refuses.
 * g16_nzcp_gadget_program: ONE template of the library (the names of g16_nzcp_gadget); its private inputs are the input
 * words, in g16_nzcp_gadget's order (sha256Var: the length in bits, then the 512 << blockSpace message BITS), its output
 * values the wires g16_wtns_calc_outputs lists.  Both images are g16_free'd; building takes seconds at the full size, so
 * callers keep the image.
 * g16_wtns_calc_create: the image is validated COMPLETELY on the host before any device is touched (every wire defined
 * exactly once, every term reading a wire of a strictly lower level, every index and the level index in range):
 * G16_E_FORMAT and "witness program: ..." otherwise.  device >= 0: the program resident there (csrc/wtns_calc.hip, one
 * workgroup per witness, a barrier per level); device = -1: host threads (at most 16, one witness each).  Not thread-safe.
 * g16_wtns_calc: `count` witnesses; inputs = count * n_inputs canonical 32-byte little-endian words (a word >= r:
 * G16_E_FORMAT, "witness I: input NAME[J] is not reduced modulo the scalar field"); out_bodies (or NULL) = count * n_wires
 * words, the body of a .wtns each; status[i] = the lowest violated check of witness i, or 0xffffffff.  A VIOLATED CHECK IS A
 * VERDICT: the call succeeds; g16_wtns_calc_check_text words it (the builder's text for that constraint; NULL out of
 * range).  On the device a batch runs in chunks of as many witnesses as 4 GiB hold at 32 bytes per wire, at most 1024
 * (G16_WTNS_CALC_CHUNK=<witnesses>, read at create, overrides); only the status words come back unless out_bodies asks.
 * g16_wtns_calc_wtns: the .wtns image of one witness (g16_free); with a violated check *wtns stays NULL.
 * g16_wtns_calc_info: n_wires, n_public, n_inputs, levels, outputs, named inputs.  g16_wtns_calc_input: the name, first
 * word and count of named input i.  g16_wtns_calc_timings: device ms of the last call's upload, kernels and download.
 * g16_stage_inputs: the witness evaluated on the prover's stream INTO slot `slot` of the prover, only the public signals
 * copied back; g16_prove_staged then works unchanged.  Refused with a text: a calculator on another device or on the host
 * route, a program whose wire or public counts differ from the key's, a prover between g16_shard_begin and _end.  With a
 * violated check the call succeeds, *status names it and the slot is left unstaged.
 * g16_fullprove_batch, g16_plonk_fullprove_batch: `count` passes in, proofs and public signals out; the witnesses never
 * leave the device.  inputs as for g16_wtns_calc (a word >= r fails the whole call with its text before the device is
 * touched); rs = count * 64 bytes (r | s per proof), blinding = count * 9 * 32 bytes, or NULL: the OS CSPRNG; out = count
 * proofs; pub (or NULL) = count rows of n_public words, words 1..n_public of each witness; status as for g16_wtns_calc.
 * A VIOLATED CHECK IS A VERDICT: the call succeeds, proof i and row i of pub are all zero bytes, and the other proofs
 * are unaffected.  With explicit rs / blinding proof i is byte for byte what g16_wtns_calc_wtns + g16_stage_witness +
 * g16_prove_staged (g16_plonk_prove) give.  count = 0 succeeds and touches nothing.  Refused with g16_stage_inputs'
 * texts behind "fullprove:" ("plonk fullprove:"): a calculator on the host route or on another device, wire or public
 * counts that differ from the key's (PLONK: the key's R1CS wire count, nVars less the addition signals); a sharded
 * Groth16 handle, or one between g16_shard_begin and _end, as g16_prove_batch refuses it.  The calculator computes chunks
 * (the 4 GiB rule above, G16_WTNS_CALC_CHUNK) on its own stream into TWO chunk buffers -- chunk k + 1 while the Groth16
 * proofs of chunk k run through g16_prove_batch's pipeline; PLONK proofs run one after another from one buffer -- so a
 * batched fullprove holds at most 2 x 4 GiB of witnesses on the device (2 x min(count, chunk) x n_wires x 32 bytes), and
 * only inputs, status words, public signals and proofs cross the bus.  On an error exit every launch and copy of the call
 * is drained first; the prover's witness slots are untouched, and both handles stay usable. */
typedef struct g16_wtns_calculator g16_wtns_calculator;
int g16_nzcp_witness_program(const uint32_t params[7], uint8_t** prog, size_t* len);
int g16_nzcp_gadget_program(const char* name, const uint32_t* params, uint32_t nparams, uint8_t** prog, size_t* len);
int g16_nzcp_inputs(const uint8_t* tbs, uint32_t len, uint32_t max_bytes, uint8_t* out_words);
int g16_wtns_calc_create(const uint8_t* prog, size_t len, int device /* -1 = host threads */, g16_wtns_calculator** out);
int g16_wtns_calc(g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, size_t count, uint8_t* out_bodies, uint32_t* status);
const char* g16_wtns_calc_check_text(const g16_wtns_calculator* h, uint32_t k);
int g16_wtns_calc_wtns(g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, uint32_t* status, uint8_t** wtns, size_t* len);
int g16_wtns_calc_info(const g16_wtns_calculator* h, uint32_t info[6]);
int g16_wtns_calc_outputs(const g16_wtns_calculator* h, uint32_t* wires);
const char* g16_wtns_calc_input(const g16_wtns_calculator* h, uint32_t i, uint32_t* first, uint32_t* count);
int g16_wtns_calc_timings(const g16_wtns_calculator* h, float ms[3]);
void g16_wtns_calc_destroy(g16_wtns_calculator* h);
int g16_stage_inputs(g16_prover* p, uint32_t slot, g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, uint32_t* status);
int g16_fullprove_batch(g16_prover* p, g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, size_t count,
                        const uint8_t* rs /* count * 64 (r | s) or NULL */, g16_proof* out /* count */,
                        uint8_t* pub /* count * n_public * 32, or NULL */, uint32_t* status /* count */);
int g16_plonk_fullprove_batch(g16_plonk* p, g16_wtns_calculator* h, const uint8_t* inputs, size_t n_inputs, size_t count,
                              const uint8_t* blinding /* count * 9 * 32 or NULL */, g16_plonk_proof* out, uint8_t* pub,
                              uint32_t* status);

/* ---------------------------------------------------------------------------------------------------------------
 * NZCP pass verification: ES256 (ECDSA over NIST P-256 with SHA-256, COSE alg -7) for batches of signatures against a
 * few resident issuer keys.  The circuit does not check the pass signature; it publishes toBeSignedSha256 so that the
 * relying party can.  One handle = the 4-bit window tables of G and of every key (61 KB per point), resident on one
 * GPU, or in host memory with device -1: the same code on at most 16 host threads, no GPU needed.
 *
 * keys: n_keys x 64 bytes, x | y big-endian (the JWK / COSE form), 1 <= n_keys <= 16.  G16_E_FORMAT, the text names the
 *       key index: a coordinate >= p, a point off the curve, (0, 0).  n_keys out of range: G16_E_ARG.
 * hashes: count x 32 (SHA-256 digests, big-endian; reduced modulo n here); sigs: count x 64 (r | s big-endian);
 * key_idx: count x u32 or NULL (= key 0); an entry >= n_keys is G16_E_ARG, the text names the item.
 * ok[i] = 1 iff signature i verifies under its key.  An invalid signature -- r or s outside [1, n), a sum at
 * infinity, a different x -- is a verdict (0), never an error.  One batch at a time per handle (serialised). */
typedef struct g16_es256_verifier g16_es256_verifier;
int g16_es256_verifier_create(const uint8_t* keys, uint32_t n_keys, int device, g16_es256_verifier** out);
int g16_es256_verify_batch(g16_es256_verifier* v, const uint8_t* hashes, const uint8_t* sigs, const uint32_t* key_idx,
                           size_t count, uint8_t* ok);
/* time of the last batch, ms: [0] scalars (s^-1, u1, u2), [1] point sum + compare (device time; wall time on the host route) */
int g16_es256_verifier_timings(const g16_es256_verifier* v, float ms[2]);
void g16_es256_verifier_destroy(g16_es256_verifier* v);
/* Layer-test operator of csrc/p256.cuh, n items, device -1 = host threads.  Every value is 32 bytes big-endian,
 * standard form, below its modulus (else G16_E_ARG naming the item).  op 0 / 1 / 2: base field a + b, a - b, a b;
 * 3 / 4 / 5: the same in the scalar field; 6 / 7: inverse in the scalar / base field (b unused, inverse of 0 = 0);
 * 8: affine a + affine b (x | y, 64 bytes each; (0, 0) = infinity in and out; points are not checked) by the mixed
 * addition, 9: the same sum by the full addition on rescaled operands; 10: a = X | Z, b = r (below n) -> one byte:
 * Z != 0 and x(X : Z) mod n == r, compared projectively. */
int g16_p256_op(int device, int op, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n);
/* The relying party's combined verdict for proofs of NZCPPubIdentity (public.json: 256 credSubjSha256 bits, 256
 * toBeSignedSha256 bits MSB-first, exp -- n_public of the verifier must be 513, else G16_E_ARG).  The digest each
 * signature is checked against is packed from public signals 256..511 of that proof: the caller never supplies it.
 * sigs / key_idx as above; both handles on the same device (else G16_E_ARG; the proof verifier has no host route).
 * verdict[i]: 0 ok, 1 proof rejected, 2 signals 0..511 are not all 0 / 1, 3 signature rejected, 4 expired (exp <= now;
 * now = 0 skips the test) -- the first that applies, in this order.  The proofs take g16_verify_batch's path; the
 * signatures run on the ES256 handle's own stream meanwhile. */
int g16_nzcp_pass_proof_verify_batch(g16_verifier* v, g16_es256_verifier* e, const g16_proof* proofs, const uint8_t* pubs,
                                     const uint8_t* sigs, const uint32_t* key_idx, uint64_t now, size_t count, uint8_t* verdict);

/* ---------------------------------------------------------------------------------------------------------------
 * NZCP pass verification from URIs: the whole of a relying party's offline check in one call for many passes -- text,
 * base32, the COSE_Sign1 / CWT walk, SHA-256(ToBeSigned), the issuer-key lookup, the ES256 signature, nbf / exp.  On a
 * device the front end is one kernel that writes digests, signatures and key indices into the scratch of the ES256
 * handle this handle owns; with device -1 the same code runs on at most 16 host threads.  One fixed-size record per pass.
 *
 * Passes are attacker-supplied bytes: whatever is wrong with one is a verdict in its record, never an error code.  A
 * pass is WELL-FORMED when all of 1 to 6 hold; anything else is G16_PASS_MALFORMED.
 * 1. Text.  Leading and trailing ' ' / \t / \r / \n are trimmed; then the literal "NZCP:/1/", at least one character of
 *    A-Z2-7, and an optional run of trailing '='.  Other version digits, '=' elsewhere, any other character fail.
 * 2. Base32, RFC 4648 alphabet: 5 bits a character, a byte whenever 8 bits are held, leftover bits dropped unchecked.
 * 3. CBOR.  The first item of the decoded bytes is tag 18 around an array of exactly 4; items 0, 2 and 3 are byte
 *    strings, item 1 is any well-formed item and is skipped; bytes after the first item are ignored.  A well-formed
 *    item: major types 0..6, additional info < 24 or 24..27 (non-minimal encodings accepted; 28..31 -- indefinite
 *    lengths among them -- and major type 7 refused), every length inside its buffer, and at most G16_PASS_CBOR_DEPTH
 *    arrays, non-empty maps and tags open at once inside any one skipped item, itself included.  Every item of every
 *    structure walked is validated, not only the entries that are read.
 * 4. Protected header: its first item is a map; key 1 is alg, key 4 is kid, a later duplicate overrides an earlier one.
 *    alg other than the integer -7, or absent, is G16_PASS_ALG.  kid is compared bytewise, as a byte or text string;
 *    of another type or absent it matches no key.
 * 5. Payload: its first item is a map; key 1 iss is a text string; keys 4 exp and 5 nbf are integers that fit int64;
 *    text key "vc" is a map whose text key "credentialSubject" is a map (the last duplicate decides, everywhere).  If
 *    its givenName, familyName and dob are all text strings, cred_subj_sha256 = SHA-256(given "," family "," dob) over
 *    their raw bytes and G16_PASS_HAS_SUBJECT is set; otherwise the digest is zero and the flag clear.
 * 6. The signature is exactly 64 bytes.  ToBeSigned = 84 6A "Signature1" bstr(protected) 40 bstr(payload), the heads
 *    of bstr in their shortest form; tbs_sha256 is its SHA-256, the digest the signature is checked against.
 * Verdict: the first that applies of 1 malformed, 2 alg, 3 no key with this iss and kid, 4 the signature does not
 * verify, 5 now < nbf, 6 now >= exp; else 0.  G16_PASS_TOO_LONG (7) is decided before all of them, on the item's length
 * alone (offsets[i + 1] - offsets[i] > G16_PASS_URI_MAX, the untrimmed text): such text is never read.
 * Stricter than js/nzcpInput.js on purpose: the nesting cap, the int64 range of nbf / exp, verdict 7 (the JS reader has
 * no such limits), and a kid that is neither a byte nor a text string matches nothing (the JS reader prints it).
 * A well-formed pass has every field of its record filled whatever its verdict (key_idx = 0 when no key matched);
 * a malformed or too long one has all but the verdict zero.
 *
 * keys as for g16_es256_verifier_create, with the same checks and texts; iss[j] / kid[j]: the NUL-terminated name of
 * key j, each 1 to G16_PASS_NAME_MAX bytes (else G16_E_ARG); the first key whose iss and kid both match is taken.
 * text + offsets: pass i is text[offsets[i], offsets[i + 1]); offsets ascend (else G16_E_ARG).  count = 0 is accepted.
 * One batch at a time per handle (serialised). */
#define G16_PASS_URI_MAX 2048
#define G16_PASS_CBOR_DEPTH 16
#define G16_PASS_NAME_MAX 128
#define G16_PASS_HAS_SUBJECT 1u
enum { G16_PASS_OK = 0, G16_PASS_MALFORMED = 1, G16_PASS_ALG = 2, G16_PASS_KEY = 3, G16_PASS_SIGNATURE = 4,
       G16_PASS_NOT_YET = 5, G16_PASS_EXPIRED = 6, G16_PASS_TOO_LONG = 7 };
typedef struct {
  uint32_t verdict, key_idx, tbs_len, flags;
  int64_t nbf, exp;
  uint8_t tbs_sha256[32], cred_subj_sha256[32];
} g16_pass_result;
typedef struct g16_pass_verifier g16_pass_verifier;
int g16_pass_verifier_create(const uint8_t* keys /* n x (x|y), big-endian */, const char* const* iss, const char* const* kid,
                             uint32_t n_keys /* <= 16 */, int device, g16_pass_verifier** out);
int g16_pass_verify_batch(g16_pass_verifier* v, const uint8_t* text, const uint64_t* offsets /* count + 1 */, size_t count,
                          int64_t now, g16_pass_result* out);
/* time of the last batch, ms: [0] the front end, [1] scalars, [2] point sum + compare (device time; wall time on the host route) */
int g16_pass_verifier_timings(const g16_pass_verifier* v, float ms[3]);
void g16_pass_verifier_destroy(g16_pass_verifier* v);
/* Layer-test operator of csrc/nzcp_pass.cuh and csrc/sha256.cuh over the items text[offsets[i], offsets[i + 1]), device
 * -1 = host threads.  op 0: base32-decode each item (A-Z2-7 then trailing '=', at most G16_PASS_URI_MAX characters):
 * out is count x (4 + 1280) bytes, a u32 length (0xffffffff: not base32, or too long) then the bytes.  op 1: SHA-256 of
 * each item's bytes, out count x 32.  op 2: the front end alone on pass URIs with an empty key table, out count x
 * g16_pass_result: verdict 1, 2, 7, or 3 for every well-formed ES256 pass; no signature work is done. */
int g16_pass_op(int device, int op, const uint8_t* text, const uint64_t* offsets, size_t count, uint8_t* out);

/* ---------------------------------------------------------------------------------------------------------------
 * Proving passes from their URIs: the holder's side in one call -- pass URI in, proof out.  The front end and the ES256
 * kernels of g16_pass_verify_batch run first for the whole batch (on the pass verifier's ES256 stream); the host decides
 * the outcome of every pass; the passes to prove are cut into the calculator's chunks (the 4 GiB rule, G16_WTNS_CALC_CHUNK)
 * and their input words -- toBeSigned[8 M], a bit a word, and toBeSignedLen, the image g16_nzcp_inputs writes -- are
 * formed by one kernel (csrc/pass_prove.hip, a workgroup per pass) on the calculator's stream, straight into the chunk
 * buffer the witness kernel reads; the proofs then run as g16_fullprove_batch / g16_plonk_fullprove_batch run them.
 * Only text, records, status words, public signals and proofs cross the bus.
 * M comes from the program: its named inputs must be exactly toBeSigned with 8 M words and toBeSignedLen with 1 word, in
 * this order, 1 <= M <= 503; otherwise G16_E_ARG, "pass prove: the program's inputs are not toBeSigned[8 M] and
 * toBeSignedLen".
 * res[i].outcome, the first that applies:
 *   G16_PROVE_PASS      pass.verdict is nonzero (and not one of 3..6 with G16_PASS_PROVE_UNSIGNED)
 *   G16_PROVE_TOO_LONG  ToBeSigned is longer than M bytes
 *   G16_PROVE_CHECK     the witness violates check `check` of the program (g16_wtns_calc_check_text words it)
 *   G16_PROVE_MISMATCH  with G16_PASS_PROVE_MATCH_PUBLIC: public signals 0..255 are not the bits of pass.cred_subj_sha256
 *                       (MSB first), 256..511 not those of pass.tbs_sha256, 512 not pass.exp, or the record lacks
 *                       G16_PASS_HAS_SUBJECT -- the front end and the circuit computed differently
 *   G16_PROVE_DONE      proof i and row i of pub are the pass's
 * Every outcome but DONE leaves proof i and row i of pub all zero and the other passes unaffected.  res[i].pass is the
 * record g16_pass_verify_batch gives for (text, now); check is 0xffffffff unless the outcome is CHECK.  With explicit rs
 * (blinding) proof i is byte for byte what g16_pass_inputs + g16_wtns_calc_wtns + g16_stage_witness + g16_prove_staged
 * (g16_plonk_prove) give.  count = 0 succeeds and touches nothing.
 * Refused before the device is touched, with g16_stage_inputs' texts behind "pass prove:" ("plonk pass prove:"): a
 * calculator on the host route or on another device, wire or public counts that differ from the key's, a sharded Groth16
 * handle; "...: the pass verifier runs on the host route (create it on the prover's device)" / "...: the pass verifier is
 * on device A, the prover on device B" (G16_E_STATE); MATCH_PUBLIC with a program of other than 513 public signals
 * (G16_E_ARG); the item checks of g16_pass_verify_batch.  A pass the host selected and the kernel refuses is
 * G16_E_STATE, "pass prove: the device disagrees with the front end on pass I", never a proof.
 * The prover and the pass verifier are locked for the length of the call (the calculator is not thread-safe, as ever).
 * On an error exit every launch and copy of the call is drained first; all three handles stay usable.
 * g16_pass_inputs: the layer operator -- the input words alone.  device -1 = host threads (at most 16), the same
 * csrc/nzcp_pass.cuh code; out_words = count x (8 max_bytes + 1) x 32 bytes; a row of zeros and ok[i] = 0 for a pass that
 * is not well-formed (g16_pass_verify_batch's rules 1 to 6) or whose ToBeSigned exceeds max_bytes.
 * g16_pass_wtns_public: the device calculator alone over pass URIs, its chunks filled by the same kernel -- no key, no
 * proof, no signature work: status[i] = 0xffffffff and row i of pub (n_public words) the witness's public signals, or the
 * violated check and a zero row, or G16_PASS_WTNS_NO_ROW for a pass that g16_pass_inputs gives no row.  The program's
 * inputs as above; a host-route calculator is G16_E_STATE. */
#define G16_PASS_PROVE_UNSIGNED 1u     /* verdicts 3 (no key), 4 (signature), 5 (nbf), 6 (exp) are recorded but do not
                                          block the proof: the circuit itself does not check the signature */
#define G16_PASS_PROVE_MATCH_PUBLIC 2u /* NZCPPubIdentity programs only (n_public == 513, else G16_E_ARG) */
enum { G16_PROVE_DONE = 0, G16_PROVE_PASS = 1 /* blocked by pass.verdict */, G16_PROVE_TOO_LONG = 2 /* tbs_len > M */,
       G16_PROVE_CHECK = 3 /* the circuit refuses the pass: `check` names it */, G16_PROVE_MISMATCH = 4 };
typedef struct {
  uint32_t outcome, check /* 0xffffffff unless outcome 3 */;
  g16_pass_result pass;
} g16_pass_prove_result;
int g16_pass_fullprove_batch(g16_prover* p, g16_wtns_calculator* h, g16_pass_verifier* v, const uint8_t* text,
                             const uint64_t* offsets /* count + 1 */, size_t count, int64_t now, uint32_t flags,
                             const uint8_t* rs /* count * 64 (r | s) or NULL */, g16_proof* out /* count */,
                             uint8_t* pub /* count * n_public * 32, or NULL */, g16_pass_prove_result* res /* count */);
int g16_plonk_pass_fullprove_batch(g16_plonk* p, g16_wtns_calculator* h, g16_pass_verifier* v, const uint8_t* text,
                                   const uint64_t* offsets, size_t count, int64_t now, uint32_t flags,
                                   const uint8_t* blinding /* count * 9 * 32 or NULL */, g16_plonk_proof* out, uint8_t* pub,
                                   g16_pass_prove_result* res);
int g16_pass_inputs(int device, const uint8_t* text, const uint64_t* offsets, size_t count, uint32_t max_bytes,
                    uint8_t* out_words, uint8_t* ok);
#define G16_PASS_WTNS_NO_ROW 0xfffffffeu
int g16_pass_wtns_public(g16_wtns_calculator* h, const uint8_t* text, const uint64_t* offsets, size_t count, uint8_t* pub,
                         uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* G16_PROVER_H */
