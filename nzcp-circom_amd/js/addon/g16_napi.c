/*
 * Thin raw-C N-API binding over the C ABI of libg16hip.so (include/g16_prover.h).
 * Host code stays Node.js (BASELINE.json north_star); this file only marshals Buffers.
 *
 * snarkjs never blocks the event loop (its work runs in web-workers: ffjavascript threadman.js,
 * pin /root/reference/yarn.lock:408-416), so create/prove run in napi async work and return
 * Promises; nothing keeps the loop alive after the Promise settles (Threading).
 *
 * Exports:  create(zkey: Buffer, opts: {device, devices: [..], windowBits, taskLen}) -> Promise<handle>
 *             (devices with more than one entry: ONE proof sharded over those GPUs, g16_multi_* -- BASELINE config 4)
 *           prove(handle, wtns: Buffer, r: Buffer|null, s: Buffer|null) -> Promise<{proof: Buffer(256), pub: Buffer}>
 *           proveBatch(handle, wtns: Buffer[], rs: Buffer|null) -> Promise<[{proof, pub}]>
 *           info(handle) -> {nVars, nPublic, domainSize, nCoefs}
 *           timings(handle) -> {...ms}
 *           destroy(handle)
 *           createVerifier(vkey: Buffer, nPublic, montgomery: 0|1, device) -> Promise<vhandle>   (g16_verifier_create)
 *           verifyBatch(vhandle, proofs: Buffer(count*256), pubs: Buffer(count*nPublic*32)) -> Promise<Buffer(count)>
 *           destroyVerifier(vhandle)
 *           plonkCreate(zkey: Buffer, device) -> Promise<phandle>                                  (g16_plonk_create)
 *           plonkProve(phandle, wtns: Buffer, blinding: Buffer(288)|null) -> Promise<{proof: Buffer(832), pub: Buffer}>
 *           plonkDestroy(phandle)
 *           plonkSetupFiles(r1csPath, ptauPath, zkeyPath, device, withLagrange) -> Promise<undefined>   (g16_plonk_setup_files)
 *           groth16SetupFiles(r1csPath, ptauPath, zkeyPath, device) -> Promise<undefined>   (g16_groth16_setup_files)
 *           zkeyNewFiles(r1csPath, ptauPath, zkeyPath, device) -> Promise<Buffer(64): csHash>   (g16_zkey_new_files)
 *           zkeyCsHashFiles(zkeyPath, ptauPath, device) -> Promise<Buffer(64): csHash>   (g16_zkey_cs_hash_files)
 *           ptauPrepareFiles(inPath, outPath, device) -> Promise<undefined>   (g16_ptau_prepare_files)
 *           zkeyContributeFiles(inPath, outPath, name | null, secret Buffer(64) | null, device) -> Promise<Buffer(64)>
 *                                                                              (g16_zkey_contribute_files: the hash)
 *           ptauNewFile(power, outPath) -> Promise<undefined>                  (g16_ptau_new_file)
 *           ptauContributeFiles(inPath, outPath, name | null, secret Buffer(192) | null, device) -> Promise<Buffer(64)>
 *                                                                              (g16_ptau_contribute_files: the hash)
 *           ptauVerifyFile(path, device) -> Promise<{ok, reason}>              (g16_ptau_verify_file)
 *           wtnsCheckFiles(r1csPath, wtnsPath, device) -> Promise<{constraint, nFailed, a, b, c}>  (g16_wtns_check_files;
 *               constraint -1 = every constraint holds; a, b, c: Buffers of 32 bytes, little-endian)
 *           ptauExportChallengeFiles(ptauPath, challengePath) -> Promise<Buffer(64)>   (g16_ptau_export_challenge_files: the
 *                                                                              challenge hash)
 *           ptauChallengeContributeFiles(challengePath, responsePath, secret Buffer(192) | null, device) -> Promise<Buffer(64)>
 *                                                                              (g16_ptau_challenge_contribute_files)
 *           ptauImportResponseFiles(oldPath, responsePath, newPath, name | null, device) -> Promise<Buffer(64)>; a failed
 *                                                                              check rejects with its text
 *                                                                              (g16_ptau_import_response_files)
 *           nzcpProgramFile(params[7] | null, gadget | null, gadgetParams, path); wtnsCalculate(programPath, names, values,
 *               device) -> {status, text, wtns}   (g16_nzcp_witness_program, g16_wtns_calc_wtns: see above their code)
 *           fullProveBatch(plonk: bool, programPath, zkey: Buffer, names: string[][], values: Buffer[][], device,
 *               blinding: Buffer | null) -> [{status, text, proof, pub}]   (g16_fullprove_batch, g16_plonk_fullprove_batch)
 *           zkeyVerifyFromInitFiles(initPath, zkeyPath, device) -> Promise<{ok, reason}>   (g16_zkey_verify_from_init_files)
 *           zkeyVerifyFromInitPtauFiles(initPath, ptauPath, zkeyPath, device) -> Promise<{ok, reason}>   (..._from_init_ptau_files)
 *           zkeyVerifyR1csFiles(r1csPath, ptauPath, zkeyPath, device) -> Promise<{ok, reason}>   (g16_zkey_verify_r1cs_files)
 *           ptauBeaconFiles(inPath, outPath, name | null, beaconHash: Buffer, numIterationsExp, device) -> Promise<Buffer(64)>
 *           zkeyBeaconFiles(inPath, outPath, name | null, beaconHash: Buffer, numIterationsExp, device) -> Promise<Buffer(64)>
 *                                                            (g16_ptau_beacon_files, g16_zkey_beacon_files: the hash)
 *           es256VerifyBatch(keys: Buffer(nKeys*64), hashes: Buffer(count*32), sigs: Buffer(count*64),
 *               keyIdx: Buffer(count*4, u32 LE) | null, device) -> Promise<Buffer(count)>   (g16_es256_verify_batch: ONE batch
 *               under a verifier created for the call; device -1 = host threads)
 *           nzcpPassProofVerify(vkey: Buffer, nPublic, keys, proofs: Buffer(count*256), pubs: Buffer(count*nPublic*32), sigs,
 *               keyIdx | null, now, device) -> Promise<Buffer(count): verdict codes>   (g16_nzcp_pass_proof_verify_batch)
 *           passVerifyBatch(keys: Buffer(nKeys*64), names: Buffer("iss\0kid\0" per key), text: Buffer, offsets:
 *               Buffer((count+1)*8, u64 LE), now, device) -> Promise<Buffer(count*96): g16_pass_result records>
 *               (g16_pass_verify_batch: ONE batch under a verifier created for the call; device -1 = host threads)
 *           passProveBatch(plonk, programPath, zkey, keys, names, text, offsets, now, flags, device, blinding | null)
 *               -> [{outcome, check, text, record: Buffer(96), proof, pub}]   (g16_pass_fullprove_batch and its PLONK twin)
 */
#include <node_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/g16_prover.h"

#define NAPI_OK(call)                                                         \
  do {                                                                        \
    if ((call) != napi_ok) {                                                  \
      napi_throw_error(env, NULL, "g16 addon: N-API call failed: " #call);    \
      return NULL;                                                            \
    }                                                                         \
  } while (0)

/* `inflight` and `closing` are touched on the main (JS) thread only: jobs are queued by js_prove* and retired by
 * job_complete, both of which run there.  destroy() while a proof is queued or running only marks the handle;
 * the native prover (its mutex, streams, HBM buffers) is released when the last job retires -- never under a
 * worker thread that still dereferences it. */
typedef struct {
  g16_prover* p;   /* one GPU ... */
  g16_multi* m;    /* ... or one proof sharded over several (exactly one of the two is set) */
  uint32_t inflight;
  int closing;
} handle_t;

static int handle_live(const handle_t* h) { return h && (h->p || h->m); }
static int handle_info(const handle_t* h, g16_info* inf) {
  return h->m ? g16_multi_get_info(h->m, inf, NULL) : g16_get_info(h->p, inf);
}

static void handle_release(handle_t* h) {
  if (h->p) g16_destroy(h->p);
  if (h->m) g16_multi_destroy(h->m);
  h->p = NULL;
  h->m = NULL;
}

static void handle_finalize(napi_env env, void* data, void* hint) {
  handle_t* h = (handle_t*)data;   /* no job can be in flight: every job holds a reference on the external */
  handle_release(h);
  free(h);
}

typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref refs[4];      /* keep input Buffers alive while the worker runs */
  int nrefs;
  /* create */
  const uint8_t* zkey; size_t zkey_len; g16_opts opts; g16_prover* created;
  int32_t devices[64]; uint32_t ndev; g16_multi* created_multi;
  /* prove */
  handle_t* h; const uint8_t* wtns; size_t wtns_len; int have_r, have_s; uint8_t r[32], s[32];
  g16_proof proof; uint8_t* pub; size_t pub_len;
  /* batch */
  size_t bcount; const uint8_t** bw; size_t* blen; uint8_t* brs; g16_proof* bproofs; uint8_t* bpub; size_t bpub_each;
  napi_ref* brefs;
  int rc; char err[512];
  int is_create;   /* 1 = create, 0 = prove, 2 = prove batch */
} job_t;

static void job_execute(napi_env env, void* data) {
  job_t* j = (job_t*)data;
  if (j->is_create == 1) {
    if (j->ndev > 1) j->rc = g16_multi_create(j->zkey, j->zkey_len, j->devices, j->ndev, &j->opts, &j->created_multi);
    else j->rc = g16_create(j->zkey, j->zkey_len, &j->opts, &j->created);
  } else if (j->is_create == 2) {
    j->rc = g16_prove_batch(j->h->p, j->bw, j->blen, j->bcount, j->brs, j->bproofs, j->bpub);
  } else {
    if (j->h->m)
      j->rc = g16_multi_prove(j->h->m, j->wtns, j->wtns_len, j->have_r ? j->r : NULL, j->have_s ? j->s : NULL,
                              &j->proof, j->pub);
    else
      j->rc = g16_prove(j->h->p, j->wtns, j->wtns_len, j->have_r ? j->r : NULL, j->have_s ? j->s : NULL,
                        &j->proof, j->pub);
  }
  if (j->rc) {
    strncpy(j->err, g16_last_error(), sizeof(j->err) - 1);   /* thread-local: read on the worker */
    j->err[sizeof(j->err) - 1] = 0;
  }
}

static void job_complete(napi_env env, napi_status status, void* data) {
  job_t* j = (job_t*)data;
  napi_value result;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->rc ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->is_create == 2) {
    napi_create_array_with_length(env, j->bcount, &result);
    for (size_t i = 0; i < j->bcount; i++) {
      napi_value item, proof, pub;
      void* dst;
      napi_create_object(env, &item);
      napi_create_buffer_copy(env, sizeof(g16_proof), &j->bproofs[i], &dst, &proof);
      napi_create_buffer_copy(env, j->bpub_each, j->bpub + i * j->bpub_each, &dst, &pub);
      napi_set_named_property(env, item, "proof", proof);
      napi_set_named_property(env, item, "pub", pub);
      napi_set_element(env, result, (uint32_t)i, item);
    }
    napi_resolve_deferred(env, j->deferred, result);
  } else if (j->is_create == 1) {
    handle_t* h = (handle_t*)calloc(1, sizeof(handle_t));
    h->p = j->created;
    h->m = j->created_multi;
    napi_create_external(env, h, handle_finalize, NULL, &result);
    napi_resolve_deferred(env, j->deferred, result);
  } else {
    napi_value proof, pub;
    void* dst;
    napi_create_object(env, &result);
    napi_create_buffer_copy(env, sizeof(g16_proof), &j->proof, &dst, &proof);
    napi_create_buffer_copy(env, j->pub_len, j->pub, &dst, &pub);
    napi_set_named_property(env, result, "proof", proof);
    napi_set_named_property(env, result, "pub", pub);
    napi_resolve_deferred(env, j->deferred, result);
  }
  if (j->h) {   /* prove / proveBatch: retire the job; a destroy() issued meanwhile takes effect now */
    j->h->inflight--;
    if (j->h->closing && j->h->inflight == 0) handle_release(j->h);
  }
  for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
  if (j->brefs) { for (size_t i = 0; i < j->bcount; i++) napi_delete_reference(env, j->brefs[i]); free(j->brefs); }
  napi_delete_async_work(env, j->work);
  free(j->pub); free(j->bw); free(j->blen); free(j->brs); free(j->bproofs); free(j->bpub);
  free(j);
}

static int32_t get_i32(napi_env env, napi_value obj, const char* key, int32_t dflt) {
  napi_value v;
  napi_valuetype t;
  bool has = false;
  if (napi_has_named_property(env, obj, key, &has) != napi_ok || !has) return dflt;
  if (napi_get_named_property(env, obj, key, &v) != napi_ok) return dflt;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return dflt;
  int32_t out = dflt;
  napi_get_value_int32(env, v, &out);
  return out;
}

static napi_value queue_job(napi_env env, job_t* j, const char* name) {
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, job_execute, job_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value js_create(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool isbuf = false;
  if (argc < 1 || napi_is_buffer(env, argv[0], &isbuf) != napi_ok || !isbuf) {
    napi_throw_type_error(env, NULL, "create(zkey: Buffer, opts)");
    return NULL;
  }
  job_t* j = (job_t*)calloc(1, sizeof(job_t));
  j->is_create = 1;
  void* data;
  NAPI_OK(napi_get_buffer_info(env, argv[0], &data, &j->zkey_len));
  j->zkey = (const uint8_t*)data;
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  if (argc > 1) {
    napi_valuetype t;
    if (napi_typeof(env, argv[1], &t) == napi_ok && t == napi_object) {
      j->opts.device = get_i32(env, argv[1], "device", 0);
      j->opts.window_bits = get_i32(env, argv[1], "windowBits", 0);
      j->opts.task_len = get_i32(env, argv[1], "taskLen", 0);
      /* devices: [ordinal, ...] -> one shard of the key per entry; a single entry is the plain one-GPU handle */
      napi_value dv;
      bool has = false, isarr = false;
      if (napi_has_named_property(env, argv[1], "devices", &has) == napi_ok && has &&
          napi_get_named_property(env, argv[1], "devices", &dv) == napi_ok && napi_is_array(env, dv, &isarr) == napi_ok && isarr) {
        uint32_t n = 0;
        napi_get_array_length(env, dv, &n);
        if (n > 64) { free(j); napi_throw_range_error(env, NULL, "devices: at most 64 entries"); return NULL; }
        for (uint32_t i = 0; i < n; i++) {
          napi_value el;
          int32_t d = 0;
          if (napi_get_element(env, dv, i, &el) != napi_ok || napi_get_value_int32(env, el, &d) != napi_ok) {
            free(j);
            napi_throw_type_error(env, NULL, "devices: array of integers expected");
            return NULL;
          }
          j->devices[i] = d;
        }
        j->ndev = n;
        if (n == 1) j->opts.device = j->devices[0];
      }
    }
  }
  return queue_job(env, j, "g16_create");
}

static napi_value js_prove(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  handle_t* h = NULL;
  bool isbuf = false;
  if (argc < 2 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !handle_live(h) || h->closing ||
      napi_is_buffer(env, argv[1], &isbuf) != napi_ok || !isbuf) {
    napi_throw_type_error(env, NULL, "prove(handle, wtns: Buffer, r, s): bad arguments or handle already destroyed");
    return NULL;
  }
  job_t* j = (job_t*)calloc(1, sizeof(job_t));
  j->h = h;
  void* data;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &j->wtns_len));
  j->wtns = (const uint8_t*)data;
  NAPI_OK(napi_create_reference(env, argv[1], 1, &j->refs[j->nrefs++]));
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  for (int k = 0; k < 2; k++) {
    if (argc > (size_t)(2 + k) && napi_is_buffer(env, argv[2 + k], &isbuf) == napi_ok && isbuf) {
      size_t len;
      NAPI_OK(napi_get_buffer_info(env, argv[2 + k], &data, &len));
      if (len != 32) { free(j); napi_throw_range_error(env, NULL, "r and s must be 32-byte Buffers"); return NULL; }
      memcpy(k == 0 ? j->r : j->s, data, 32);
      if (k == 0) j->have_r = 1; else j->have_s = 1;
    }
  }
  g16_info inf;
  handle_info(h, &inf);
  j->pub_len = (size_t)inf.n_public * 32;
  j->pub = (uint8_t*)malloc(j->pub_len ? j->pub_len : 1);
  h->inflight++;
  return queue_job(env, j, "g16_prove");
}

/* proveBatch(handle, wtns: Buffer[], rs: Buffer(count*64)|null) -> Promise<[{proof, pub}]>  (g16_prove_batch:
 * the library pipelines the proofs over two scratch contexts) */
static napi_value js_prove_batch(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  handle_t* h = NULL;
  bool isarr = false, isbuf = false;
  uint32_t n = 0;
  if (argc < 2 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !h || !h->p || h->closing ||
      napi_is_array(env, argv[1], &isarr) != napi_ok || !isarr || napi_get_array_length(env, argv[1], &n) != napi_ok || n == 0) {
    napi_throw_type_error(env, NULL, "proveBatch(handle, wtns: Buffer[], rs): bad arguments, destroyed handle, or a "
                                     "multi-device handle (batches run on one-GPU handles: replicas, SURVEY 8e)");
    return NULL;
  }
  job_t* j = (job_t*)calloc(1, sizeof(job_t));
  j->is_create = 2;
  j->bcount = n;
  j->bw = (const uint8_t**)calloc(n, sizeof(uint8_t*));
  j->blen = (size_t*)calloc(n, sizeof(size_t));
  j->brefs = (napi_ref*)calloc(n, sizeof(napi_ref));
  j->bproofs = (g16_proof*)calloc(n, sizeof(g16_proof));
  g16_info inf;
  g16_get_info(h->p, &inf);
  j->bpub_each = (size_t)inf.n_public * 32;
  j->bpub = (uint8_t*)malloc(j->bpub_each * n + 1);
  for (uint32_t i = 0; i < n; i++) {
    napi_value el;
    void* data;
    if (napi_get_element(env, argv[1], i, &el) != napi_ok || napi_is_buffer(env, el, &isbuf) != napi_ok || !isbuf ||
        napi_get_buffer_info(env, el, &data, &j->blen[i]) != napi_ok || napi_create_reference(env, el, 1, &j->brefs[i]) != napi_ok) {
      napi_throw_type_error(env, NULL, "proveBatch: every witness must be a Buffer");
      return NULL;   /* small leak on a caller bug; the job never ran */
    }
    j->bw[i] = (const uint8_t*)data;
  }
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  if (argc > 2 && napi_is_buffer(env, argv[2], &isbuf) == napi_ok && isbuf) {
    void* data;
    size_t len;
    NAPI_OK(napi_get_buffer_info(env, argv[2], &data, &len));
    if (len != (size_t)n * 64) { napi_throw_range_error(env, NULL, "rs must hold count*64 bytes"); return NULL; }
    j->brs = (uint8_t*)malloc(len);
    memcpy(j->brs, data, len);
  }
  j->h = h;   /* set last: the early error returns above must not retire a job that was never counted */
  h->inflight++;
  return queue_job(env, j, "g16_prove_batch");
}

static napi_value js_info(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out, v;
  handle_t* h = NULL;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !handle_live(h)) {
    napi_throw_type_error(env, NULL, "info(handle)");
    return NULL;
  }
  g16_info inf;
  handle_info(h, &inf);
  NAPI_OK(napi_create_object(env, &out));
  const char* keys[4] = {"nVars", "nPublic", "domainSize", "nCoefs"};
  uint32_t vals[4] = {inf.n_vars, inf.n_public, inf.domain_size, inf.n_coefs};
  for (int i = 0; i < 4; i++) {
    NAPI_OK(napi_create_uint32(env, vals[i], &v));
    NAPI_OK(napi_set_named_property(env, out, keys[i], v));
  }
  return out;
}

static napi_value js_timings(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out, v;
  handle_t* h = NULL;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !h || !h->p) {
    napi_throw_type_error(env, NULL, "timings(handle)");
    return NULL;
  }
  g16_timings t;
  g16_get_timings(h->p, &t);
  NAPI_OK(napi_create_object(env, &out));
  const char* keys[4] = {"uploadMs", "qapMs", "nttMs", "totalMs"};
  double vals[4] = {t.upload_ms, t.qap_ms, t.ntt_ms, t.total_ms};
  for (int i = 0; i < 4; i++) {
    NAPI_OK(napi_create_double(env, vals[i], &v));
    NAPI_OK(napi_set_named_property(env, out, keys[i], v));
  }
  return out;
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  handle_t* h = NULL;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc >= 1 && napi_get_value_external(env, argv[0], (void**)&h) == napi_ok && handle_live(h)) {
    h->closing = 1;                       /* no new jobs; info()/timings() stay valid until the release */
    if (h->inflight == 0) handle_release(h);
  }
  return NULL;
}

/* ------------------------------------------------------------------ verifier (g16_verifier_*): snarkjs groth16.verify */
typedef struct {
  g16_verifier* v;            /* Groth16 ... */
  g16_plonk_verifier* pv;     /* ... or PLONK (exactly one of the two is set) */
  uint32_t n_public;
  uint32_t inflight;
  int closing;
} vhandle_t;
static void vhandle_release(vhandle_t* h) {
  if (h->v) g16_verifier_destroy(h->v);
  if (h->pv) g16_plonk_verifier_destroy(h->pv);
  h->v = NULL;
  h->pv = NULL;
}

static void vhandle_finalize(napi_env env, void* data, void* hint) {
  vhandle_t* h = (vhandle_t*)data;
  vhandle_release(h);
  free(h);
}

typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref refs[3];
  int nrefs;
  int kind;                 /* 0 = create, 1 = verify */
  int plonk;                /* the PLONK verifier (vkey = the 712-byte image, proofs of 832 bytes) */
  const uint8_t* vkey; size_t vkey_len; uint32_t n_public; int montgomery, device; g16_verifier* created;
  g16_plonk_verifier* created_pv;
  vhandle_t* h; const uint8_t* proofs; const uint8_t* pubs; size_t count; uint8_t* ok;
  int rc; char err[512];
} vjob_t;

static void vjob_execute(napi_env env, void* data) {
  vjob_t* j = (vjob_t*)data;
  if (j->plonk) {
    if (j->kind == 0) j->rc = g16_plonk_verifier_create(j->vkey, j->vkey_len, j->device, &j->created_pv);
    else j->rc = g16_plonk_verify_batch(j->h->pv, (const g16_plonk_proof*)j->proofs, j->pubs, j->count, j->ok);
  } else if (j->kind == 0) {
    j->rc = g16_verifier_create(j->vkey, j->vkey_len, j->n_public, j->montgomery, j->device, &j->created);
  } else {
    j->rc = g16_verify_batch(j->h->v, (const g16_proof*)j->proofs, j->pubs, j->count, j->ok);
  }
  if (j->rc) {
    strncpy(j->err, g16_last_error(), sizeof(j->err) - 1);
    j->err[sizeof(j->err) - 1] = 0;
  }
}

static void vjob_complete(napi_env env, napi_status status, void* data) {
  vjob_t* j = (vjob_t*)data;
  napi_value result;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->rc ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->kind == 0) {
    vhandle_t* h = (vhandle_t*)calloc(1, sizeof(vhandle_t));
    h->v = j->created;
    h->pv = j->created_pv;
    h->n_public = j->n_public;
    napi_create_external(env, h, vhandle_finalize, NULL, &result);
    napi_resolve_deferred(env, j->deferred, result);
  } else {
    void* dst;
    napi_create_buffer_copy(env, j->count, j->ok, &dst, &result);
    napi_resolve_deferred(env, j->deferred, result);
  }
  if (j->h) {
    j->h->inflight--;
    if (j->h->closing && j->h->inflight == 0) vhandle_release(j->h);
  }
  for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
  napi_delete_async_work(env, j->work);
  free(j->ok);
  free(j);
}

static napi_value queue_vjob(napi_env env, vjob_t* j, const char* name) {
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, vjob_execute, vjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value js_create_verifier(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  bool isbuf = false;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4 || napi_is_buffer(env, argv[0], &isbuf) != napi_ok || !isbuf) {
    napi_throw_type_error(env, NULL, "createVerifier(vkey: Buffer, nPublic, montgomery, device[, plonk])");
    return NULL;
  }
  vjob_t* j = (vjob_t*)calloc(1, sizeof(vjob_t));
  void* data;
  int32_t mont = 0, dev = 0, pl = 0;
  if (argc > 4) napi_get_value_int32(env, argv[4], &pl);
  j->plonk = pl != 0;
  NAPI_OK(napi_get_buffer_info(env, argv[0], &data, &j->vkey_len));
  j->vkey = (const uint8_t*)data;
  NAPI_OK(napi_get_value_uint32(env, argv[1], &j->n_public));
  NAPI_OK(napi_get_value_int32(env, argv[2], &mont));
  NAPI_OK(napi_get_value_int32(env, argv[3], &dev));
  j->montgomery = mont;
  j->device = dev;
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  return queue_vjob(env, j, "g16_verifier_create");
}

static napi_value js_verify_batch(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  vhandle_t* h = NULL;
  bool b1 = false, b2 = false;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !h || (!h->v && !h->pv) || h->closing ||
      napi_is_buffer(env, argv[1], &b1) != napi_ok || !b1 || napi_is_buffer(env, argv[2], &b2) != napi_ok || !b2) {
    napi_throw_type_error(env, NULL, "verifyBatch(vhandle, proofs: Buffer, pubs: Buffer)");
    return NULL;
  }
  void *pd, *ud;
  size_t plen, ulen;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &pd, &plen));
  NAPI_OK(napi_get_buffer_info(env, argv[2], &ud, &ulen));
  const size_t psz = h->pv ? sizeof(g16_plonk_proof) : sizeof(g16_proof);
  if (plen % psz || ulen != (plen / psz) * (size_t)h->n_public * 32) {
    napi_throw_range_error(env, NULL, "verifyBatch: proofs must be count*256 (groth16) / count*832 (plonk) bytes and pubs count*nPublic*32 bytes");
    return NULL;
  }
  vjob_t* j = (vjob_t*)calloc(1, sizeof(vjob_t));
  j->kind = 1;
  j->plonk = h->pv != NULL;
  j->h = h;
  j->proofs = (const uint8_t*)pd;
  j->pubs = (const uint8_t*)ud;
  j->count = plen / psz;
  j->ok = (uint8_t*)calloc(j->count ? j->count : 1, 1);
  h->inflight++;
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  NAPI_OK(napi_create_reference(env, argv[1], 1, &j->refs[j->nrefs++]));
  NAPI_OK(napi_create_reference(env, argv[2], 1, &j->refs[j->nrefs++]));
  return queue_vjob(env, j, "g16_verify_batch");
}

static napi_value js_destroy_verifier(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  vhandle_t* h = NULL;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc >= 1 && napi_get_value_external(env, argv[0], (void**)&h) == napi_ok && h && (h->v || h->pv)) {
    h->closing = 1;
    if (h->inflight == 0) vhandle_release(h);
  }
  return NULL;
}

/* ------------------------------------------------------------------ PLONK prover (g16_plonk_*): snarkjs plonk.prove */
typedef struct {
  g16_plonk* p;
  uint32_t n_public;
  uint32_t inflight;
  int closing;
} phandle_t;

static void phandle_finalize(napi_env env, void* data, void* hint) {
  phandle_t* h = (phandle_t*)data;
  if (h->p) g16_plonk_destroy(h->p);
  free(h);
}

typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  napi_ref refs[3];
  int nrefs;
  int kind;                 /* 0 = create, 1 = prove */
  const uint8_t* zkey; size_t zkey_len; int device; g16_plonk* created; uint32_t info[6];
  phandle_t* h; const uint8_t* wtns; size_t wtns_len; int have_blind; uint8_t blind[288];
  g16_plonk_proof proof; uint8_t* pub; size_t pub_len;
  int rc; char err[512];
} pjob_t;

static void pjob_execute(napi_env env, void* data) {
  pjob_t* j = (pjob_t*)data;
  if (j->kind == 0) {
    j->rc = g16_plonk_create(j->zkey, j->zkey_len, j->device, &j->created);
    if (!j->rc) g16_plonk_get_info(j->created, j->info);
  } else {
    j->rc = g16_plonk_prove(j->h->p, j->wtns, j->wtns_len, j->have_blind ? j->blind : NULL, &j->proof, j->pub);
  }
  if (j->rc) {
    strncpy(j->err, g16_last_error(), sizeof(j->err) - 1);
    j->err[sizeof(j->err) - 1] = 0;
  }
}

static void pjob_complete(napi_env env, napi_status status, void* data) {
  pjob_t* j = (pjob_t*)data;
  napi_value result;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->rc ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->kind == 0) {
    phandle_t* h = (phandle_t*)calloc(1, sizeof(phandle_t));
    h->p = j->created;
    h->n_public = j->info[1];
    napi_create_external(env, h, phandle_finalize, NULL, &result);
    napi_resolve_deferred(env, j->deferred, result);
  } else {
    napi_value proof, pub;
    void* dst;
    napi_create_object(env, &result);
    napi_create_buffer_copy(env, sizeof(g16_plonk_proof), &j->proof, &dst, &proof);
    napi_create_buffer_copy(env, j->pub_len, j->pub, &dst, &pub);
    napi_set_named_property(env, result, "proof", proof);
    napi_set_named_property(env, result, "pub", pub);
    napi_resolve_deferred(env, j->deferred, result);
  }
  if (j->h) {
    j->h->inflight--;
    if (j->h->closing && j->h->inflight == 0 && j->h->p) { g16_plonk_destroy(j->h->p); j->h->p = NULL; }
  }
  for (int i = 0; i < j->nrefs; i++) napi_delete_reference(env, j->refs[i]);
  napi_delete_async_work(env, j->work);
  free(j->pub);
  free(j);
}

static napi_value queue_pjob(napi_env env, pjob_t* j, const char* name) {
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, pjob_execute, pjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value js_plonk_create(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  bool isbuf = false;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1 || napi_is_buffer(env, argv[0], &isbuf) != napi_ok || !isbuf) {
    napi_throw_type_error(env, NULL, "plonkCreate(zkey: Buffer, device)");
    return NULL;
  }
  pjob_t* j = (pjob_t*)calloc(1, sizeof(pjob_t));
  void* data;
  int32_t dev = 0;
  NAPI_OK(napi_get_buffer_info(env, argv[0], &data, &j->zkey_len));
  j->zkey = (const uint8_t*)data;
  if (argc > 1) napi_get_value_int32(env, argv[1], &dev);
  j->device = dev;
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  return queue_pjob(env, j, "g16_plonk_create");
}

static napi_value js_plonk_prove(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  phandle_t* h = NULL;
  bool isbuf = false;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2 || napi_get_value_external(env, argv[0], (void**)&h) != napi_ok || !h || !h->p || h->closing ||
      napi_is_buffer(env, argv[1], &isbuf) != napi_ok || !isbuf) {
    napi_throw_type_error(env, NULL, "plonkProve(phandle, wtns: Buffer, blinding: Buffer|null)");
    return NULL;
  }
  pjob_t* j = (pjob_t*)calloc(1, sizeof(pjob_t));
  j->kind = 1;
  j->h = h;
  void* data;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &data, &j->wtns_len));
  j->wtns = (const uint8_t*)data;
  if (argc > 2) {
    bool b = false;
    size_t bl = 0;
    void* bd;
    if (napi_is_buffer(env, argv[2], &b) == napi_ok && b) {
      if (napi_get_buffer_info(env, argv[2], &bd, &bl) != napi_ok || bl != 288) {
        free(j);
        napi_throw_range_error(env, NULL, "plonkProve: blinding must be nine 32-byte scalars (288 bytes)");
        return NULL;
      }
      memcpy(j->blind, bd, 288);
      j->have_blind = 1;
    }
  }
  j->pub_len = (size_t)h->n_public * 32;
  j->pub = (uint8_t*)calloc(j->pub_len ? j->pub_len : 1, 1);
  h->inflight++;
  NAPI_OK(napi_create_reference(env, argv[0], 1, &j->refs[j->nrefs++]));
  NAPI_OK(napi_create_reference(env, argv[1], 1, &j->refs[j->nrefs++]));
  return queue_pjob(env, j, "g16_plonk_prove");
}

static napi_value js_plonk_destroy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  phandle_t* h = NULL;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc >= 1 && napi_get_value_external(env, argv[0], (void**)&h) == napi_ok && h && h->p) {
    h->closing = 1;
    if (h->inflight == 0) { g16_plonk_destroy(h->p); h->p = NULL; }
  }
  return NULL;
}

/* plonk setup from / to files (the inputs may exceed a Buffer) */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  char r1cs[1024], ptau[1024], zkey[1024];
  int device, lagrange, rc;
  int groth16;   /* 1: g16_groth16_setup_files (groth16SetupFiles) */
  int prepare;   /* 1: g16_ptau_prepare_files (ptauPrepareFiles): ptau = input, zkey = output */
  int cshash;    /* 1: g16_zkey_new_files (zkeyNewFiles); 2: g16_zkey_cs_hash_files (zkeyCsHashFiles): zkey = input.  Resolve with hash */
  uint8_t hash[64];
  char err[512];
} sjob_t;
static void sjob_execute(napi_env env, void* data) {
  sjob_t* j = (sjob_t*)data;
  j->rc = j->cshash == 1 ? g16_zkey_new_files(j->r1cs, j->ptau, j->zkey, j->device, j->hash)
          : j->cshash  ? g16_zkey_cs_hash_files(j->zkey, j->ptau, j->device, j->hash)
          : j->prepare ? g16_ptau_prepare_files(j->ptau, j->zkey, j->device)
          : j->groth16 ? g16_groth16_setup_files(j->r1cs, j->ptau, j->zkey, j->device)
                       : g16_plonk_setup_files(j->r1cs, j->ptau, j->zkey, j->device, j->lagrange);
  if (j->rc) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
}
static void sjob_complete(napi_env env, napi_status status, void* data) {
  sjob_t* j = (sjob_t*)data;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->rc ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->cshash) {
    napi_value buf;
    void* q = NULL;
    if (napi_create_buffer_copy(env, 64, j->hash, &q, &buf) == napi_ok) napi_resolve_deferred(env, j->deferred, buf);
    else {
      napi_value msg, err;
      napi_create_string_utf8(env, "g16 addon: cannot create the hash buffer", NAPI_AUTO_LENGTH, &msg);
      napi_create_error(env, NULL, msg, &err);
      napi_reject_deferred(env, j->deferred, err);
    }
  } else {
    napi_value undef;
    napi_get_undefined(env, &undef);
    napi_resolve_deferred(env, j->deferred, undef);
  }
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value js_plonk_setup_files(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5], promise, resname;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) { napi_throw_type_error(env, NULL, "plonkSetupFiles(r1csPath, ptauPath, zkeyPath, device, withLagrange)"); return NULL; }
  sjob_t* j = (sjob_t*)calloc(1, sizeof(sjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->r1cs, sizeof(j->r1cs), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->ptau, sizeof(j->ptau), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[2], j->zkey, sizeof(j->zkey), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "plonkSetupFiles: three path strings expected");
    return NULL;
  }
  int32_t v = 0;
  if (argc > 3 && napi_get_value_int32(env, argv[3], &v) == napi_ok) j->device = v;
  v = 0;
  if (argc > 4 && napi_get_value_int32(env, argv[4], &v) == napi_ok) j->lagrange = v;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_plonk_setup_files", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, sjob_execute, sjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* groth16 setup from / to files: the same async job as plonkSetupFiles */
static napi_value js_groth16_setup_files(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], promise, resname;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) { napi_throw_type_error(env, NULL, "groth16SetupFiles(r1csPath, ptauPath, zkeyPath, device)"); return NULL; }
  sjob_t* j = (sjob_t*)calloc(1, sizeof(sjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->r1cs, sizeof(j->r1cs), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->ptau, sizeof(j->ptau), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[2], j->zkey, sizeof(j->zkey), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "groth16SetupFiles: three path strings expected");
    return NULL;
  }
  j->groth16 = 1;
  int32_t v = 0;
  if (argc > 3 && napi_get_value_int32(env, argv[3], &v) == napi_ok) j->device = v;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_groth16_setup_files", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, sjob_execute, sjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* zkey new with the circuit hash, and the hash of an initial key alone: the same async job, resolved with the 64 bytes */
static napi_value js_zkey_new_files(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], promise, resname;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) { napi_throw_type_error(env, NULL, "zkeyNewFiles(r1csPath, ptauPath, zkeyPath, device)"); return NULL; }
  sjob_t* j = (sjob_t*)calloc(1, sizeof(sjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->r1cs, sizeof(j->r1cs), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->ptau, sizeof(j->ptau), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[2], j->zkey, sizeof(j->zkey), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "zkeyNewFiles: three path strings expected");
    return NULL;
  }
  j->cshash = 1;
  int32_t v = 0;
  if (argc > 3 && napi_get_value_int32(env, argv[3], &v) == napi_ok) j->device = v;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_zkey_new_files", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, sjob_execute, sjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}
static napi_value js_zkey_cs_hash_files(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], promise, resname;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) { napi_throw_type_error(env, NULL, "zkeyCsHashFiles(zkeyPath, ptauPath, device)"); return NULL; }
  sjob_t* j = (sjob_t*)calloc(1, sizeof(sjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->zkey, sizeof(j->zkey), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->ptau, sizeof(j->ptau), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "zkeyCsHashFiles: two path strings expected");
    return NULL;
  }
  j->cshash = 2;
  int32_t v = 0;
  if (argc > 2 && napi_get_value_int32(env, argv[2], &v) == napi_ok) j->device = v;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_zkey_cs_hash_files", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, sjob_execute, sjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* powersoftau prepare phase2 from / to files: the same async job */
static napi_value js_ptau_prepare_files(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], promise, resname;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) { napi_throw_type_error(env, NULL, "ptauPrepareFiles(inPath, outPath, device)"); return NULL; }
  sjob_t* j = (sjob_t*)calloc(1, sizeof(sjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->ptau, sizeof(j->ptau), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->zkey, sizeof(j->zkey), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "ptauPrepareFiles: two path strings expected");
    return NULL;
  }
  j->prepare = 1;
  int32_t v = 0;
  if (argc > 2 && napi_get_value_int32(env, argv[2], &v) == napi_ok) j->device = v;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_ptau_prepare_files", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, sjob_execute, sjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* zkey contribute / zkey verify frominit from / to files */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  char a[1024], b[1024], c[1024], name[512];
  uint8_t secret[64], hash[64];
  int has_name, has_secret, verify, device, rc, ok;   /* verify: 1 = a init, b zkey; 2 = a init, c ptau, b zkey; 3 = a r1cs, c ptau, b zkey */
  int bellman;   /* 1 = export: a zkey, b mpcparams; 2 = contribute: a challenge, b response; 3 = import: a old, c response, b new */
  char err[512];
} zjob_t;
static void zjob_execute(napi_env env, void* data) {
  zjob_t* j = (zjob_t*)data;
  if (j->bellman) {
    j->rc = j->bellman == 1   ? g16_zkey_export_bellman_files(j->a, j->b, j->device)
            : j->bellman == 2 ? g16_zkey_bellman_contribute_files(j->a, j->b, j->has_secret ? j->secret : NULL, j->device, j->hash)
                              : g16_zkey_import_bellman_files(j->a, j->c, j->b, j->has_name ? j->name : NULL, j->device, &j->ok);
    if (j->rc || (j->bellman == 3 && !j->ok)) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
    return;
  }
  j->rc = j->verify == 3 ? g16_zkey_verify_r1cs_files(j->a, j->c, j->b, j->device, &j->ok)
          : j->verify == 2 ? g16_zkey_verify_from_init_ptau_files(j->a, j->c, j->b, j->device, &j->ok)
          : j->verify ? g16_zkey_verify_from_init_files(j->a, j->b, j->device, &j->ok)
                    : g16_zkey_contribute_files(j->a, j->b, j->has_name ? j->name : NULL, j->has_secret ? j->secret : NULL,
                                                j->device, j->hash);
  if (j->rc || (j->verify && !j->ok)) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
}
static void zjob_complete(napi_env env, napi_status status, void* data) {
  zjob_t* j = (zjob_t*)data;
  const int refused = j->bellman == 3 && !j->ok;   /* a verdict of the import: its text, nothing written */
  if (status != napi_ok || j->rc || refused) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->rc || refused ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->bellman == 1 || j->bellman == 3) {
    napi_value undef;
    napi_get_undefined(env, &undef);
    napi_resolve_deferred(env, j->deferred, undef);
  } else if (j->verify) {
    napi_value obj, ok, reason;
    napi_create_object(env, &obj);
    napi_get_boolean(env, j->ok != 0, &ok);
    napi_create_string_utf8(env, j->ok ? "" : j->err, NAPI_AUTO_LENGTH, &reason);
    napi_set_named_property(env, obj, "ok", ok);
    napi_set_named_property(env, obj, "reason", reason);
    napi_resolve_deferred(env, j->deferred, obj);
  } else {
    napi_value buf;
    void* copy = NULL;
    napi_create_buffer_copy(env, 64, j->hash, &copy, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  }
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value zjob_start(napi_env env, zjob_t* j, const char* resource) {
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, resource, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, zjob_execute, zjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}
static napi_value js_zkey_contribute_files(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) { napi_throw_type_error(env, NULL, "zkeyContributeFiles(inPath, outPath, name, secret, device)"); return NULL; }
  zjob_t* j = (zjob_t*)calloc(1, sizeof(zjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->b, sizeof(j->b), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "zkeyContributeFiles: two path strings expected");
    return NULL;
  }
  if (argc > 2 && napi_get_value_string_utf8(env, argv[2], j->name, sizeof(j->name), &n) == napi_ok) j->has_name = 1;
  bool is_buf = false;
  if (argc > 3 && napi_is_buffer(env, argv[3], &is_buf) == napi_ok && is_buf) {
    void* p = NULL;
    size_t len = 0;
    if (napi_get_buffer_info(env, argv[3], &p, &len) != napi_ok || len != 64) {
      free(j);
      napi_throw_type_error(env, NULL, "zkeyContributeFiles: the secret is a Buffer of 64 bytes (d | s) or null");
      return NULL;
    }
    memcpy(j->secret, p, 64);
    j->has_secret = 1;
  }
  int32_t v = 0;
  if (argc > 4 && napi_get_value_int32(env, argv[4], &v) == napi_ok) j->device = v;
  return zjob_start(env, j, "g16_zkey_contribute_files");
}
/* zkeyExportBellmanFiles(zkeyPath, mpcparamsPath, device) -> undefined
 * zkeyBellmanContributeFiles(challengePath, responsePath, secret, device) -> the 64-byte contribution hash
 * zkeyImportBellmanFiles(oldPath, responsePath, newPath, name, device) -> undefined; a refused response rejects with the verdict's text */
static napi_value zkey_bellman(napi_env env, napi_callback_info info, int mode, const char* usage, const char* resource) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  zjob_t* j = (zjob_t*)calloc(1, sizeof(zjob_t));
  size_t n = 0;
  const size_t npath = mode == 3 ? 3 : 2;
  char* dst[3] = {j->a, mode == 3 ? j->c : j->b, j->b};
  bool bad = argc < npath;
  for (size_t k = 0; !bad && k < npath; k++) bad = napi_get_value_string_utf8(env, argv[k], dst[k], sizeof(j->a), &n) != napi_ok;
  if (bad) {
    free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  j->bellman = mode;
  size_t next = npath;
  if (mode == 3 && argc > next && napi_get_value_string_utf8(env, argv[next], j->name, sizeof(j->name), &n) == napi_ok) j->has_name = 1;
  if (mode == 3) next++;
  bool is_buf = false;
  if (mode == 2) {
    if (argc > next && napi_is_buffer(env, argv[next], &is_buf) == napi_ok && is_buf) {
      void* p = NULL;
      size_t len = 0;
      if (napi_get_buffer_info(env, argv[next], &p, &len) != napi_ok || len != 64) {
        free(j);
        napi_throw_type_error(env, NULL, "zkeyBellmanContributeFiles: the secret is a Buffer of 64 bytes (d | s) or null");
        return NULL;
      }
      memcpy(j->secret, p, 64);
      j->has_secret = 1;
    }
    next++;
  }
  int32_t v = 0;
  if (argc > next && napi_get_value_int32(env, argv[next], &v) == napi_ok) j->device = v;
  return zjob_start(env, j, resource);
}
static napi_value js_zkey_export_bellman_files(napi_env env, napi_callback_info info) {
  return zkey_bellman(env, info, 1, "zkeyExportBellmanFiles(zkeyPath, mpcparamsPath, device): two path strings expected",
                      "g16_zkey_export_bellman_files");
}
static napi_value js_zkey_bellman_contribute_files(napi_env env, napi_callback_info info) {
  return zkey_bellman(env, info, 2, "zkeyBellmanContributeFiles(challengePath, responsePath, secret, device): two path strings expected",
                      "g16_zkey_bellman_contribute_files");
}
static napi_value js_zkey_import_bellman_files(napi_env env, napi_callback_info info) {
  return zkey_bellman(env, info, 3, "zkeyImportBellmanFiles(oldPath, responsePath, newPath, name, device): three path strings expected",
                      "g16_zkey_import_bellman_files");
}
static napi_value js_zkey_verify_from_init_files(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) { napi_throw_type_error(env, NULL, "zkeyVerifyFromInitFiles(initPath, zkeyPath, device)"); return NULL; }
  zjob_t* j = (zjob_t*)calloc(1, sizeof(zjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->b, sizeof(j->b), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "zkeyVerifyFromInitFiles: two path strings expected");
    return NULL;
  }
  j->verify = 1;
  int32_t v = 0;
  if (argc > 2 && napi_get_value_int32(env, argv[2], &v) == napi_ok) j->device = v;
  return zjob_start(env, j, "g16_zkey_verify_from_init_files");
}
/* zkeyVerifyFromInitPtauFiles(initPath, ptauPath, zkeyPath, device) / zkeyVerifyR1csFiles(r1csPath, ptauPath, zkeyPath, device) */
static napi_value zkey_verify_three(napi_env env, napi_callback_info info, int mode, const char* usage, const char* resource) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  zjob_t* j = (zjob_t*)calloc(1, sizeof(zjob_t));
  size_t n = 0;
  if (argc < 3 || napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->c, sizeof(j->c), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[2], j->b, sizeof(j->b), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  j->verify = mode;
  int32_t v = 0;
  if (argc > 3 && napi_get_value_int32(env, argv[3], &v) == napi_ok) j->device = v;
  return zjob_start(env, j, resource);
}
static napi_value js_zkey_verify_from_init_ptau_files(napi_env env, napi_callback_info info) {
  return zkey_verify_three(env, info, 2, "zkeyVerifyFromInitPtauFiles(initPath, ptauPath, zkeyPath, device): three path strings expected",
                           "g16_zkey_verify_from_init_ptau_files");
}
static napi_value js_zkey_verify_r1cs_files(napi_env env, napi_callback_info info) {
  return zkey_verify_three(env, info, 3, "zkeyVerifyR1csFiles(r1csPath, ptauPath, zkeyPath, device): three path strings expected",
                           "g16_zkey_verify_r1cs_files");
}

/* powersoftau new / contribute / verify / export challenge / challenge contribute / import response from / to files */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  char a[1024], b[1024], c[1024], name[512];
  uint8_t secret[192], hash[64];
  /* 0: g16_ptau_new_file(power, a); 1: g16_ptau_contribute_files(a, b, ..); 2: g16_ptau_verify_file(a);
   * 3: g16_ptau_export_challenge_files(a, b); 4: g16_ptau_challenge_contribute_files(a, b, ..);
   * 5: g16_ptau_import_response_files(a, c, b, ..) */
  int mode;
  int has_name, has_secret, device, rc, ok;
  uint32_t power;
  char err[512];
} tjob_t;
static void tjob_execute(napi_env env, void* data) {
  tjob_t* j = (tjob_t*)data;
  if (j->mode == 0) j->rc = g16_ptau_new_file(j->power, j->a);
  else if (j->mode == 1)
    j->rc = g16_ptau_contribute_files(j->a, j->b, j->has_name ? j->name : NULL, j->has_secret ? j->secret : NULL, j->device, j->hash);
  else if (j->mode == 2) j->rc = g16_ptau_verify_file(j->a, j->device, &j->ok);
  else if (j->mode == 3) j->rc = g16_ptau_export_challenge_files(j->a, j->b, j->hash);
  else if (j->mode == 4) j->rc = g16_ptau_challenge_contribute_files(j->a, j->b, j->has_secret ? j->secret : NULL, j->device, j->hash);
  else j->rc = g16_ptau_import_response_files(j->a, j->c, j->b, j->has_name ? j->name : NULL, j->device, j->hash, &j->ok);
  if (j->rc || ((j->mode == 2 || j->mode == 5) && !j->ok)) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
}
static void tjob_complete(napi_env env, napi_status status, void* data) {
  tjob_t* j = (tjob_t*)data;
  if (status != napi_ok || j->rc || (j->mode == 5 && !j->ok)) {
    napi_value msg, err;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else if (j->mode == 2) {
    napi_value obj, ok, reason;
    napi_create_object(env, &obj);
    napi_get_boolean(env, j->ok != 0, &ok);
    napi_create_string_utf8(env, j->ok ? "" : j->err, NAPI_AUTO_LENGTH, &reason);
    napi_set_named_property(env, obj, "ok", ok);
    napi_set_named_property(env, obj, "reason", reason);
    napi_resolve_deferred(env, j->deferred, obj);
  } else if (j->mode != 0) {
    napi_value buf;
    void* copy = NULL;
    napi_create_buffer_copy(env, 64, j->hash, &copy, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  } else {
    napi_value undef;
    napi_get_undefined(env, &undef);
    napi_resolve_deferred(env, j->deferred, undef);
  }
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value tjob_start(napi_env env, tjob_t* j, const char* resource) {
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, resource, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, tjob_execute, tjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}
static napi_value js_ptau_new_file(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tjob_t* j = (tjob_t*)calloc(1, sizeof(tjob_t));
  size_t n = 0;
  if (argc < 2 || napi_get_value_uint32(env, argv[0], &j->power) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->a, sizeof(j->a), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "ptauNewFile(power, outPath)");
    return NULL;
  }
  j->mode = 0;
  return tjob_start(env, j, "g16_ptau_new_file");
}
static napi_value js_ptau_contribute_files(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) { napi_throw_type_error(env, NULL, "ptauContributeFiles(inPath, outPath, name, secret, device)"); return NULL; }
  tjob_t* j = (tjob_t*)calloc(1, sizeof(tjob_t));
  size_t n = 0;
  if (napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->b, sizeof(j->b), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "ptauContributeFiles: two path strings expected");
    return NULL;
  }
  if (argc > 2 && napi_get_value_string_utf8(env, argv[2], j->name, sizeof(j->name), &n) == napi_ok) j->has_name = 1;
  bool is_buf = false;
  if (argc > 3 && napi_is_buffer(env, argv[3], &is_buf) == napi_ok && is_buf) {
    void* p = NULL;
    size_t len = 0;
    if (napi_get_buffer_info(env, argv[3], &p, &len) != napi_ok || len != 192) {
      free(j);
      napi_throw_type_error(env, NULL, "ptauContributeFiles: the secret is a Buffer of 192 bytes (six scalars) or null");
      return NULL;
    }
    memcpy(j->secret, p, 192);
    j->has_secret = 1;
  }
  int32_t v = 0;
  if (argc > 4 && napi_get_value_int32(env, argv[4], &v) == napi_ok) j->device = v;
  j->mode = 1;
  return tjob_start(env, j, "g16_ptau_contribute_files");
}
static napi_value js_ptau_verify_file(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tjob_t* j = (tjob_t*)calloc(1, sizeof(tjob_t));
  size_t n = 0;
  if (argc < 1 || napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "ptauVerifyFile(path, device)");
    return NULL;
  }
  int32_t v = 0;
  if (argc > 1 && napi_get_value_int32(env, argv[1], &v) == napi_ok) j->device = v;
  j->mode = 2;
  return tjob_start(env, j, "g16_ptau_verify_file");
}
/* (inPath, outPath[, third path]) of the challenge / response commands -> a job, or NULL after a thrown TypeError */
static tjob_t* tjob_paths(napi_env env, napi_value* argv, size_t argc, size_t npaths, const char* usage) {
  tjob_t* j = (tjob_t*)calloc(1, sizeof(tjob_t));
  char* dst[3] = {j->a, j->b, j->c};
  size_t n = 0;
  bool ok = argc >= npaths;
  for (size_t k = 0; k < npaths && ok; k++) ok = napi_get_value_string_utf8(env, argv[k], dst[k], 1024, &n) == napi_ok;
  if (!ok) {
    free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  return j;
}
static napi_value js_ptau_export_challenge_files(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tjob_t* j = tjob_paths(env, argv, argc, 2, "ptauExportChallengeFiles(ptauPath, challengePath)");
  if (!j) return NULL;
  j->mode = 3;
  return tjob_start(env, j, "g16_ptau_export_challenge_files");
}
static napi_value js_ptau_challenge_contribute_files(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tjob_t* j = tjob_paths(env, argv, argc, 2, "ptauChallengeContributeFiles(challengePath, responsePath, secret, device)");
  if (!j) return NULL;
  bool is_buf = false;
  if (argc > 2 && napi_is_buffer(env, argv[2], &is_buf) == napi_ok && is_buf) {
    void* p = NULL;
    size_t len = 0;
    if (napi_get_buffer_info(env, argv[2], &p, &len) != napi_ok || len != 192) {
      free(j);
      napi_throw_type_error(env, NULL, "ptauChallengeContributeFiles: the secret is a Buffer of 192 bytes (six scalars) or null");
      return NULL;
    }
    memcpy(j->secret, p, 192);
    j->has_secret = 1;
  }
  int32_t v = 0;
  if (argc > 3 && napi_get_value_int32(env, argv[3], &v) == napi_ok) j->device = v;
  j->mode = 4;
  return tjob_start(env, j, "g16_ptau_challenge_contribute_files");
}
static napi_value js_ptau_import_response_files(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  /* (a = old, b = new, c = response: the job's field order, not the argument order) */
  tjob_t* j = tjob_paths(env, argv, argc, 3, "ptauImportResponseFiles(oldPath, responsePath, newPath, name, device)");
  if (!j) return NULL;
  char tmp[1024];
  memcpy(tmp, j->b, sizeof(tmp)); memcpy(j->b, j->c, sizeof(tmp)); memcpy(j->c, tmp, sizeof(tmp));
  size_t n = 0;
  if (argc > 3 && napi_get_value_string_utf8(env, argv[3], j->name, sizeof(j->name), &n) == napi_ok) j->has_name = 1;
  int32_t v = 0;
  if (argc > 4 && napi_get_value_int32(env, argv[4], &v) == napi_ok) j->device = v;
  j->mode = 5;
  return tjob_start(env, j, "g16_ptau_import_response_files");
}

/* powersoftau beacon / zkey beacon from / to files.  The delay function runs in the worker, off the event loop. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  char a[1024], b[1024], name[512];
  uint8_t beacon[256], hash[64];   /* (a hash of more than 255 bytes is cut to 256: the library refuses it by its length) */
  size_t beacon_len;
  uint32_t exp;
  int zkey, has_name, device, rc;
  char err[512];
} bjob_t;
static void bjob_execute(napi_env env, void* data) {
  bjob_t* j = (bjob_t*)data;
  j->rc = (j->zkey ? g16_zkey_beacon_files : g16_ptau_beacon_files)(j->a, j->b, j->has_name ? j->name : NULL, j->beacon, j->beacon_len,
                                                                     j->exp, j->device, j->hash);
  if (j->rc) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
}
static void bjob_complete(napi_env env, napi_status status, void* data) {
  bjob_t* j = (bjob_t*)data;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value buf;
    void* copy = NULL;
    napi_create_buffer_copy(env, 64, j->hash, &copy, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  }
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value beacon_files(napi_env env, napi_callback_info info, int zkey, const char* usage, const char* resource) {
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bjob_t* j = (bjob_t*)calloc(1, sizeof(bjob_t));
  size_t n = 0, len = 0;
  void* p = NULL;
  bool is_buf = false;
  if (argc < 5 || napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->b, sizeof(j->b), &n) != napi_ok ||
      napi_is_buffer(env, argv[3], &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, argv[3], &p, &len) != napi_ok ||
      napi_get_value_uint32(env, argv[4], &j->exp) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  if (napi_get_value_string_utf8(env, argv[2], j->name, sizeof(j->name), &n) == napi_ok) j->has_name = 1;
  j->beacon_len = len < sizeof(j->beacon) ? len : sizeof(j->beacon);
  if (j->beacon_len) memcpy(j->beacon, p, j->beacon_len);
  int32_t v = 0;
  if (argc > 5 && napi_get_value_int32(env, argv[5], &v) == napi_ok) j->device = v;
  j->zkey = zkey;
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, resource, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, bjob_execute, bjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}
static napi_value js_ptau_beacon_files(napi_env env, napi_callback_info info) {
  return beacon_files(env, info, 0, "ptauBeaconFiles(inPath, outPath, name, beaconHash: Buffer, numIterationsExp, device)", "g16_ptau_beacon_files");
}
static napi_value js_zkey_beacon_files(napi_env env, napi_callback_info info) {
  return beacon_files(env, info, 1, "zkeyBeaconFiles(inPath, outPath, name, beaconHash: Buffer, numIterationsExp, device)", "g16_zkey_beacon_files");
}

/* wtns check from files: the verdict of g16_wtns_check_files (an unsatisfied witness resolves, a malformed file rejects) */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  char a[1024], b[1024];
  int device, rc;
  g16_wtns_verdict v;
  char err[512];
} wjob_t;
static void wjob_execute(napi_env env, void* data) {
  wjob_t* j = (wjob_t*)data;
  j->rc = g16_wtns_check_files(j->a, j->b, j->device, &j->v);
  if (j->rc) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
}
static void wjob_complete(napi_env env, napi_status status, void* data) {
  wjob_t* j = (wjob_t*)data;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value obj, v;
    napi_create_object(env, &obj);
    napi_create_int64(env, j->v.constraint, &v);
    napi_set_named_property(env, obj, "constraint", v);
    napi_create_uint32(env, j->v.n_failed, &v);
    napi_set_named_property(env, obj, "nFailed", v);
    const uint8_t* vals[3] = {j->v.a, j->v.b, j->v.c};
    const char* names[3] = {"a", "b", "c"};
    for (int k = 0; k < 3; k++) {
      void* copy = NULL;
      napi_create_buffer_copy(env, 32, vals[k], &copy, &v);
      napi_set_named_property(env, obj, names[k], v);
    }
    napi_resolve_deferred(env, j->deferred, obj);
  }
  napi_delete_async_work(env, j->work);
  free(j);
}
static napi_value js_wtns_check_files(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  wjob_t* j = (wjob_t*)calloc(1, sizeof(wjob_t));
  size_t n = 0;
  if (argc < 2 || napi_get_value_string_utf8(env, argv[0], j->a, sizeof(j->a), &n) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], j->b, sizeof(j->b), &n) != napi_ok) {
    free(j);
    napi_throw_type_error(env, NULL, "wtnsCheckFiles(r1csPath, wtnsPath, device)");
    return NULL;
  }
  int32_t v = 0;
  if (argc > 2 && napi_get_value_int32(env, argv[2], &v) == napi_ok) j->device = v;
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_wtns_check_files", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, wjob_execute, wjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* wtns calculate.  Both calls are synchronous: a command-line step each (the program of the full circuit takes seconds).
 * nzcpProgramFile(params: number[7] | null, gadget: string | null, gadgetParams: number[], path): the witness program
 * of NZCPPubIdentity(params), or of one template, written to `path`.
 * wtnsCalculate(programPath, names: string[], values: Buffer[], device) -> {status, text, wtns}: values[i] = the words of
 * input names[i] (32 bytes each, little-endian); status -1 and the .wtns image, or the violated check, its text and null. */
static int read_u32_array(napi_env env, napi_value arr, uint32_t* out, uint32_t cap, uint32_t* n) {
  bool is_arr = false;
  if (napi_is_array(env, arr, &is_arr) != napi_ok || !is_arr || napi_get_array_length(env, arr, n) != napi_ok || *n > cap) return 0;
  for (uint32_t i = 0; i < *n; i++) {
    napi_value v;
    if (napi_get_element(env, arr, i, &v) != napi_ok || napi_get_value_uint32(env, v, &out[i]) != napi_ok) return 0;
  }
  return 1;
}
static napi_value js_nzcp_program_file(napi_env env, napi_callback_info info) {
  size_t argc = 4, n = 0;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t params[64], np = 0, gparams[64], ngp = 0;
  char gadget[64] = "", path[1024];
  const int whole = argc > 0 && read_u32_array(env, argv[0], params, 64, &np);
  const int one = argc > 1 && napi_get_value_string_utf8(env, argv[1], gadget, sizeof(gadget), &n) == napi_ok;
  if (argc < 4 || (whole ? np != 7 : !one) || (one && !read_u32_array(env, argv[2], gparams, 64, &ngp)) ||
      napi_get_value_string_utf8(env, argv[3], path, sizeof(path), &n) != napi_ok) {
    napi_throw_type_error(env, NULL, "nzcpProgramFile(params[7] | null, gadget | null, gadgetParams, path)");
    return NULL;
  }
  uint8_t* prog = NULL;
  size_t len = 0;
  const int rc = whole ? g16_nzcp_witness_program(params, &prog, &len) : g16_nzcp_gadget_program(gadget, gparams, ngp, &prog, &len);
  if (rc) { napi_throw_error(env, NULL, g16_last_error()); return NULL; }
  FILE* f = fopen(path, "wb");
  const int ok = f && fwrite(prog, 1, len, f) == len;
  if (f && fclose(f) != 0) { g16_free(prog); napi_throw_error(env, NULL, "nzcp program: cannot write the file"); return NULL; }
  g16_free(prog);
  if (!ok) { napi_throw_error(env, NULL, "nzcp program: cannot write the file"); return NULL; }
  return NULL;
}
/* the witness program at `path` -> a calculator on `device`; msg: why not */
static g16_wtns_calculator* open_calculator(const char* path, int32_t device, char* msg, size_t msg_len) {
  FILE* f = fopen(path, "rb");
  long flen = -1;
  uint8_t* prog = NULL;
  if (f && fseek(f, 0, SEEK_END) == 0 && (flen = ftell(f)) >= 0 && fseek(f, 0, SEEK_SET) == 0 && (prog = (uint8_t*)malloc((size_t)flen + 1)) &&
      fread(prog, 1, (size_t)flen, f) != (size_t)flen) { free(prog); prog = NULL; }
  if (f) fclose(f);
  if (!prog) { snprintf(msg, msg_len, "wtns calculate: cannot read %s", path); return NULL; }
  g16_wtns_calculator* h = NULL;
  const int rc = g16_wtns_calc_create(prog, (size_t)flen, device, &h);
  free(prog);
  if (rc) { snprintf(msg, msg_len, "%s", g16_last_error()); return NULL; }
  return h;
}
/* the named inputs of one pass (names[i], values[i] = its words) -> the program's input words (inf[2] of them, zeroed by
 * the caller); msg: what does not match the program's input table */
static void input_words(napi_env env, g16_wtns_calculator* h, const uint32_t inf[6], napi_value names, napi_value values, uint8_t* words,
                        char* msg, size_t msg_len) {
  char name[256];
  size_t n = 0;
  uint32_t count = 0, nvals = 0;
  uint8_t* seen = (uint8_t*)calloc((size_t)inf[5] + 1, 1);
  if (!seen) { snprintf(msg, msg_len, "wtns calculate: out of memory"); return; }
  if (napi_get_array_length(env, names, &count) != napi_ok || napi_get_array_length(env, values, &nvals) != napi_ok || nvals != count)
    snprintf(msg, msg_len, "wtns calculate: bad input");
  for (uint32_t i = 0; i < count && !msg[0]; i++) {
    napi_value nm, val;
    void* p = NULL;
    size_t len = 0;
    if (napi_get_element(env, names, i, &nm) != napi_ok || napi_get_value_string_utf8(env, nm, name, sizeof(name), &n) != napi_ok ||
        napi_get_element(env, values, i, &val) != napi_ok || napi_get_buffer_info(env, val, &p, &len) != napi_ok) {
      snprintf(msg, msg_len, "wtns calculate: bad input %u", i);
      break;
    }
    uint32_t k = 0, first = 0, cnt = 0;
    const char* have = NULL;
    for (; k < inf[5]; k++)
      if ((have = g16_wtns_calc_input(h, k, &first, &cnt)) && strcmp(have, name) == 0) break;
    if (k == inf[5]) snprintf(msg, msg_len, "wtns calculate: the program has no input %s", name);
    else if (len != (size_t)cnt * 32) snprintf(msg, msg_len, "wtns calculate: input %s takes %u values, %zu given", name, cnt, len / 32);
    else { memcpy(words + (size_t)first * 32, p, len); seen[k] = 1; }
  }
  for (uint32_t k = 0; k < inf[5] && !msg[0]; k++)
    if (!seen[k]) snprintf(msg, msg_len, "wtns calculate: input %s is missing", g16_wtns_calc_input(h, k, NULL, NULL));
  free(seen);
}
static napi_value js_wtns_calculate(napi_env env, napi_callback_info info) {
  size_t argc = 4, n = 0;
  napi_value argv[4], out = NULL, v;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  char path[1024], msg[512];
  uint32_t count = 0, nvals = 0;
  int32_t device = -1;
  if (argc < 3 || napi_get_value_string_utf8(env, argv[0], path, sizeof(path), &n) != napi_ok ||
      napi_get_array_length(env, argv[1], &count) != napi_ok || napi_get_array_length(env, argv[2], &nvals) != napi_ok || nvals != count) {
    napi_throw_type_error(env, NULL, "wtnsCalculate(programPath, names, values, device)");
    return NULL;
  }
  if (argc > 3) napi_get_value_int32(env, argv[3], &device);
  msg[0] = 0;
  g16_wtns_calculator* h = open_calculator(path, device, msg, sizeof(msg));
  if (!h) { napi_throw_error(env, NULL, msg); return NULL; }
  uint32_t inf[6];
  g16_wtns_calc_info(h, inf);
  uint8_t* words = (uint8_t*)calloc((size_t)inf[2] + 1, 32);
  if (words) input_words(env, h, inf, argv[1], argv[2], words, msg, sizeof(msg));
  else snprintf(msg, sizeof(msg), "wtns calculate: out of memory");
  uint32_t status = 0xffffffffu;
  uint8_t* wt = NULL;
  size_t wl = 0;
  if (!msg[0] && g16_wtns_calc_wtns(h, words, inf[2], &status, &wt, &wl)) snprintf(msg, sizeof(msg), "%s", g16_last_error());
  if (!msg[0]) {
    napi_create_object(env, &out);
    napi_create_int64(env, status == 0xffffffffu ? -1 : (int64_t)status, &v);
    napi_set_named_property(env, out, "status", v);
    const char* text = status == 0xffffffffu ? "" : g16_wtns_calc_check_text(h, status);
    napi_create_string_utf8(env, text ? text : "", NAPI_AUTO_LENGTH, &v);
    napi_set_named_property(env, out, "text", v);
    if (wt) { void* copy = NULL; napi_create_buffer_copy(env, wl, wt, &copy, &v); } else napi_get_null(env, &v);
    napi_set_named_property(env, out, "wtns", v);
  }
  g16_free(wt);
  free(words);
  g16_wtns_calc_destroy(h);
  if (msg[0]) { napi_throw_error(env, NULL, msg); return NULL; }
  return out;
}

/* fullProveBatch(plonk, programPath, zkey, names[][], values[][], device, blinding): inputs in, proofs out, the witnesses
 * computed on `device` and proved there from the calculator's chunk buffers (g16_fullprove_batch,
 * g16_plonk_fullprove_batch).  Pass i's inputs are names[i] / values[i], matched against the program's input table as
 * wtnsCalculate matches them.  blinding: count * 64 bytes (r | s; PLONK: count * 288, nine scalars) or null.  Synchronous,
 * like wtnsCalculate.  -> [{status, text, proof, pub}]: status -1 with the proof and public-signal bytes, or the violated
 * check and its text with nulls. */
static napi_value js_full_prove_batch(napi_env env, napi_callback_info info) {
  size_t argc = 7, n = 0;
  napi_value argv[7], out = NULL, v;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  char path[1024], msg[512];
  bool is_plonk = false;
  uint32_t count = 0, nvals = 0;
  int32_t device = 0;
  void *zkey = NULL, *blind = NULL;
  size_t zlen = 0, blen = 0;
  if (argc < 6 || napi_get_value_bool(env, argv[0], &is_plonk) != napi_ok ||
      napi_get_value_string_utf8(env, argv[1], path, sizeof(path), &n) != napi_ok ||
      napi_get_array_length(env, argv[3], &count) != napi_ok || napi_get_array_length(env, argv[4], &nvals) != napi_ok || nvals != count ||
      napi_get_value_int32(env, argv[5], &device) != napi_ok) {
    napi_throw_type_error(env, NULL, "fullProveBatch(plonk, programPath, zkey, names, values, device, blinding)");
    return NULL;
  }
  bool is_buf = false;   /* (napi_get_buffer_info asserts on a value that is no Buffer in older Node releases) */
  if (napi_is_buffer(env, argv[2], &is_buf) != napi_ok || !is_buf) {
    napi_throw_type_error(env, NULL, "fullProveBatch(plonk, programPath, zkey, names, values, device, blinding)");
    return NULL;
  }
  napi_get_buffer_info(env, argv[2], &zkey, &zlen);
  if (argc > 6 && napi_is_buffer(env, argv[6], &is_buf) == napi_ok && is_buf) napi_get_buffer_info(env, argv[6], &blind, &blen);
  const size_t proof_bytes = is_plonk ? sizeof(g16_plonk_proof) : sizeof(g16_proof);
  if (blind && blen != (size_t)count * (is_plonk ? 288 : 64)) {
    napi_throw_error(env, NULL, "fullprove: the blinding takes 64 bytes per proof (plonk: 288)");
    return NULL;
  }
  msg[0] = 0;
  g16_wtns_calculator* h = open_calculator(path, device, msg, sizeof(msg));
  if (!h) { napi_throw_error(env, NULL, msg); return NULL; }
  uint32_t inf[6];
  g16_wtns_calc_info(h, inf);
  const size_t in_bytes = (size_t)inf[2] * 32, pub_bytes = (size_t)inf[1] * 32;
  uint8_t* words = (uint8_t*)calloc((size_t)count * inf[2] + 1, 32);
  uint8_t* proofs = (uint8_t*)calloc((size_t)count + 1, proof_bytes);
  uint8_t* pub = (uint8_t*)calloc((size_t)count * inf[1] + 1, 32);
  uint32_t* status = (uint32_t*)calloc((size_t)count + 1, 4);
  if (!words || !proofs || !pub || !status) snprintf(msg, sizeof(msg), "fullprove: out of memory");
  for (uint32_t i = 0; i < count && !msg[0]; i++) {
    napi_value nm, val;
    if (napi_get_element(env, argv[3], i, &nm) != napi_ok || napi_get_element(env, argv[4], i, &val) != napi_ok)
      snprintf(msg, sizeof(msg), "wtns calculate: bad input");
    else
      input_words(env, h, inf, nm, val, words + i * in_bytes, msg, sizeof(msg));
  }
  g16_prover* gp = NULL;
  g16_plonk* pp = NULL;
  if (!msg[0]) {
    int rc;
    if (is_plonk) {
      rc = g16_plonk_create((const uint8_t*)zkey, zlen, device, &pp);
      if (!rc) rc = g16_plonk_fullprove_batch(pp, h, words, inf[2], count, (const uint8_t*)blind, (g16_plonk_proof*)proofs, pub, status);
    } else {
      g16_opts o;
      memset(&o, 0, sizeof(o));
      o.device = device;
      o.shard_count = 1;
      rc = g16_create((const uint8_t*)zkey, zlen, &o, &gp);
      if (!rc) rc = g16_fullprove_batch(gp, h, words, inf[2], count, (const uint8_t*)blind, (g16_proof*)proofs, pub, status);
    }
    if (rc) snprintf(msg, sizeof(msg), "%s", g16_last_error());
  }
  if (!msg[0]) {
    napi_create_array_with_length(env, count, &out);
    for (uint32_t i = 0; i < count; i++) {
      napi_value obj;
      void* copy = NULL;
      const int good = status[i] == 0xffffffffu;
      napi_create_object(env, &obj);
      napi_create_int64(env, good ? -1 : (int64_t)status[i], &v);
      napi_set_named_property(env, obj, "status", v);
      const char* text = good ? "" : g16_wtns_calc_check_text(h, status[i]);
      napi_create_string_utf8(env, text ? text : "", NAPI_AUTO_LENGTH, &v);
      napi_set_named_property(env, obj, "text", v);
      if (good) napi_create_buffer_copy(env, proof_bytes, proofs + i * proof_bytes, &copy, &v); else napi_get_null(env, &v);
      napi_set_named_property(env, obj, "proof", v);
      if (good) napi_create_buffer_copy(env, pub_bytes, pub + i * pub_bytes, &copy, &v); else napi_get_null(env, &v);
      napi_set_named_property(env, obj, "pub", v);
      napi_set_element(env, out, i, obj);
    }
  }
  if (gp) g16_destroy(gp);
  if (pp) g16_plonk_destroy(pp);
  g16_wtns_calc_destroy(h);
  free(words); free(proofs); free(pub); free(status);
  if (msg[0]) { napi_throw_error(env, NULL, msg); return NULL; }
  return out;
}

/* ES256 pass signatures, and the combined verdict with the Groth16 proofs: one batch per call, the handles live for the
 * call (the tables of a few keys are built in well under a millisecond on the device).  The inputs are copied: the work
 * runs off the main thread. */
typedef struct {
  napi_async_work work;
  napi_deferred deferred;
  uint8_t* in[6];   /* keys, hashes | proofs, sigs, keyIdx, vkey, pubs */
  size_t len[6];
  uint32_t n_public;
  uint64_t now;
  size_t count;
  uint8_t* out;
  int combined, device, rc;
  char err[512];
} ejob_t;
static void ejob_free(ejob_t* j) {
  for (int k = 0; k < 6; k++) free(j->in[k]);
  free(j->out);
  free(j);
}
static void ejob_execute(napi_env env, void* data) {
  ejob_t* j = (ejob_t*)data;
  g16_es256_verifier* e = NULL;
  g16_verifier* v = NULL;
  const uint32_t* idx = j->len[3] ? (const uint32_t*)j->in[3] : NULL;
  j->rc = g16_es256_verifier_create(j->in[0], (uint32_t)(j->len[0] / 64), j->device, &e);
  if (!j->rc && j->combined) j->rc = g16_verifier_create(j->in[4], j->len[4], j->n_public, 0, j->device, &v);
  if (!j->rc)
    j->rc = j->combined ? g16_nzcp_pass_proof_verify_batch(v, e, (const g16_proof*)j->in[1], j->in[5], j->in[2], idx, j->now, j->count, j->out)
                        : g16_es256_verify_batch(e, j->in[1], j->in[2], idx, j->count, j->out);
  if (j->rc) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
  if (v) g16_verifier_destroy(v);
  if (e) g16_es256_verifier_destroy(e);
}
static void ejob_complete(napi_env env, napi_status status, void* data) {
  ejob_t* j = (ejob_t*)data;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value buf;
    void* copy = NULL;
    napi_create_buffer_copy(env, j->count, j->out, &copy, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  }
  napi_delete_async_work(env, j->work);
  ejob_free(j);
}
/* argv[slot[k]] -> in[k]: a Buffer (copied), or null / undefined where `optional` */
static int ejob_take(napi_env env, ejob_t* j, int k, napi_value v, int optional) {
  bool is_buf = false;
  void* p = NULL;
  size_t len = 0;
  if (napi_is_buffer(env, v, &is_buf) != napi_ok || !is_buf) return optional;
  if (napi_get_buffer_info(env, v, &p, &len) != napi_ok) return 0;
  j->in[k] = (uint8_t*)malloc(len ? len : 1);
  if (!j->in[k]) return 0;
  if (len) memcpy(j->in[k], p, len);
  j->len[k] = len;
  return 1;
}
static napi_value ejob_start(napi_env env, ejob_t* j, const char* usage, const char* resource) {
  j->count = j->len[2] / 64;
  const int sized = j->len[0] % 64 == 0 && j->len[2] == j->count * 64 && (!j->len[3] || j->len[3] == j->count * 4) &&
                    (j->combined ? j->len[1] == j->count * 256 && j->len[5] == j->count * (size_t)j->n_public * 32
                                 : j->len[1] == j->count * 32);
  j->out = (uint8_t*)calloc(j->count ? j->count : 1, 1);
  if (!sized || !j->out) {
    ejob_free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, resource, NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, ejob_execute, ejob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}
static napi_value js_es256_verify_batch(napi_env env, napi_callback_info info) {
  static const char* usage = "es256VerifyBatch(keys: Buffer(n*64), hashes: Buffer(count*32), sigs: Buffer(count*64), keyIdx: Buffer(count*4) | null, device)";
  size_t argc = 5;
  napi_value argv[5];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ejob_t* j = (ejob_t*)calloc(1, sizeof(ejob_t));
  if (!j || argc < 5 || !ejob_take(env, j, 0, argv[0], 0) || !ejob_take(env, j, 1, argv[1], 0) || !ejob_take(env, j, 2, argv[2], 0) ||
      !ejob_take(env, j, 3, argv[3], 1) || napi_get_value_int32(env, argv[4], &j->device) != napi_ok) {
    if (j) ejob_free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  return ejob_start(env, j, usage, "g16_es256_verify_batch");
}
static napi_value js_nzcp_pass_proof_verify(napi_env env, napi_callback_info info) {
  static const char* usage = "nzcpPassProofVerify(vkey: Buffer, nPublic, keys: Buffer(n*64), proofs: Buffer(count*256), pubs: Buffer(count*nPublic*32), sigs: Buffer(count*64), keyIdx: Buffer(count*4) | null, now, device)";
  size_t argc = 9;
  napi_value argv[9];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ejob_t* j = (ejob_t*)calloc(1, sizeof(ejob_t));
  double now = 0;
  if (!j || argc < 9 || !ejob_take(env, j, 4, argv[0], 0) || napi_get_value_uint32(env, argv[1], &j->n_public) != napi_ok ||
      !ejob_take(env, j, 0, argv[2], 0) || !ejob_take(env, j, 1, argv[3], 0) || !ejob_take(env, j, 5, argv[4], 0) ||
      !ejob_take(env, j, 2, argv[5], 0) || !ejob_take(env, j, 3, argv[6], 1) || napi_get_value_double(env, argv[7], &now) != napi_ok ||
      now < 0 || napi_get_value_int32(env, argv[8], &j->device) != napi_ok) {
    if (j) ejob_free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  j->combined = 1;
  j->now = (uint64_t)now;
  return ejob_start(env, j, usage, "g16_nzcp_pass_proof_verify_batch");
}

/* Passes from their URIs: one g16_pass_verify_batch per call, the handle lives for the call.  in[0] keys, in[1] the key
 * names ("iss\0kid\0" per key), in[2] the URI text, in[3] the count + 1 offsets (u64 LE); out: count g16_pass_result. */
static void passjob_execute(napi_env env, void* data) {
  ejob_t* j = (ejob_t*)data;
  const uint32_t n_keys = (uint32_t)(j->len[0] / 64);
  const char* iss[16];
  const char* kid[16];
  const char* p = (const char*)j->in[1];
  const char* end = p + j->len[1];
  uint32_t k = 0;
  for (; k < n_keys && k < 16 && p < end; k++) {
    iss[k] = p;
    p += strlen(p) + 1;
    if (p >= end) break;
    kid[k] = p;
    p += strlen(p) + 1;
  }
  g16_pass_verifier* v = NULL;
  if (k != n_keys || n_keys > 16) {
    j->rc = -1;
    strcpy(j->err, "passVerifyBatch: one iss and one kid per key, at most 16 keys");
    return;
  }
  j->rc = g16_pass_verifier_create(j->in[0], iss, kid, n_keys, j->device, &v);
  if (!j->rc) j->rc = g16_pass_verify_batch(v, j->in[2], (const uint64_t*)j->in[3], j->count, (int64_t)j->now, (g16_pass_result*)j->out);
  if (j->rc) { strncpy(j->err, g16_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
  if (v) g16_pass_verifier_destroy(v);
}
static void passjob_complete(napi_env env, napi_status status, void* data) {
  ejob_t* j = (ejob_t*)data;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, status == napi_ok ? j->err : "g16 addon: async work cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_value buf;
    void* copy = NULL;
    napi_create_buffer_copy(env, j->count * sizeof(g16_pass_result), j->out, &copy, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  }
  napi_delete_async_work(env, j->work);
  ejob_free(j);
}
static napi_value js_pass_verify_batch(napi_env env, napi_callback_info info) {
  static const char* usage = "passVerifyBatch(keys: Buffer(n*64), names: Buffer('iss\\0kid\\0' per key), text: Buffer, offsets: Buffer((count+1)*8, u64 LE), now, device)";
  size_t argc = 6;
  napi_value argv[6];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ejob_t* j = (ejob_t*)calloc(1, sizeof(ejob_t));
  double now = 0;
  int ok = j && argc >= 6 && ejob_take(env, j, 0, argv[0], 0) && ejob_take(env, j, 1, argv[1], 0) && ejob_take(env, j, 2, argv[2], 0) &&
           ejob_take(env, j, 3, argv[3], 0) && napi_get_value_double(env, argv[4], &now) == napi_ok &&
           napi_get_value_int32(env, argv[5], &j->device) == napi_ok;
  /* the names end with a NUL, the offsets are whole words that ascend and stay inside the text */
  if (ok) ok = j->len[0] % 64 == 0 && j->len[1] > 0 && j->in[1][j->len[1] - 1] == 0 && j->len[3] >= 8 && j->len[3] % 8 == 0;
  if (ok) {
    j->count = j->len[3] / 8 - 1;
    uint64_t prev = 0, cur = 0;
    for (size_t i = 0; i <= j->count && ok; i++, prev = cur) {
      memcpy(&cur, j->in[3] + i * 8, 8);
      ok = cur >= prev && cur <= j->len[2];
    }
    j->out = (uint8_t*)calloc(j->count ? j->count : 1, sizeof(g16_pass_result));
    ok = ok && j->out;
  }
  if (!ok) {
    if (j) ejob_free(j);
    napi_throw_type_error(env, NULL, usage);
    return NULL;
  }
  j->now = (uint64_t)(int64_t)now;
  napi_value promise, resname;
  NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
  NAPI_OK(napi_create_string_utf8(env, "g16_pass_verify_batch", NAPI_AUTO_LENGTH, &resname));
  NAPI_OK(napi_create_async_work(env, NULL, resname, passjob_execute, passjob_complete, j, &j->work));
  NAPI_OK(napi_queue_async_work(env, j->work));
  return promise;
}

/* passProveBatch(plonk, programPath, zkey, keys, names, text, offsets, now, flags, device, blinding): pass URIs in, proofs
 * out (g16_pass_fullprove_batch, g16_plonk_pass_fullprove_batch): the three handles live for the call; keys / names / text /
 * offsets as passVerifyBatch takes them; blinding as fullProveBatch.  Synchronous, like fullProveBatch.
 * -> [{outcome, check, text, record: Buffer(96), proof, pub}]: proof and pub are null unless outcome is 0. */
static napi_value js_pass_prove_batch(napi_env env, napi_callback_info info) {
  static const char* usage = "passProveBatch(plonk, programPath, zkey, keys: Buffer(n*64), names: Buffer('iss\\0kid\\0' per key), text: Buffer, offsets: Buffer((count+1)*8, u64 LE), now, flags, device, blinding)";
  size_t argc = 11, n = 0;
  napi_value argv[11], out = NULL, v;
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  char path[1024], msg[512];
  bool is_plonk = false, is_buf = false;
  int32_t device = 0;
  uint32_t flags = 0;
  double now = 0;
  void* buf[5] = {NULL, NULL, NULL, NULL, NULL};   /* zkey, keys, names, text, offsets */
  size_t len[5] = {0, 0, 0, 0, 0};
  void* blind = NULL;
  size_t blen = 0;
  int ok = argc >= 10 && napi_get_value_bool(env, argv[0], &is_plonk) == napi_ok &&
           napi_get_value_string_utf8(env, argv[1], path, sizeof(path), &n) == napi_ok &&
           napi_get_value_double(env, argv[7], &now) == napi_ok && napi_get_value_uint32(env, argv[8], &flags) == napi_ok &&
           napi_get_value_int32(env, argv[9], &device) == napi_ok;
  for (int k = 0; k < 5 && ok; k++) {
    ok = napi_is_buffer(env, argv[2 + k], &is_buf) == napi_ok && is_buf;
    if (ok) napi_get_buffer_info(env, argv[2 + k], &buf[k], &len[k]);
  }
  /* the names end with a NUL, the offsets are whole words that ascend and stay inside the text */
  if (ok) ok = len[1] % 64 == 0 && len[1] / 64 <= 16 && len[2] > 0 && ((const char*)buf[2])[len[2] - 1] == 0 && len[4] >= 8 && len[4] % 8 == 0;
  const size_t count = ok ? len[4] / 8 - 1 : 0;
  uint64_t prev = 0, cur = 0;
  for (size_t i = 0; i <= count && ok; i++, prev = cur) {
    memcpy(&cur, (const uint8_t*)buf[4] + i * 8, 8);
    ok = cur >= prev && cur <= len[3];
  }
  const uint32_t n_keys = (uint32_t)(len[1] / 64);
  const char* iss[16];
  const char* kid[16];
  uint32_t k = 0;
  if (ok) {
    const char* p = (const char*)buf[2];
    const char* end = p + len[2];
    for (; k < n_keys && p < end; k++) {
      iss[k] = p;
      p += strlen(p) + 1;
      if (p >= end) break;
      kid[k] = p;
      p += strlen(p) + 1;
    }
    ok = k == n_keys;
  }
  if (!ok) { napi_throw_type_error(env, NULL, usage); return NULL; }
  if (argc > 10 && napi_is_buffer(env, argv[10], &is_buf) == napi_ok && is_buf) napi_get_buffer_info(env, argv[10], &blind, &blen);
  const size_t proof_bytes = is_plonk ? sizeof(g16_plonk_proof) : sizeof(g16_proof);
  if (blind && blen != count * (is_plonk ? 288 : 64)) {
    napi_throw_error(env, NULL, "pass prove: the blinding takes 64 bytes per proof (plonk: 288)");
    return NULL;
  }
  msg[0] = 0;
  g16_wtns_calculator* h = open_calculator(path, device, msg, sizeof(msg));
  if (!h) { napi_throw_error(env, NULL, msg); return NULL; }
  uint32_t inf[6];
  g16_wtns_calc_info(h, inf);
  const size_t pub_bytes = (size_t)inf[1] * 32;
  uint8_t* proofs = (uint8_t*)calloc(count + 1, proof_bytes);
  uint8_t* pub = (uint8_t*)calloc(count * inf[1] + 1, 32);
  g16_pass_prove_result* res = (g16_pass_prove_result*)calloc(count + 1, sizeof(g16_pass_prove_result));
  if (!proofs || !pub || !res) snprintf(msg, sizeof(msg), "pass prove: out of memory");
  g16_prover* gp = NULL;
  g16_plonk* pp = NULL;
  g16_pass_verifier* pv = NULL;
  if (!msg[0]) {
    int rc = g16_pass_verifier_create((const uint8_t*)buf[1], iss, kid, n_keys, device, &pv);
    if (!rc && is_plonk) {
      rc = g16_plonk_create((const uint8_t*)buf[0], len[0], device, &pp);
      if (!rc)
        rc = g16_plonk_pass_fullprove_batch(pp, h, pv, (const uint8_t*)buf[3], (const uint64_t*)buf[4], count, (int64_t)now, flags,
                                            (const uint8_t*)blind, (g16_plonk_proof*)proofs, pub, res);
    } else if (!rc) {
      g16_opts o;
      memset(&o, 0, sizeof(o));
      o.device = device;
      o.shard_count = 1;
      rc = g16_create((const uint8_t*)buf[0], len[0], &o, &gp);
      if (!rc)
        rc = g16_pass_fullprove_batch(gp, h, pv, (const uint8_t*)buf[3], (const uint64_t*)buf[4], count, (int64_t)now, flags,
                                      (const uint8_t*)blind, (g16_proof*)proofs, pub, res);
    }
    if (rc) snprintf(msg, sizeof(msg), "%s", g16_last_error());
  }
  if (!msg[0]) {
    napi_create_array_with_length(env, count, &out);
    for (size_t i = 0; i < count; i++) {
      napi_value obj;
      void* copy = NULL;
      const int done = res[i].outcome == G16_PROVE_DONE;
      napi_create_object(env, &obj);
      napi_create_uint32(env, res[i].outcome, &v);
      napi_set_named_property(env, obj, "outcome", v);
      napi_create_int64(env, res[i].check == 0xffffffffu ? -1 : (int64_t)res[i].check, &v);
      napi_set_named_property(env, obj, "check", v);
      const char* text = res[i].outcome == G16_PROVE_CHECK ? g16_wtns_calc_check_text(h, res[i].check) : "";
      napi_create_string_utf8(env, text ? text : "", NAPI_AUTO_LENGTH, &v);
      napi_set_named_property(env, obj, "text", v);
      napi_create_buffer_copy(env, sizeof(g16_pass_result), &res[i].pass, &copy, &v);
      napi_set_named_property(env, obj, "record", v);
      if (done) napi_create_buffer_copy(env, proof_bytes, proofs + i * proof_bytes, &copy, &v); else napi_get_null(env, &v);
      napi_set_named_property(env, obj, "proof", v);
      if (done) napi_create_buffer_copy(env, pub_bytes, pub + i * pub_bytes, &copy, &v); else napi_get_null(env, &v);
      napi_set_named_property(env, obj, "pub", v);
      napi_set_element(env, out, (uint32_t)i, obj);
    }
  }
  if (gp) g16_destroy(gp);
  if (pp) g16_plonk_destroy(pp);
  if (pv) g16_pass_verifier_destroy(pv);
  g16_wtns_calc_destroy(h);
  free(proofs); free(pub); free(res);
  if (msg[0]) { napi_throw_error(env, NULL, msg); return NULL; }
  return out;
}


static napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"create", NULL, js_create, NULL, NULL, NULL, napi_default, NULL},
      {"prove", NULL, js_prove, NULL, NULL, NULL, napi_default, NULL},
      {"proveBatch", NULL, js_prove_batch, NULL, NULL, NULL, napi_default, NULL},
      {"info", NULL, js_info, NULL, NULL, NULL, napi_default, NULL},
      {"timings", NULL, js_timings, NULL, NULL, NULL, napi_default, NULL},
      {"destroy", NULL, js_destroy, NULL, NULL, NULL, napi_default, NULL},
      {"createVerifier", NULL, js_create_verifier, NULL, NULL, NULL, napi_default, NULL},
      {"verifyBatch", NULL, js_verify_batch, NULL, NULL, NULL, napi_default, NULL},
      {"destroyVerifier", NULL, js_destroy_verifier, NULL, NULL, NULL, napi_default, NULL},
      {"plonkCreate", NULL, js_plonk_create, NULL, NULL, NULL, napi_default, NULL},
      {"plonkProve", NULL, js_plonk_prove, NULL, NULL, NULL, napi_default, NULL},
      {"plonkDestroy", NULL, js_plonk_destroy, NULL, NULL, NULL, napi_default, NULL},
      {"plonkSetupFiles", NULL, js_plonk_setup_files, NULL, NULL, NULL, napi_default, NULL},
      {"groth16SetupFiles", NULL, js_groth16_setup_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyNewFiles", NULL, js_zkey_new_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyCsHashFiles", NULL, js_zkey_cs_hash_files, NULL, NULL, NULL, napi_default, NULL},
      {"ptauPrepareFiles", NULL, js_ptau_prepare_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyContributeFiles", NULL, js_zkey_contribute_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyExportBellmanFiles", NULL, js_zkey_export_bellman_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyBellmanContributeFiles", NULL, js_zkey_bellman_contribute_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyImportBellmanFiles", NULL, js_zkey_import_bellman_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyVerifyFromInitFiles", NULL, js_zkey_verify_from_init_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyVerifyFromInitPtauFiles", NULL, js_zkey_verify_from_init_ptau_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyVerifyR1csFiles", NULL, js_zkey_verify_r1cs_files, NULL, NULL, NULL, napi_default, NULL},
      {"ptauNewFile", NULL, js_ptau_new_file, NULL, NULL, NULL, napi_default, NULL},
      {"ptauContributeFiles", NULL, js_ptau_contribute_files, NULL, NULL, NULL, napi_default, NULL},
      {"ptauBeaconFiles", NULL, js_ptau_beacon_files, NULL, NULL, NULL, napi_default, NULL},
      {"zkeyBeaconFiles", NULL, js_zkey_beacon_files, NULL, NULL, NULL, napi_default, NULL},
      {"ptauVerifyFile", NULL, js_ptau_verify_file, NULL, NULL, NULL, napi_default, NULL},
      {"ptauExportChallengeFiles", NULL, js_ptau_export_challenge_files, NULL, NULL, NULL, napi_default, NULL},
      {"ptauChallengeContributeFiles", NULL, js_ptau_challenge_contribute_files, NULL, NULL, NULL, napi_default, NULL},
      {"ptauImportResponseFiles", NULL, js_ptau_import_response_files, NULL, NULL, NULL, napi_default, NULL},
      {"wtnsCheckFiles", NULL, js_wtns_check_files, NULL, NULL, NULL, napi_default, NULL},
      {"es256VerifyBatch", NULL, js_es256_verify_batch, NULL, NULL, NULL, napi_default, NULL},
      {"nzcpPassProofVerify", NULL, js_nzcp_pass_proof_verify, NULL, NULL, NULL, napi_default, NULL},
      {"passVerifyBatch", NULL, js_pass_verify_batch, NULL, NULL, NULL, napi_default, NULL},
      {"nzcpProgramFile", NULL, js_nzcp_program_file, NULL, NULL, NULL, napi_default, NULL},
      {"wtnsCalculate", NULL, js_wtns_calculate, NULL, NULL, NULL, napi_default, NULL},
      {"fullProveBatch", NULL, js_full_prove_batch, NULL, NULL, NULL, napi_default, NULL},
      {"passProveBatch", NULL, js_pass_prove_batch, NULL, NULL, NULL, napi_default, NULL},
  };
  NAPI_OK(napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props));
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
