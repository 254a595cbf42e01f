"""nzcp-circom_amd -- MI355X-native Groth16 prover for the compiled NZCP circuits.

This Python module is PLUMBING: a ctypes binding over the C ABI of libg16hip.so
(include/g16_prover.h) used by tests/ and bench.py.  The product host is the Node.js shim in
nzcp-circom_amd/js (snarkjs-shaped `groth16.prove`); both sit on the same C ABI.

There is no CPU fallback: `load()` raises if the shared library is missing, and every compute
entry point returns G16_E_NOGPU (raised here as G16Error) when no HIP device is present.
The API mirrors snarkjs 0.4.12 `groth16.prove` (pin /root/reference/yarn.lock:987-1001):
`Prover(zkey).prove(wtns, r, s) -> (proof_dict, public_signals)` with snarkjs's JSON shapes and
error messages.
"""
import ctypes as C
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", os.environ.get("G16_LIB_NAME", "libg16hip.so"))   # (G16_LIB_NAME: A/B of two builds)
PARTIAL_BYTES = 128 * 4 + 256
LAZY_FR_BYTES = 40

_lib = None


class G16Error(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class Opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("shard_rank", C.c_int32), ("shard_count", C.c_int32),
                ("window_bits", C.c_int32), ("task_len", C.c_int32), ("flags", C.c_uint32)]


class Proof(C.Structure):
    _fields_ = [("a", C.c_uint8 * 64), ("b", C.c_uint8 * 128), ("c", C.c_uint8 * 64)]


class PlonkProof(C.Structure):
    _fields_ = ([(k, C.c_uint8 * 64) for k in ("A", "B", "C", "Z", "T1", "T2", "T3")] +
                [(k, C.c_uint8 * 32) for k in ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw", "eval_r")] +
                [("Wxi", C.c_uint8 * 64), ("Wxiw", C.c_uint8 * 64)])


class WtnsVerdictC(C.Structure):
    _fields_ = [("constraint", C.c_int64), ("n_failed", C.c_uint32), ("a", C.c_uint8 * 32), ("b", C.c_uint8 * 32),
                ("c", C.c_uint8 * 32)]


class Info(C.Structure):
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain_size", C.c_uint32),
                ("n_coefs", C.c_uint32), ("n_a", C.c_uint32), ("n_b1", C.c_uint32),
                ("n_b2", C.c_uint32), ("n_c", C.c_uint32), ("n_h", C.c_uint32),
                ("window_bits", C.c_uint32 * 5)]


class Timings(C.Structure):
    _fields_ = [("upload_ms", C.c_float), ("qap_ms", C.c_float), ("ntt_ms", C.c_float),
                ("msm_ms", C.c_float * 5), ("tail_ms", C.c_float), ("total_ms", C.c_float),
                ("msm_accum_kernel_ms", C.c_float * 5)]


class PassResult(C.Structure):
    _fields_ = [("verdict", C.c_uint32), ("key_idx", C.c_uint32), ("tbs_len", C.c_uint32), ("flags", C.c_uint32),
                ("nbf", C.c_int64), ("exp", C.c_int64), ("tbs_sha256", C.c_uint8 * 32), ("cred_subj_sha256", C.c_uint8 * 32)]


class PassProveResult(C.Structure):
    _fields_ = [("outcome", C.c_uint32), ("check", C.c_uint32), ("record", PassResult)]


EXPORTS = ["g16_create", "g16_prove", "g16_prove_batch", "g16_stage_witness", "g16_prove_staged",
           "g16_prove_partial", "g16_prove_finish", "g16_get_info", "g16_get_timings", "g16_destroy",
           "g16_last_error", "g16_fr_fft", "g16_fr_ifft", "g16_fr_batch_mul", "g16_field_op",
           "g16_ec_add", "g16_g1_multiexp", "g16_g2_multiexp", "g16_synth_setup",
           "g16_synth_witness", "g16_free", "g16_finish_host", "g16_shard_range", "g16_r1cs_setup",
           "g16_sha256_chain_setup", "g16_sha256_message_setup", "g16_nzcp_fixed_layout_setup",
           "g16_f29_op", "g16_x29_op", "g16_qap_eval", "g16_shard_begin", "g16_shard_end",
           "g16_multi_create", "g16_multi_prove", "g16_multi_get_info", "g16_multi_destroy",
           "g16_nzcp_gadget", "g16_nzcp_circuit_setup", "g16_setup_device",
           "g16_verifier_create", "g16_verify_batch", "g16_verifier_timings", "g16_verifier_destroy", "g16_pairing_op",
           "g16_plonk_create", "g16_plonk_prove", "g16_plonk_get_info", "g16_plonk_destroy", "g16_plonk_setup", "g16_plonk_timings", "g16_plonk_setup_ptau", "g16_plonk_setup_files",
           "g16_plonk_verifier_create", "g16_plonk_verify_batch", "g16_plonk_verifier_destroy",
           "g16_groth16_setup_ptau", "g16_groth16_setup_files", "g16_r1cs_setup_trapdoor", "g16_ptau_synth",
           "g16_ptau_prepare", "g16_ptau_prepare_files",
           "g16_zkey_contribute", "g16_zkey_contribute_files", "g16_zkey_verify_from_init",
           "g16_zkey_verify_from_init_files", "g16_blake2b512", "g16_zkey_hash_to_g2",
           "g16_zkey_verify_from_init_ptau", "g16_zkey_verify_from_init_ptau_files", "g16_zkey_verify_r1cs",
           "g16_zkey_verify_r1cs_files", "g16_zkey_h_scalars",
           "g16_zkey_export_bellman", "g16_zkey_export_bellman_files", "g16_zkey_bellman_contribute",
           "g16_zkey_bellman_contribute_files", "g16_zkey_import_bellman", "g16_zkey_import_bellman_files", "g16_zkey_h_basis",
           "g16_ptau_new", "g16_ptau_new_file", "g16_ptau_contribute", "g16_ptau_contribute_files", "g16_ptau_verify",
           "g16_ptau_verify_file", "g16_ptau_secret_from_text",
           "g16_ptau_export_challenge", "g16_ptau_export_challenge_files", "g16_ptau_challenge_contribute",
           "g16_ptau_challenge_contribute_files", "g16_ptau_import_response", "g16_ptau_import_response_files",
           "g16_ptau_points_from_be", "g16_ptau_points_compress", "g16_ptau_points_decompress", "g16_fq_sqrt_batch",
           "g16_r1cs_checker_create", "g16_wtns_check", "g16_wtns_check_batch", "g16_wtns_check_files",
           "g16_r1cs_checker_timings", "g16_r1cs_checker_destroy",
           "g16_nzcp_witness_program", "g16_nzcp_gadget_program", "g16_nzcp_inputs", "g16_wtns_calc_create", "g16_wtns_calc",
           "g16_wtns_calc_check_text", "g16_wtns_calc_wtns", "g16_wtns_calc_info", "g16_wtns_calc_outputs",
           "g16_wtns_calc_input", "g16_wtns_calc_timings", "g16_wtns_calc_destroy", "g16_stage_inputs",
           "g16_fullprove_batch", "g16_plonk_fullprove_batch",
           "g16_beacon_scalars", "g16_ptau_beacon", "g16_ptau_beacon_files", "g16_zkey_beacon", "g16_zkey_beacon_files",
           "g16_zkey_new", "g16_zkey_new_files", "g16_zkey_cs_hash", "g16_zkey_cs_hash_files", "g16_zkey_h_monomial",
           "g16_blake2b512_parts",
           "g16_es256_verifier_create", "g16_es256_verify_batch", "g16_es256_verifier_timings", "g16_es256_verifier_destroy",
           "g16_p256_op", "g16_nzcp_pass_proof_verify_batch",
           "g16_pass_verifier_create", "g16_pass_verify_batch", "g16_pass_verifier_timings", "g16_pass_verifier_destroy",
           "g16_pass_op",
           "g16_pass_fullprove_batch", "g16_plonk_pass_fullprove_batch", "g16_pass_inputs", "g16_pass_wtns_public"]


def load():
    """dlopen libg16hip.so; fails loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise G16Error(-4, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(LIB_PATH)
    u8p, sz, vp = C.POINTER(C.c_uint8), C.c_size_t, C.c_void_p
    lib.g16_last_error.restype = C.c_char_p
    lib.g16_create.argtypes = [C.c_char_p, sz, C.POINTER(Opts), C.POINTER(vp)]
    lib.g16_prove.argtypes = [vp, C.c_char_p, sz, C.c_char_p, C.c_char_p, C.POINTER(Proof), C.c_char_p]
    lib.g16_stage_witness.argtypes = [vp, C.c_uint32, C.c_char_p, sz]
    lib.g16_prove_staged.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(Proof), C.c_char_p]
    lib.g16_prove_partial.argtypes = [vp, C.c_uint32, C.c_char_p]
    lib.g16_prove_finish.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p,
                                     C.POINTER(Proof), C.c_char_p]
    lib.g16_prove_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.c_char_p,
                                    C.POINTER(Proof), C.c_char_p]
    lib.g16_get_info.argtypes = [vp, C.POINTER(Info)]
    lib.g16_get_timings.argtypes = [vp, C.POINTER(Timings)]
    lib.g16_destroy.argtypes = [vp]
    lib.g16_destroy.restype = None
    lib.g16_fr_fft.argtypes = [C.c_int, C.c_char_p, sz]
    lib.g16_fr_ifft.argtypes = [C.c_int, C.c_char_p, sz]
    lib.g16_fr_batch_mul.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, sz, C.c_int]
    lib.g16_field_op.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, sz]
    lib.g16_ec_add.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, sz]
    lib.g16_f29_op.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz]
    lib.g16_x29_op.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz]
    lib.g16_qap_eval.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.g16_shard_begin.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    lib.g16_shard_end.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.c_char_p]
    lib.g16_nzcp_gadget.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32,
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.g16_nzcp_circuit_setup.argtypes = [C.POINTER(C.c_uint32), C.c_char_p, C.c_uint32, C.c_uint64, C.c_int] + \
        [C.c_void_p] * 8 + [C.POINTER(C.c_uint32)]
    lib.g16_multi_create.argtypes = [C.c_char_p, sz, C.POINTER(C.c_int32), C.c_uint32, C.POINTER(Opts), C.POINTER(vp)]
    lib.g16_multi_prove.argtypes = [vp, C.c_char_p, sz, C.c_char_p, C.c_char_p, C.POINTER(Proof), C.c_char_p]
    lib.g16_multi_get_info.argtypes = [vp, C.POINTER(Info), C.POINTER(C.c_uint32)]
    lib.g16_multi_destroy.argtypes = [vp]
    lib.g16_multi_destroy.restype = None
    lib.g16_g1_multiexp.argtypes = [C.c_int, C.c_char_p, C.c_char_p, sz, C.c_int, C.c_char_p]
    lib.g16_g2_multiexp.argtypes = [C.c_int, C.c_char_p, C.c_char_p, sz, C.c_int, C.c_char_p]
    lib.g16_synth_setup.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int,
                                    C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz),
                                    C.POINTER(vp), C.POINTER(sz)]
    lib.g16_synth_witness.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64,
                                      C.POINTER(vp), C.POINTER(sz)]
    lib.g16_setup_device.argtypes = [C.c_int]
    lib.g16_verifier_create.argtypes = [C.c_char_p, sz, C.c_uint32, C.c_int, C.c_int, C.POINTER(vp)]
    lib.g16_verify_batch.argtypes = [vp, C.c_char_p, C.c_char_p, sz, C.c_char_p]
    lib.g16_verifier_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.g16_verifier_destroy.argtypes = [vp]
    lib.g16_verifier_destroy.restype = None
    lib.g16_pairing_op.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
    lib.g16_plonk_create.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(vp)]
    lib.g16_plonk_prove.argtypes = [vp, C.c_char_p, sz, C.c_char_p, C.POINTER(PlonkProof), C.c_char_p]
    lib.g16_plonk_get_info.argtypes = [vp, C.POINTER(C.c_uint32)]
    lib.g16_plonk_destroy.argtypes = [vp]
    lib.g16_plonk_destroy.restype = None
    lib.g16_plonk_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.g16_plonk_setup.argtypes = [C.c_char_p, sz, C.c_uint64, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_plonk_verifier_create.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(vp)]
    lib.g16_plonk_verify_batch.argtypes = [vp, C.c_char_p, C.c_char_p, sz, C.c_char_p]
    lib.g16_plonk_verifier_destroy.argtypes = [vp]
    lib.g16_plonk_verifier_destroy.restype = None
    lib.g16_plonk_setup_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    lib.g16_plonk_setup_ptau.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_groth16_setup_ptau.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_groth16_setup_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
    lib.g16_r1cs_setup_trapdoor.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp),
                                            C.POINTER(sz)]
    lib.g16_ptau_synth.argtypes = [C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_ptau_prepare.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_ptau_prepare_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.g16_zkey_contribute.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    lib.g16_zkey_contribute_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.g16_zkey_verify_from_init.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_verify_from_init_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_verify_from_init_ptau.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_verify_from_init_ptau_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_verify_r1cs.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_verify_r1cs_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_h_scalars.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p]
    lib.g16_zkey_export_bellman.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_zkey_export_bellman_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.g16_zkey_bellman_contribute.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    lib.g16_zkey_bellman_contribute_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.g16_zkey_import_bellman.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz),
                                            C.POINTER(C.c_int)]
    lib.g16_zkey_import_bellman_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.g16_zkey_h_basis.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_int, C.c_char_p]
    lib.g16_zkey_new.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    lib.g16_zkey_new_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.g16_zkey_cs_hash.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_int, C.c_char_p]
    lib.g16_zkey_cs_hash_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.g16_zkey_h_monomial.argtypes = [C.c_int, C.c_char_p, C.c_uint32, C.c_char_p]
    lib.g16_blake2b512_parts.argtypes = [C.c_char_p, sz, C.POINTER(sz), sz, C.c_char_p]
    lib.g16_ptau_new.argtypes = [C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_ptau_new_file.argtypes = [C.c_uint32, C.c_char_p]
    lib.g16_ptau_contribute.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    lib.g16_ptau_contribute_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.g16_beacon_scalars.argtypes = [C.c_char_p, sz, C.c_uint32, C.c_int, C.c_char_p]
    for fn in (lib.g16_ptau_beacon, lib.g16_zkey_beacon):
        fn.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_char_p, sz, C.c_uint32, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    for fn in (lib.g16_ptau_beacon_files, lib.g16_zkey_beacon_files):
        fn.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, sz, C.c_uint32, C.c_int, C.c_char_p]
    lib.g16_ptau_verify.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(C.c_int)]
    lib.g16_ptau_verify_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int)]
    lib.g16_ptau_secret_from_text.argtypes = [C.c_char_p, C.c_char_p]
    lib.g16_ptau_export_challenge.argtypes = [C.c_char_p, sz, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    lib.g16_ptau_export_challenge_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    lib.g16_ptau_challenge_contribute.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz), C.c_char_p]
    lib.g16_ptau_challenge_contribute_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.g16_ptau_import_response.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(sz),
                                             C.c_char_p, C.POINTER(C.c_int)]
    lib.g16_ptau_import_response_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p,
                                                   C.POINTER(C.c_int)]
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    lib.g16_ptau_points_from_be.argtypes = [C.c_int, C.c_char_p, sz, C.c_int, C.c_char_p, i64p, f32p]
    lib.g16_ptau_points_compress.argtypes = [C.c_int, C.c_char_p, sz, C.c_int, C.c_char_p, i64p, f32p]
    lib.g16_ptau_points_decompress.argtypes = [C.c_int, C.c_char_p, sz, C.c_int, C.c_char_p, C.c_char_p, i64p, f32p]
    lib.g16_fq_sqrt_batch.argtypes = [C.c_int, C.c_char_p, sz, C.c_int, C.c_char_p, C.c_char_p]
    lib.g16_r1cs_checker_create.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(vp)]
    lib.g16_wtns_check.argtypes = [vp, C.c_char_p, sz, C.POINTER(WtnsVerdictC)]
    lib.g16_wtns_check_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.POINTER(WtnsVerdictC)]
    lib.g16_wtns_check_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(WtnsVerdictC)]
    lib.g16_r1cs_checker_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.g16_r1cs_checker_destroy.argtypes = [vp]
    lib.g16_r1cs_checker_destroy.restype = None
    u32p = C.POINTER(C.c_uint32)
    lib.g16_nzcp_witness_program.argtypes = [u32p, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_nzcp_gadget_program.argtypes = [C.c_char_p, u32p, C.c_uint32, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_nzcp_inputs.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p]
    lib.g16_wtns_calc_create.argtypes = [C.c_char_p, sz, C.c_int, C.POINTER(vp)]
    lib.g16_wtns_calc.argtypes = [vp, C.c_char_p, sz, sz, C.c_char_p, u32p]
    lib.g16_wtns_calc_check_text.argtypes = [vp, C.c_uint32]
    lib.g16_wtns_calc_check_text.restype = C.c_char_p
    lib.g16_wtns_calc_wtns.argtypes = [vp, C.c_char_p, sz, u32p, C.POINTER(vp), C.POINTER(sz)]
    lib.g16_wtns_calc_info.argtypes = [vp, u32p]
    lib.g16_wtns_calc_outputs.argtypes = [vp, u32p]
    lib.g16_wtns_calc_input.argtypes = [vp, C.c_uint32, u32p, u32p]
    lib.g16_wtns_calc_input.restype = C.c_char_p
    lib.g16_wtns_calc_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.g16_wtns_calc_destroy.argtypes = [vp]
    lib.g16_wtns_calc_destroy.restype = None
    lib.g16_stage_inputs.argtypes = [vp, C.c_uint32, vp, C.c_char_p, sz, u32p]
    lib.g16_fullprove_batch.argtypes = [vp, vp, C.c_char_p, sz, sz, C.c_char_p, vp, C.c_char_p, u32p]
    lib.g16_plonk_fullprove_batch.argtypes = [vp, vp, C.c_char_p, sz, sz, C.c_char_p, vp, C.c_char_p, u32p]
    lib.g16_blake2b512.argtypes = [C.c_char_p, sz, C.c_char_p]
    lib.g16_zkey_hash_to_g2.argtypes = [C.c_char_p, C.c_char_p]
    lib.g16_r1cs_setup.argtypes = [C.c_char_p, sz, C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
    lib.g16_sha256_chain_setup.argtypes = [C.c_uint32, C.c_char_p, C.c_uint64, C.c_int] + [C.c_void_p] * 8
    lib.g16_sha256_message_setup.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64, C.c_int] + [C.c_void_p] * 8
    lib.g16_nzcp_fixed_layout_setup.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                                C.c_uint32, C.c_uint64, C.c_int] + [C.c_void_p] * 8
    lib.g16_finish_host.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(Proof)]
    lib.g16_shard_range.argtypes = [C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.g16_shard_range.restype = None
    lib.g16_es256_verifier_create.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.POINTER(vp)]
    lib.g16_es256_verify_batch.argtypes = [vp, C.c_char_p, C.c_char_p, u32p, sz, C.c_char_p]
    lib.g16_es256_verifier_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.g16_es256_verifier_destroy.argtypes = [vp]
    lib.g16_es256_verifier_destroy.restype = None
    lib.g16_p256_op.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, sz]
    lib.g16_nzcp_pass_proof_verify_batch.argtypes = [vp, vp, C.c_char_p, C.c_char_p, C.c_char_p, u32p, C.c_uint64, sz, C.c_char_p]
    u64p, strs = C.POINTER(C.c_uint64), C.POINTER(C.c_char_p)
    lib.g16_pass_verifier_create.argtypes = [C.c_char_p, strs, strs, C.c_uint32, C.c_int, C.POINTER(vp)]
    lib.g16_pass_verify_batch.argtypes = [vp, C.c_char_p, u64p, sz, C.c_int64, C.POINTER(PassResult)]
    lib.g16_pass_verifier_timings.argtypes = [vp, C.POINTER(C.c_float)]
    lib.g16_pass_verifier_destroy.argtypes = [vp]
    lib.g16_pass_verifier_destroy.restype = None
    lib.g16_pass_op.argtypes = [C.c_int, C.c_int, C.c_char_p, u64p, sz, C.c_char_p]
    lib.g16_pass_fullprove_batch.argtypes = [vp, vp, vp, C.c_char_p, u64p, sz, C.c_int64, C.c_uint32, C.c_char_p, vp, vp, vp]
    lib.g16_plonk_pass_fullprove_batch.argtypes = lib.g16_pass_fullprove_batch.argtypes
    lib.g16_pass_inputs.argtypes = [C.c_int, C.c_char_p, u64p, sz, C.c_uint32, vp, vp]
    lib.g16_pass_wtns_public.argtypes = [vp, C.c_char_p, u64p, sz, vp, u32p]
    lib.g16_free.argtypes = [vp]
    lib.g16_free.restype = None
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise G16Error(rc, load().g16_last_error().decode("utf-8", "replace"))


def _take(ptr, n):
    """Copy a malloc'd buffer into bytes and free it."""
    # (string_at takes a C int size: a 2^22-constraint zkey is > 2 GiB)
    data = bytes((C.c_char * n.value).from_address(ptr.value)) if n.value else b""
    load().g16_free(ptr)
    return data


# ------------------------------------------------------------------ snarkjs-shaped helpers
def _dec(b):
    return str(int.from_bytes(b, "little"))


def proof_to_obj(pr):
    """g16_proof -> the object snarkjs returns (decimal strings, key order of groth16_prove.js)."""
    a, b, c = bytes(pr.a), bytes(pr.b), bytes(pr.c)

    def g1(x):
        return ["0", "1", "0"] if x == bytes(64) else [_dec(x[:32]), _dec(x[32:]), "1"]
    if b == bytes(128):
        pb = [["0", "0"], ["1", "0"], ["0", "0"]]
    else:
        pb = [[_dec(b[0:32]), _dec(b[32:64])], [_dec(b[64:96]), _dec(b[96:128])], ["1", "0"]]
    return {"pi_a": g1(a), "pi_b": pb, "pi_c": g1(c), "protocol": "groth16", "curve": "bn128"}


def stringify(obj):
    """JSON.stringify(obj, null, 1), what the snarkjs CLI writes to proof.json / public.json."""
    return json.dumps(obj, indent=1, separators=(",", ": "))


class Prover:
    """Resident proving key on one GPU (or one shard of it)."""

    def __init__(self, zkey, device=0, shard_rank=0, shard_count=1, window_bits=0, task_len=0, precomp=0):
        lib = load()
        if isinstance(zkey, (str, os.PathLike)):
            with open(zkey, "rb") as f:
                zkey = f.read()
        self._h = C.c_void_p()
        opts = Opts(device, shard_rank, shard_count, window_bits, task_len, (precomp & 0xff) << 8)
        _check(lib.g16_create(zkey, len(zkey), C.byref(opts), C.byref(self._h)))
        self.info = Info()
        _check(lib.g16_get_info(self._h, C.byref(self.info)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _pub(self):
        return C.create_string_buffer(max(1, self.info.n_public * 32))

    def _unpack(self, pr, pub):
        p = self.info.n_public
        return proof_to_obj(pr), [_dec(pub.raw[i * 32:(i + 1) * 32]) for i in range(p)]

    def prove(self, wtns, r=None, s=None):
        """snarkjs groth16.prove(zkey, wtns) -> (proof, publicSignals); r, s = 32-byte LE or None."""
        if isinstance(wtns, (str, os.PathLike)):
            with open(wtns, "rb") as f:
                wtns = f.read()
        pr, pub = Proof(), self._pub()
        _check(load().g16_prove(self._h, wtns, len(wtns), r, s, C.byref(pr), pub))
        return self._unpack(pr, pub)

    def stage(self, slot, wtns):
        _check(load().g16_stage_witness(self._h, slot, wtns, len(wtns)))

    def stage_inputs(self, slot, calc, inputs):
        """The witness of `inputs` computed on this prover's device into `slot` (WitnessCalculator on the same device):
        -> status (NO_CHECK = staged; else the violated check, and the slot is left unstaged)."""
        words = calc.words(inputs)
        st = C.c_uint32()
        _check(load().g16_stage_inputs(self._h, slot, calc._h, words, len(words) // 32, C.byref(st)))
        return st.value

    def fullprove_batch(self, calc, inputs_list, rs=None):
        """Inputs in, proofs out; the witnesses stay on the device (WitnessCalculator on the same device).  rs: None, or
        one (r, s) pair of 32-byte LE scalars per pass.  -> [(proof, public_bytes, NO_CHECK)], or (None, None, the
        violated check) for a pass whose witness violates one."""
        n, p = len(inputs_list), self.info.n_public * 32
        blob = b"".join(calc.words(x) for x in inputs_list)
        prs = (Proof * max(1, n))()
        pub = C.create_string_buffer(max(1, n * p))
        st = (C.c_uint32 * max(1, n))()
        blind = None if rs is None else b"".join(bytes(r) + bytes(s) for r, s in rs)
        if blind is not None and len(blind) != n * 64:
            raise G16Error(-1, "fullprove: rs takes one (r, s) pair of 32-byte scalars per pass")
        _check(load().g16_fullprove_batch(self._h, calc._h, blob, len(blob) // 32 // n if n else calc.n_inputs, n, blind,
                                          prs, pub, st))
        return [(proof_to_obj(prs[i]), pub.raw[i * p:(i + 1) * p], st[i]) if st[i] == NO_CHECK else (None, None, st[i])
                for i in range(n)]

    def pass_fullprove_batch(self, calc, verifier, uris, now, flags=0, rs=None):
        """Pass URIs in, proofs out (g16_pass_fullprove_batch): the front end and the signature check of
        PassVerifier.verify_batch, the circuit's input words formed on the device, the witnesses and the proofs; calc and
        verifier on this prover's device.  flags: PASS_PROVE_UNSIGNED | PASS_PROVE_MATCH_PUBLIC; rs as for
        fullprove_batch.  -> one dict per pass: outcome (an index of PROVE_OUTCOMES), check, text (the violated check's
        for outcome 3, else None), pass (verify_batch's record), proof and public (bytes) -- both None unless outcome 0."""
        blind = None if rs is None else b"".join(bytes(r) + bytes(s) for r, s in rs)
        if blind is not None and len(blind) != len(uris) * 64:
            raise G16Error(-1, "pass prove: rs takes one (r, s) pair of 32-byte scalars per pass")
        return _pass_prove(load().g16_pass_fullprove_batch, self._h, Proof, proof_to_obj, self.info.n_public, calc, verifier,
                           uris, now, flags, blind)

    def prove_staged(self, slot, r=None, s=None):
        pr, pub = Proof(), self._pub()
        _check(load().g16_prove_staged(self._h, slot, r, s, C.byref(pr), pub))
        return self._unpack(pr, pub)

    def prove_staged_raw(self, slot, r, s, pr, pub):
        """Timed path of bench.py: no Python-side formatting."""
        return load().g16_prove_staged(self._h, slot, r, s, C.byref(pr), pub)

    def prove_partial(self, slot):
        buf = C.create_string_buffer(PARTIAL_BYTES)
        _check(load().g16_prove_partial(self._h, slot, buf))
        return buf.raw

    def prove_finish(self, slot, partials, r=None, s=None):
        pr, pub = Proof(), self._pub()
        blob = b"".join(partials)
        _check(load().g16_prove_finish(self._h, slot, blob, len(partials), r, s, C.byref(pr), pub))
        return self._unpack(pr, pub)

    def shard_begin(self, slot, vec_mask, out_ptrs):
        """Sharded H pipeline, first half: out_ptrs = three addresses (ints; 0 where the mask bit is clear) of
        buffers of domain_size * LAZY_FR_BYTES bytes the device can write (host or device memory)."""
        arr = (C.c_void_p * 3)(*[C.c_void_p(p or None) for p in out_ptrs])
        _check(load().g16_shard_begin(self._h, slot, vec_mask, arr))

    def shard_end(self, slot, slice_ptrs):
        """... second half: the three slices [lo, hi) of this shard's H range -> the partial-sum blob."""
        arr = (C.c_void_p * 3)(*[C.c_void_p(p or None) for p in slice_ptrs])
        buf = C.create_string_buffer(PARTIAL_BYTES)
        _check(load().g16_shard_end(self._h, slot, arr, buf))
        return buf.raw

    def qap_eval(self, slot):
        """buildABC1 of a staged witness -> (A_T, B_T, C_T) as lists of canonical Montgomery(2^256) residues."""
        n = self.info.domain_size
        bufs = [C.create_string_buffer(n * 32) for _ in range(3)]
        _check(load().g16_qap_eval(self._h, slot, *bufs))
        return [[int.from_bytes(b.raw[i * 32:(i + 1) * 32], "little") for i in range(n)] for b in bufs]

    def timings(self):
        t = Timings()
        _check(load().g16_get_timings(self._h, C.byref(t)))
        return {"upload_ms": t.upload_ms, "qap_ms": t.qap_ms, "ntt_ms": t.ntt_ms,
                "msm_ms": list(t.msm_ms), "tail_ms": t.tail_ms, "total_ms": t.total_ms,
                "msm_accum_kernel_ms": list(t.msm_accum_kernel_ms)}


class WtnsVerdict:
    """Verdict of a witness check: ok; constraint = the lowest failing row (-1: none); n_failed = how many rows fail;
    a, b, c = the values A.w, B.w, C.w of that row (ints; 0 when ok); reason = the library's text for a failure."""

    def __init__(self, v, reason=""):
        self.constraint, self.n_failed = int(v.constraint), int(v.n_failed)
        self.ok = self.constraint < 0
        self.a, self.b, self.c = (int.from_bytes(bytes(x), "little") for x in (v.a, v.b, v.c))
        self.reason = "" if self.ok else reason

    def as_dict(self):
        return {k: getattr(self, k) for k in ("ok", "constraint", "n_failed", "a", "b", "c")}

    def __repr__(self):
        return f"WtnsVerdict({self.as_dict()})"


def _verdict_text(v):
    return f"wtns check: constraint {v.constraint} is not satisfied ({v.n_failed} in all)"


class R1csChecker:
    """Resident .r1cs for witness checks (g16_wtns_check): device = a HIP device ordinal, or -1 = host threads."""

    def __init__(self, r1cs, device=0):
        lib = load()
        if isinstance(r1cs, (str, os.PathLike)):
            with open(r1cs, "rb") as f:
                r1cs = f.read()
        self._h = C.c_void_p()
        _check(lib.g16_r1cs_checker_create(r1cs, len(r1cs), device, C.byref(self._h)))

    @staticmethod
    def _bytes(wtns):
        if isinstance(wtns, (str, os.PathLike)):
            with open(wtns, "rb") as f:
                return f.read()
        return bytes(wtns)

    def check(self, wtns):
        """-> WtnsVerdict; a malformed witness raises G16Error with g16_prove's texts."""
        wtns = self._bytes(wtns)
        v = WtnsVerdictC()
        _check(load().g16_wtns_check(self._h, wtns, len(wtns), C.byref(v)))
        return WtnsVerdict(v, _verdict_text(v))

    def check_batch(self, wtns_list):
        """One verdict per witness; a malformed witness K fails the whole call ("witness K: ...")."""
        ws = [self._bytes(w) for w in wtns_list]
        n = len(ws)
        ptrs = (C.c_char_p * max(1, n))(*ws)
        lens = (C.c_size_t * max(1, n))(*[len(w) for w in ws])
        out = (WtnsVerdictC * max(1, n))()
        _check(load().g16_wtns_check_batch(self._h, ptrs, lens, n, out))
        return [WtnsVerdict(out[i], _verdict_text(out[i])) for i in range(n)]

    def timings(self):
        ms = (C.c_float * 2)()
        _check(load().g16_r1cs_checker_timings(self._h, ms))
        return {"upload_ms": ms[0], "kernel_ms": ms[1]}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_r1cs_checker_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


NO_CHECK = 0xffffffff   # the status of a witness that violates no check


def nzcp_witness_program(params):
    """The witness program of NZCPPubIdentity(*params): bytes for WitnessCalculator (takes seconds; keep them)."""
    ptr, n = C.c_void_p(), C.c_size_t()
    _check(load().g16_nzcp_witness_program((C.c_uint32 * 7)(*params), C.byref(ptr), C.byref(n)))
    return _take(ptr, n)


def nzcp_gadget_program(name, params):
    """The witness program of one template of the library (the names and parameters of nzcp_gadget)."""
    ptr, n = C.c_void_p(), C.c_size_t()
    prm = (C.c_uint32 * max(1, len(params)))(*params)
    _check(load().g16_nzcp_gadget_program(name.encode(), prm, len(params), C.byref(ptr), C.byref(n)))
    return _take(ptr, n)


def nzcp_inputs(tbs, max_bytes):
    """The input words of an NZCP witness program for the ToBeSigned bytes: (8 * max_bytes + 1) * 32 bytes."""
    out = C.create_string_buffer((8 * max_bytes + 1) * 32)
    _check(load().g16_nzcp_inputs(bytes(tbs), len(tbs), max_bytes, out))
    return out.raw


class WitnessCalculator:
    """A resident witness program (g16_wtns_calc): device = a HIP device ordinal, or -1 = host threads.  Inputs are
    bytes of 32-byte little-endian words, a list of ints, or a dict of the program's named inputs."""

    def __init__(self, prog, device=0):
        lib = load()
        if isinstance(prog, (str, os.PathLike)):
            with open(prog, "rb") as f:
                prog = f.read()
        self._h = C.c_void_p()
        _check(lib.g16_wtns_calc_create(prog, len(prog), device, C.byref(self._h)))
        info = (C.c_uint32 * 6)()
        _check(lib.g16_wtns_calc_info(self._h, info))
        self.n_wires, self.n_public, self.n_inputs, self.n_levels = info[0], info[1], info[2], info[3]
        outs = (C.c_uint32 * max(1, info[4]))()
        _check(lib.g16_wtns_calc_outputs(self._h, outs))
        self.outputs = list(outs[:info[4]])
        self.inputs = {}
        for i in range(info[5]):
            first, count = C.c_uint32(), C.c_uint32()
            name = lib.g16_wtns_calc_input(self._h, i, C.byref(first), C.byref(count))
            self.inputs[name.decode()] = (first.value, count.value)

    def words(self, inputs):
        if isinstance(inputs, (bytes, bytearray)):
            return bytes(inputs)
        if isinstance(inputs, dict):
            vals = [0] * self.n_inputs
            for name, v in inputs.items():
                if name not in self.inputs:
                    raise G16Error(-1, f"wtns calc: the program has no input {name}")
                first, count = self.inputs[name]
                v = list(v) if isinstance(v, (list, tuple)) else [v]
                if len(v) != count:
                    raise G16Error(-1, f"wtns calc: input {name} takes {count} words, {len(v)} given")
                vals[first:first + count] = [int(x) for x in v]
            inputs = vals
        return b"".join(int(x).to_bytes(32, "little") for x in inputs)

    def calculate_batch(self, inputs_list, want_words=True):
        """-> [(words or None, status)]: words = the n_wires * 32 bytes of a .wtns body (None when not asked for)."""
        blob = b"".join(self.words(x) for x in inputs_list)
        n = len(inputs_list)
        out = C.create_string_buffer(max(1, n * self.n_wires * 32)) if want_words else None
        st = (C.c_uint32 * max(1, n))()
        _check(load().g16_wtns_calc(self._h, blob, len(blob) // 32 // n if n else self.n_inputs, n, out, st))
        w = self.n_wires * 32
        return [(out.raw[i * w:(i + 1) * w] if want_words else None, st[i]) for i in range(n)]

    def calculate(self, inputs, want_words=True):
        """-> (words or None, status); status = NO_CHECK or the lowest violated check (check_text words it)."""
        return self.calculate_batch([inputs], want_words)[0]

    def wtns(self, inputs):
        """The .wtns image; a violated check raises G16Error with the check's text."""
        words = self.words(inputs)
        st, ptr, n = C.c_uint32(), C.c_void_p(), C.c_size_t()
        _check(load().g16_wtns_calc_wtns(self._h, words, len(words) // 32, C.byref(st), C.byref(ptr), C.byref(n)))
        if st.value != NO_CHECK:
            raise G16Error(-5, "constraint not satisfied: " + (self.check_text(st.value) or "?"))
        return _take(ptr, n)

    def check_text(self, k):
        t = load().g16_wtns_calc_check_text(self._h, k)
        return None if t is None else t.decode()

    def timings(self):
        ms = (C.c_float * 3)()
        _check(load().g16_wtns_calc_timings(self._h, ms))
        return {"upload_ms": ms[0], "kernel_ms": ms[1], "download_ms": ms[2]}

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_wtns_calc_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


def wtns_check(r1cs, wtns, device=0):
    """`snarkjs wtns check circuit.r1cs witness.wtns` (later snarkjs; bytes or paths) -> WtnsVerdict."""
    k = R1csChecker(r1cs, device)
    try:
        return k.check(wtns)
    finally:
        k.close()


class MultiProver:
    """One process, several GPUs: one shard of the key per entry of `devices` (g16_multi_*)."""

    def __init__(self, zkey, devices, window_bits=0, task_len=0):
        lib = load()
        self._h = C.c_void_p()
        opts = Opts(0, 0, 1, window_bits, task_len, 0)
        devs = (C.c_int32 * len(devices))(*devices)
        _check(lib.g16_multi_create(zkey, len(zkey), devs, len(devices), C.byref(opts), C.byref(self._h)))
        self.info = Info()
        ns = C.c_uint32()
        _check(lib.g16_multi_get_info(self._h, C.byref(self.info), C.byref(ns)))
        self.n_shards = ns.value

    def prove(self, wtns, r=None, s=None):
        pr, pub = Proof(), C.create_string_buffer(max(1, self.info.n_public * 32))
        _check(load().g16_multi_prove(self._h, wtns, len(wtns), r, s, C.byref(pr), pub))
        p = self.info.n_public
        return proof_to_obj(pr), [_dec(pub.raw[i * 32:(i + 1) * 32]) for i in range(p)]

    def prove_raw(self, wtns, r, s, pr, pub):
        return load().g16_multi_prove(self._h, wtns, len(wtns), r, s, C.byref(pr), pub)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_multi_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


def finish_host(zkey, partials, r, s):
    """Assemble a proof from gathered partial-sum blobs on the host (no GPU handle)."""
    pr = Proof()
    blob = b"".join(partials)
    _check(load().g16_finish_host(zkey, len(zkey), blob, len(partials), r, s, C.byref(pr)))
    return proof_to_obj(pr)


def shard_vector_owner(v, count):
    """Sharded H pipeline: the shard that evaluates vector v (0 = A, 1 = B, 2 = C) on the coset."""
    return v % count


def shard_range(total, rank, count):
    lo, hi = C.c_uint32(), C.c_uint32()
    load().g16_shard_range(total, rank, count, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


# ------------------------------------------------------------------ operator-level (ffjavascript twins)
def fr_fft(buf, inverse=False, device=0):
    out = C.create_string_buffer(bytes(buf), len(buf))
    fn = load().g16_fr_ifft if inverse else load().g16_fr_fft
    _check(fn(device, out, len(buf) // 32))
    return out.raw


def field_op(field, op, a, b, device=0):
    out = C.create_string_buffer(len(a))
    _check(load().g16_field_op(device, field, op, a, b, out, len(a) // 32))
    return out.raw


def ec_add(curve, a, b, device=0):
    psz = 128 if curve == 2 else 64
    out = C.create_string_buffer(len(a))
    _check(load().g16_ec_add(device, curve, a, b, out, len(a) // psz))
    return out.raw


# raw limb images of the kernels' lazy 9 x 29-bit format (layer tests of the arithmetic the hot path runs)
F29_BYTES = 40


def f29_pack(v):
    """int (below 2^293) -> raw F29 image: limbs 0..7 of 29 bits, limb 8 takes the rest, one pad word."""
    out = bytearray(F29_BYTES)
    for i in range(8):
        out[4 * i:4 * i + 4] = ((v >> (29 * i)) & 0x1FFFFFFF).to_bytes(4, "little")
    out[32:36] = (v >> 232).to_bytes(4, "little")
    return bytes(out)


def f29_unpack(b):
    return sum(int.from_bytes(b[4 * i:4 * i + 4], "little") << (29 * i) for i in range(9))


def f29_op(field, op, a, b=None, c=None, d=None, device=0):
    """a..d: lists of ints (values of the lazy elements) -> list of ints."""
    n = len(a)
    enc = [None if v is None else b"".join(f29_pack(x) for x in v) for v in (a, b, c, d)]
    out = C.create_string_buffer(n * F29_BYTES)
    _check(load().g16_f29_op(device, field, op, enc[0], enc[1], enc[2], enc[3], out, n))
    return [f29_unpack(out.raw[i * F29_BYTES:(i + 1) * F29_BYTES]) for i in range(n)]


def x29_op(curve, op, acc, q=None, device=0):
    """acc: list of XYZZ coordinate tuples (4 ints for G1, 4 pairs for G2); q: affine (2) or XYZZ (4) tuples.
    -> (list of XYZZ tuples, list of redo flags)."""
    n = len(acc)

    def enc(pts):
        if pts is None:
            return None
        if curve == 1:
            return b"".join(f29_pack(x) for pt in pts for x in pt)
        return b"".join(f29_pack(x) for pt in pts for co in pt for x in co)
    cb = F29_BYTES * (2 if curve == 2 else 1)
    out = C.create_string_buffer(n * 4 * cb)
    flags = C.create_string_buffer(max(1, n))
    _check(load().g16_x29_op(device, curve, op, enc(acc), enc(q), out, flags, n))
    res = []
    for i in range(n):
        co = []
        for k in range(4):
            raw = out.raw[(4 * i + k) * cb:(4 * i + k + 1) * cb]
            co.append(f29_unpack(raw) if curve == 1 else (f29_unpack(raw[:F29_BYTES]), f29_unpack(raw[F29_BYTES:])))
        res.append(tuple(co))
    return res, list(flags.raw[:n])


def multiexp(curve, bases, scalars, window_bits=0, device=0):
    psz = 128 if curve == 2 else 64
    out = C.create_string_buffer(psz)
    fn = load().g16_g2_multiexp if curve == 2 else load().g16_g1_multiexp
    _check(fn(device, bases, scalars, len(scalars) // 32, window_bits, out))
    return out.raw


# ------------------------------------------------------------------ test-only setup tool
def synth_setup(n_vars, n_public, n_constraints, seed, threads=0):
    """-> (zkey bytes, wtns bytes, vkey bytes)  (host only, no GPU needed)."""
    lib = load()
    z, w, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    zl, wl, vl = C.c_size_t(), C.c_size_t(), C.c_size_t()
    _check(lib.g16_synth_setup(n_vars, n_public, n_constraints, seed, threads, C.byref(z), C.byref(zl),
                               C.byref(w), C.byref(wl), C.byref(v), C.byref(vl)))
    return _take(z, zl), _take(w, wl), _take(v, vl)


def sha256_chain_setup(blocks, msg, seed, threads=0, want_zkey=True, want_r1cs=False, chain=True):
    """SHA-256 chain circuit (chain=True: `blocks` compressions over a 32-byte message) or plain SHA-256 of `msg`
    (chain=False): a real constraint system -> dict(zkey, wtns, vkey, r1cs) of bytes / None."""
    lib = load()
    assert not chain or len(msg) == 32
    ptrs = [C.c_void_p() for _ in range(4)]
    lens = [C.c_size_t() for _ in range(4)]
    want = [want_zkey, True, want_zkey, want_r1cs]
    args = []
    for p_, l_, w_ in zip(ptrs, lens, want):
        args += [C.byref(p_) if w_ else None, C.byref(l_) if w_ else None]
    if chain:
        _check(lib.g16_sha256_chain_setup(blocks, msg, seed, threads, *args))
    else:
        _check(lib.g16_sha256_message_setup(msg, len(msg), seed, threads, *args))
    out = [(_take(p_, l_) if w_ else None) for p_, l_, w_ in zip(ptrs, lens, want)]
    return {"zkey": out[0], "wtns": out[1], "vkey": out[2], "r1cs": out[3]}


def nzcp_fixed_layout_setup(tbs, segs, exp_off, seed, threads=0, want_zkey=True, want_r1cs=False):
    """The NZCP public interface on a fixed pass layout: segs = [(offset, length)] x 3 of givenName, familyName,
    dob inside ToBeSigned; exp_off = offset of the 4 big-endian exp bytes.  -> dict(zkey, wtns, vkey, r1cs)."""
    lib = load()
    ptrs = [C.c_void_p() for _ in range(4)]
    lens = [C.c_size_t() for _ in range(4)]
    want = [want_zkey, True, want_zkey, want_r1cs]
    args = []
    for p_, l_, w_ in zip(ptrs, lens, want):
        args += [C.byref(p_) if w_ else None, C.byref(l_) if w_ else None]
    off = (C.c_uint32 * 3)(*[o for o, _ in segs])
    ln = (C.c_uint32 * 3)(*[n for _, n in segs])
    _check(lib.g16_nzcp_fixed_layout_setup(tbs, len(tbs), off, ln, exp_off, seed, threads, *args))
    out = [(_take(p_, l_) if w_ else None) for p_, l_, w_ in zip(ptrs, lens, want)]
    return {"zkey": out[0], "wtns": out[1], "vkey": out[2], "r1cs": out[3]}


def nzcp_gadget(name, params, inputs, max_out=4096):
    """One template of the NZCP circuit library built natively over `inputs` (the reference's *_test.circom
    twins): -> (outputs, n_constraints); raises G16Error where circom's witness generator would throw."""
    lib = load()
    prm = (C.c_uint32 * max(1, len(params)))(*params)
    inp = (C.c_uint64 * max(1, len(inputs)))(*inputs)
    out = (C.c_uint64 * max_out)()
    nout, ncons = C.c_uint32(max_out), C.c_uint32()
    _check(lib.g16_nzcp_gadget(name.encode(), prm, len(params), inp, len(inputs), out, C.byref(nout), C.byref(ncons)))
    return list(out[:nout.value]), ncons.value


NZCP_EXAMPLE_PARAMS = (0, 314, 0, 4, 2, 4, 5)    # /root/reference/circuits/nzcp_exampleTest.circom
NZCP_LIVE_PARAMS = (1, 355, 0, 4, 2, 4, 6)       # /root/reference/circuits/nzcp_liveTest.circom


def nzcp_circuit_setup(params, tbs, seed, threads=0, want_zkey=True, want_r1cs=False):
    """NZCPPubIdentity(*params) with the CBOR search in the circuit, built natively for the ToBeSigned bytes `tbs`
    -> dict(zkey, wtns, vkey, r1cs, n_constraints)."""
    lib = load()
    ptrs = [C.c_void_p() for _ in range(4)]
    lens = [C.c_size_t() for _ in range(4)]
    want = [want_zkey, True, want_zkey, want_r1cs]
    args = []
    for p_, l_, w_ in zip(ptrs, lens, want):
        args += [C.byref(p_) if w_ else None, C.byref(l_) if w_ else None]
    ncons = C.c_uint32()
    prm = (C.c_uint32 * 7)(*params)
    _check(lib.g16_nzcp_circuit_setup(prm, tbs, len(tbs), seed, threads, *args, C.byref(ncons)))
    out = [(_take(p_, l_) if w_ else None) for p_, l_, w_ in zip(ptrs, lens, want)]
    return {"zkey": out[0], "wtns": out[1], "vkey": out[2], "r1cs": out[3], "n_constraints": ncons.value}


def sha256_message_setup(msg, seed, threads=0, want_zkey=True, want_r1cs=False):
    return sha256_chain_setup(0, msg, seed, threads, want_zkey, want_r1cs, chain=False)


def setup_device(device):
    """Where the fixed-base multiplications of the *_setup builders run: a HIP device ordinal, or -1 = host threads."""
    _check(load().g16_setup_device(int(device)))


def r1cs_setup(r1cs, seed, threads=0):
    """Trapdoor setup of a real .r1cs (bytes) -> (zkey bytes, vkey point bytes)."""
    lib = load()
    z, v = C.c_void_p(), C.c_void_p()
    zl, vl = C.c_size_t(), C.c_size_t()
    _check(lib.g16_r1cs_setup(r1cs, len(r1cs), seed, threads, C.byref(z), C.byref(zl), C.byref(v), C.byref(vl)))
    return _take(z, zl), _take(v, vl)


_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def vkey_json(vkey, n_public):
    """vkey point bytes (alpha1 | beta2 | gamma2 | delta2 | IC[], affine Montgomery LE) -> the
    verification_key.json object snarkjs's `groth16.verify` takes (without the redundant vk_alphabeta_12)."""
    rinv = pow(1 << 256, -1, _Q)

    def fq(b):
        return str(int.from_bytes(b, "little") * rinv % _Q)

    def g1(b):
        return ["0", "1", "0"] if b == bytes(64) else [fq(b[:32]), fq(b[32:64]), "1"]

    def g2(b):
        if b == bytes(128):
            return [["0", "0"], ["1", "0"], ["0", "0"]]
        return [[fq(b[0:32]), fq(b[32:64])], [fq(b[64:96]), fq(b[96:128])], ["1", "0"]]
    return {"protocol": "groth16", "curve": "bn128", "nPublic": n_public,
            "vk_alpha_1": g1(vkey[0:64]), "vk_beta_2": g2(vkey[64:192]), "vk_gamma_2": g2(vkey[192:320]),
            "vk_delta_2": g2(vkey[320:448]),
            "IC": [g1(vkey[448 + 64 * i:512 + 64 * i]) for i in range(n_public + 1)]}


# ------------------------------------------------------------------ verifier (snarkjs groth16.verify, batched)
def _le32(x):
    return (int(x) % (1 << 256)).to_bytes(32, "little")


def proof_from_obj(obj):
    """proof.json object (decimal strings) -> g16_proof bytes (affine standard LE; infinity = zeros)."""
    def g1(t):
        return bytes(64) if str(t[2]) == "0" else _le32(t[0]) + _le32(t[1])
    b = obj["pi_b"]
    pb = bytes(128) if (str(b[2][0]), str(b[2][1])) == ("0", "0") else _le32(b[0][0]) + _le32(b[0][1]) + _le32(b[1][0]) + _le32(b[1][1])
    return g1(obj["pi_a"]) + pb + g1(obj["pi_c"])


def vkey_from_json(vk):
    """verification_key.json object -> (point bytes in STANDARD form, nPublic) for Verifier(..., montgomery=False)."""
    def g1(t):
        return bytes(64) if str(t[2]) == "0" else _le32(t[0]) + _le32(t[1])

    def g2(t):
        if (str(t[2][0]), str(t[2][1])) == ("0", "0"):
            return bytes(128)
        return _le32(t[0][0]) + _le32(t[0][1]) + _le32(t[1][0]) + _le32(t[1][1])
    n_public = int(vk["nPublic"])
    if len(vk["IC"]) != n_public + 1:
        raise G16Error(-2, "verification key: IC length does not match nPublic")
    return (g1(vk["vk_alpha_1"]) + g2(vk["vk_beta_2"]) + g2(vk["vk_gamma_2"]) + g2(vk["vk_delta_2"]) +
            b"".join(g1(t) for t in vk["IC"])), n_public


class Verifier:
    """Resident verification key on one GPU: snarkjs `groth16.verify(vk, publicSignals, proof)` for batches."""

    def __init__(self, vkey, n_public=None, montgomery=True, device=0):
        if isinstance(vkey, dict):
            vkey, n_public = vkey_from_json(vkey)
            montgomery = False
        self.n_public = int(n_public)
        self._h = C.c_void_p()
        _check(load().g16_verifier_create(vkey, len(vkey), self.n_public, 1 if montgomery else 0, device, C.byref(self._h)))

    def verify_raw(self, proofs, pubs, count):
        """proofs: count * 256 bytes of g16_proof; pubs: count * n_public * 32 bytes -> list of bools."""
        ok = C.create_string_buffer(max(1, count))
        _check(load().g16_verify_batch(self._h, proofs, pubs, count, ok))
        return [b != 0 for b in ok.raw[:count]]

    def verify(self, public_signals, proof):
        """One proof: snarkjs's signature (publicSignals as decimal strings / ints, proof as the proof.json object)."""
        if len(public_signals) != self.n_public:
            return False
        return self.verify_raw(proof_from_obj(proof), b"".join(_le32(x) for x in public_signals), 1)[0]

    def verify_batch(self, items):
        """items: [(public_signals, proof_obj)] -> list of bools."""
        bad = [len(ps) != self.n_public for ps, _ in items]
        pr = b"".join(proof_from_obj(p) for _, p in items)
        pub = b"".join(b"".join(_le32(x) for x in (ps if not b else [0] * self.n_public)) for (ps, _), b in zip(items, bad))
        res = self.verify_raw(pr, pub, len(items))
        return [r and not b for r, b in zip(res, bad)]

    def timings(self):
        ms = (C.c_float * 3)()
        _check(load().g16_verifier_timings(self._h, ms))
        return list(ms)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_verifier_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


# ------------------------------------------------------------------ NZCP pass verification (ES256 on NIST P-256)
P256_OPS = {"fp_add": 0, "fp_sub": 1, "fp_mul": 2, "fn_add": 3, "fn_sub": 4, "fn_mul": 5, "fn_inv": 6, "fp_inv": 7,
            "madd": 8, "add": 9, "xcmp": 10}


def p256_op(op, a, b=None, device=0):
    """Layer operator of csrc/p256.cuh (g16_p256_op): `op` a name of P256_OPS; a, b packed big-endian items (32 bytes a
    field value, 64 a point x | y or X | Z); device -1 = host threads.  Returns the packed results."""
    code = P256_OPS[op] if isinstance(op, str) else int(op)
    sa = 64 if code in (8, 9, 10) else 32
    so = 1 if code == 10 else sa
    n = len(a) // sa
    out = C.create_string_buffer(max(1, n * so))
    _check(load().g16_p256_op(device, code, bytes(a), None if b is None else bytes(b), out, n))
    return out.raw[:n * so]


def _key_idx(key_idx, count):
    if key_idx is None:
        return None
    if len(key_idx) != count:
        raise G16Error(-1, "key_idx: one entry per item")
    return (C.c_uint32 * max(1, count))(*key_idx)


class Es256Verifier:
    """Resident ES256 issuer keys (x | y, 64 big-endian bytes each, at most 16) on one GPU, or on host threads with
    device=-1: batches of (SHA-256 digest, r | s) -> one verdict each."""

    def __init__(self, keys, device=0):
        keys = [bytes(k) for k in ([keys] if isinstance(keys, (bytes, bytearray)) else keys)]
        if any(len(k) != 64 for k in keys):
            raise G16Error(-1, "es256 verifier: a key is 64 bytes, x | y")
        self.n_keys = len(keys)
        self._h = C.c_void_p()
        _check(load().g16_es256_verifier_create(b"".join(keys) or b"\0", self.n_keys, device, C.byref(self._h)))

    def verify_batch(self, hashes, sigs, key_idx=None):
        """hashes: count 32-byte digests (a list, or packed); sigs: count 64-byte r | s -> list of bool."""
        hashes = hashes if isinstance(hashes, (bytes, bytearray)) else b"".join(hashes)
        sigs = sigs if isinstance(sigs, (bytes, bytearray)) else b"".join(sigs)
        count = len(sigs) // 64
        if len(sigs) != 64 * count or len(hashes) != 32 * count:
            raise G16Error(-1, "es256 verify: 32 bytes per digest and 64 per signature, as many of each")
        ok = C.create_string_buffer(max(1, count))
        _check(load().g16_es256_verify_batch(self._h, bytes(hashes), bytes(sigs), _key_idx(key_idx, count), count, ok))
        return [b != 0 for b in ok.raw[:count]]

    def timings(self):
        ms = (C.c_float * 2)()
        _check(load().g16_es256_verifier_timings(self._h, ms))
        return list(ms)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_es256_verifier_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


NZCP_VERDICTS = ("ok", "proof rejected", "public signals 0..511 are not all bits", "signature rejected", "expired")


def nzcp_pass_proof_verify(verifier, es, proofs, pubs, sigs, key_idx=None, now=0):
    """The relying party's combined check (g16_nzcp_pass_proof_verify_batch): verifier a Verifier of a 513-signal key,
    es an Es256Verifier on the same device; proofs: proof.json objects or packed g16_proof bytes; pubs: per proof the 513
    public signals (or packed 32-byte LE words); sigs: the 64 bytes r | s of each pass -> verdict codes (NZCP_VERDICTS)."""
    pr = proofs if isinstance(proofs, (bytes, bytearray)) else b"".join(proof_from_obj(p) for p in proofs)
    pb = pubs if isinstance(pubs, (bytes, bytearray)) else b"".join(b"".join(_le32(x) for x in ps) for ps in pubs)
    sg = sigs if isinstance(sigs, (bytes, bytearray)) else b"".join(sigs)
    count = len(sg) // 64
    if len(sg) != 64 * count or len(pr) != 256 * count or len(pb) != 32 * verifier.n_public * count:
        raise G16Error(-1, "nzcp pass proof: as many proofs, public-signal rows and 64-byte signatures")
    out = C.create_string_buffer(max(1, count))
    _check(load().g16_nzcp_pass_proof_verify_batch(verifier._h, es._h, bytes(pr), bytes(pb), bytes(sg), _key_idx(key_idx, count),
                                                   int(now), count, out))
    return list(out.raw[:count])


# ------------------------------------------------------------------ NZCP pass verification from URIs
PASS_VERDICTS = ("ok", "malformed", "alg", "key", "signature", "not yet valid", "expired", "too long")
PASS_HAS_SUBJECT = 1
PASS_URI_MAX = 2048
PASS_OPS = {"base32": 0, "sha256": 1, "front": 2}
_PASS_B32_STRIDE = 4 + PASS_URI_MAX * 5 // 8


def _pass_items(items):
    """texts (str or bytes) -> (packed bytes, the count + 1 offsets)"""
    items = [u.encode("utf-8") if isinstance(u, str) else bytes(u) for u in items]
    offsets = (C.c_uint64 * (len(items) + 1))()
    for i, u in enumerate(items):
        offsets[i + 1] = offsets[i] + len(u)
    return b"".join(items), offsets


def _pass_record(r):
    return {"verdict": r.verdict, "key_idx": r.key_idx, "tbs_len": r.tbs_len, "flags": r.flags, "nbf": r.nbf, "exp": r.exp,
            "tbs_sha256": bytes(r.tbs_sha256), "cred_subj_sha256": bytes(r.cred_subj_sha256)}


def pass_op(op, items, device=0):
    """Layer operator of csrc/nzcp_pass.cuh and csrc/sha256.cuh (g16_pass_op) over a list of items (str or bytes); device
    -1 = host threads.  "base32": the decoded bytes of each item, None where it is not base32; "sha256": the 32-byte
    digests; "front": the front end's records (dicts; no key table, no signature work)."""
    code = PASS_OPS[op] if isinstance(op, str) else int(op)
    text, offsets = _pass_items(items)
    n = len(items)
    stride = {0: _PASS_B32_STRIDE, 1: 32, 2: C.sizeof(PassResult)}.get(code, 1)
    out = (PassResult * max(1, n))() if code == 2 else C.create_string_buffer(max(1, n * stride))
    _check(load().g16_pass_op(device, code, text, offsets, n, C.cast(out, C.c_char_p)))
    if code == 2:
        return [_pass_record(r) for r in out[:n]]
    rows = [out.raw[i * stride:(i + 1) * stride] for i in range(n)]
    if code == 1:
        return rows
    lens = [int.from_bytes(r[:4], "little") for r in rows]
    return [None if k == 0xFFFFFFFF else r[4:4 + k] for r, k in zip(rows, lens)]


PASS_PROVE_UNSIGNED, PASS_PROVE_MATCH_PUBLIC = 1, 2
PROVE_OUTCOMES = ("done", "pass", "too long", "check", "mismatch")


def pass_inputs(uris, max_bytes, device=0):
    """Layer operator g16_pass_inputs: the circuit's input words of each pass, toBeSigned[8 max_bytes] (a bit a word) and
    toBeSignedLen; device -1 = host threads.  -> [(words: (8 max_bytes + 1) * 32 bytes, ok)]; a pass that is not
    well-formed or whose ToBeSigned exceeds max_bytes has a row of zeros and ok False."""
    text, offsets = _pass_items(uris)
    n, row = len(uris), (8 * max_bytes + 1) * 32
    out = C.create_string_buffer(max(1, n * row))
    ok = C.create_string_buffer(max(1, n))
    _check(load().g16_pass_inputs(device, text, offsets, n, max_bytes, out, ok))
    return [(out.raw[i * row:(i + 1) * row], ok.raw[i] != 0) for i in range(n)]


PASS_WTNS_NO_ROW = 0xFFFFFFFE


def pass_wtns_public(calc, uris):
    """g16_pass_wtns_public: the device calculator alone over pass URIs, fed on the device -> [(public bytes, NO_CHECK)],
    (None, the violated check) or (None, PASS_WTNS_NO_ROW) for a pass that pass_inputs gives no row."""
    text, offsets = _pass_items(uris)
    n, p = len(uris), calc.n_public * 32
    pub = C.create_string_buffer(max(1, n * p))
    st = (C.c_uint32 * max(1, n))()
    _check(load().g16_pass_wtns_public(calc._h, text, offsets, n, pub, st))
    return [(pub.raw[i * p:(i + 1) * p], st[i]) if st[i] == NO_CHECK else (None, st[i]) for i in range(n)]


def _pass_prove(fn, handle, proof_type, to_obj, n_public, calc, verifier, uris, now, flags, blind):
    text, offsets = _pass_items(uris)
    n, p = len(uris), n_public * 32
    prs = (proof_type * max(1, n))()
    pub = C.create_string_buffer(max(1, n * p))
    res = (PassProveResult * max(1, n))()
    _check(fn(handle, calc._h, verifier._h, text, offsets, n, int(now), flags, blind, prs, pub, res))
    out = []
    for i in range(n):
        done = res[i].outcome == 0
        out.append({"outcome": res[i].outcome, "check": res[i].check,
                    "text": calc.check_text(res[i].check) if res[i].outcome == 3 else None, "pass": _pass_record(res[i].record),
                    "proof": to_obj(prs[i]) if done else None, "public": pub.raw[i * p:(i + 1) * p] if done else None})
    return out


class PassVerifier:
    """A relying party's offline check of NZ COVID Passes from their URIs (g16_pass_*): keys is the {"<iss>#<kid>": {x, y}}
    object of a DID document's keys (base64url P-256 coordinates, at most 16); on one GPU, or on host threads with
    device=-1.  verify_batch(uris, now) -> one record (dict) per pass: verdict (an index of PASS_VERDICTS), key_idx,
    tbs_len, flags, nbf, exp, tbs_sha256, cred_subj_sha256."""

    def __init__(self, keys, device=0):
        import base64
        names = list(keys)

        def coord(v):
            b = base64.urlsafe_b64decode(v + "=" * (-len(v) % 4))
            if len(b) != 32:
                raise G16Error(-1, "pass verifier: a key coordinate is not 32 bytes")
            return b
        packed = b"".join(coord(keys[n]["x"]) + coord(keys[n]["y"]) for n in names)
        parts = [n.rpartition("#") for n in names]
        arr = C.c_char_p * max(1, len(names))
        iss = arr(*[p[0].encode("utf-8") for p in parts])
        kid = arr(*[p[2].encode("utf-8") for p in parts])
        self.names = names
        self._h = C.c_void_p()
        _check(load().g16_pass_verifier_create(packed or b"\0", iss, kid, len(names), device, C.byref(self._h)))

    def verify_batch(self, uris, now):
        text, offsets = _pass_items(uris)
        out = (PassResult * max(1, len(uris)))()
        _check(load().g16_pass_verify_batch(self._h, text, offsets, len(uris), int(now), out))
        return [_pass_record(r) for r in out[:len(uris)]]

    def timings(self):
        """ms of the last batch: the front end, the scalars, the point sums + compare"""
        ms = (C.c_float * 3)()
        _check(load().g16_pass_verifier_timings(self._h, ms))
        return list(ms)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_pass_verifier_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


_PLONK_G1 = ("A", "B", "C", "Z", "T1", "T2", "T3")
_PLONK_EV = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw", "eval_r")


class PlonkProver:
    """Resident PLONK proving key on one GPU: snarkjs `plonk.prove(zkey, wtns)` -> (proof, publicSignals)."""

    def __init__(self, zkey, device=0):
        if isinstance(zkey, (str, os.PathLike)):
            with open(zkey, "rb") as f:
                zkey = f.read()
        self._h = C.c_void_p()
        _check(load().g16_plonk_create(zkey, len(zkey), device, C.byref(self._h)))
        info = (C.c_uint32 * 6)()
        _check(load().g16_plonk_get_info(self._h, info))
        self.n_vars, self.n_public, self.domain_size, self.n_additions, self.n_constraints, self.levels = list(info)

    def prove_raw(self, wtns, blinding=None):
        pr = PlonkProof()
        pub = C.create_string_buffer(max(1, self.n_public * 32))
        _check(load().g16_plonk_prove(self._h, wtns, len(wtns), blinding, C.byref(pr), pub))
        return pr, pub.raw[:self.n_public * 32]

    def prove(self, wtns, blinding=None):
        """blinding: None, or the nine scalars b1..b9 as ints (reproducible proof)."""
        if blinding is not None and not isinstance(blinding, (bytes, bytearray)):
            blinding = b"".join(int(x).to_bytes(32, "little") for x in blinding)
        pr, pub = self.prove_raw(wtns, blinding)
        return plonk_proof_to_obj(pr), [_dec(pub[i * 32:(i + 1) * 32]) for i in range(self.n_public)]

    def fullprove_batch(self, calc, inputs_list, blindings=None):
        """Inputs in, proofs out; the witnesses stay on the device (WitnessCalculator on the same device).  blindings:
        None, or per pass the nine scalars b1..b9 (ints, or 288 bytes).  -> [(proof, public_bytes, NO_CHECK)], or
        (None, None, the violated check) for a pass whose witness violates one."""
        n, p = len(inputs_list), self.n_public * 32
        blob = b"".join(calc.words(x) for x in inputs_list)
        prs = (PlonkProof * max(1, n))()
        pub = C.create_string_buffer(max(1, n * p))
        st = (C.c_uint32 * max(1, n))()
        blind = None
        if blindings is not None:
            blind = b"".join(bytes(b) if isinstance(b, (bytes, bytearray)) else b"".join(int(x).to_bytes(32, "little") for x in b)
                             for b in blindings)
            if len(blind) != n * 288:
                raise G16Error(-1, "plonk fullprove: blindings takes nine 32-byte scalars per pass")
        _check(load().g16_plonk_fullprove_batch(self._h, calc._h, blob, len(blob) // 32 // n if n else calc.n_inputs, n, blind,
                                                prs, pub, st))
        return [(plonk_proof_to_obj(prs[i]), pub.raw[i * p:(i + 1) * p], st[i]) if st[i] == NO_CHECK else (None, None, st[i])
                for i in range(n)]

    def pass_fullprove_batch(self, calc, verifier, uris, now, flags=0, blindings=None):
        """Prover.pass_fullprove_batch's twin (g16_plonk_pass_fullprove_batch); blindings as for fullprove_batch."""
        blind = None
        if blindings is not None:
            blind = b"".join(bytes(b) if isinstance(b, (bytes, bytearray)) else b"".join(int(x).to_bytes(32, "little") for x in b)
                             for b in blindings)
            if len(blind) != len(uris) * 288:
                raise G16Error(-1, "plonk pass prove: blindings takes nine 32-byte scalars per pass")
        return _pass_prove(load().g16_plonk_pass_fullprove_batch, self._h, PlonkProof, plonk_proof_to_obj, self.n_public, calc,
                           verifier, uris, now, flags, blind)

    def fullprove(self, calc, inputs, blinding=None):
        """snarkjs `plonk.fullProve` -> (proof, publicSignals); a violated check raises G16Error with the check's text."""
        proof, pub, st = self.fullprove_batch(calc, [inputs], None if blinding is None else [blinding])[0]
        if st != NO_CHECK:
            raise G16Error(-5, "constraint not satisfied: " + (calc.check_text(st) or "?"))
        return proof, [_dec(pub[i * 32:(i + 1) * 32]) for i in range(self.n_public)]

    def timings(self):
        ms = (C.c_float * 6)()
        _check(load().g16_plonk_timings(self._h, ms))
        return dict(zip(("witness_round1", "round2", "round3", "round4", "round5", "total"), [round(x, 3) for x in ms]))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_plonk_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


def plonk_proof_from_obj(o):
    """proof.json object of `plonk prove` -> g16_plonk_proof bytes (standard LE)."""
    def g1(t):
        return bytes(64) if str(t[2]) == "0" else _le32(t[0]) + _le32(t[1])
    return (b"".join(g1(o[k]) for k in _PLONK_G1) + b"".join(_le32(o[k]) for k in _PLONK_EV) + g1(o["Wxi"]) + g1(o["Wxiw"]))


def plonk_vkey_bytes(vk):
    """verification_key.json object of a PLONK key -> the C ABI's 712-byte image."""
    def g1(t):
        return bytes(64) if str(t[2]) == "0" else _le32(t[0]) + _le32(t[1])
    x2 = vk["X_2"]
    return (int(vk["power"]).to_bytes(4, "little") + int(vk["nPublic"]).to_bytes(4, "little") + _le32(vk["k1"]) + _le32(vk["k2"]) +
            b"".join(g1(vk[k]) for k in ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")) +
            _le32(x2[0][0]) + _le32(x2[0][1]) + _le32(x2[1][0]) + _le32(x2[1][1]))


class PlonkVerifier:
    """snarkjs `plonk.verify(vk, publicSignals, proof)` for batches: one verdict per proof."""

    def __init__(self, vk, device=0):
        self.n_public = int(vk["nPublic"])
        b = plonk_vkey_bytes(vk)
        self._h = C.c_void_p()
        _check(load().g16_plonk_verifier_create(b, len(b), device, C.byref(self._h)))

    def verify_batch(self, items):
        """items: [(public_signals, proof_obj)] -> list of bools."""
        short = [len(ps) != self.n_public for ps, _ in items]
        pr = b"".join(plonk_proof_from_obj(p) for _, p in items)
        pub = b"".join(b"".join(_le32(x) for x in (ps if not s else [0] * self.n_public)) for (ps, _), s in zip(items, short))
        ok = C.create_string_buffer(max(1, len(items)))
        _check(load().g16_plonk_verify_batch(self._h, pr, pub, len(items), ok))
        return [ok.raw[i] != 0 and not short[i] for i in range(len(items))]

    def verify(self, public_signals, proof):
        return self.verify_batch([(public_signals, proof)])[0]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            load().g16_plonk_verifier_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


def plonk_setup(r1cs, seed, device=0, with_lagrange=True):
    """Test-only PLONK setup with a known tau: .r1cs bytes -> snarkjs-layout PLONK .zkey bytes."""
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_plonk_setup(r1cs, len(r1cs), seed, device, 1 if with_lagrange else 0, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def plonk_setup_ptau(r1cs, ptau, device=0, with_lagrange=True):
    """`snarkjs plonk setup c.r1cs pot.ptau c.zkey`: .r1cs and .ptau bytes -> PLONK .zkey bytes."""
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_plonk_setup_ptau(r1cs, len(r1cs), ptau, len(ptau), device, 1 if with_lagrange else 0, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def groth16_setup_ptau(r1cs, ptau, device=0):
    """`snarkjs groth16 setup c.r1cs pot.ptau c_0000.zkey`: .r1cs and prepared .ptau bytes -> Groth16 .zkey bytes
    (gamma = delta = 1, no contribution yet)."""
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_groth16_setup_ptau(r1cs, len(r1cs), ptau, len(ptau), device, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def ptau_prepare(ptau, device=0):
    """`snarkjs powersoftau prepare phase2 in.ptau out.ptau`: .ptau bytes (sections 1-7) -> the prepared .ptau bytes
    (sections 1-7, then 12-15 computed on the device)."""
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_ptau_prepare(ptau, len(ptau), device, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def ptau_new(power):
    """`snarkjs powersoftau new bn128 <power>`: the .ptau bytes of a ceremony without contributions (host only)."""
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_ptau_new(power, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def ptau_contribute(ptau, name=None, secret=None, device=0):
    """`snarkjs powersoftau contribute`: .ptau bytes -> (contributed .ptau bytes, 64-byte contribution hash).  secret:
    (tau, alpha, beta, s_tau, s_alpha, s_beta), ints in [1, r), or None for the OS CSPRNG."""
    blob = _ptau_secret_blob("ptau_contribute", secret)
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    nm = None if name is None else name.encode("utf-8")
    _check(load().g16_ptau_contribute(ptau, len(ptau), nm, blob, device, C.byref(z), C.byref(zl), h))
    return _take(z, zl), h.raw


def beacon_scalars(beacon, exp, count):
    """The secret scalars of a beacon contribution (ints in [1, r)): count 6 = (tau, alpha, beta, s_tau, s_alpha,
    s_beta), count 2 = (d, s), the first two of the same stream.  beacon: 1 to 255 bytes; exp: 10 to 63, and the call
    hashes 2^exp times on this thread.  This library's derivation, not snarkjs's (host only)."""
    if not 0 <= exp < 1 << 32:
        raise ValueError("beacon_scalars: exp does not fit 32 bits")
    out = C.create_string_buffer(192)
    _check(load().g16_beacon_scalars(bytes(beacon), len(beacon), exp, count, out))
    return tuple(int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(count))


def _beacon(fn, data, beacon, exp, name, device):
    if not 0 <= exp < 1 << 32:
        raise ValueError("beacon: exp does not fit 32 bits")
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    nm = None if name is None else name.encode("utf-8")
    _check(fn(data, len(data), nm, bytes(beacon), len(beacon), exp, device, C.byref(z), C.byref(zl), h))
    return _take(z, zl), h.raw


def ptau_beacon(ptau, beacon, exp, name=None, device=0):
    """`snarkjs powersoftau beacon`: .ptau bytes -> (the .ptau bytes with the beacon contribution, 64-byte contribution
    hash): ptau_contribute with secret = beacon_scalars(beacon, exp, 6), and a record of type 1 that states the beacon."""
    return _beacon(load().g16_ptau_beacon, ptau, beacon, exp, name, device)


def zkey_beacon(zkey, beacon, exp, name=None, device=0):
    """`snarkjs zkey beacon`: Groth16 .zkey bytes -> (the .zkey bytes with the beacon contribution, 64-byte contribution
    hash): zkey_contribute with (d, s) = beacon_scalars(beacon, exp, 2), and a record of type 1 that states the beacon."""
    return _beacon(load().g16_zkey_beacon, zkey, beacon, exp, name, device)


def ptau_verify(ptau, device=0):
    """`snarkjs powersoftau verify` -> (ok, reason): is the file the generator file plus a chain of honest contributions?
    reason is empty when ok.  A malformed file raises G16Error(-2)."""
    ok = C.c_int(0)
    lib = load()
    _check(lib.g16_ptau_verify(ptau, len(ptau), device, C.byref(ok)))
    return bool(ok.value), ("" if ok.value else lib.g16_last_error().decode("utf-8", "replace"))


def _ptau_secret_blob(route, secret):
    if secret is None:
        return None
    if len(secret) != 6:
        raise ValueError(route + ": six secret scalars expected")
    return b"".join(int(x).to_bytes(32, "little") for x in secret)


def ptau_export_challenge(ptau, with_hash=False):
    """`snarkjs powersoftau export challenge`: .ptau bytes -> the challenge file's bytes (host only); with_hash: ->
    (challenge file, its Blake2b-512: the challenge the next contribution answers)."""
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    _check(load().g16_ptau_export_challenge(ptau, len(ptau), C.byref(z), C.byref(zl), h))
    out = _take(z, zl)
    return (out, h.raw) if with_hash else out


def ptau_challenge_contribute(challenge, secret=None, device=0):
    """`snarkjs powersoftau challenge contribute`: challenge file bytes -> (response file bytes, 64-byte contribution
    hash).  secret as in ptau_contribute."""
    blob = _ptau_secret_blob("ptau_challenge_contribute", secret)
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    _check(load().g16_ptau_challenge_contribute(challenge, len(challenge), blob, device, C.byref(z), C.byref(zl), h))
    return _take(z, zl), h.raw


def ptau_import_response(ptau, response, name=None, device=0):
    """`snarkjs powersoftau import response`: (.ptau bytes, response file bytes) -> (the new .ptau bytes, 64-byte
    contribution hash).  A response that fails a check of its record is a verdict, not a malformed file: G16Error with
    code 0 (G16_OK) and the check's text; nothing is returned."""
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    ok = C.c_int(0)
    nm = None if name is None else name.encode("utf-8")
    lib = load()
    _check(lib.g16_ptau_import_response(ptau, len(ptau), response, len(response), nm, device, C.byref(z), C.byref(zl), h, C.byref(ok)))
    if not ok.value:
        raise G16Error(0, lib.g16_last_error().decode("utf-8", "replace"))
    return _take(z, zl), h.raw


def _ptau_points(fn, group, data, in_size, out_size, device, want_be=False):
    """-> (output bytes, first bad index or -1, kernel ms[, big-endian images])."""
    if group not in (1, 2) or len(data) % (in_size * group):
        raise ValueError("ptau points: whole points of group 1 or 2 expected")
    n = len(data) // (in_size * group)
    out = C.create_string_buffer(max(1, n * out_size * group))
    bad, ms = C.c_int64(-1), C.c_float(0)
    if want_be is None:
        _check(fn(group, data, n, device, out, C.byref(bad), C.byref(ms)))
        return out.raw[:n * out_size * group], bad.value, ms.value
    be = C.create_string_buffer(max(1, n * 64 * group)) if want_be else None
    _check(fn(group, data, n, device, out, be, C.byref(bad), C.byref(ms)))
    return out.raw[:n * out_size * group], bad.value, ms.value, (be.raw[:n * 64 * group] if want_be else None)


def ptau_points_from_be(group, data, device=0):
    """TEST-ONLY layer entry: uncompressed big-endian points -> (file-form bytes, first bad index or -1, kernel ms)."""
    return _ptau_points(load().g16_ptau_points_from_be, group, data, 64, 64, device, None)


def ptau_points_compress(group, data, device=0):
    """TEST-ONLY layer entry: file-form points -> (compressed bytes, -1, kernel ms)."""
    return _ptau_points(load().g16_ptau_points_compress, group, data, 64, 32, device, None)


def ptau_points_decompress(group, data, device=0, want_be=True):
    """TEST-ONLY layer entry: compressed points -> (file-form bytes, first bad index or -1, kernel ms, big-endian images)."""
    return _ptau_points(load().g16_ptau_points_decompress, group, data, 32, 64, device, want_be)


def fq_sqrt_batch(ext, values, device=0):
    """TEST-ONLY layer entry: ints below q (ext 0) or pairs (c0, c1) (ext 1) -> [root or None] by the device routine."""
    if ext:
        data = b"".join(int(a).to_bytes(32, "little") + int(b).to_bytes(32, "little") for a, b in values)
    else:
        data = b"".join(int(a).to_bytes(32, "little") for a in values)
    n, esz = len(values), 64 if ext else 32
    out, has = C.create_string_buffer(max(1, n * esz)), C.create_string_buffer(max(1, n))
    _check(load().g16_fq_sqrt_batch(1 if ext else 0, data, n, device, out, has))
    res = []
    for i in range(n):
        w = [int.from_bytes(out.raw[i * esz + 32 * k:i * esz + 32 * k + 32], "little") for k in range(esz // 32)]
        res.append(None if has.raw[i] == 0 else (tuple(w) if ext else w[0]))
    return res


def ptau_secret_from_text(text):
    """The CLI's `-e=<text>` rule -> the six secret scalars (ints)."""
    out = C.create_string_buffer(192)
    _check(load().g16_ptau_secret_from_text(text.encode("utf-8"), out))
    return tuple(int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(6))


def zkey_contribute(zkey, name=None, d=None, s=None, device=0):
    """`snarkjs zkey contribute`: Groth16 .zkey bytes -> (contributed .zkey bytes, 64-byte contribution hash).  d, s:
    the contribution's secret scalars in [1, r) (both or neither; neither = OS CSPRNG): delta <- d delta."""
    if (d is None) != (s is None):
        raise ValueError("zkey_contribute: give both d and s, or neither")
    secret = None if d is None else int(d).to_bytes(32, "little") + int(s).to_bytes(32, "little")
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    nm = None if name is None else name.encode("utf-8")
    _check(load().g16_zkey_contribute(zkey, len(zkey), nm, secret, device, C.byref(z), C.byref(zl), h))
    return _take(z, zl), h.raw


def zkey_verify_from_init(init, zkey, device=0, ptau=None):
    """`snarkjs zkey verify frominit` -> (ok, reason): is `zkey` the key `init` plus a chain of honest contributions?
    reason is empty when ok.  ptau = .ptau bytes (prepared or not): the ptau leg as well -- section 9 of `zkey` is the H
    basis of that ceremony's section 2 scaled by 1 / delta; None: without the leg.  A malformed file raises
    G16Error(-2)."""
    ok = C.c_int(0)
    lib = load()
    if ptau is None:
        _check(lib.g16_zkey_verify_from_init(init, len(init), zkey, len(zkey), device, C.byref(ok)))
    else:
        _check(lib.g16_zkey_verify_from_init_ptau(init, len(init), ptau, len(ptau), zkey, len(zkey), device, C.byref(ok)))
    return bool(ok.value), ("" if ok.value else lib.g16_last_error().decode("utf-8", "replace"))


def zkey_verify_r1cs(r1cs, ptau, zkey, device=0):
    """`snarkjs zkey verify c.r1cs pot.ptau c.zkey` -> (ok, reason): the initial key is set up again from the .r1cs and
    the prepared .ptau in memory, then zkey_verify_from_init with the ptau leg."""
    ok = C.c_int(0)
    lib = load()
    _check(lib.g16_zkey_verify_r1cs(r1cs, len(r1cs), ptau, len(ptau), zkey, len(zkey), device, C.byref(ok)))
    return bool(ok.value), ("" if ok.value else lib.g16_last_error().decode("utf-8", "replace"))


def zkey_export_bellman(zkey, device=0):
    """`snarkjs zkey export bellman`: Groth16 .zkey bytes -> the MPCParams file's bytes (H in the monomial basis)."""
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_zkey_export_bellman(zkey, len(zkey), device, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def zkey_bellman_contribute(challenge, d=None, s=None, device=0):
    """`snarkjs zkey bellman contribute`: MPCParams bytes -> (response bytes, 64-byte contribution hash).  d, s as in
    zkey_contribute: the same pair gives the same record and hash through either route."""
    if (d is None) != (s is None):
        raise ValueError("zkey_bellman_contribute: give both d and s, or neither")
    secret = None if d is None else int(d).to_bytes(32, "little") + int(s).to_bytes(32, "little")
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    _check(load().g16_zkey_bellman_contribute(challenge, len(challenge), secret, device, C.byref(z), C.byref(zl), h))
    return _take(z, zl), h.raw


def zkey_import_bellman(old, response, name=None, device=0):
    """`snarkjs zkey import bellman`: (old .zkey bytes, response bytes) -> the new .zkey bytes.  A response the import
    refuses is a verdict, not a malformed file: G16Error with code 0 (G16_OK) and the check's text."""
    z, zl = C.c_void_p(), C.c_size_t()
    ok = C.c_int(0)
    nm = None if name is None else name.encode("utf-8")
    lib = load()
    _check(lib.g16_zkey_import_bellman(old, len(old), response, len(response), nm, device, C.byref(z), C.byref(zl), C.byref(ok)))
    if not ok.value:
        raise G16Error(0, lib.g16_last_error().decode("utf-8", "replace"))
    return _take(z, zl)


def zkey_h_basis(points, log_n, inverse=False, device=0):
    """TEST-ONLY layer entry of the MPCParams exchange: 2^log_n file-form G1 points (64 bytes each) -> as many, the basis
    change of section 9 alone (forward: all N values of T, T[N-1] included)."""
    if len(points) != 64 << log_n:
        raise ValueError("zkey_h_basis: 2^log_n points of 64 bytes expected")
    out = C.create_string_buffer(len(points))
    _check(load().g16_zkey_h_basis(device, points, log_n, 1 if inverse else 0, out))
    return out.raw


def zkey_h_scalars(u, log_n, device=0):
    """TEST-ONLY layer entry of the ptau leg: u = 2^log_n ints below r with u[-1] = 0 -> (rho, t), lists of ints, as the
    device forms them: rho[i] = (1 / N) sum_k u[k] w^((2i+1) k), t = u[:N-1] | 0 | -u[:N-1] mod r."""
    n = 1 << log_n
    if len(u) != n:
        raise ValueError("zkey_h_scalars: 2^log_n values expected")
    rho, t = C.create_string_buffer(n * 32), C.create_string_buffer((2 * n - 1) * 32)
    _check(load().g16_zkey_h_scalars(device, b"".join(_le32(x) for x in u), log_n, rho, t))
    return tuple([int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)] for raw in (rho.raw, t.raw))


def blake2b512(data):
    out = C.create_string_buffer(64)
    _check(load().g16_blake2b512(data, len(data), out))
    return out.raw


def blake2b512_parts(data, cuts):
    """TEST-ONLY layer entry: Blake2b-512 by the library's streaming hasher, `data` fed in the parts the ascending
    offsets `cuts` split it into (host only)."""
    out = C.create_string_buffer(64)
    arr = (C.c_size_t * max(1, len(cuts)))(*cuts)
    _check(load().g16_blake2b512_parts(data, len(data), arr, len(cuts), out))
    return out.raw


def zkey_new(r1cs, ptau, device=0):
    """`snarkjs zkey new` with the circuit hash: .r1cs and prepared .ptau bytes -> (Groth16 .zkey bytes, 64-byte csHash).
    The key is groth16_setup_ptau's except for the first 64 bytes of section 10, which hold the hash."""
    z, zl = C.c_void_p(), C.c_size_t()
    h = C.create_string_buffer(64)
    _check(load().g16_zkey_new(r1cs, len(r1cs), ptau, len(ptau), device, C.byref(z), C.byref(zl), h))
    return _take(z, zl), h.raw


def zkey_cs_hash(zkey, ptau, device=0):
    """The circuit hash zkey_new stores for this INITIAL key over this ceremony file (prepared or not): 64 bytes.  What
    section 10 already holds is not read, so a legacy zero-hash key can be checked or upgraded."""
    h = C.create_string_buffer(64)
    _check(load().g16_zkey_cs_hash(zkey, len(zkey), ptau, len(ptau), device, h))
    return h.raw


def zkey_h_monomial(points, log_n, device=0):
    """TEST-ONLY layer entry of the circuit hash: 2^(log_n + 1) - 1 file-form G1 points P -> the big-endian images of
    P[k + N] - P[k], k < N - 1, N = 2^log_n (64 bytes each)."""
    if len(points) != 64 * ((2 << log_n) - 1):
        raise ValueError("zkey_h_monomial: 2^(log_n + 1) - 1 points of 64 bytes expected")
    n = (1 << log_n) - 1
    out = C.create_string_buffer(max(1, 64 * n))
    _check(load().g16_zkey_h_monomial(device, points, log_n, out))
    return out.raw[:64 * n]


def zkey_hash_to_g2(transcript):
    """The point on G2 a contribution's 64-byte transcript hash selects (affine little-endian Montgomery, 128 bytes)."""
    if len(transcript) != 64:
        raise ValueError("zkey_hash_to_g2: 64 bytes expected")
    out = C.create_string_buffer(128)
    _check(load().g16_zkey_hash_to_g2(transcript, out))
    return out.raw


def r1cs_setup_trapdoor(r1cs, td, threads=0):
    """TEST-ONLY trapdoor setup of a .r1cs with td = dict(tau, alpha, beta, gamma, delta) of ints -> (zkey, vkey) bytes;
    runs where setup_device() says."""
    lib = load()
    blob = b"".join(int(td[k]).to_bytes(32, "little") for k in ("tau", "alpha", "beta", "gamma", "delta"))
    z, v = C.c_void_p(), C.c_void_p()
    zl, vl = C.c_size_t(), C.c_size_t()
    _check(lib.g16_r1cs_setup_trapdoor(r1cs, len(r1cs), blob, threads, C.byref(z), C.byref(zl), C.byref(v), C.byref(vl)))
    return _take(z, zl), _take(v, vl)


def ptau_synth(power, tau, alpha, beta, prepared=True, device=0):
    """TEST-ONLY .ptau image for a known (tau, alpha, beta); device -1 = host threads."""
    blob = b"".join(int(x).to_bytes(32, "little") for x in (tau, alpha, beta))
    z, zl = C.c_void_p(), C.c_size_t()
    _check(load().g16_ptau_synth(power, blob, 1 if prepared else 0, device, C.byref(z), C.byref(zl)))
    return _take(z, zl)


def plonk_proof_to_obj(pr):
    """g16_plonk_proof -> the object `snarkjs plonk prove` stringifies (its key order)."""
    def g1(b):
        b = bytes(b)
        return ["0", "1", "0"] if b == bytes(64) else [_dec(b[:32]), _dec(b[32:]), "1"]
    o = {}
    for k in _PLONK_G1:
        o[k] = g1(getattr(pr, k))
    for k in _PLONK_EV:
        o[k] = _dec(bytes(getattr(pr, k)))
    o["Wxi"], o["Wxiw"] = g1(pr.Wxi), g1(pr.Wxiw)
    o["protocol"], o["curve"] = "plonk", "bn128"
    return o


def pairing_op(pairs, device=0):
    """[(G1 affine ints, G2 affine ((x0, x1), (y0, y1)))] -> per pair the 12 tower coordinates (ints) of the pairing
    value the verifier kernels compute."""
    buf = b"".join(_le32(P[0]) + _le32(P[1]) + _le32(Q[0][0]) + _le32(Q[0][1]) + _le32(Q[1][0]) + _le32(Q[1][1]) for P, Q in pairs)
    out = C.create_string_buffer(max(1, 384 * len(pairs)))
    _check(load().g16_pairing_op(device, buf, len(pairs), out))
    raw = out.raw
    return [[int.from_bytes(raw[384 * i + 32 * k:384 * i + 32 * k + 32], "little") for k in range(12)] for i in range(len(pairs))]


def synth_witness(n_vars, n_public, n_constraints, seed, wseed):
    lib = load()
    w, wl = C.c_void_p(), C.c_size_t()
    _check(lib.g16_synth_witness(n_vars, n_public, n_constraints, seed, wseed, C.byref(w), C.byref(wl)))
    return _take(w, wl)
