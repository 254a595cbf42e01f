"""Pass verification from URIs on the host route (device -1: the nzcp_pass.cuh / sha256.cuh code the kernel runs, on host
threads): the layer operator against hashlib and the reference's base32, the verifier against pass_ref record by record,
the argument errors, and the front end under ASan + UBSan on a corpus of damaged passes.  No GPU needed."""
import os
import struct
import subprocess

from conftest import ROOT

import pass_cases as cases
import pass_ref

DEV = -1


def test_case_expectations():
    """every verdict the case lists state is the reference's, and the corpus has the mix it promises"""
    for group in (cases.padding_cases(), cases.cbor_cases(), cases.precedence_cases(), cases.cap_cases()):
        cases.check_expectations(group)
    uris, records = cases.corpus()
    assert len(uris) == len(records) == 140


def test_example_pass(amd):
    cases.run_example(amd, DEV)


def test_sha256_padding_edges(amd):
    cases.run_sha256_edges(amd, DEV)


def test_full_call_padding_edges(amd):
    cases.run_cases(amd, DEV, cases.padding_cases())


def test_base32_tails(amd):
    cases.run_base32_tails(amd, DEV)


def test_cbor_heads(amd):
    cases.run_cases(amd, DEV, cases.cbor_cases())


def test_front_end_operator(amd):
    cases.run_front_op(amd, DEV)


def test_verdict_precedence(amd):
    cases.run_cases(amd, DEV, cases.precedence_cases())


def test_uri_cap(amd):
    cases.run_cases(amd, DEV, cases.cap_cases())


def test_grid_tails(amd):
    cases.run_grid_tails(amd, DEV)


def test_whole_corpus(amd):
    cases.run_corpus(amd, DEV)


def test_errors(amd):
    cases.run_errors(amd, DEV)


def _damaged():
    """the example pass's decoded bytes: every truncation (370), every substitution of one of its first 64 bytes by a byte
    that opens a long, nested, indefinite or refused item, and the edge cases and the corpus besides"""
    cose = pass_ref.base32_decode(cases.example_uri()[8:].encode())
    assert len(cose) == 370
    items = [cases.uri_of(cose[:n]) for n in range(370)]
    for spot in range(64):
        for byte in (0x00, 0x1F, 0x5B, 0x7F, 0x9F, 0xBF, 0xFF):
            items.append(cases.uri_of(cose[:spot] + bytes([byte]) + cose[spot + 1:]))
    items += [c[1] for c in cases.cbor_cases() + cases.padding_cases() + cases.cap_cases() + cases.precedence_cases()] + cases.corpus()[0]
    return items


def test_front_end_under_sanitizers(amd, tmp_path):
    """tests/native/pass_test.cpp: each pass's text and decoded bytes on the heap at their exact sizes; the records equal
    the reference's and the library's"""
    exe = tmp_path / "pass_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nzcp-circom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pass_test.cpp"),
                           "-o", str(exe)])
    items = [u.encode() for u in _damaged()]
    _, names, _, _ = cases.key_set()
    blob = struct.pack("<I", len(names))
    for n in names:
        iss, _, kid = n.rpartition("#")
        blob += struct.pack("<I", len(iss)) + iss.encode() + struct.pack("<I", len(kid)) + kid.encode()
    offsets = [0]
    for u in items:
        offsets.append(offsets[-1] + len(u))
    blob += struct.pack("<I", len(items)) + struct.pack(f"<{len(offsets)}Q", *offsets) + b"".join(items)
    (tmp_path / "corpus.bin").write_bytes(blob)
    run = subprocess.run([str(exe), str(tmp_path / "corpus.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    out = (tmp_path / "out.bin").read_bytes()
    size = 96
    assert len(out) == len(items) * (size + 64)
    got = []
    for i in range(len(items)):
        verdict, key_idx, tbs_len, flags, nbf, exp = struct.unpack_from("<IIIIqq", out, i * size)
        got.append({"verdict": verdict, "key_idx": key_idx, "tbs_len": tbs_len, "flags": flags, "nbf": nbf, "exp": exp,
                    "tbs_sha256": out[i * size + 32:i * size + 64], "cred_subj_sha256": out[i * size + 64:i * size + 96]})
    sigs = out[len(items) * size:]
    for i, u in enumerate(items):
        want, sig = pass_ref.front(u, names)
        assert got[i] == want, (i, u[:60], got[i], want)
        assert sigs[i * 64:(i + 1) * 64] == (sig if want["verdict"] == 0 else bytes(64)), i
    # and the library's host route says the same of the damaged passes (signatures included)
    v = amd.PassVerifier(cases.key_set()[0], device=DEV)
    lib = v.verify_batch(items[:370 + 64 * 7], cases.NOW)
    v.close()
    for i, rec in enumerate(lib):
        assert rec == cases.expected(items[i].decode(), cases.NOW), i
