"""ES256 pass-signature verification on the host route (device -1: the code the kernels run, on host threads): the
P-256 layer operator against Python ints, the verifier against the big-int reference p256_ref and the NZCP
specification's example pass, and the argument / key errors.  No GPU needed."""
import os
import subprocess

import pytest
from conftest import ROOT

import es256_cases as cases
import p256_ref as ref

DEV = -1


def test_field_ops(amd):
    cases.run_field_ops(amd, DEV)


def test_point_additions(amd):
    cases.run_point_adds(amd, DEV)


def test_projective_x_comparison(amd):
    cases.run_xcmp(amd, DEV)


def test_golden_key_and_pass():
    key = cases.golden_key()
    assert key.hex() == ("cd147e5c6b02a75d95bdb82e8b80c3e8ee9caa685f3ee5cc862d4ec4f97cefad"
                         "22fe5253a16e5be4d1621e7f18eac995c57f82917f1a9150842383f0b4a4dd3d")
    q = (int.from_bytes(key[:32], "big"), int.from_bytes(key[32:], "big"))
    assert ref.on_curve(q)
    digest, sig, _ = cases.golden_pass()
    assert ref.verify(q, int.from_bytes(digest, "big"), int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big"))


def test_signature_vectors(amd):
    """golden pass, bit flips, range checks, digests >= n, the crafted doubling / infinity sums, counts 0 and 1"""
    cases.run_signature_cases(amd, DEV)


def test_batch_of_130_over_three_keys(amd):
    keys, digests, sigs, idx, want = cases.batch130()
    v = amd.Es256Verifier(keys, device=DEV)
    assert v.verify_batch(digests, sigs, idx) == want
    v.close()


def test_mixed_wave(amd):
    keys, digests, sigs, idx, want = cases.mixed_wave()
    v = amd.Es256Verifier(keys, device=DEV)
    assert v.verify_batch(digests, sigs, idx) == want
    v.close()


def test_key_errors(amd):
    good = cases.golden_key()
    gx, gy = ref.G
    for bad, text in ((ref.be(ref.P) + good[32:], "key 1: coordinate not below"),
                      (good[:32] + ref.be(2**256 - 1), "key 1: coordinate not below"),
                      (ref.be(gx) + ref.be(gy + 1), "key 1 is not on the curve"),
                      (bytes(64), "key 1 is (0, 0)")):
        with pytest.raises(amd.G16Error) as e:
            amd.Es256Verifier([good, bad], device=DEV)
        assert e.value.code == -2 and text in str(e.value), str(e.value)
    for n in (0, 17):
        with pytest.raises(amd.G16Error) as e:
            amd.Es256Verifier([good] * n, device=DEV)
        assert e.value.code == -1 and "1 to 16 keys" in str(e.value)
    v = amd.Es256Verifier([good] * 16, device=DEV)
    digest, sig, _ = cases.golden_pass()
    assert v.verify_batch([digest] * 2, [sig] * 2, [0, 15]) == [True, True]
    with pytest.raises(amd.G16Error) as e:
        v.verify_batch([digest] * 3, [sig] * 3, [0, 15, 16])
    assert e.value.code == -1 and "item 2" in str(e.value)
    v.close()


def test_operator_argument_errors(amd):
    with pytest.raises(amd.G16Error) as e:
        amd.p256_op("fp_add", cases.pack([1, ref.P]), cases.pack([1, 1]), device=DEV)
    assert e.value.code == -1 and "item 1" in str(e.value)
    with pytest.raises(amd.G16Error):
        amd.p256_op("fn_inv", cases.pack([ref.N]), device=DEV)
    with pytest.raises(amd.G16Error):
        amd.p256_op(11, cases.pack([1]), cases.pack([1]), device=DEV)
    assert amd.p256_op("fp_mul", b"", b"", device=DEV) == b""


class _NativeOp:
    """p256_op through tests/native/p256_test.cpp: the same cases on the device's 8 x 32-bit limb forms, under ASan + UBSan."""

    def __init__(self, amd, exe, tmp):
        self.amd, self.exe, self.tmp = amd, exe, tmp

    def p256_op(self, op, a, b=None, device=None):
        fa, fb, fo = (self.tmp / n for n in ("a.bin", "b.bin", "out.bin"))
        fa.write_bytes(a)
        fb.write_bytes(b or b"")
        run = subprocess.run([str(self.exe), str(self.amd.P256_OPS[op]), str(fa), str(fb) if b is not None else "-", str(fo)],
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        return fo.read_bytes()


def test_device_limb_forms_on_the_host(amd, tmp_path):
    exe = tmp_path / "p256_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DG16_HOST_MUL32", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nzcp-circom_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "p256_test.cpp"), "-o", str(exe)])
    native = _NativeOp(amd, exe, tmp_path)
    cases.run_field_ops(native, None)
    cases.run_point_adds(native, None)
    cases.run_xcmp(native, None)
    # whole verifications on the 8 x 32 forms: the schedule's exceptional additions, compare branches and scalar edges
    # (families b to e of es256_cases), verdict by verdict against the construction's
    every = cases.exponent_cases("bcde")
    keys = list(dict.fromkeys(c[1] for c in every))
    files = [tmp_path / n for n in ("keys.bin", "digests.bin", "sigs.bin", "idx.bin", "ok.bin")]
    for path, blob in zip(files, (b"".join(keys), b"".join(c[3] for c in every), b"".join(c[4] for c in every),
                                  b"".join(keys.index(c[1]).to_bytes(4, "little") for c in every))):
        path.write_bytes(blob)
    run = subprocess.run([str(exe), "verify"] + [str(p) for p in files], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    got = [bool(v) for v in files[4].read_bytes()]
    assert len(got) == len(every)
    assert [(c[0], g) for c, g in zip(every, got) if g != c[5]] == []
