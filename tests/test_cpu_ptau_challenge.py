"""CPU side of the phase-1 challenge / response exchange (csrc/ptau_mpc.cpp): `export challenge` is host code and is
checked whole against the Python twin (tests/ptau_challenge_ref.py); every input error of `challenge contribute` and
`import response` comes out with its own text before the device is touched; the twin itself reproduces the
contribution twin byte for byte and is pinned by tests/golden/ptau_challenge.json."""
import ctypes
import json
import struct
import sys

import pytest

from bn254 import Q, R
from conftest import golden_path
from ptau_challenge_ref import (KEYS_BYTES, challenge_contribute_ref, compress, decompress, export_challenge_ref, from_be,
                                import_response_ref)
from ptau_mpc_ref import (G1_LEM, G2_LEM, challenge_hash, contribute_ref, first_challenge, generator_sections, key_points,
                          parse_section7, response_hash, write_record)
from ptau_prepare_ref import split
from ptau_prepared import rewrite, write_ptau_prepared
from zkey_mpc_ref import blake2b, g1_uncompressed, g2_uncompressed

SECRET = tuple(pow(5 + i, 91 + i, R) for i in range(6))


def _err(amd, call):
    with pytest.raises(amd.G16Error) as e:
        call()
    return e.value


def _with_sealed_record(ptau, power):
    """The file with one record written by the twin's write_record whose nextChallenge is that of the file's points (the
    points stay the generators: the record need not verify, it must parse and seal the state)."""
    secs = split(ptau)[1]
    challenge = first_challenge(generator_sections(power))
    rec = key_points(challenge, SECRET)
    rec.update({"tauG1": G1_LEM, "tauG2": G2_LEM, "alphaG1": G1_LEM, "betaG1": G1_LEM, "betaG2": G2_LEM})
    rec["nextChallenge"] = challenge_hash(secs, response_hash(challenge, rec))
    s7 = struct.pack("<I", 1) + write_record(rec, "sealed")
    return rewrite(ptau, lambda sid, d: s7 if sid == 7 else d), rec


# ------------------------------------------------------------------ export challenge (host only)
@pytest.mark.parametrize("power", range(4))
def test_export_equals_the_twin_and_hashes_to_the_first_challenge(amd, power):
    p0 = amd.ptau_new(power)
    got, h = amd.ptau_export_challenge(p0, with_hash=True)
    n = 1 << power
    assert len(got) == 384 * n + 128
    assert got == export_challenge_ref(p0)
    assert got[:64] == blake2b(b"")
    assert h == blake2b(got) == first_challenge(split(p0)[1])
    assert amd.ptau_export_challenge(p0) == got


@pytest.mark.parametrize("power", range(4))
def test_export_after_a_record_is_its_next_challenge(amd, power):
    sealed, rec = _with_sealed_record(amd.ptau_new(power), power)
    got, h = amd.ptau_export_challenge(sealed, with_hash=True)
    assert got == export_challenge_ref(sealed)
    assert got[:64] == response_hash(first_challenge(generator_sections(power)), rec)
    assert h == blake2b(got) == rec["nextChallenge"]
    # a wrong nextChallenge in the last record is refused
    at = 4 + 1432 + 17
    wrong = rewrite(sealed, lambda sid, d: d[:at] + bytes([d[at] ^ 1]) + d[at + 1:] if sid == 7 else d)
    e = _err(amd, lambda: amd.ptau_export_challenge(wrong))
    assert e.code == -2 and str(e) == "ptau export challenge: the file's points are not the last contribution's challenge"


def test_export_of_a_prepared_file_and_of_infinity_points(amd):
    prep = write_ptau_prepared(2, 5, 6, 7, prepared=True)
    assert amd.ptau_export_challenge(prep) == export_challenge_ref(prep)
    holes = rewrite(amd.ptau_new(2), lambda sid, d: bytes(64) + d[64:] if sid == 4 else (bytes(len(d)) if sid == 6 else d))
    got = amd.ptau_export_challenge(holes)
    assert got == export_challenge_ref(holes)
    assert got[64 + 7 * 64 + 4 * 128:][:64] == bytes([0x40]) + bytes(63) and got[-128:] == bytes([0x40]) + bytes(127)


def test_export_input_errors(amd):
    p2 = amd.ptau_new(2)
    for cut in (0, 11, len(p2) // 2, len(p2) - 1):
        e = _err(amd, lambda: amd.ptau_export_challenge(p2[:cut]))
        assert e.code == -2 and "ptau: Invalid File format" in str(e), cut
    e = _err(amd, lambda: amd.ptau_export_challenge(rewrite(p2, lambda sid, d: d[:36] + struct.pack("<I", 25) + d[40:] if sid == 1 else d)))
    assert e.code == -1 and "limit of 24" in str(e)
    e = _err(amd, lambda: amd.ptau_export_challenge(rewrite(p2, lambda sid, d: d[:-64] if sid == 5 else d)))
    assert e.code == -2 and str(e).endswith("ptau: Invalid File format")


def test_export_file_form(amd, tmp_path):
    lib = amd.load()
    p3 = amd.ptau_new(3)
    (tmp_path / "in.ptau").write_bytes(p3)
    h = ctypes.create_string_buffer(64)
    out = tmp_path / "challenge"
    assert lib.g16_ptau_export_challenge_files(str(tmp_path / "in.ptau").encode(), str(out).encode(), h) == 0
    assert out.read_bytes() == export_challenge_ref(p3) and h.raw == blake2b(out.read_bytes())
    rc = lib.g16_ptau_export_challenge_files(str(tmp_path / "missing").encode(), str(tmp_path / "x").encode(), None)
    assert rc == -1 and b"cannot open" in lib.g16_last_error() and not (tmp_path / "x").exists()


# ------------------------------------------------------------------ challenge contribute: before the device
def test_challenge_size_errors(amd):
    good = amd.ptau_export_challenge(amd.ptau_new(2))
    sizes = [0, 1, 127, 128, 128 + 383, len(good) - 1, len(good) + 1, len(good) + 384,      # 5 n: not a power of two
             128 + 384 * 3, 128 + 384 * 6]
    for size in sizes:
        e = _err(amd, lambda: amd.ptau_challenge_contribute((good * 3)[:size], SECRET))
        assert e.code == -2 and str(e) == "ptau challenge: Invalid File format", size


def test_challenge_power_zero_is_refused_by_name(amd):
    e = _err(amd, lambda: amd.ptau_challenge_contribute(amd.ptau_export_challenge(amd.ptau_new(0)), SECRET))
    assert e.code == -1 and str(e).startswith("ptau challenge contribute: power 0 is not supported"), str(e)


def test_challenge_secret_out_of_range(amd):
    good = amd.ptau_export_challenge(amd.ptau_new(1))
    for pos in range(6):
        for bad in (0, R, (1 << 256) - 1):
            secret = list(SECRET)
            secret[pos] = bad
            e = _err(amd, lambda: amd.ptau_challenge_contribute(good, tuple(secret)))
            assert e.code == -1 and str(e) == "ptau challenge contribute: the secret scalars must be in [1, r)", (pos, bad)


# ------------------------------------------------------------------ import response: before the device
@pytest.fixture(scope="module")
def round2(amd):
    """Power 2: the generator file, the twin's response to its challenge, the file the import must write."""
    p0 = amd.ptau_new(2)
    response, h = challenge_contribute_ref(export_challenge_ref(p0), SECRET)
    return p0, response, h


def test_import_size_errors(amd, round2):
    p0, response, _ = round2
    assert len(response) == 192 * 4 + 864
    for bad in (response[:-1], response + b"\0", response[:64], b"", response[:192 * 2 + 864], response + response[64:256]):
        e = _err(amd, lambda: amd.ptau_import_response(p0, bad, "x"))
        assert e.code == -2 and str(e) == "ptau import response: Invalid File format", len(bad)
    # everything open_ceremony checks
    e = _err(amd, lambda: amd.ptau_import_response(p0[:len(p0) // 2], response, "x"))
    assert e.code == -2 and "ptau: Invalid File format" in str(e)
    e = _err(amd, lambda: amd.ptau_import_response(rewrite(p0, lambda sid, d: d[:-128] if sid == 3 else d), response, "x"))
    assert e.code == -2 and str(e).endswith("ptau: Invalid File format")


def test_import_power_zero_is_refused_by_name(amd, round2):
    e = _err(amd, lambda: amd.ptau_import_response(amd.ptau_new(0), round2[1], "x"))
    assert e.code == -1 and str(e).startswith("ptau import response: power 0 is not supported"), str(e)


def test_import_response_that_answers_another_challenge(amd, round2):
    p0, response, _ = round2
    for bad in (bytes([response[0] ^ 1]) + response[1:], response[:63] + bytes([response[63] ^ 0x80]) + response[64:]):
        e = _err(amd, lambda: amd.ptau_import_response(p0, bad, "x"))
        assert e.code == 0 and str(e) == "ptau import response: the response does not answer this file's challenge"
    # the same response against the file one record later
    sealed, rec = _with_sealed_record(p0, 2)
    e = _err(amd, lambda: amd.ptau_import_response(sealed, response, "x"))
    assert e.code == 0 and "does not answer this file's challenge" in str(e)
    # and accepted as far as the device when it does answer it
    answered = rec["nextChallenge"] + response[64:]
    e = _err(amd, lambda: amd.ptau_import_response(sealed, answered, "x")) if not _gpu_present(amd) else None
    assert e is None or (e.code == -4 and str(e) == "ptau import response: no HIP device (there is no CPU path)")


def test_import_bad_key_point_images(amd, round2):
    p0, response, _ = round2
    keys_at = len(response) - KEYS_BYTES

    def edit(at, new):
        return response[:keys_at + at] + new + response[keys_at + at + len(new):]
    bad = [edit(64 + 63, bytes([response[keys_at + 64 + 63] ^ 1])),          # tau.g1_sx off its curve
           edit(128 + 32, Q.to_bytes(32, "big")),                              # alpha.g1_s: y = q
           edit(384 + 128, bytes([response[keys_at + 384 + 128] | 0x80])),     # alpha.g2_spx: a set 0x80
           edit(0, bytes([0x40]) + bytes(62) + b"\1"),                         # tau.g1_s: 0x40 with a stray byte
           edit(384 + 256, bytes(128)),                                        # beta.g2_spx: zeros without the flag
           edit(384, (Q + 1).to_bytes(32, "big"))]                             # tau.g2_spx: x.c1 above q
    for b in bad:
        e = _err(amd, lambda: amd.ptau_import_response(p0, b, "x"))
        assert e.code == -2 and str(e) == "ptau import response: a key point is not a valid image"
    # an infinity key point is a valid image: it passes these checks (the record check on the device names it)
    inf = edit(0, bytes([0x40]) + bytes(63))
    if not _gpu_present(amd):
        assert _err(amd, lambda: amd.ptau_import_response(p0, inf, "x")).code == -4


def _gpu_present(amd):
    try:
        amd.ptau_verify(amd.ptau_new(0), device=0)
        return True
    except amd.G16Error as e:
        assert e.code == -4, str(e)
        return False


def test_no_cpu_path_for_the_device_stages(amd, round2):
    if _gpu_present(amd):
        pytest.skip("GPU present")
    p0, response, _ = round2
    e = _err(amd, lambda: amd.ptau_challenge_contribute(export_challenge_ref(p0), SECRET))
    assert e.code == -4 and str(e) == "ptau challenge contribute: no HIP device (there is no CPU path)"
    e = _err(amd, lambda: amd.ptau_import_response(p0, response, "x"))
    assert e.code == -4 and str(e) == "ptau import response: no HIP device (there is no CPU path)"


def test_files_forms_report_errors_and_leave_no_output(amd, round2, tmp_path):
    lib = amd.load()
    p0, response, _ = round2
    old, resp, out = tmp_path / "old.ptau", tmp_path / "response", tmp_path / "new.ptau"
    old.write_bytes(p0)
    resp.write_bytes(bytes([response[0] ^ 1]) + response[1:])
    ok = ctypes.c_int(7)
    rc = lib.g16_ptau_import_response_files(str(old).encode(), str(resp).encode(), str(out).encode(), None, 0, None, ctypes.byref(ok))
    assert rc == 0 and ok.value == 0 and b"does not answer this file's challenge" in lib.g16_last_error()
    assert not out.exists() and old.read_bytes() == p0
    rc = lib.g16_ptau_import_response_files(str(old).encode(), str(tmp_path / "missing").encode(), str(out).encode(), None, 0, None,
                                            ctypes.byref(ok))
    assert rc == -1 and b"cannot open" in lib.g16_last_error() and not out.exists()
    (tmp_path / "short").write_bytes(bytes(500))
    rc = lib.g16_ptau_challenge_contribute_files(str(tmp_path / "short").encode(), str(out).encode(), None, 0, None)
    assert rc == -2 and lib.g16_last_error() == b"ptau challenge: Invalid File format" and not out.exists()


# ------------------------------------------------------------------ the twin itself
# (self-checks of the reference: they call no library code, pass without the feature and are no evidence for it)
def test_twin_point_codecs():
    import bn254 as b
    import formats as f
    for k in (1, 2, 3, 77, R - 1):
        for lem, unc in ((f.g1_to_lem(b.G1.mul(b.G1_GEN, k)), g1_uncompressed), (f.g2_to_lem(b.G2.mul(b.G2_GEN, k)), g2_uncompressed)):
            c = compress(lem)
            assert len(c) == len(lem) // 2 and decompress(c) == lem and from_be(unc(lem)) == lem
            other = decompress(bytes([c[0] ^ 0x80]) + c[1:])       # the opposite point
            assert other != lem and other[:len(lem) // 2] == lem[:len(lem) // 2]
    for size in (64, 128):
        inf = bytes(size)
        assert compress(inf) == bytes([0x40]) + bytes(size // 2 - 1) and decompress(compress(inf)) == inf
        assert decompress(bytes([0x40]) + bytes(size // 2 - 2) + b"\1") is None
        assert decompress(bytes([0xc0]) + bytes(size // 2 - 1)) is None
        assert decompress(bytes(size // 2 - 32) + Q.to_bytes(32, "big")) is None
        assert from_be(bytes(size)) is None and from_be(bytes([0x40]) + bytes(size - 1)) == inf


@pytest.mark.parametrize("power", [1, 2])
def test_twin_exchange_is_the_contribution_twin(amd, power):
    """import(old, contribute(export(old), secret), name) = contribute(old, name, secret), twice in a row."""
    ptau = amd.ptau_new(power)
    for name, secret in (("one", SECRET), (None, tuple(reversed(SECRET)))):
        challenge = export_challenge_ref(ptau)
        response, h = challenge_contribute_ref(challenge, secret)
        assert len(response) == 192 * (1 << power) + 864 and response[:64] == blake2b(challenge)
        assert h == blake2b(response[:64] + response[-KEYS_BYTES:])
        got, gh = import_response_ref(ptau, response, name)
        want, wh = contribute_ref(ptau, name, secret)
        assert got == want and gh == wh == h
        ptau = got
    assert len(parse_section7(split(ptau)[1][7])) == 2


def test_twin_is_the_golden_twin():
    sys.path.insert(0, golden_path(""))
    try:
        import make_ptau_challenge
    finally:
        sys.path.pop(0)
    with open(golden_path("ptau_challenge.json")) as fh:
        want = json.load(fh)
    assert make_ptau_challenge.run() == want
