"""CPU side of `powersoftau new / contribute / verify` (csrc/ptau_mpc.cpp): `new` is host code and is checked whole;
every input error of contribute and verify comes out before the device is touched; no mutated file crashes the readers;
and the Python twin the GPU tests compare against (tests/ptau_mpc_ref.py) is itself checked through the oracle pairing."""
import random
import struct

import pytest

from bn254 import R
from ptau_mpc_ref import REC_FIXED, contribute_ref, parse_section7, verify_ref
from ptau_prepare_ref import split
from ptau_prepared import rewrite, write_ptau_prepared

SECRET = tuple(pow(3 + i, 77 + i, R) for i in range(6))


def _calls(amd):
    return {"contribute": lambda p: amd.ptau_contribute(p, "cpu", SECRET, device=0), "verify": lambda p: amd.ptau_verify(p, device=0)}


@pytest.fixture(scope="module")
def ptau4(amd):
    return amd.ptau_new(4)


def _with_record(ptau):
    """A well-formed file with one (arbitrary but parseable) record: the generator points in every slot."""
    from ptau_mpc_ref import G1_LEM, G2_LEM, write_record
    rec = {"tauG1": G1_LEM, "tauG2": G2_LEM, "alphaG1": G1_LEM, "betaG1": G1_LEM, "betaG2": G2_LEM, "nextChallenge": bytes(64)}
    for k in ("tau", "alpha", "beta"):
        rec[k + ".g1_s"], rec[k + ".g1_sx"], rec[k + ".g2_spx"] = G1_LEM, G1_LEM, G2_LEM
    s7 = struct.pack("<I", 1) + write_record(rec, "someone")
    return rewrite(ptau, lambda sid, d: s7 if sid == 7 else d)


def _err(amd, call, ptau):
    with pytest.raises(amd.G16Error) as e:
        call(ptau)
    return e.value


_GPU = []


def _gpu_present(amd):
    """Whether the library itself finds a device: the generator file of power 0 ends at G16_E_NOGPU, or is verified."""
    if not _GPU:
        try:
            amd.ptau_verify(amd.ptau_new(0), device=0)
            _GPU.append(True)
        except amd.G16Error as e:
            assert e.code == -4, str(e)
            _GPU.append(False)
    return _GPU[0]


def _accepted(amd, call, ptau):
    """A well-formed file passes every check: the call then succeeds, or -- no device, the last check of all -- ends at
    G16_E_NOGPU."""
    try:
        call(ptau)
    except amd.G16Error as e:
        assert e.code == -4 and "no HIP device" in str(e), str(e)


# ------------------------------------------------------------------ new
@pytest.mark.parametrize("power", range(6))
def test_new_is_the_generator_file(amd, power):
    got = amd.ptau_new(power)
    ids, gs = split(got)
    _, ws = split(write_ptau_prepared(power, 1, 1, 1, prepared=False))
    assert ids == [1, 2, 3, 4, 5, 6, 7]
    for sid in range(1, 7):
        assert gs[sid] == ws[sid], sid
    assert gs[7] == bytes(4)
    assert got == amd.ptau_synth(power, 1, 1, 1, prepared=False, device=-1)


def test_new_power_above_the_limit_names_the_limit(amd):
    with pytest.raises(amd.G16Error) as e:
        amd.ptau_new(25)
    assert e.value.code == -1 and "limit of 24" in str(e.value) and "power 25" in str(e.value)


def test_new_file_form(amd, tmp_path):
    out = tmp_path / "new.ptau"
    assert amd.load().g16_ptau_new_file(3, str(out).encode()) == 0
    assert out.read_bytes() == amd.ptau_new(3)


# ------------------------------------------------------------------ input errors, before the device
@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_well_formed_files_pass_the_checks(amd, ptau4, route):
    call = _calls(amd)[route]
    _accepted(amd, call, ptau4)
    _accepted(amd, call, _with_record(ptau4))
    _accepted(amd, call, rewrite(ptau4, lambda sid, d: None if sid == 7 else d))
    _accepted(amd, call, write_ptau_prepared(2, 5, 6, 7, prepared=True))


@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_not_a_ptau_and_truncated_files(amd, ptau4, route):
    call = _calls(amd)[route]
    for cut in (0, 5, 12, 100, len(ptau4) // 2, len(ptau4) - 1):
        e = _err(amd, call, ptau4[:cut])
        assert e.code == -2 and "ptau: Invalid File format" in str(e), (cut, str(e))
    e = _err(amd, call, b"zkey" + ptau4[4:])
    assert e.code == -2 and "ptau: Invalid File format" in str(e)
    e = _err(amd, call, ptau4[:4] + struct.pack("<I", 2) + ptau4[8:])
    assert e.code == -2 and "Version not supported" in str(e)


@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_not_bn128(amd, ptau4, route):
    call = _calls(amd)[route]
    e = _err(amd, call, rewrite(ptau4, lambda sid, d: d[:4] + bytes([d[4] ^ 1]) + d[5:] if sid == 1 else d))
    assert e.code == -2 and "ptau: Invalid File format (bn128 powers of tau expected)" in str(e)
    e = _err(amd, call, rewrite(ptau4, lambda sid, d: None if sid == 1 else d))
    assert e.code == -2 and "bn128 powers of tau expected" in str(e)


@pytest.mark.parametrize("route", ["contribute", "verify"])
@pytest.mark.parametrize("sid", [2, 3, 4, 5, 6])
def test_section_missing_or_of_the_wrong_size(amd, ptau4, sid, route):
    call = _calls(amd)[route]
    psz = 128 if sid in (3, 6) else 64
    for edit in (lambda d: None, lambda d: d[:-psz], lambda d: d + d[:psz], lambda d: d[:-1]):
        e = _err(amd, call, rewrite(ptau4, lambda s, d: edit(d) if s == sid else d))
        assert e.code == -2 and str(e).endswith("ptau: Invalid File format"), str(e)


@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_sizes_follow_the_header_power(amd, ptau4, route):
    call = _calls(amd)[route]
    for power in (3, 5):
        e = _err(amd, call, rewrite(ptau4, lambda sid, d: d[:36] + struct.pack("<I", power) + d[40:] if sid == 1 else d))
        assert e.code == -2 and "ptau: Invalid File format" in str(e)


@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_power_above_the_limit_names_the_limit(amd, ptau4, route):
    call = _calls(amd)[route]
    e = _err(amd, call, rewrite(ptau4, lambda sid, d: d[:36] + struct.pack("<I", 25) + d[40:] if sid == 1 else d))
    assert e.code == -1 and "limit of 24" in str(e) and "power 25" in str(e), str(e)


@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_section_7_must_parse(amd, ptau4, route):
    call = _calls(amd)[route]
    good = _with_record(ptau4)
    s7 = split(good)[1][7]
    assert len(parse_section7(s7)) == 1
    bad7 = [s7[:-1],                                    # shorter than its record says
            s7 + b"\0",                                 # trailing bytes
            struct.pack("<I", 2) + s7[4:],              # a second record that is not there
            s7[:3],                                     # not even a count
            s7[:4 + 1500] + struct.pack("<I", 1000) + s7[4 + 1504:],   # params longer than the section
            s7[:4] + bytes([s7[4] ^ 1]) + s7[5:]]       # tauG1 off its curve
    for s in bad7:
        e = _err(amd, call, rewrite(good, lambda sid, d: s if sid == 7 else d))
        assert e.code == -2 and str(e).endswith("ptau: Invalid File format"), str(e)
    assert REC_FIXED == 1504


def test_secret_out_of_range_is_an_argument_error(amd, ptau4):
    for pos in range(6):
        for bad in (0, R, R + 5, (1 << 256) - 1):
            secret = list(SECRET)
            secret[pos] = bad
            with pytest.raises(amd.G16Error) as e:
                amd.ptau_contribute(ptau4, None, tuple(secret), device=0)
            assert e.value.code == -1 and "must be in [1, r)" in str(e.value), (pos, bad)


def test_no_cpu_path(amd, ptau4):
    if _gpu_present(amd):
        pytest.skip("GPU present")
    for call in _calls(amd).values():
        assert _err(amd, call, ptau4).code == -4


def test_files_forms_report_a_missing_input_and_leave_no_output(amd, ptau4, tmp_path):
    lib = amd.load()
    missing, out = str(tmp_path / "missing.ptau").encode(), tmp_path / "out.ptau"
    rc = lib.g16_ptau_contribute_files(missing, str(out).encode(), None, None, 0, None)
    assert rc == -1 and b"cannot open" in lib.g16_last_error()
    assert not out.exists()
    import ctypes
    ok = ctypes.c_int(7)
    rc = lib.g16_ptau_verify_file(missing, 0, ctypes.byref(ok))
    assert rc == -1 and b"cannot open" in lib.g16_last_error()
    (tmp_path / "cut.ptau").write_bytes(ptau4[:len(ptau4) // 2])
    rc = lib.g16_ptau_contribute_files(str(tmp_path / "cut.ptau").encode(), str(out).encode(), None, None, 0, None)
    assert rc == -2 and b"ptau: Invalid File format" in lib.g16_last_error()
    assert not out.exists()


@pytest.mark.parametrize("route", ["contribute", "verify"])
def test_mutated_ptau_images(amd, ptau4, route):
    """An error, a verdict or G16_E_NOGPU; never a crash or an allocation sized by an untrusted field."""
    if _gpu_present(amd):
        pytest.skip("GPU present")
    call = _calls(amd)[route]
    base = _with_record(ptau4)
    rng = random.Random(7 if route == "verify" else 8)

    def mutate(buf, head):
        b = bytearray(buf)
        k = rng.randrange(4)
        if k == 0:
            for _j in range(rng.randrange(1, 4)):
                b[rng.randrange(min(len(b), head))] = rng.randrange(256)
        elif k == 1:
            b = b[:rng.randrange(len(b))]
        elif k == 2:
            i = rng.randrange(min(len(b) - 4, head))
            b[i:i + 4] = struct.pack("<I", rng.choice([0, 1, 0xffffffff, 0x7fffffff, rng.randrange(1 << 32)]))
        else:
            i = 12 + rng.randrange(100)
            b[i:i + 8] = struct.pack("<Q", rng.choice([0, 1, len(b), 1 << 40, (1 << 64) - 1]))
        return bytes(b)
    codes = set()
    for k in range(600):
        try:
            call(mutate(base, len(base) if k % 3 == 0 else 600))
        except amd.G16Error as e:
            codes.add(e.code)
    assert codes <= {-1, -2, -4} and -2 in codes


def test_secret_from_text_rule(amd):
    import hashlib
    got = amd.ptau_secret_from_text("some entropy")
    want = [0] * 6
    for j in range(3):
        h = hashlib.blake2b(b"some entropy" + bytes([j]), digest_size=64).digest()
        want[j] = int.from_bytes(h[:32], "little") % R or 1
        want[3 + j] = int.from_bytes(h[32:], "little") % R or 1
    assert list(got) == want


# ------------------------------------------------------------------ the twin itself
def test_twin_contributes_and_verifies_at_power_2(amd):
    p0 = amd.ptau_new(2)
    assert verify_ref(p0)
    p1, h1 = contribute_ref(p0, "first", SECRET)
    p2, h2 = contribute_ref(p1, None, tuple(reversed(SECRET)))
    assert h1 != h2 and len(parse_section7(split(p2)[1][7])) == 2
    assert verify_ref(p1) and verify_ref(p2)
    # the sections are those of the product ceremony
    tau, alpha, beta = (SECRET[i] * SECRET[5 - i] % R for i in range(3))
    want = split(write_ptau_prepared(2, tau, alpha, beta, prepared=False))[1]
    for sid in range(2, 7):
        assert split(p2)[1][sid] == want[sid], sid
    # one byte of the last record: g1_sx of the alpha key
    at = 4 + len(parse_section7(split(p2)[1][7])[0]["raw"]) + 448 + 128 + 64 + 5
    flipped = rewrite(p2, lambda sid, d: d[:at] + bytes([d[at] ^ 1]) + d[at + 1:] if sid == 7 else d)
    try:
        verdict = verify_ref(flipped)
    except (ValueError, AssertionError, ZeroDivisionError):
        verdict = False     # (the flipped coordinate may not decode to a point at all)
    assert not verdict
    at = 4 + len(parse_section7(split(p2)[1][7])[0]["raw"]) + 1432 + 9      # nextChallenge
    assert not verify_ref(rewrite(p2, lambda sid, d: d[:at] + bytes([d[at] ^ 1]) + d[at + 1:] if sid == 7 else d))
