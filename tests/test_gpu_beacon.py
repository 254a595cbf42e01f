"""`powersoftau beacon` and `zkey beacon` on the device, through the existing scaling kernels (csrc/ptau_scale.hip,
csrc/zkey_scale.hip) and the new entry points.  The defining property: beacon(old, name, beaconHash, e) is
contribute(old, name, secret = the twin's scalars) byte for byte and with the same hash, outside the new record's type,
paramsLen and params, which are the twin's (tests/beacon_ref.py).  Both verifiers accept the result and a further
contribution on top of it, and reject every record that claims a beacon it is not, each with its text."""
import ctypes
import struct

import pytest

import bn254 as b
import formats as f
import synth
import zkey_mpc_ref as zref
from beacon_ref import params as beacon_params
from beacon_ref import scalars, walk
from bn254 import R
from conftest import golden_path
from ptau_mpc_ref import REC_FIXED as PTAU_FIXED
from ptau_mpc_ref import parse_section7
from ptau_prepare_ref import split
from ptau_prepared import rewrite
from zkey_mpc_ref import REC_FIXED as ZKEY_FIXED
from zkey_mpc_ref import name_params, parse_section10

pytestmark = pytest.mark.gpu

BEACON = bytes((37 * i + 11) & 0xff for i in range(32))
EXP = 10
NOT_STATED, NOT_THE_KEY = "a beacon contribution does not state its beacon", "a beacon contribution's key is not the beacon's"
PTAU_CASES = [(power, earlier) for power in (0, 1, 4) for earlier in (0, 1)]
TINY = (24, 2, 12, 1)   # the circuit of tests/golden/tiny.zkey: domain 2^4


def _secret(seed):
    return tuple(pow(seed + 2 + i, 1000 + 7 * i + seed, R) for i in range(6))


# ------------------------------------------------------------------ the files under test, once
@pytest.fixture(scope="module")
def twin_scalars():
    return scalars(BEACON, EXP, 6)


@pytest.fixture(scope="module")
def ptaus(amd):
    """(power, earlier) -> the file before the beacon, (file, hash) with a named and with an unnamed beacon."""
    out = {}
    for power, earlier in PTAU_CASES:
        old = amd.ptau_new(power)
        if earlier:
            old, _ = amd.ptau_contribute(old, "earlier", _secret(power), device=0)
        out[(power, earlier)] = {"old": old, "named": amd.ptau_beacon(old, BEACON, EXP, "final", device=0),
                                 "bare": amd.ptau_beacon(old, BEACON, EXP, device=0)}
    return out


@pytest.fixture(scope="module")
def zkeys(amd):
    """tiny.zkey as it is, small.zkey with one earlier contribution; the same three entries."""
    tiny = open(golden_path("tiny.zkey"), "rb").read()
    small, _ = amd.zkey_contribute(open(golden_path("small.zkey"), "rb").read(), "earlier", 0x1234567 ** 5 % R, 0x7654321 ** 5 % R, device=0)
    return {name: {"old": old, "named": amd.zkey_beacon(old, BEACON, EXP, "final", device=0), "bare": amd.zkey_beacon(old, BEACON, EXP, device=0)}
            for name, old in (("tiny", tiny), ("small", small))}


@pytest.fixture(scope="module")
def ceremony(amd, ptaus):
    """Phase 1 closed by a beacon at power 4, prepared; the tiny circuit set up from it; phase 2 with one contribution
    and then a beacon."""
    n, p, m, seed = TINY
    rows, _ = synth.make(n, p, m, seed)
    r1cs = f.write_r1cs(n, p, 0, rows)
    ptau = amd.ptau_prepare(ptaus[(4, 1)]["named"][0], device=0)
    init = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    one, _ = amd.zkey_contribute(init, "first", 0x1f2e3d4c5b6a7988 ** 3 % R, 0x0123456789abcdef ** 3 % R, device=0)
    final, _ = amd.zkey_beacon(one, BEACON, EXP, "final", device=0)
    return {"r1cs": r1cs, "ptau": ptau, "init": init, "one": one, "final": final}


# ------------------------------------------------------------------ record surgery: type and params enter no hash
def _ptau_retype(ptau, index, typ, params):
    recs = parse_section7(split(ptau)[1][7])
    raws = [r["raw"] for r in recs]
    raws[index] = raws[index][:PTAU_FIXED - 8] + struct.pack("<II", typ, len(params)) + params
    s7 = struct.pack("<I", len(raws)) + b"".join(raws)
    return rewrite(ptau, lambda sid, d: s7 if sid == 7 else d)


def _zkey_sections(buf):
    secs = f.read_binfile(buf, "zkey", 2)
    return {sid: f.section(buf, secs, sid) for sid in secs}


def _zkey_retype(zkey, index, typ, params):
    secs = f.read_binfile(zkey, "zkey", 2)
    order = sorted(secs, key=lambda sid: secs[sid][0][0])
    cs, recs = parse_section10(f.section(zkey, secs, 10))
    raws = [r["raw"] for r in recs]
    raws[index] = raws[index][:ZKEY_FIXED - 8] + struct.pack("<II", typ, len(params)) + params
    s10 = cs + struct.pack("<I", len(raws)) + b"".join(raws)
    return f.write_binfile("zkey", struct.unpack_from("<I", zkey, 4)[0], [(sid, s10 if sid == 10 else f.section(zkey, secs, sid)) for sid in order])


def _tampers(name):
    """(params of the beacon record, the verdict's text) per tamper of the issue's list"""
    good = beacon_params(name, BEACON, EXP)
    other = BEACON[:7] + bytes([BEACON[7] ^ 1]) + BEACON[8:]
    return {"hash_byte": (beacon_params(name, other, EXP), NOT_THE_KEY),
            "e_10_to_11": (beacon_params(name, BEACON, EXP + 1), NOT_THE_KEY),
            "id3_removed": (good[:len(good) - 2 - len(BEACON)], NOT_STATED),
            "e_9": (beacon_params(name, BEACON, 9), NOT_STATED)}


# ------------------------------------------------------------------ 1. powersoftau beacon
@pytest.mark.parametrize("power,earlier", PTAU_CASES)
def test_ptau_beacon_is_the_contribution_of_the_twins_scalars(amd, ptaus, twin_scalars, power, earlier):
    c = ptaus[(power, earlier)]
    for key, name in (("named", "final"), ("bare", None)):
        got, h = c[key]
        want, wh = amd.ptau_contribute(c["old"], name, twin_scalars, device=0)
        assert h == wh
        (gids, gs), (wids, ws) = split(got), split(want)
        assert gids == wids == [1, 2, 3, 4, 5, 6, 7]
        for sid in range(1, 7):
            assert gs[sid] == ws[sid], sid
        grecs, wrecs = parse_section7(gs[7]), parse_section7(ws[7])
        assert len(grecs) == len(wrecs) == earlier + 1
        assert [r["raw"] for r in grecs[:-1]] == [r["raw"] for r in wrecs[:-1]]
        assert grecs[-1]["raw"][:PTAU_FIXED - 8] == wrecs[-1]["raw"][:PTAU_FIXED - 8]
        assert (wrecs[-1]["type"], wrecs[-1]["params"]) == (0, name_params(name))
        assert (grecs[-1]["type"], grecs[-1]["params"]) == (1, beacon_params(name, BEACON, EXP))
        assert walk(grecs[-1]["params"]) == (EXP, BEACON)
        assert got == _ptau_retype(want, -1, 1, beacon_params(name, BEACON, EXP))   # nothing else differs


@pytest.mark.parametrize("power,earlier", PTAU_CASES)
def test_ptau_verify_accepts_the_beacon_and_a_contribution_on_top(amd, ptaus, power, earlier):
    c = ptaus[(power, earlier)]
    for key in ("named", "bare"):
        ok, why = amd.ptau_verify(c[key][0], device=0)
        assert ok and why == "", why
    more, _ = amd.ptau_contribute(c["named"][0], "after", _secret(9), device=0)
    recs = parse_section7(split(more)[1][7])
    assert [r["type"] for r in recs] == [0] * earlier + [1, 0] and recs[-2]["raw"] == parse_section7(split(c["named"][0])[1][7])[-1]["raw"]
    ok, why = amd.ptau_verify(more, device=0)
    assert ok and why == "", why


def test_ptau_beacon_file_form_equals_the_memory_form(amd, ptaus, tmp_path):
    c = ptaus[(4, 1)]
    src, out = tmp_path / "old.ptau", tmp_path / "new.ptau"
    src.write_bytes(c["old"])
    hb = ctypes.create_string_buffer(64)
    assert amd.load().g16_ptau_beacon_files(str(src).encode(), str(out).encode(), b"final", BEACON, len(BEACON), EXP, 0, hb) == 0
    assert (out.read_bytes(), hb.raw) == c["named"]


@pytest.mark.parametrize("power,earlier", [(0, 0), (4, 1)])
@pytest.mark.parametrize("tamper", ["hash_byte", "e_10_to_11", "id3_removed", "e_9"])
def test_ptau_verify_rejects_a_record_that_is_not_its_beacon(amd, ptaus, tamper, power, earlier):
    params, text = _tampers("final")[tamper]
    ok, why = amd.ptau_verify(_ptau_retype(ptaus[(power, earlier)]["named"][0], -1, 1, params), device=0)
    assert not ok and why == "ptau verify: " + text


def test_ptau_verify_rejects_an_ordinary_record_that_claims_to_be_a_beacon(amd, ptaus):
    good = ptaus[(4, 1)]["named"][0]
    ok, why = amd.ptau_verify(_ptau_retype(good, 0, 1, name_params("earlier")), device=0)
    assert not ok and why == "ptau verify: " + NOT_STATED
    ok, why = amd.ptau_verify(_ptau_retype(good, 0, 1, b""), device=0)
    assert not ok and why == "ptau verify: " + NOT_STATED
    # ... and the beacon record demoted to an ordinary one is an honest contribution of a secret that happens to be public
    ok, why = amd.ptau_verify(_ptau_retype(good, 1, 0, name_params("final")), device=0)
    assert ok, why


def test_a_ptau_with_a_beacon_flows_through_the_exchange_and_prepare(amd, ptaus):
    beacon = ptaus[(4, 1)]["named"][0]
    challenge = amd.ptau_export_challenge(beacon)
    response, _ = amd.ptau_challenge_contribute(challenge, _secret(7), device=0)
    imported, _ = amd.ptau_import_response(beacon, response, "imported", device=0)
    assert imported == amd.ptau_contribute(beacon, "imported", _secret(7), device=0)[0]
    assert [r["type"] for r in parse_section7(split(imported)[1][7])] == [0, 1, 0]
    ok, why = amd.ptau_verify(imported, device=0)
    assert ok, why
    prepared = amd.ptau_prepare(beacon, device=0)
    assert split(prepared)[1][7] == split(beacon)[1][7]
    ok, why = amd.ptau_verify(prepared, device=0)
    assert ok, why


# ------------------------------------------------------------------ 2. zkey beacon
@pytest.mark.parametrize("which", ["tiny", "small"])
def test_zkey_beacon_is_the_contribution_of_the_twins_scalars(amd, zkeys, twin_scalars, which):
    c = zkeys[which]
    d, s = twin_scalars[:2]
    assert (d, s) == scalars(BEACON, EXP, 2)
    for key, name in (("named", "final"), ("bare", None)):
        got, h = c[key]
        want, wh = amd.zkey_contribute(c["old"], name, d, s, device=0)
        assert h == wh
        gs, ws = _zkey_sections(got), _zkey_sections(want)
        for sid in range(1, 10):
            assert gs[sid] == ws[sid], sid
        (gcs, grecs), (wcs, wrecs) = parse_section10(gs[10]), parse_section10(ws[10])
        assert gcs == wcs and len(grecs) == len(wrecs) == (2 if which == "small" else 1)
        assert [r["raw"] for r in grecs[:-1]] == [r["raw"] for r in wrecs[:-1]]
        assert grecs[-1]["raw"][:ZKEY_FIXED - 8] == wrecs[-1]["raw"][:ZKEY_FIXED - 8]
        assert (wrecs[-1]["type"], wrecs[-1]["params"]) == (0, name_params(name))
        assert (grecs[-1]["type"], grecs[-1]["params"]) == (1, beacon_params(name, BEACON, EXP))
        assert got == _zkey_retype(want, -1, 1, beacon_params(name, BEACON, EXP))
        assert h == zref.contribution_hash(grecs[-1])


def test_zkey_beacon_file_form_equals_the_memory_form(amd, zkeys, tmp_path):
    c = zkeys["tiny"]
    src, out = tmp_path / "old.zkey", tmp_path / "new.zkey"
    src.write_bytes(c["old"])
    hb = ctypes.create_string_buffer(64)
    assert amd.load().g16_zkey_beacon_files(str(src).encode(), str(out).encode(), None, BEACON, len(BEACON), EXP, 0, hb) == 0
    assert (out.read_bytes(), hb.raw) == c["bare"]


@pytest.mark.parametrize("which", ["tiny", "small"])
def test_zkey_verify_from_init_accepts_the_beacon_and_a_contribution_on_top(amd, zkeys, which):
    c = zkeys[which]
    base = open(golden_path(which + ".zkey"), "rb").read()
    for key in ("named", "bare"):
        for init in {base, c["old"]}:
            ok, why = amd.zkey_verify_from_init(init, c[key][0], device=0)
            assert ok and why == "", why
    more, _ = amd.zkey_contribute(c["named"][0], "after", 5, 7, device=0)
    assert [r["type"] for r in parse_section10(_zkey_sections(more)[10])[1]][-2:] == [1, 0]
    ok, why = amd.zkey_verify_from_init(base, more, device=0)
    assert ok and why == "", why


@pytest.mark.parametrize("tamper", ["hash_byte", "e_10_to_11", "id3_removed", "e_9"])
def test_zkey_verify_rejects_a_record_that_is_not_its_beacon(amd, zkeys, ceremony, tamper):
    params, text = _tampers("final")[tamper]
    c = zkeys["small"]
    ok, why = amd.zkey_verify_from_init(c["old"], _zkey_retype(c["named"][0], -1, 1, params), device=0)
    assert not ok and why == "zkey verify: " + text
    bad = _zkey_retype(ceremony["final"], -1, 1, params)
    ok, why = amd.zkey_verify_from_init(ceremony["init"], bad, device=0, ptau=ceremony["ptau"])
    assert not ok and why == "zkey verify: " + text
    ok, why = amd.zkey_verify_r1cs(ceremony["r1cs"], ceremony["ptau"], bad, device=0)
    assert not ok and why == "zkey verify: " + text


def test_zkey_verify_rejects_an_ordinary_record_that_claims_to_be_a_beacon(amd, zkeys, ceremony):
    c = zkeys["small"]
    base = open(golden_path("small.zkey"), "rb").read()
    flipped = _zkey_retype(c["named"][0], 0, 1, name_params("earlier"))
    ok, why = amd.zkey_verify_from_init(base, flipped, device=0)
    assert not ok and why == "zkey verify: " + NOT_STATED
    # a type-1 record among the INITIAL key's is carried, not judged: only further records are checked
    ok, why = amd.zkey_verify_from_init(_zkey_retype(c["old"], 0, 1, name_params("earlier")), flipped, device=0)
    assert ok, why
    ok, why = amd.zkey_verify_r1cs(ceremony["r1cs"], ceremony["ptau"], _zkey_retype(ceremony["final"], 0, 1, name_params("first")), device=0)
    assert not ok and why == "zkey verify: " + NOT_STATED


def test_zkey_verify_reports_a_broken_chain_before_a_beacon_that_is_not_its_key(amd, zkeys):
    """Two failures in one run: the first new record's delta does not continue the chain (the initial key states
    another delta1), and the LATER beacon record's key is not the beacon's.  The verdicts of the pairing checks come
    first, in the order the checks were collected; a beacon's verdict follows them."""
    chain_text = "zkey verify: a contribution's delta does not continue the chain"
    base = open(golden_path("small.zkey"), "rb").read()
    secs = f.read_binfile(base, "zkey", 2)
    order = sorted(secs, key=lambda sid: secs[sid][0][0])
    hdr = f.section(base, secs, 2)
    doubled = f.g1_to_lem(b.G1.mul(f.g1_from_lem(hdr[468:532]), 2))
    other_init = f.write_binfile("zkey", struct.unpack_from("<I", base, 4)[0],
                                 [(sid, hdr[:468] + doubled + hdr[532:] if sid == 2 else f.section(base, secs, sid)) for sid in order])
    good = zkeys["small"]["named"][0]
    bad_beacon = _zkey_retype(good, -1, 1, _tampers("final")["hash_byte"][0])
    assert [r["type"] for r in parse_section10(_zkey_sections(bad_beacon)[10])[1]] == [0, 1]
    assert amd.zkey_verify_from_init(other_init, good, device=0) == (False, chain_text)                      # each alone
    assert amd.zkey_verify_from_init(base, bad_beacon, device=0) == (False, "zkey verify: " + NOT_THE_KEY)
    assert amd.zkey_verify_from_init(other_init, bad_beacon, device=0) == (False, chain_text)                # together


def test_a_ceremony_closed_by_two_beacons_verifies_from_the_r1cs(amd, ceremony):
    """phase 1 ends with a beacon, `groth16 setup` reads that file, phase 2 ends with a beacon: every verifier accepts,
    a further contribution included, and the key still goes through `export bellman`"""
    for key in (ceremony["init"], ceremony["one"], ceremony["final"]):
        ok, why = amd.zkey_verify_r1cs(ceremony["r1cs"], ceremony["ptau"], key, device=0)
        assert ok and why == "", why
    ok, why = amd.zkey_verify_from_init(ceremony["init"], ceremony["final"], device=0, ptau=ceremony["ptau"])
    assert ok and why == "", why
    more, _ = amd.zkey_contribute(ceremony["final"], None, 11, 13, device=0)
    ok, why = amd.zkey_verify_r1cs(ceremony["r1cs"], ceremony["ptau"], more, device=0)
    assert ok and why == "", why
    recs = parse_section10(_zkey_sections(ceremony["final"])[10])[1]
    assert [r["type"] for r in recs] == [0, 1] and walk(recs[1]["params"]) == (EXP, BEACON)
    assert len(amd.zkey_export_bellman(ceremony["final"], device=0)) > 0
