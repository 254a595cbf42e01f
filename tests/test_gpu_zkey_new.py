"""`zkey new` with the circuit hash on the device (csrc/zkey_cshash.hip, csrc/zkey_cshash_host.cpp).  The ceremony's tau
is known, so the hash is compared with hashlib's Blake2b-512 over the twin's MPCParams image (tests/zkey_bellman_ref.py)
whose H run is the closed form [tau^k (tau^N - 1)] G from big-integer scalars -- nothing in common with the kernel; the
second device route to the same bytes, `zkey export bellman` (a basis change over section 9), must agree; the
difference kernel alone is compared with (a[k+N] - a[k]) G for arbitrary scalars, every kind of exceptional operand
included; and `zkey verify` accepts a chain from the hashed key and names a tampered hash."""
import subprocess
import sys

import pytest

import formats as f
import test_gpu_zkey_contribute as zc
import zkey_bellman_ref as ref
import zkey_mpc_ref as mref
from bn254 import R
from conftest import ROOT
from test_gpu_zkey_contribute import CASES, D1, D2, S

pytestmark = pytest.mark.gpu

H_BATCH = 8     # kHBatch of csrc/zkey_cshash.hip: consecutive k one lane inverts together; a workgroup has 256 lanes
BEACON = bytes((37 * i + 11) & 0xff for i in range(32))
HASH_TEXT = "zkey verify: the circuit hash differs from the initial key's"
_made = {}


def _log(N):
    return N.bit_length() - 1


def _made_of(amd, name):
    """the case's r1cs and ptau, its legacy key (groth16_setup_ptau) and its hashed key (zkey_new), once"""
    if name not in _made:
        c = zc._case(amd, name)
        n, p, _, _ = CASES[name]
        td = c["td"]
        N = c["zk"]["domainSize"]
        r1cs = f.write_r1cs(n, p, 0, c["rows"])
        ptau = amd.ptau_synth(_log(N), td["tau"], td["alpha"], td["beta"], device=0)
        key, h = amd.zkey_new(r1cs, ptau, device=0)
        _made[name] = {"c": c, "N": N, "r1cs": r1cs, "ptau": ptau, "legacy": c["init"], "key": key, "hash": h}
    return _made[name]


def _image_hash(sections, h_be):
    """Blake2b-512 of the twin's MPCParams image with this H run, cut at its csHash field"""
    image = ref.write_mpcparams(sections, h_be)
    return mref.blake2b(image[:ref.parse_mpcparams(image)["at"]["csHash"]])


# ------------------------------------------------------------------ 1. closed form
@pytest.mark.parametrize("name", list(CASES))
def test_key_and_hash_equal_the_closed_form(amd, name):
    m = _made_of(amd, name)
    got, want = zc._sections(m["key"]), zc._sections(m["legacy"])
    assert list(got) == list(want) and sorted(got) == list(range(1, 11))     # section order and ids
    for sid in range(1, 10):
        assert got[sid] == want[sid], f"section {sid}"
    assert want[10] == bytes(68)
    assert got[10] == m["hash"] + bytes(4)
    h_be = ref.run_be(ref.points(ref.h_closed_form(m["c"]["td"]["tau"], m["N"], 1)), 64)
    assert m["hash"] == _image_hash(want, h_be)
    assert amd.zkey_cs_hash(m["legacy"], m["ptau"], device=0) == m["hash"]
    assert amd.zkey_cs_hash(m["key"], m["ptau"], device=0) == m["hash"]       # section 10 is not read


# ------------------------------------------------------------------ 2. two routes
@pytest.mark.parametrize("name", list(CASES))
def test_export_bellman_hashes_to_the_same_value(amd, name):
    m = _made_of(amd, name)
    image = amd.zkey_export_bellman(m["key"], device=0)
    p = ref.parse_mpcparams(image)
    assert p["csHash"] == m["hash"]
    assert mref.blake2b(image[:p["at"]["csHash"]]) == m["hash"]


# ------------------------------------------------------------------ 3. the kernel alone
_layer = {}


def _diff_be(a, L):
    N = 1 << L
    return ref.run_be(ref.points([(a[k + N] - a[k]) % R for k in range(N - 1)]), 64)


def _layer_case(L):
    if L not in _layer:
        a = [pow(13 + i, 900 + 5 * i, R) for i in range((2 << L) - 1)]
        _layer[L] = (ref.points(a), _diff_be(a, L))
    return _layer[L]


@pytest.mark.parametrize("L", [0, 1, 2, 8, 9, 10])
def test_h_monomial_equals_the_difference_in_the_exponent(amd, L):
    """L = 0: nothing to write; 1, 2: one short run; 8, 9, 10: 255, 511, 1023 differences = 32, 64, 128 runs of H_BATCH = 8
    with a last run of 7 -- half a wavefront, one, two."""
    pts, want = _layer_case(L)
    got = amd.zkey_h_monomial(pts, L)
    assert len(got) == 64 * ((1 << L) - 1)
    assert got == want


CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
amd = entry.load_package()
pts = open(sys.argv[2], "rb").read()
for i, (chunk, lanes) in enumerate(((96, 64), (1000, 64), (1000, 128), (8, 64), (9, 192))):
    os.environ["G16_CSHASH_CHUNK"], os.environ["G16_CSHASH_LANES"] = str(chunk), str(lanes)
    open(sys.argv[3] + str(i), "wb").write(amd.zkey_h_monomial(pts, 10))
"""


def test_h_monomial_chunk_and_lane_knobs_in_a_fresh_process(amd, tmp_path):
    """1023 differences in a child process that sets the knobs before the library reads them: chunks of 96 (eleven, the
    last of 63, twelve runs each); chunks of 1000 over 64 lanes (125 runs: grid-stride passes) and over 128 (two
    workgroups of 64); chunks of one run and of one run and a point."""
    pts, want = _layer_case(10)
    (tmp_path / "pts").write_bytes(pts)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "pts"), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for i in range(5):
        assert (tmp_path / ("out%d" % i)).read_bytes() == want, i


# ------------------------------------------------------------------ 4. exceptional operands
def _special(what, L):
    """scalars a[0 .. 2N-1) whose differences a[k+N] - a[k] are of the wanted kinds"""
    N = 1 << L
    lo = [pow(5 + k, 77 + k, R) for k in range(N)]
    hi = [pow(9 + k, 55 + k, R) for k in range(N - 1)]
    for k in range(N - 1):
        kind = {"all_equal": 0, "all_opposite": 1, "infinity_low": 2, "infinity_high": 3, "infinity_both": 4,
                "alternating": (0, 1, 2, 5, 3, 5, 4, 5)[k % 8], "alternating_shifted": (5, 5, 5, 0, 1, 5, 2, 3)[(k + 3) % 8]}[what]
        if kind == 0:
            hi[k] = lo[k]
        elif kind == 1:
            hi[k] = R - lo[k]
        elif kind == 2:
            lo[k] = 0
        elif kind == 3:
            hi[k] = 0
        elif kind == 4:
            lo[k] = hi[k] = 0
    return lo + hi


@pytest.mark.parametrize("L", [3, 8])
@pytest.mark.parametrize("what", ["all_equal", "all_opposite", "infinity_low", "infinity_high", "infinity_both",
                                  "alternating", "alternating_shifted"])
def test_h_monomial_exceptional_operands(amd, what, L):
    """equal operands (infinity out), opposite ones (doublings), infinity on either side and on both, and runs in which
    these and ordinary differences alternate, so entries without a denominator sit between entries with one"""
    a = _special(what, L)
    got = amd.zkey_h_monomial(ref.points(a), L)
    if what in ("all_equal", "infinity_both"):
        assert got == ref.G1_INF_BE * ((1 << L) - 1)
    assert got == _diff_be(a, L)


def test_tau_one_the_image_holds_no_h_point(amd):
    """powersoftau new + prepare phase2: every point of section 2 is the generator, every difference infinity"""
    n, p, _, _ = CASES["small"]
    c = zc._case(amd, "small")
    N = c["zk"]["domainSize"]
    r1cs = f.write_r1cs(n, p, 0, c["rows"])
    ptau = amd.ptau_prepare(amd.ptau_new(_log(N)), device=0)
    key, h = amd.zkey_new(r1cs, ptau, device=0)
    legacy = zc._sections(amd.groth16_setup_ptau(r1cs, ptau, device=0))
    # (section 9 itself is NOT all infinity here: the top block of `prepare phase2` deviates from the Lagrange basis by
    # a multiple of tau^(M-1), which the monomial entries k <= N - 2 do not see -- the export below shows that)
    assert h == _image_hash(legacy, ref.G1_INF_BE * (N - 1))
    assert zc._sections(key)[10] == h + bytes(4)
    image = amd.zkey_export_bellman(key, device=0)
    assert mref.blake2b(image[:ref.parse_mpcparams(image)["at"]["csHash"]]) == h


# ------------------------------------------------------------------ 5. the chain
def test_chain_from_the_hashed_key(amd):
    m = _made_of(amd, "small")
    one, _ = amd.zkey_contribute(m["key"], "first", D1, S, device=0)
    two, _ = amd.zkey_beacon(one, BEACON, 10, "final", device=0)
    ok, why = amd.zkey_verify_r1cs(m["r1cs"], m["ptau"], two, device=0)
    assert ok and why == "", why
    # the first record's transcript is chained from the real hash
    cs, recs = mref.parse_section10(zc._sections(one)[10])
    assert cs == m["hash"]
    assert recs[0]["transcript"] == mref.transcript_hash(m["hash"], [], recs[0]["g1_s"], recs[0]["g1_sx"])
    assert recs[0]["transcript"] != mref.transcript_hash(bytes(64), [], recs[0]["g1_s"], recs[0]["g1_sx"])
    # one bit of csHash flipped
    s10 = bytearray(zc._sections(two)[10])
    s10[17] ^= 0x20
    ok, why = amd.zkey_verify_r1cs(m["r1cs"], m["ptau"], zc._rewrite(two, {10: bytes(s10)}), device=0)
    assert not ok and why == HASH_TEXT
    # against the initial keys themselves: each chain belongs to its own
    ok, why = amd.zkey_verify_from_init(m["key"], two, device=0, ptau=m["ptau"])
    assert ok, why
    ok, why = amd.zkey_verify_from_init(m["legacy"], two, device=0)
    assert not ok and why == HASH_TEXT


def test_a_legacy_chain_is_still_accepted(amd):
    m = _made_of(amd, "small")
    one, _ = amd.zkey_contribute(m["legacy"], "first", D1, S, device=0)
    two, _ = amd.zkey_contribute(one, "second", D2, S + 1, device=0)
    assert zc._sections(two)[10][:64] == bytes(64)
    ok, why = amd.zkey_verify_r1cs(m["r1cs"], m["ptau"], two, device=0)
    assert ok and why == "", why
    ok, why = amd.zkey_verify_r1cs(m["r1cs"], m["ptau"], m["legacy"], device=0)
    assert ok and why == "", why
    ok, why = amd.zkey_verify_r1cs(m["r1cs"], m["ptau"], m["key"], device=0)
    assert ok and why == "", why


# ------------------------------------------------------------------ 6. file forms
def test_file_forms_give_the_same_bytes(amd, tmp_path):
    import ctypes as C
    m = _made_of(amd, "small")
    lib = amd.load()
    for name, data in (("c.r1cs", m["r1cs"]), ("pot.ptau", m["ptau"]), ("legacy.zkey", m["legacy"])):
        (tmp_path / name).write_bytes(data)
    path = {k: str(tmp_path / k).encode() for k in ("c.r1cs", "pot.ptau", "legacy.zkey", "new.zkey")}
    h = C.create_string_buffer(64)
    assert lib.g16_zkey_new_files(path["c.r1cs"], path["pot.ptau"], path["new.zkey"], 0, h) == 0, lib.g16_last_error()
    assert (tmp_path / "new.zkey").read_bytes() == m["key"] and h.raw == m["hash"]
    h2 = C.create_string_buffer(64)
    assert lib.g16_zkey_cs_hash_files(path["legacy.zkey"], path["pot.ptau"], 0, h2) == 0, lib.g16_last_error()
    assert h2.raw == m["hash"]
    assert lib.g16_zkey_new_files(path["c.r1cs"], path["pot.ptau"], path["new.zkey"], 0, None) == 0
    assert (tmp_path / "new.zkey").read_bytes() == m["key"]
    ok = C.c_int(0)
    assert lib.g16_zkey_verify_r1cs_files(path["c.r1cs"], path["pot.ptau"], path["new.zkey"], 0, C.byref(ok)) == 0
    assert ok.value == 1, lib.g16_last_error()


def test_driver_knobs_do_not_change_the_hash(amd, monkeypatch):
    """mid: 127 H points, 143 of L, 150 of A -- several chunks with a short last one through every run of the image"""
    m = _made_of(amd, "mid")
    for k, v in {"G16_CSHASH_CHUNK": "50", "G16_CSHASH_LANES": "64", "G16_PTAU_CHUNK": "50", "G16_PTAU_LANES": "64"}.items():
        monkeypatch.setenv(k, v)
    assert amd.zkey_cs_hash(m["legacy"], m["ptau"], device=0) == m["hash"]
