"""The phase-2 MPCParams exchange on the device (csrc/zkey_bellman.hip, csrc/zkey_bellman_host.cpp, the to-be stage of
csrc/ptau_points.hip): `zkey export bellman`, `zkey bellman contribute`, `zkey import bellman`.  The ceremony's tau is
known, so H of an exported key is compared byte for byte with the closed form [tau^k (tau^N - 1) / delta] G from the
oracle's fixed-base multiplication (no transform in common with the code under test); the basis change alone is compared
with the twin's O(N^2) sum (tests/zkey_bellman_ref.py); both contribution routes must agree; `zkey verify` accepts what
the import writes and names what is wrong with tampered responses."""
import struct

import pytest

import bn254 as b
import formats as f
import groth16 as g
import test_gpu_zkey_contribute as zc
import zkey_bellman_ref as ref
import zkey_mpc_ref as mref
from bn254 import R
from test_gpu_zkey_contribute import CASES, D1, D2, S

pytestmark = pytest.mark.gpu

S9_TEXT = "zkey verify: sections 8 and 9 are not the initial key's scaled by 1 / delta"
H_TEXT = "zkey verify: section 9 is not the ceremony's H basis scaled by 1 / delta"
_ptau, _route = {}, {}


def _domain(c):
    return c["zk"]["domainSize"]


def _log(N):
    return N.bit_length() - 1


def _ptau_of(amd, name):
    if name not in _ptau:
        c = zc._case(amd, name)
        td = c["td"]
        _ptau[name] = amd.ptau_synth(_log(_domain(c)), td["tau"], td["alpha"], td["beta"], device=0)
    return _ptau[name]


def _s9_scalars(c, delta):
    """Section 9 in the exponent: L^{2N}_{2i+1}(tau) / delta."""
    N = _domain(c)
    lag = g.lagrange_at(2 * N, c["td"]["tau"])
    dinv = pow(delta, -1, R)
    return [lag[2 * i + 1] * dinv % R for i in range(N)]


def _routes(amd, name):
    """z1 = zkey contribute, z1p = the same contribution through the file exchange; once per case."""
    if name not in _route:
        c = zc._case(amd, name)
        init = c["init"]
        z1, h1 = amd.zkey_contribute(init, "first", D1, S, device=0)
        exp = amd.zkey_export_bellman(init, device=0)
        resp, hr = amd.zkey_bellman_contribute(exp, D1, S, device=0)
        z1p = amd.zkey_import_bellman(init, resp, "first", device=0)
        _route[name] = {"c": c, "init": init, "z1": z1, "h1": h1, "exp": exp, "resp": resp, "hr": hr, "z1p": z1p}
    return _route[name]


def _h_be(c, delta):
    return ref.run_be(ref.points(ref.h_closed_form(c["td"]["tau"], _domain(c), delta)), 64)


# ------------------------------------------------------------------ 1. closed form
@pytest.mark.parametrize("name", list(CASES))
def test_export_equals_closed_form_and_twin(amd, name):
    c = zc._case(amd, name)
    N = _domain(c)
    got = amd.zkey_export_bellman(c["init"], device=0)
    m = ref.parse_mpcparams(got)
    want_h = _h_be(c, 1)
    assert len(m["H"]) == 64 * (N - 1) and m["H"] == want_h
    assert got == ref.write_mpcparams(zc._sections(c["init"]), want_h)
    z1, _ = amd.zkey_contribute(c["init"], "first", D1, S, device=0)
    got1 = amd.zkey_export_bellman(z1, device=0)
    want_h1 = _h_be(c, D1)
    assert ref.parse_mpcparams(got1)["H"] == want_h1
    assert got1 == ref.write_mpcparams(zc._sections(z1), want_h1)
    assert len(ref.parse_mpcparams(got1)["records"]) == 1


# ------------------------------------------------------------------ 2. the basis change alone
_layer = {}


def _layer_case(L):
    if L not in _layer:
        N = 1 << L
        a = [pow(11 + i, 1000 + 3 * i, R) for i in range(N)]
        _layer[L] = (a, ref.points(a), ref.points(ref.basis_forward(a, L)), ref.points(ref.basis_inverse(a, L)))
    return _layer[L]


@pytest.mark.parametrize("L", [0, 1, 2, 8, 9, 10])
def test_h_basis_equals_the_plain_sum(amd, L):
    """L = 0: the twist alone; 8, 9, 10: around one 256-lane workgroup and the first stages that cross workgroups."""
    _, pts, fwd, inv = _layer_case(L)
    got_f = amd.zkey_h_basis(pts, L)
    got_i = amd.zkey_h_basis(pts, L, inverse=True)
    assert got_f == fwd
    assert got_i == inv
    assert amd.zkey_h_basis(got_f, L, inverse=True) == pts
    assert amd.zkey_h_basis(got_i, L) == pts


SPECIAL = {"all_infinity": [0] * 8, "only_first": [5] + [0] * 7, "only_last": [0] * 7 + [5], "all_equal": [9] * 8,
           "opposite_pairs": [3, R - 3] * 4}


@pytest.mark.parametrize("what", list(SPECIAL))
def test_h_basis_special_inputs(amd, what):
    """Infinity, equal and opposite operands in the butterflies (L = 3)."""
    a = SPECIAL[what]
    pts = ref.points(a)
    assert amd.zkey_h_basis(pts, 3) == ref.points(ref.basis_forward(a, 3))
    assert amd.zkey_h_basis(pts, 3, inverse=True) == ref.points(ref.basis_inverse(a, 3))


def test_h_basis_lane_knob_gives_the_same_bytes(amd, monkeypatch):
    _, pts, fwd, inv = _layer_case(9)
    monkeypatch.setenv("G16_BELLMAN_LANES", "64")
    assert amd.zkey_h_basis(pts, 9) == fwd
    monkeypatch.setenv("G16_BELLMAN_LANES", "192")
    assert amd.zkey_h_basis(pts, 9, inverse=True) == inv


# ------------------------------------------------------------------ 3. special ceremonies
def _key_for_tau(amd, tau, transformed=False):
    """The small circuit's fresh key for another tau.  transformed: the Lagrange sections come from `prepare phase2` over
    a ceremony one power larger (a full block for this domain) instead of ptau_synth's closed form, which divides by
    tau - w^j and so cannot take a root of unity."""
    n, p, m, seed = CASES["small"]
    c = zc._case(amd, "small")
    td = c["td"]
    N = _domain(c)
    if transformed:
        ptau = amd.ptau_prepare(amd.ptau_synth(_log(N) + 1, tau, td["alpha"], td["beta"], prepared=False, device=0), device=0)
    else:
        ptau = amd.ptau_synth(_log(N), tau, td["alpha"], td["beta"], device=0)
    return amd.groth16_setup_ptau(f.write_r1cs(n, p, 0, c["rows"]), ptau, device=0), N


def test_tau_one_every_h_point_is_infinity(amd):
    init, N = _key_for_tau(amd, 1)
    assert zc._sections(init)[9] == bytes(64 * N)
    exp = amd.zkey_export_bellman(init, device=0)
    assert ref.parse_mpcparams(exp)["H"] == ref.G1_INF_BE * (N - 1)
    resp, _ = amd.zkey_bellman_contribute(exp, D1, S, device=0)
    assert ref.parse_mpcparams(resp)["H"] == ref.G1_INF_BE * (N - 1)
    new = amd.zkey_import_bellman(init, resp, "one", device=0)
    assert zc._sections(new)[9] == bytes(64 * N)


def test_tau_a_root_of_unity(amd):
    N = _domain(zc._case(amd, "small"))
    w = b.fr_root(_log(N) + 1)
    init, _ = _key_for_tau(amd, w, transformed=True)
    assert zc._sections(init)[9] == f.g1_to_lem(b.G1_GEN) + bytes(64 * (N - 1))
    exp = amd.zkey_export_bellman(init, device=0)
    assert ref.parse_mpcparams(exp)["H"] == ref.run_be(ref.points(ref.h_closed_form(w, N)), 64)
    resp, _ = amd.zkey_bellman_contribute(exp, D1, S, device=0)
    new = amd.zkey_import_bellman(init, resp, None, device=0)
    a = [pow(D1, -1, R)] + [0] * (N - 1)
    assert zc._sections(new)[9] == ref.points(ref.project(a, _log(N)))


# ------------------------------------------------------------------ 4. both routes agree
@pytest.mark.parametrize("name", ["small", "large"])
def test_both_routes_agree(amd, name):
    r = _routes(amd, name)
    c = r["c"]
    L = _log(_domain(c))
    a, bb = zc._sections(r["z1"]), zc._sections(r["z1p"])
    assert sorted(a) == sorted(bb) == list(range(1, 11))
    for sid in (1, 2, 3, 4, 5, 6, 7, 8, 10):
        assert a[sid] == bb[sid], f"section {sid}"
    assert r["hr"] == r["h1"]
    assert bb[9] == ref.points(ref.project(_s9_scalars(c, D1), L))
    assert a[9] == ref.points(_s9_scalars(c, D1)) and a[9] != bb[9]
    # from the imported key on, the two routes give the same bytes
    z2, h2 = amd.zkey_contribute(r["z1p"], "second", D2, S + 1, device=0)
    resp2, hr2 = amd.zkey_bellman_contribute(amd.zkey_export_bellman(r["z1p"], device=0), D2, S + 1, device=0)
    z2p = amd.zkey_import_bellman(r["z1p"], resp2, "second", device=0)
    assert z2p == z2 and hr2 == h2


def test_a_response_with_two_new_records(amd):
    r = _routes(amd, "small")
    c = r["c"]
    resp2, _ = amd.zkey_bellman_contribute(r["resp"], D2, S + 1, device=0)
    assert len(ref.parse_mpcparams(resp2)["records"]) == 2
    got = zc._sections(amd.zkey_import_bellman(r["init"], resp2, "both", device=0))
    one, _ = amd.zkey_contribute(r["init"], "both", D1, S, device=0)
    two, _ = amd.zkey_contribute(one, "both", D2, S + 1, device=0)
    want = zc._sections(two)
    for sid in (1, 2, 3, 4, 5, 6, 7, 8, 10):
        assert got[sid] == want[sid], f"section {sid}"
    assert got[9] == ref.points(ref.project(_s9_scalars(c, D1 * D2 % R), _log(_domain(c))))


# ------------------------------------------------------------------ 5. proofs
@pytest.mark.parametrize("name", ["small", "large"])
def test_both_keys_give_the_same_proof(amd, name):
    r = _routes(amd, name)
    c = r["c"]
    wtns = f.write_wtns(c["w"])
    rr, ss = f.le(0x1111 ** 9 % R), f.le(0x2222 ** 9 % R)
    proofs = []
    for key in (r["z1"], r["z1p"]):
        prover = amd.Prover(key, device=0)
        proofs.append(prover.prove(wtns, rr, ss))
        prover.close()
    assert proofs[0] == proofs[1]
    proof, pub = proofs[1]
    pts = (f.g1_from_obj(proof["pi_a"]), f.g2_from_obj(proof["pi_b"]), f.g1_from_obj(proof["pi_c"]))
    assert g.verify(f.read_zkey(r["z1p"]), [int(x) for x in pub], pts)


# ------------------------------------------------------------------ 6. verify accepts
@pytest.mark.parametrize("name", ["small", "large"])
def test_verify_accepts_the_imported_key(amd, name):
    r = _routes(amd, name)
    ok, why = amd.zkey_verify_from_init(r["init"], r["z1p"], device=0)
    assert ok and why == "", why
    ok, why = amd.zkey_verify_from_init(r["init"], r["z1p"], device=0, ptau=_ptau_of(amd, name))
    assert ok and why == "", why


def test_verify_accepts_a_chain_that_continues_the_imported_key(amd):
    r = _routes(amd, "small")
    z2, _ = amd.zkey_contribute(r["z1p"], "second", D2, S + 1, device=0)
    for ptau in (None, _ptau_of(amd, "small")):
        ok, why = amd.zkey_verify_from_init(r["init"], z2, device=0, ptau=ptau)
        assert ok, why
    ok, why = amd.zkey_verify_from_init(r["z1p"], z2, device=0)
    assert ok, why


# ------------------------------------------------------------------ 7. verify rejects
def _with_h(resp, h):
    m = ref.parse_mpcparams(resp)
    at = m["at"]["H"] + 4
    return resp[:at] + h + resp[at + len(h):]


@pytest.mark.parametrize("what", ["h_of_another_d", "h_swapped"])
def test_verify_rejects_a_tampered_h(amd, what):
    r = _routes(amd, "small")
    h = ref.parse_mpcparams(r["resp"])["H"]
    if what == "h_of_another_d":
        other, _ = amd.zkey_bellman_contribute(r["exp"], D1 + 5, S, device=0)
        bad_h = ref.parse_mpcparams(other)["H"]
    else:
        assert h[:64] != h[64:128]
        bad_h = h[64:128] + h[:64] + h[128:]
    assert bad_h != h
    key = amd.zkey_import_bellman(r["init"], _with_h(r["resp"], bad_h), "first", device=0)   # the import does not judge
    ok, why = amd.zkey_verify_from_init(r["init"], key, device=0)
    assert not ok and why == S9_TEXT, why
    ok, why = amd.zkey_verify_from_init(r["init"], key, device=0, ptau=_ptau_of(amd, "small"))
    assert not ok and why in (S9_TEXT, H_TEXT), why


# ------------------------------------------------------------------ 8. import verdicts
def _import_verdict(amd, key, resp):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_import_bellman(key, resp, "x", device=0)
    assert e.value.code == 0, str(e.value)
    return str(e.value)


def test_import_verdicts(amd):
    r = _routes(amd, "small")
    init, resp = r["init"], r["resp"]
    m = ref.parse_mpcparams(resp)
    at = m["at"]
    lead = "zkey import bellman: "
    fewer = resp[:at["L"]] + struct.pack(">I", len(m["L"]) // 64 - 1) + m["L"][64:] + resp[at["A"]:]
    assert _import_verdict(amd, init, fewer) == lead + "a count is not the key's"
    a = m["A"]
    i, j = [k for k in range(len(a) // 64) if a[k * 64:(k + 1) * 64] != ref.G1_INF_BE][:2]
    assert a[i * 64:(i + 1) * 64] != a[j * 64:(j + 1) * 64]
    swapped = resp[:at["A"] + 4] + zc._swap(a, i, j, 64) + resp[at["B1"]:]
    assert _import_verdict(amd, init, swapped) == lead + "alpha, beta, gamma, IC, A, B1 or B2 differ from the key's"
    cs = at["csHash"]
    assert _import_verdict(amd, init, resp[:cs] + bytes([resp[cs] ^ 1]) + resp[cs + 1:]) == lead + "the circuit hash differs from the key's"
    assert _import_verdict(amd, init, r["exp"]) == lead + "the response holds no new contribution"
    # the key after the contribution against a response of two records whose first one is altered
    resp2, _ = amd.zkey_bellman_contribute(resp, D2, S + 1, device=0)
    ra = ref.parse_mpcparams(resp2)["at"]["records"]
    altered = resp2[:ra + 330] + bytes([resp2[ra + 330] ^ 1]) + resp2[ra + 331:]
    assert _import_verdict(amd, r["z1p"], altered) == lead + "the contributions do not begin with the key's"
    assert zc._sections(amd.zkey_import_bellman(r["z1p"], resp2, "x", device=0))[10][64:68] == struct.pack("<I", 2)
    inf = resp[:ref.DELTA1] + ref.G1_INF_BE + resp[ref.DELTA1 + 64:]
    assert _import_verdict(amd, init, inf) == lead + "delta1 or delta2 is the point at infinity"


def test_a_point_off_its_curve_is_a_format_error(amd):
    r = _routes(amd, "small")
    at = ref.parse_mpcparams(r["resp"])["at"]
    for run in ("H", "L", "B1"):
        pos = at[run] + 4 + 32
        bad = r["resp"][:pos] + (5).to_bytes(32, "big") + r["resp"][pos + 32:]
        with pytest.raises(amd.G16Error) as e:
            amd.zkey_import_bellman(r["init"], bad, "x", device=0)
        assert e.value.code == -2 and str(e.value) == "mpcparams: Invalid File format"
    pos = at["H"] + 4 + 32
    bad = r["exp"][:pos] + (5).to_bytes(32, "big") + r["exp"][pos + 32:]
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_bellman_contribute(bad, D1, S, device=0)
    assert e.value.code == -2 and str(e.value) == "mpcparams: Invalid File format"


# ------------------------------------------------------------------ 9. driver knobs
@pytest.mark.parametrize("env", [{"G16_PTAU_CHUNK": "50", "G16_PTAU_LANES": "64", "G16_BELLMAN_LANES": "64",
                                  "G16_CONTRIBUTE_CHUNK": "50", "G16_CONTRIBUTE_LANES": "64"},
                                 {"G16_PTAU_CHUNK": "127", "G16_BELLMAN_LANES": "192"}],
                         ids=["chunk50_lanes64", "chunk127_lanes192"])
def test_chunk_and_lane_knobs_give_the_same_bytes(amd, monkeypatch, env):
    """mid: 127 H points, 143 L points, 150 of A -- several chunks with a short last one, grid-stride passes."""
    r = _routes(amd, "mid")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    exp = amd.zkey_export_bellman(r["init"], device=0)
    assert exp == r["exp"]
    resp, h = amd.zkey_bellman_contribute(exp, D1, S, device=0)
    assert resp == r["resp"] and h == r["hr"]
    assert amd.zkey_import_bellman(r["init"], resp, "first", device=0) == r["z1p"]


# ------------------------------------------------------------------ 10. the CSPRNG path
def test_random_contribution_verifies(amd):
    r = _routes(amd, "small")
    resp, h = amd.zkey_bellman_contribute(r["exp"], device=0)
    assert resp != r["resp"] and h == mref.blake2b(ref.parse_mpcparams(resp)["records"][0])
    ok, why = amd.zkey_verify_from_init(r["init"], amd.zkey_import_bellman(r["init"], resp, None, device=0), device=0)
    assert ok, why
