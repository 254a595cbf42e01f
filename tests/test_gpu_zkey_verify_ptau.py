"""The ptau leg of `zkey verify` on the device (csrc/zkey_verify_h.hip, csrc/zkey_mpc.cpp step 6): the two scalar vectors
against the big-integer twin (tests/zkey_verify_ptau_ref.py) and the closed form; honest keys of every kind of ceremony
are accepted with 0, 1 and 2 contributions; a ceremony of another tau and a forged H basis -- which the check without
the ptau accepts -- are rejected."""
import pytest

import formats as f
import groth16 as g
import synth
from bn254 import R
from zkey_verify_ptau_ref import h_block, h_scalars_ref

pytestmark = pytest.mark.gpu

CASES = {"small": (24, 2, 12, 1), "mid": (150, 6, 120, 2), "tau1": (10, 1, 5, 3)}   # domains 2^4, 2^7, 2^3
S = 0x0123456789abcdef ** 3 % R
D1, D2 = 0x1f2e3d4c5b6a7988 ** 3 % R, 0x2b3f5d7c9e1a3b5c ** 3 % R
H_TEXT = "zkey verify: section 9 is not the ceremony's H basis scaled by 1 / delta"
SMALL_TEXT = "zkey verify: the ptau is too small for this key"
_cache = {}


def _log_domain(name):
    _, p, m, _ = CASES[name]
    L = 0
    while (1 << L) < m + p + 1:
        L += 1
    return L


def _chain(amd, name, kind):
    """The circuit `name` set up from a ceremony of `kind`, once: its .r1cs, the ceremony file and the keys with 0, 1 and
    2 contributions.  full: g16_ptau_synth at power = L (the full Lagrange block); bigger: at power L + 1; truncated:
    g16_ptau_prepare of the unprepared file at power = L (block L + 1 from 2N - 1 powers); tau1: g16_ptau_new at power 3,
    prepared (every H point is infinity)."""
    if (name, kind) not in _cache:
        n, p, m, seed = CASES[name]
        rows, _ = synth.make(n, p, m, seed)
        t = g.trapdoor(seed + 1000)
        L = _log_domain(name)
        if kind == "full":
            ptau = amd.ptau_synth(L, t["tau"], t["alpha"], t["beta"], device=0)
        elif kind == "bigger":
            ptau = amd.ptau_synth(L + 1, t["tau"], t["alpha"], t["beta"], device=0)
        elif kind == "truncated":
            ptau = amd.ptau_prepare(amd.ptau_synth(L, t["tau"], t["alpha"], t["beta"], prepared=False, device=0), device=0)
        else:
            assert kind == "tau1" and L == 3
            ptau = amd.ptau_prepare(amd.ptau_new(3), device=0)
        r1cs = f.write_r1cs(n, p, 0, rows)
        init = amd.groth16_setup_ptau(r1cs, ptau, device=0)
        one, _ = amd.zkey_contribute(init, "first", D1, S, device=0)
        two, _ = amd.zkey_contribute(one, "second", D2, S + 1, device=0)
        _cache[(name, kind)] = {"L": L, "tau": t, "r1cs": r1cs, "ptau": ptau, "keys": [init, one, two]}
    return _cache[(name, kind)]


def _sections(buf):
    secs = f.read_binfile(buf, "zkey", 2)
    return {sid: f.section(buf, secs, sid) for sid in secs}


def _rewrite(buf, repl):
    secs = f.read_binfile(buf, "zkey", 2)
    order = sorted(secs, key=lambda sid: secs[sid][0][0])
    return f.write_binfile("zkey", 1, [(sid, repl.get(sid, f.section(buf, secs, sid))) for sid in order])


def _forge(key):
    """points 0 and 1 of section 9 swapped"""
    s9 = _sections(key)[9]
    assert s9[:64] != s9[64:128] and bytes(64) not in (s9[:64], s9[64:128])
    return _rewrite(key, {9: s9[64:128] + s9[:64] + s9[128:]})


# ------------------------------------------------------------------ 1. the scalar vectors
def _u(L):
    N = 1 << L
    rng = synth.Xoshiro(40 + L)
    u = [rng.rand_fr() for _ in range(N - 1)] + [0]
    # the edges among random values (N = 2: r - 1 alone; N = 4: r - 1, 0, 1)
    for k, edge in zip(range(0, N - 1, max(1, (N - 1) // 5)), (R - 1, 0, 1, R - 2, 2)):
        u[k] = edge
    return u


@pytest.mark.parametrize("L", [1, 2, 5, 10, 11])
def test_h_scalars_equal_the_twin(amd, L):
    """L = 10, 11: more than one tile, so a second NTT pass runs"""
    N = 1 << L
    u = _u(L)
    rho, t = amd.zkey_h_scalars(u, L, device=0)
    want_rho, want_t = h_scalars_ref(u, L)
    assert len(t) == 2 * N - 1 and t[N - 1] == 0
    assert t == want_t
    assert rho == want_rho


@pytest.mark.parametrize("L", [1, 2, 5])
def test_h_scalars_satisfy_the_closed_form(amd, L):
    """the device's pair against the closed form itself, for both forms of the H block: the twin and the kernel cannot be
    wrong together"""
    N = 1 << L
    u = _u(L)
    tau = synth.Xoshiro(90 + L).rand_fr()
    rho, t = amd.zkey_h_scalars(u, L, device=0)
    rhs = sum(x * pow(tau, j, R) for j, x in enumerate(t)) % R
    assert rhs == sum(u[k] * (pow(tau, k, R) - pow(tau, k + N, R)) for k in range(N - 1)) % R
    for truncated in (False, True):
        assert 2 * N * sum(r * h for r, h in zip(rho, h_block(L, tau, truncated))) % R == rhs


# ------------------------------------------------------------------ 2. accepts
ACCEPT = [("small", "full"), ("small", "bigger"), ("small", "truncated"), ("tau1", "tau1"), ("mid", "full"),
          ("mid", "truncated")]


@pytest.mark.parametrize("contributions", [0, 1, 2])
@pytest.mark.parametrize("name,kind", ACCEPT, ids=["%s-%s" % nk for nk in ACCEPT])
def test_verify_accepts(amd, name, kind, contributions):
    c = _chain(amd, name, kind)
    ok, why = amd.zkey_verify_from_init(c["keys"][0], c["keys"][contributions], device=0, ptau=c["ptau"])
    assert ok and why == "", why


def test_tau1_ceremony_of_a_larger_power_has_only_infinity_in_section_9(amd):
    """below the ceremony's power the H block is the full Lagrange basis, at tau = 1 the point at infinity throughout: S
    is infinity point by point (at L = power, the case above, the points are -w^(2i+1) / 2N G and only their sum is)"""
    n, p = 6, 1
    rows = [([(2, 1)], [(3, 1)], [(4, 1)]), ([(1, 1)], [(2, 5)], [(3, R - 2)])]   # domain 2^2
    ptau = amd.ptau_prepare(amd.ptau_new(3), device=0)
    init = amd.groth16_setup_ptau(f.write_r1cs(n, p, 0, rows), ptau, device=0)
    assert _sections(init)[9] == bytes(4 * 64)
    one, _ = amd.zkey_contribute(init, None, D1, S, device=0)
    ok, why = amd.zkey_verify_from_init(init, one, device=0, ptau=ptau)
    assert ok, why


def test_an_unprepared_ptau_is_enough(amd):
    """only section 2 is read"""
    c = _chain(amd, "small", "full")
    t = c["tau"]
    bare = amd.ptau_synth(c["L"], t["tau"], t["alpha"], t["beta"], prepared=False, device=0)
    ok, why = amd.zkey_verify_from_init(c["keys"][0], c["keys"][2], device=0, ptau=bare)
    assert ok, why


# ------------------------------------------------------------------ 3. rejects
@pytest.mark.parametrize("contributions", [0, 2])
def test_a_ceremony_of_another_tau_is_rejected(amd, contributions):
    c = _chain(amd, "small", "full")
    t = c["tau"]
    other = amd.ptau_synth(c["L"], (t["tau"] + 1) % R, t["alpha"], t["beta"], prepared=False, device=0)
    ok, why = amd.zkey_verify_from_init(c["keys"][0], c["keys"][contributions], device=0, ptau=other)
    assert not ok and why == H_TEXT


def test_forged_h_basis_passes_without_the_ptau_and_is_rejected_with_it(amd):
    """The hole the leg closes: an initial key of unknown provenance with wrong H points, and its contributed key with
    the same wrong points scaled."""
    c = _chain(amd, "small", "full")
    init, one = _forge(c["keys"][0]), _forge(c["keys"][1])
    ok, why = amd.zkey_verify_from_init(init, one, device=0)
    assert ok, why
    ok, why = amd.zkey_verify_from_init(init, one, device=0, ptau=c["ptau"])
    assert not ok and why == H_TEXT
    ok, why = amd.zkey_verify_from_init(init, init, device=0, ptau=c["ptau"])
    assert not ok and why == H_TEXT


def test_a_smaller_ceremony_is_rejected(amd):
    c = _chain(amd, "small", "full")
    t = c["tau"]
    small = amd.ptau_synth(c["L"] - 1, t["tau"], t["alpha"], t["beta"], prepared=False, device=0)
    ok, why = amd.zkey_verify_from_init(c["keys"][0], c["keys"][1], device=0, ptau=small)
    assert not ok and why == SMALL_TEXT


# ------------------------------------------------------------------ 4. from the .r1cs
@pytest.mark.parametrize("kind", ["full", "truncated"])
def test_verify_r1cs(amd, kind):
    c = _chain(amd, "small", kind)
    for key in c["keys"]:
        ok, why = amd.zkey_verify_r1cs(c["r1cs"], c["ptau"], key, device=0)
        assert ok and why == "", why
    ok, why = amd.zkey_verify_r1cs(c["r1cs"], c["ptau"], _forge(c["keys"][1]), device=0)   # never sees a forged init
    assert not ok and why.startswith("zkey verify: "), why
