"""Groth16 setup from a prepared .ptau on the device (csrc/setup_ptau.hip via g16_groth16_setup_ptau).  For a ceremony
file made for a KNOWN (tau, alpha, beta), the key must be byte for byte the trapdoor setup's with
(tau, alpha, beta, gamma = 1, delta = 1): the Python oracle's at small sizes, g16_r1cs_setup_trapdoor's on the real
bit-level SHA-256 and NZCP circuits.  The keys prove, and the proofs pass the pairing check."""
import hashlib
import os
import time

import pytest

import formats as f
import groth16 as g
import synth
from bn254 import R
from conftest import ROOT
from ptau_prepared import write_ptau_prepared

pytestmark = pytest.mark.gpu


def _td(seed):
    t = g.trapdoor(seed)
    return {"tau": t["tau"], "alpha": t["alpha"], "beta": t["beta"], "gamma": 1, "delta": 1}


def _power(m, p):
    L = 0
    while (1 << L) < m + p + 1:
        L += 1
    return L


def _proof_points(obj):
    return f.g1_from_obj(obj["pi_a"]), f.g2_from_obj(obj["pi_b"]), f.g1_from_obj(obj["pi_c"])


def _crafted():
    """Wire 5 in > 10 000 rows, private wire 7 in none, and the coefficient classes r-1, r-2, 2^63, 2^64, 2^200 and a
    random full-width element (every row is satisfied by any witness with w3 = w1 * w2)."""
    n, p = 12, 3
    full = 0x2b3f5d7c9e1a3b5c7d9f1e3a5c7b9d1f2e4a6c8b0d2f4e6a8c0b2d4f6e8a0c2 % R
    coefs = [R - 1, R - 2, 1 << 63, 1 << 64, 1 << 200, full, 1, 3, 1 << 20]
    rows = [([(1, 1)], [(2, 1)], [(3, 1)])]
    for c in range(10_050):
        cf = coefs[c % len(coefs)]
        other = 8 + c % 4
        lc = [(5, cf), (other, coefs[(c // 9) % len(coefs)])]
        rows.append((lc, [(0, 1)], lc))
    rows.append(([(4, R - 2), (6, 1 << 64)], [(0, 1)], [(4, R - 2), (6, 1 << 64)]))
    w = [1] + [(0x9e3779b97f4a7c15 * (i + 3)) ** 3 % R for i in range(1, n)]
    w[3] = w[1] * w[2] % R
    return n, p, rows, w


CASES = [(24, 2, 12, 1), (150, 6, 120, 2), (1000, 513, 400, 5), "crafted"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c if isinstance(c, str) else "n%d_p%d_m%d_s%d" % c)
def test_ptau_key_equals_oracle_and_proves(amd, case):
    if case == "crafted":
        n, p, rows, w = _crafted()
        seed = 99
    else:
        n, p, m, seed = case
        rows, w = synth.make(n, p, m, seed)
    m = len(rows)
    td = _td(seed + 1000)
    r1cs = f.write_r1cs(n, p, 0, rows)
    L = _power(m, p)
    ptau = amd.ptau_synth(L, td["tau"], td["alpha"], td["beta"], device=0)
    key = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    if case == "crafted":
        # the oracle's 2^14-point H basis takes minutes in Python: the host trapdoor route (pinned against the oracle
        # by test_cpu_groth16_ptau.py) stands in, and the oracle checks the points of the long and unused wires
        want, _ = amd.r1cs_setup_trapdoor(r1cs, td, 0)
        assert key == want
        zk = f.read_zkey(key)
        import bn254 as b
        Lg = g.lagrange_at(1 << L, td["tau"])
        u5 = sum(cf * Lg[c] for c, (A, _, _) in enumerate(rows) for s, cf in A if s == 5) % R
        assert zk["A"][5] == b.G1.mul(b.G1_GEN, u5)
        assert zk["A"][7] is None and zk["B1"][7] is None and zk["B2"][7] is None and zk["C"][7 - p - 1] is None
    else:
        zk, _ = g.setup(n, p, rows, td)
        assert key == f.write_zkey(zk)
        zk = f.read_zkey(key)
    # one power more than needed: the same key
    bigger = amd.ptau_synth(L + 1, td["tau"], td["alpha"], td["beta"], device=0)
    assert amd.groth16_setup_ptau(r1cs, bigger, device=0) == key
    prover = amd.Prover(key, device=0)
    proof, pub = prover.prove(f.write_wtns(w))
    prover.close()
    assert pub == [str(x) for x in w[1:p + 1]]
    assert g.verify(zk, [int(x) for x in pub], _proof_points(proof))


@pytest.mark.parametrize("power", [5, 6, 7])
def test_ptau_synth_equals_python_writer(amd, power):
    td = _td(power)
    for prepared in (True, False):
        got = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=prepared, device=0)
        assert got == write_ptau_prepared(power, td["tau"], td["alpha"], td["beta"], prepared=prepared)


def test_several_pieces_give_the_same_key(amd, monkeypatch):
    """The term lists cut into pieces at output borders (a bound of 97 terms here) give the same key."""
    n, p, m, seed = 333, 20, 300, 9
    rows, _ = synth.make(n, p, m, seed)
    td = _td(seed)
    r1cs = f.write_r1cs(n, p, 0, rows)
    ptau = amd.ptau_synth(_power(m, p), td["tau"], td["alpha"], td["beta"], device=0)
    whole = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    monkeypatch.setenv("G16_SETUP_PIECE_TERMS", "97")
    assert amd.groth16_setup_ptau(r1cs, ptau, device=0) == whole


@pytest.mark.parametrize("blocks", [1, 2])
def test_sha256_chain_ptau_key_equals_trapdoor_and_verifies(amd, blocks):
    """A real bit-level circuit (domain 2^15 / 2^16): ptau route == trapdoor route, and the proof verifies on the
    device verifier."""
    msg = hashlib.sha256(b"groth16 setup from a ptau").digest()
    out = amd.sha256_chain_setup(blocks, msg, 5, want_zkey=False, want_r1cs=True)
    r1cs = out["r1cs"]
    td = _td(blocks + 70)
    amd.setup_device(0)
    try:
        want, vkey = amd.r1cs_setup_trapdoor(r1cs, td, 0)
    finally:
        amd.setup_device(-1)
    zk = f.read_zkey(want)
    L = zk["domainSize"].bit_length() - 1
    ptau = amd.ptau_synth(L, td["tau"], td["alpha"], td["beta"], device=0)
    key = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    assert key == want
    prover = amd.Prover(key, device=0)
    proof, pub = prover.prove(out["wtns"])
    prover.close()
    v = amd.Verifier(vkey, n_public=256, device=0)
    assert v.verify(pub, proof)
    v.close()


def test_nzcp_live_full_size(amd, capfd, monkeypatch):
    """The native nzcp_live constraint system (domain 2^20) with a power-20 synthetic ceremony: sha256 of the ptau
    key == sha256 of the trapdoor key (gamma = delta = 1).  Prints both routes' times and the term-class histogram."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nzcp_pass
    tbs = nzcp_pass.to_be_signed("Anne-Marie", "Te Whare", "1987-11-30", live=True, exp=1700000000)
    out = amd.nzcp_circuit_setup(amd.NZCP_LIVE_PARAMS, tbs, 77, want_zkey=False, want_r1cs=True)
    r1cs = out["r1cs"]
    td = _td(2020)
    amd.setup_device(0)
    try:
        t0 = time.time()
        want, _ = amd.r1cs_setup_trapdoor(r1cs, td, 0)
        t_trap = time.time() - t0
    finally:
        amd.setup_device(-1)
    t0 = time.time()
    ptau = amd.ptau_synth(20, td["tau"], td["alpha"], td["beta"], device=0)
    t_ptau = time.time() - t0
    monkeypatch.setenv("G16_TRACE_HOST", "1")
    capfd.readouterr()
    t0 = time.time()
    key = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    t_route = time.time() - t0
    trace = capfd.readouterr().err
    monkeypatch.delenv("G16_TRACE_HOST")
    del ptau
    line = [x for x in trace.splitlines() if "groth16 setup ptau" in x]
    with capfd.disabled():
        print(f"\nnzcp_live: {out['n_constraints']} rows; trapdoor route (device fixed-base) {t_trap:.2f} s, "
              f"ptau synth {t_ptau:.2f} s, ptau route {t_route:.2f} s")
        print(line[0] if line else trace)
    assert line
    assert hashlib.sha256(key).digest() == hashlib.sha256(want).digest()
