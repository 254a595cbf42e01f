"""The one-shot device routes own their stream, events and buffers per call (csrc/device_job.h).  Every route runs three
times in a row in one process at the smallest size its own tests use: the three results are byte-identical -- a stale or
doubly released buffer would show -- and equal the oracle where the neighbouring test file has one at hand.  And the one
buffer pair that grows during a call (the full-width products of setup_ptau.hip) grows between pieces."""
import random

import pytest

import bn254 as b
import formats as f
import groth16 as g
import plonk as pk
import synth
from ptau_prepare_ref import g1_bytes, split, top_block_scalar
from ptau_prepared import write_ptau_prepared
from test_cpu_pairing import oracle_value, tower_to_poly
from test_gpu_groth16_ptau import _crafted, _power, _td
from test_gpu_zkey_verify_ptau import _u
from zkey_verify_ptau_ref import h_scalars_ref

pytestmark = pytest.mark.gpu

SMALL = (24, 2, 12, 1)


def _thrice(call):
    first = call()
    assert call() == first and call() == first
    return first


@pytest.fixture()
def on_device(amd):
    amd.setup_device(0)
    yield amd
    amd.setup_device(-1)


@pytest.mark.parametrize("n,p,m,seed", [SMALL, (150, 6, 120, 2)])
def test_trapdoor_setup(on_device, n, p, m, seed):
    """(24, 2, 12, 1): every batch has fewer than 64 scalars and stays on the host threads; (150, 6, 120, 2), the
    smallest of test_gpu_setup.py, is the first to reach the device."""
    amd = on_device
    got = _thrice(lambda: amd.synth_setup(n, p, m, seed, 2))
    amd.setup_device(-1)
    assert got == amd.synth_setup(n, p, m, seed, 2)
    if (n, p, m, seed) == SMALL:
        rows, w = synth.make(n, p, m, seed)
        assert got[0] == f.write_zkey(g.setup(n, p, rows, g.trapdoor(seed + 1))[0]) and got[1] == f.write_wtns(w)


def test_ptau_synth(amd):
    td = _td(5)
    got = _thrice(lambda: amd.ptau_synth(5, td["tau"], td["alpha"], td["beta"], device=0))
    assert got == write_ptau_prepared(5, td["tau"], td["alpha"], td["beta"])


def test_ptau_prepare(amd):
    power, td = 3, _td(31)
    src = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    ids, gs = split(_thrice(lambda: amd.ptau_prepare(src, device=0)))
    _, ws = split(write_ptau_prepared(power, td["tau"], td["alpha"], td["beta"]))
    M = 2 << power
    assert ids == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert all(gs[sid] == ws[sid] for sid in ids if sid != 12)
    # section 12: the generator's blocks 0 .. power, then the top block with its last input padded by infinity
    assert gs[12] == ws[12][:(M - 1) * 64] + g1_bytes([top_block_scalar(power, j, td["tau"]) for j in range(M)])


def test_groth16_setup_ptau(amd):
    n, p, m, seed = SMALL
    rows, _ = synth.make(n, p, m, seed)
    td = _td(seed + 1000)
    ptau = amd.ptau_synth(_power(m, p), td["tau"], td["alpha"], td["beta"], device=0)
    r1cs = f.write_r1cs(n, p, 0, rows)
    assert _thrice(lambda: amd.groth16_setup_ptau(r1cs, ptau, device=0)) == f.write_zkey(g.setup(n, p, rows, td)[0])


def test_plonk_setup_both_routes(amd):
    n, p, m, seed = SMALL
    rows, _ = synth.make(n, p, m, seed)
    r1cs = f.write_r1cs(n, p, 0, synth.gen_circuit(n, p, m, seed)[1])
    tau = g.trapdoor(seed + 1)["tau"]
    zk = pk.setup(n, p, rows, tau)
    assert _thrice(lambda: amd.plonk_setup(r1cs, seed, device=0)) == pk.write_zkey(zk)
    ptau = pk.write_ptau(zk["power"] + 1, tau)
    assert _thrice(lambda: amd.plonk_setup_ptau(r1cs, ptau, device=0)) == pk.write_zkey(zk)


def test_pairing_op(amd):
    rng = random.Random(0xd0b)
    pairs = [(b.G1.mul(b.G1_GEN, rng.randrange(1, b.R)), b.G2.mul(b.G2_GEN, rng.randrange(1, b.R))) for _ in range(2)]
    got = _thrice(lambda: amd.pairing_op(pairs))
    assert [tower_to_poly(v) for v in got] == [oracle_value(P, Q) for P, Q in pairs]


def test_fr_fft(amd):
    rng = random.Random(8)
    vals = [rng.randrange(b.R) for _ in range(8)]
    mont = b"".join(f.le(v * b.RR % b.R) for v in vals)
    rinv = pow(b.RR, -1, b.R)
    for inverse in (False, True):
        out = _thrice(lambda: amd.fr_fft(mont, inverse=inverse))
        assert [int.from_bytes(out[i:i + 32], "little") * rinv % b.R for i in range(0, 256, 32)] == g.ntt(vals, inverse=inverse)


@pytest.mark.parametrize("curve", [1, 2])
def test_multiexp_and_ec_add(amd, curve):
    rng = random.Random(30 + curve)
    grp, gen = (b.G1, b.G1_GEN) if curve == 1 else (b.G2, b.G2_GEN)
    enc = f.g1_to_lem if curve == 1 else f.g2_to_lem

    def std(P):
        return b"".join(f.le(v) for v in (P if curve == 1 else (P[0][0], P[0][1], P[1][0], P[1][1])))
    ks = [rng.randrange(1, b.R) for _ in range(3)]
    sc = [rng.randrange(b.R) for _ in range(3)]
    bases = b"".join(enc(grp.mul(gen, k)) for k in ks)
    got = _thrice(lambda: amd.multiexp(curve, bases, b"".join(f.le(s) for s in sc)))
    assert got == std(grp.mul(gen, sum(k * s for k, s in zip(ks, sc)) % b.R))
    rev = b"".join(enc(grp.mul(gen, k)) for k in reversed(ks))
    got = _thrice(lambda: amd.ec_add(curve, bases, rev))
    assert got == b"".join(std(grp.mul(gen, (k + r) % b.R)) for k, r in zip(ks, reversed(ks)))


@pytest.mark.parametrize("L", [1, 3])
def test_zkey_h_scalars(amd, L):
    u = _u(L)
    assert _thrice(lambda: amd.zkey_h_scalars(u, L, device=0)) == tuple(h_scalars_ref(u, L))


def test_full_product_buffers_grow_between_pieces(amd, monkeypatch):
    """The crafted circuit cut at 97 terms: the first pieces hold no full-width coefficient, wire 5's piece holds about
    1 100, so the buffers of the full-width products are released and allocated again between pieces.  Same key."""
    n, p, rows, _ = _crafted()
    td = _td(1099)
    r1cs = f.write_r1cs(n, p, 0, rows)
    ptau = amd.ptau_synth(_power(len(rows), p), td["tau"], td["alpha"], td["beta"], device=0)
    whole = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    monkeypatch.setenv("G16_SETUP_PIECE_TERMS", "97")
    assert amd.groth16_setup_ptau(r1cs, ptau, device=0) == whole
