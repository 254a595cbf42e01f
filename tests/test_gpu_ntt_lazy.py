"""The Fr NTT kernels at their lazy-reduction bounds (ntt.hip / fr29.cuh headers): the inputs that
test_cpu_ntt_lazy.py shows to REACH the bounds on the representative-exact twin (tests/ntt_lazy_ref.py) -- DIF sums
of 8 (r - 1), subtrahends of (r - 1), 2 (r - 1), 4 (r - 1) against K = 2, 3, 5 (also from a zero minuend), a DIT
row at 14.87 r before its reduce -- run through every entry that reaches those kernels: fr_fft both ways under the
default pass plan and the two plans only G16_NTT_TILE_LOG / G16_NTT_MIN_TB select, f29_op against the twin's
integers, the Groth16 chain (QAP -> fused coset round trip -> fused join) and zkey_h_scalars.  Every output word is
compared with the Python NTT and must be canonical: a value that left its bound shows as a wrong or unreduced word."""
import ctypes
from functools import lru_cache

import pytest

import bn254 as b
import formats as f
import groth16 as g
import ntt_lazy_ref as nl
from test_gpu_fullsize import cpu_threads
from test_gpu_midsize import _abc_on_domain, _on_coset
from test_gpu_prove import kat_secrets
from zkey_verify_ptau_ref import h_scalars_ref

pytestmark = pytest.mark.gpu

R = b.R
PLANS = [(7, 9, 2), (8, 9, 2), (9, 9, 2), (10, 9, 2), (16, 9, 2), (17, 9, 2), (13, 11, 0), (10, 4, 2)]


def _fft_cases():
    return [(plan, name) for plan in PLANS for name in nl.family_names(*plan)]


@pytest.mark.parametrize("plan,name", _fft_cases(), ids=lambda v: "L%d-tile%d-tb%d" % v if isinstance(v, tuple) else v)
def test_fr_fft_at_the_bounds(amd, monkeypatch, plan, name):
    """fr_fft and fr_fft(inverse=True) on one vector of family (a), (b) or (c): every word == groth16.ntt, canonical"""
    L, tile_log, min_tb = plan
    if (tile_log, min_tb) == (9, 2):
        monkeypatch.delenv("G16_NTT_TILE_LOG", raising=False)
        monkeypatch.delenv("G16_NTT_MIN_TB", raising=False)
    else:                                    # read by ntt_tables_create, which fft_impl calls every time
        monkeypatch.setenv("G16_NTT_TILE_LOG", str(tile_log))
        monkeypatch.setenv("G16_NTT_MIN_TB", str(min_tb))
    vals = nl.family_vector(L, tile_log, min_tb, name)
    buf = b"".join((v * b.RR % R).to_bytes(32, "little") for v in vals)
    rinv = pow(b.RR, -1, R)
    for inverse in (False, True):
        raw = amd.fr_fft(buf, inverse=inverse)
        got = [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]
        assert max(got) < R, "a word left the device unreduced"
        want = g.ntt(vals, inverse=inverse)
        bad = [i for i, (x, y) in enumerate(zip(got, want)) if x * rinv % R != y]
        assert not bad, (inverse, len(bad), bad[:8])


def test_f29_op_returns_the_twins_integers(amd):
    """both Montgomery products and the weak reduction on the inputs of the host program (0, r - 1, r, 16 r - 1, k r,
    random lazy values): the same integers, not only the same residues"""
    cases = nl.primitive_cases()
    mul = [(a, c) for op, a, c in cases if op == "mul"]
    weak = [a for op, a, c in cases if op == "weak"]
    assert len(mul) > 150 and len(weak) > 90
    want = [nl.fr29_mul(x, y) for x, y in mul]
    for op in (0, 9):
        assert amd.f29_op(0, op, [x for x, _ in mul], [y for _, y in mul]) == want
    assert amd.f29_op(0, 10, weak) == [nl.fr29_weak_reduce(x) for x in weak]


@pytest.mark.parametrize("which", [0, 1], ids=["constant-e", "worst-path"])
def test_zkey_h_scalars_at_the_bounds(amd, monkeypatch, which):
    monkeypatch.delenv("G16_NTT_TILE_LOG", raising=False)
    monkeypatch.delenv("G16_NTT_MIN_TB", raising=False)
    L = 10
    u = nl.h_scalar_vectors(L)[which]
    rho, t = amd.zkey_h_scalars(u, L, device=0)
    want_rho, want_t = h_scalars_ref(u, L)
    assert t == want_t
    assert rho == want_rho


# ------------------------------------------------------------------ the Groth16 chain
SEED = 2900


@lru_cache(maxsize=None)
def _chain(amd, L):
    """The circuit of m = N - 1 rows w_i * 1 = w_i, no public input: A_T is the private wires, B_T = 1, C_T = A_T, and
    every witness is valid; the binding row fixes A_T[N - 1] = w_0 = 1.  -> (rows, key, secrets, the two witnesses)"""
    N = 1 << L
    n, p, m = N, 0, N - 1
    rows = [([(i + 1, 1)], [(0, 1)], [(i + 1, 1)]) for i in range(m)]
    td = g.trapdoor(SEED + 1)
    amd.setup_device(0)
    try:
        key, _ = amd.r1cs_setup_trapdoor(f.write_r1cs(n, p, 0, rows), td, cpu_threads())
    finally:
        amd.setup_device(-1)
    sec = kat_secrets(rows, n, p, m, SEED, N)
    avecs = nl.chain_vectors(L)
    assert all(a[N - 1] == 1 for a in avecs)
    wits = [[1] + a[:N - 1] for a in avecs]
    return rows, key, sec, wits


@lru_cache(maxsize=None)
def _b_on_coset(L):
    N = 1 << L
    return _on_coset([1] * (N - 1) + [0])


def _unpack_all(raw, N, eb):
    words = memoryview(raw).cast("I")
    per = eb // 4
    return [sum(words[i * per + k] << (29 * k) for k in range(9)) for i in range(N)]


@pytest.mark.parametrize("which", [0, 1], ids=["constant-e", "worst-path"])
@pytest.mark.parametrize("L", [10, 16])
def test_chain_coset_evaluation(amd, monkeypatch, L, which):
    """Prover.stage + shard_begin with all three vectors (QAP, then the fused coset round trip): every lazy word below
    16 r, every residue == the Python coset evaluation.  2^10: mid pass + one S = 1 pass; 2^16: + one S = 7 pass."""
    monkeypatch.delenv("G16_NTT_TILE_LOG", raising=False)
    monkeypatch.delenv("G16_NTT_MIN_TB", raising=False)
    N = 1 << L
    rows, key, _, wits = _chain(amd, L)
    w = wits[which]
    pv = amd.Prover(key, shard_rank=0, shard_count=2)
    assert pv.info.domain_size == N
    eb = amd.LAZY_FR_BYTES
    vecs = [ctypes.create_string_buffer(N * eb) for _ in range(3)]
    pv.stage(0, f.write_wtns(w))
    pv.shard_begin(0, 0b111, [ctypes.addressof(x) for x in vecs])
    pv.close()
    rinv = pow(1 << 261, -1, R)
    a, bb, cc = _abc_on_domain(rows, w, 0, N - 1, N)
    assert bb == [1] * (N - 1) + [0] and cc[:N - 1] == a[:N - 1] and a[N - 1] == 1
    for k, ev in enumerate((a, bb, cc)):
        want = _b_on_coset(L) if k == 1 else _on_coset(ev)
        got = _unpack_all(vecs[k].raw, N, eb)
        assert max(got) < 16 * R, k
        bad = [i for i in range(N) if got[i] * rinv % R != want[i]]
        assert not bad, (k, len(bad), bad[:8])


@pytest.mark.parametrize("which", [0, 1], ids=["constant-e", "worst-path"])
@pytest.mark.parametrize("L", [10, 16])
def test_chain_proof_equals_the_known_answer(amd, monkeypatch, L, which):
    """prove with fixed r, s == the trapdoor known answer: pins the fused join (S = 1 at 2^10, S = 7 at 2^16), whose
    output is not readable otherwise"""
    monkeypatch.delenv("G16_NTT_TILE_LOG", raising=False)
    monkeypatch.delenv("G16_NTT_MIN_TB", raising=False)
    rows, key, sec, wits = _chain(amd, L)
    w = wits[which]
    r, s = 0x1234567 + L, R - 2 - which
    prover = amd.Prover(key)
    assert prover.info.domain_size == 1 << L
    proof, pub = prover.prove(f.write_wtns(w), f.le(r), f.le(s))
    prover.close()
    assert pub == []
    assert proof == f.proof_obj(*g.expected_proof(sec, 0, w, r, s))
