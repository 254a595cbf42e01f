"""The Fr NTT at its lazy-reduction bounds, on the CPU: the representative-exact twin (ntt_lazy_ref.py) is pinned to
a host build of fr29.cuh integer for integer, then driven with inputs that REACH the documented bounds (ntt.hip /
fr29.cuh headers) under every pass plan the G16_NTT_TILE_LOG / G16_NTT_MIN_TB settings select here.

Attained, in units of r (asserted below; what an input attains is a property of the input, not of the kernel):
  (a) constant e, inverse route: DIF sums 8 (r - 2^h), subtrahends (r - 2^h), 2 (r - 2^h), 4 (r - 2^h) against
      K = 2, 3, 5, where h = number of index bits of the passes run before (h = 0: 8 (r - 1) and (r - 1), 2 (r - 1),
      4 (r - 1)), in every pass of every plan.
  (b) square waves: the same subtrahends against a ZERO minuend: differences r + 2^h, r + 2 * 2^h, r + 4 * 2^h
      (r + 4 at phase 2 of the first pass run: the smallest margin a K leaves).  One wave per phase of each pass; at
      2^16 and 2^17 only phase 2 of each three-phase pass, to keep this file near a minute (test_gpu_ntt_lazy.py runs
      every phase at those sizes on the device).
  (c) worst-path vector, forward route: the all-ones row of the target tile reaches 14.87 r in a first pass
      (S = 7 .. 11, before the reduce after the 7th stage or the store) and 14.85 r in the S = 7 second pass; in the
      shorter passes 2.99 r (S = 1), 4.98 r (S = 2), 8.93 r (S = 4): 1 + 2 S less the residues rho_k.  A uniformly
      random vector of the same size peaks at 11.2 r .. 13.7 r where S >= 7 (the larger the vector the higher),
      2.88 r .. 2.996 r (S = 1), 4.79 r .. 4.88 r (S = 2), 7.84 r (S = 4): below the worst path every time."""
import os
import random
import subprocess

import pytest

import ntt_lazy_ref as nl
from bn254 import R, RR
from conftest import ROOT
from groth16 import ntt
from ntt_lazy_ref import E_MONT256, Twin

# (L, tile_log, min_tb): the default plan and the two plans only the settings reach; then (8, 5, 2), passes of 5 and 3
# stages: the smallest plan whose SECOND pass has all three DIF phases (as 2^16 and 2^17 have), in milliseconds
PLANS = [(7, 9, 2), (8, 9, 2), (9, 9, 2), (10, 9, 2), (16, 9, 2), (17, 9, 2), (13, 11, 0), (10, 4, 2), (8, 5, 2)]
IDS = [f"L{L}-tile{t}-tb{m}" for L, t, m in PLANS]
RRINV = pow(RR, -1, R)


def _plain(mont256):
    return [x * RRINV % R for x in mont256]


# ------------------------------------------------------------------ the twin is the code
def test_twin_equals_the_host_build_of_fr29(tmp_path):
    """fr29_from_fr, fr29_mul, fr29_weak_reduce, fr29_sub<2|3|5>, fr29_to_fr: the same integers, at 0, r - 1, r,
    16 r - 1, every k r, and random lazy values; and the constants the twin derives are the header's."""
    exe = tmp_path / "fr29_vectors"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DG16_F29_CHECK",
                           "-I", os.path.join(ROOT, "nzcp-circom_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "fr29_vectors.cpp"), "-o", str(exe)])
    cases = nl.primitive_cases()
    assert len(cases) > 300
    text = "".join(f"{op} {a:x} {b:x}\n" for op, a, b in cases)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    for (op, a, b), line in zip(cases, lines):
        words = [int(x, 16) for x in line.split()]
        width = 32 if op == "to_fr" else 29
        got = sum(x << (width * i) for i, x in enumerate(words))
        assert got == nl.twin_value(op, a, b), (op, hex(a), hex(b))
    assert nl.fr29_from_fr(E_MONT256) == R - 1
    assert nl.fr29_weak_reduce(16 * R - 1) < R + (R >> 13)
    # the table builder's shortcut is fr29_pow_u64's 64 steps
    w = nl.tables(7).tw_fwd[1]
    assert nl.pow_table(w, 70) == [nl.fr29_pow_u64(w, i) for i in range(70)]


def test_twin_raises_on_every_breach():
    with pytest.raises(nl.BoundBreach):
        nl.fr29_sub(3, 0, 4 * (R - 1))
    with pytest.raises(nl.BoundBreach):
        nl.fr29_mul(16 * R, 1)
    with pytest.raises(nl.BoundBreach):
        nl.fr29_weak_reduce(16 * R)
    with pytest.raises(nl.BoundBreach):
        nl.fr29_to_fr(16 * R)
    with pytest.raises(nl.BoundBreach):
        nl.fr29_weak_reduce(17 * R + (R >> 1))     # quotient 17: one row past the NEGQ table


# ------------------------------------------------------------------ the inputs are adversarial
def _earlier_bits(tw, p):
    """index bits of the passes the inverse route runs before pass p"""
    return sum(S for lo, S, tb in tw.passes[p + 1:])


@pytest.mark.parametrize("L,tile_log,min_tb", PLANS, ids=IDS)
def test_constant_e_fills_the_dif_sums(L, tile_log, min_tb):
    """(a): sums 2 x, 4 x, 8 x and subtrahends x, 2 x, 4 x of x = r - 2^h in every inverse pass; 8 (r - 1) itself in
    the first pass run when it has three stages"""
    tw = Twin(L, tile_log, min_tb)
    got = tw.fft([E_MONT256] * (1 << L), inverse=True)
    assert max(got) < R and _plain(got) == ntt(nl.constant_e(L), inverse=True)
    for p, (lo, S, tb) in enumerate(tw.passes):
        x = R - (1 << _earlier_bits(tw, p))
        assert tw.rec[(("dif", p), "load", "in")] <= 8 * R
        for k in range(min(S, 3)):
            # (a later pass also loads the zeros of the earlier difference branches as r itself: r, 2 r, 4 r)
            assert x << k <= tw.sub[(("dif", p), k)][0] <= R << k and tw.sub[(("dif", p), k)][1] == (2, 3, 5)[k]
            assert x << (k + 1) <= tw.rec[(("dif", p), k, "sum")] <= R << (k + 1)
    first = len(tw.passes) - 1
    if tw.passes[first][1] >= 3:
        assert tw.rec[(("dif", first), 2, "sum")] == 8 * (R - 1)
        assert [tw.sub[(("dif", first), k)][0] for k in range(3)] == [R - 1, 2 * (R - 1), 4 * (R - 1)]
    # ... and through the forward route
    fw = Twin(L, tile_log, min_tb)
    got = fw.fft([E_MONT256] * (1 << L))
    assert max(got) < R and _plain(got) == ntt(nl.constant_e(L))


@pytest.mark.parametrize("L,tile_log,min_tb", PLANS, ids=IDS)
def test_square_waves_subtract_from_zero(L, tile_log, min_tb):
    """(b): for one index bit in each phase of each pass, the stage on that bit subtracts 2^phase x from 0"""
    passes = nl.kernel_plan(L, tile_log, min_tb)[1]
    for p, phase, beta in nl.wave_bits(passes):
        if L >= 16 and phase != 2 and passes[p][1] >= 3:
            # 2^16, 2^17: the tightest phase of each pass only, for this file's time (3 to 4 s a wave).  Phases 0 and 1 of
            # a three-phase pass run here at the smaller sizes and in the (8, 5, 2) plan, and on the device at every size.
            continue
        tw = Twin(L, tile_log, min_tb)
        vals = nl.square_wave(L, beta)
        got = tw.fft([v * RR % R for v in vals], inverse=True)
        assert max(got) < R and _plain(got) == ntt(vals, inverse=True), (p, phase)
        x = R - (1 << _earlier_bits(tw, p))
        K = (2, 3, 5)[phase]
        assert x << phase <= tw.sub[(("dif", p), phase)][0] <= R << phase
        assert K * R - (R << phase) <= tw.low[(("dif", p), phase)] <= K * R - (x << phase)
        if p == len(passes) - 1:                     # the first pass run: e itself, no zeros loaded as r
            assert tw.sub[(("dif", p), phase)][0] == (R - 1) << phase
            assert tw.low[(("dif", p), phase)] == R + (1 << phase)      # r + 4 at phase 2


def _dit_peak(tw, p):
    """the largest DIT difference before the reduce after the 7th stage (or the store)"""
    S = tw.passes[p][1]
    return max(tw.rec[(("dit", p), k, "diff")] for k in range(min(S, 7)))


@pytest.mark.parametrize("L,tile_log,min_tb", PLANS, ids=IDS)
def test_worst_path_vector_fills_the_dit_drift(L, tile_log, min_tb):
    """(c): per forward pass, the vector that drives one all-ones row up by 2 r a stage; a random vector stays below"""
    N = 1 << L
    rnd = Twin(L, tile_log, min_tb)
    rng = random.Random(L)
    rvals = [rng.randrange(R) for _ in range(N)]
    assert _plain(rnd.fft([v * RR % R for v in rvals])) == ntt(rvals)
    for p, (lo, S, tb) in enumerate(rnd.passes):
        vals, _ = nl.worst_path_vector(L, p, tile_log, min_tb)
        tw = Twin(L, tile_log, min_tb)
        got = tw.fft([v * RR % R for v in vals])
        assert max(got) < R and _plain(got) == ntt(vals), p
        peak, rpeak = _dit_peak(tw, p), _dit_peak(rnd, p)
        print(f"L={L} tile={tile_log} min_tb={min_tb} pass {p} S={S}: worst path {peak / R:.4f} r, random {rpeak / R:.4f} r")
        if S >= 7:
            assert peak >= 145 * R // 10
        else:
            assert 2 * peak >= (1 + 4 * S) * R            # 1 + 2 S - 0.5
        assert peak < 15 * R + (R >> 13)                   # the documented bound: 15.0001 r
        assert rpeak < peak
    if L < 16:      # ... and the last of them through the inverse route
        inv = Twin(L, tile_log, min_tb)
        got = inv.fft([v * RR % R for v in vals], inverse=True)
        assert max(got) < R and _plain(got) == ntt(vals, inverse=True)


# ------------------------------------------------------------------ the coset round trip and the join
def _on_coset(vals):
    L = len(vals).bit_length() - 1
    inc = nl.fr_root(L + 1)
    coef = ntt(vals, inverse=True)
    return ntt([c * pow(inc, i, R) % R for i, c in enumerate(coef)])


@pytest.mark.parametrize("L,tile_log,min_tb", [(7, 9, 2), (9, 9, 2), (10, 9, 2), (10, 4, 2), (13, 11, 0)],
                         ids=["L7-unfused", "L9-unfused", "L10", "L10-tile4", "L13-tile11"])
def test_coset_round_trip_and_join(L, tile_log, min_tb):
    """ntt_coset_roundtrip without and with the fused join (the unfused route for one-pass plans): invariants hold,
    residues equal the Python coset evaluation, P = A' B' - C'"""
    N = 1 << L
    for a in nl.chain_vectors(L, tile_log, min_tb):
        bb = [1] * (N - 1) + [0]
        cc = [x * y % R for x, y in zip(a, bb)]
        want = [_on_coset(v) for v in (a, bb, cc)]
        tw = Twin(L, tile_log, min_tb)
        vecs = [[nl.lazy(x) for x in v] for v in (a, bb, cc)]
        tw.coset_roundtrip(vecs)
        for v, w in zip(vecs, want):
            assert max(v) < 16 * R and nl.residues(v) == w
        tj = Twin(L, tile_log, min_tb)
        P = tj.coset_roundtrip([[nl.lazy(x) for x in v] for v in (a, bb, cc)], join=True)
        assert P == [(x * y - z) % R for x, y, z in zip(*want)]
    if L >= 10 and tile_log == 9:
        # witness (ii) fills the first forward pass behind the coset table
        assert _dit_peak(tw, 0) >= 145 * R // 10


# ------------------------------------------------------------------ what a wrong cadence does to these inputs
WRONG = {
    "dif-phase2-sub3": (lambda c: dict(c, dif_k=(2, 3, 3)), "const", True, "subtrahend 4.0000 r against K = 3"),
    "dit-reduce-at-k8": (lambda c: dict(c, dit_reduce_k=8), "path-p0", False, "weak-reduce input 16.87"),
    "no-reduce-on-load": (lambda c: dict(c, load_reduce=dict(c["load_reduce"], **{"pass": False})), "const", True,
                          "subtrahend 4.0000 r against K = 3"),
}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_a_wrong_cadence_breaches_on_these_inputs(name):
    """The twin under three one-line changes of ntt_tile_stages / ntt_pass_kernel at 2^10: each breaks a precondition on
    one of the families.  A reduce moved from the 7th to the 9th DIT stage is the case only the worst-path vector shows:
    the uniformly random vector of the same size stays below 16 r there."""
    change, family, inverse, text = WRONG[name]
    L = 10
    tw = Twin(L)
    tw.c = change(tw.c)
    vals = nl.family_vector(L, 9, 2, family)
    with pytest.raises(nl.BoundBreach, match=text):
        tw.fft([v * RR % R for v in vals], inverse=inverse)
    if name == "dit-reduce-at-k8":
        rng = random.Random(L)
        rt = Twin(L)
        rt.c = change(rt.c)
        rvals = [rng.randrange(R) for _ in range(1 << L)]
        assert _plain(rt.fft([v * RR % R for v in rvals])) == ntt(rvals)


def test_behind_the_coset_table_the_path_still_fills():
    """The worst-path vectors that enter the first forward pass through the coset product (the Groth16 chain's witness
    (ii) and zkey_h_scalars' u) reach 14.5 r too: the chain's A_T at 2^16 through the fused round trip, u at 2^10
    through import -> coset table -> forward passes -> export."""
    L = 16
    a = nl.chain_vectors(L)[1]
    tw = Twin(L)
    vec = [nl.lazy(x) for x in a]
    tw.coset_roundtrip([vec])
    assert max(vec) < 16 * R and nl.residues(vec) == _on_coset(a)
    assert 145 * R // 10 <= _dit_peak(tw, 0) < 15 * R + (R >> 13)
    L = 10
    from zkey_verify_ptau_ref import h_scalars_ref
    for which, u in enumerate(nl.h_scalar_vectors(L)):
        tw = Twin(L)
        assert tw.coset_forward(u) == h_scalars_ref(u, L)[0]
        if which == 1:
            assert 145 * R // 10 <= _dit_peak(tw, 0) < 15 * R + (R >> 13)
