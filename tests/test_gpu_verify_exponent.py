"""The Groth16 batch verifier on the device (csrc/verify.hip over pairing.cuh) on keys and proofs whose discrete logs
are known: every expected verdict is tests/verify_exponent_ref.py::accepts -- one congruence modulo r, no pairing --
so a VALID proof can be put on every special-case branch of the kernels (C, vk_x, A or B at infinity: a Miller value
replaced by one), on every lane / window / tree edge of verify_vkx_kernel and on every tail of the four launches, with
the rejected neighbour one step away beside it.  tests/test_cpu_verify_exponent.py pins accepts() to the oracle's
pairing check.  All proofs go through Verifier.verify_batch, the path users take."""
import copy
import random

import pytest

import bn254 as b
from bn254 import Q, R

import verify_exponent_ref as ve

pytestmark = pytest.mark.gpu

TOP = (1 << 256) - 1


def _scalars(rng, n):
    return [rng.randrange(1, R) for _ in range(n)]


def _key_scalars(rng, ics):
    return (list(ics),) + tuple(_scalars(rng, 4))


def _items(cases):
    ve.g1_points([x for a, _, c, _ in cases for x in (a, c)])
    ve.g2_points([bb for _, bb, _, _ in cases])
    return [([str(int(x)) for x in pub], ve.proof_obj(a, bb, c)) for a, bb, c, pub in cases]


def _expect(ks, cases):
    return [ve.accepts(ks, a, bb, c, pub) for a, bb, c, pub in cases]


def _check(ver, ks, cases, names=None):
    """The whole verdict list, position by position, against the congruence; both verdicts must occur."""
    got = ver.verify_batch(_items(cases))
    exp = _expect(ks, cases)
    wrong = [(i, names[i] if names else None, exp[i]) for i in range(len(exp)) if got[i] != exp[i]]
    assert not wrong, "verdicts differ from the congruence at (index, case, expected): %r" % wrong
    assert got == exp
    assert True in exp and False in exp
    return exp


def _bump(pub, j, by=1):
    out = list(pub)
    out[j] = out[j] + by if out[j] + by <= TOP else out[j] - by
    return out


# ------------------------------------------------------------------ accept through every branch, reject one step away
def _branch_cases(seed=0xb7a):
    """n_public = 5: a valid proof of each kind and its neighbours (c + 1, a + 1, b + 1, one signal + 1)."""
    rng = random.Random(seed)
    ks = _key_scalars(rng, _scalars(rng, 6))
    a, bb = _scalars(rng, 2)
    pub = [rng.randrange(R) for _ in range(5)]
    head = pub[:4]
    pub_x0 = head + [ve.solve_last_signal(ks, head)]                              # vk_x = infinity
    pub_ac = head + [ve.solve_last_signal(ks, head, ve.x_without_a_and_c(ks))]    # alpha beta + x gamma = 0
    valid = [
        ("generic", a, bb, ve.solve_c(ks, a, bb, pub), pub),
        ("C = inf", ve.solve_a(ks, bb, pub), bb, 0, pub),
        ("vk_x = inf", a, bb, ve.solve_c(ks, a, bb, pub_x0), pub_x0),
        ("A = inf", 0, bb, ve.solve_c(ks, 0, bb, pub), pub),
        ("B = inf", a, 0, ve.solve_c(ks, a, 0, pub), pub),
        ("A = inf, C = inf", 0, bb, 0, pub_ac),
        ("B = inf, C = inf", a, 0, 0, pub_ac),
        ("C = inf, vk_x = inf", ve.solve_a(ks, bb, pub_x0), bb, 0, pub_x0),
    ]
    names, cases = [], []
    for k, (name, ca, cb, cc, ps) in enumerate(valid):
        for tag, case in (("", (ca, cb, cc, ps)), (", c + 1", (ca, cb, cc + 1, ps)), (", a + 1", (ca + 1, cb, cc, ps)),
                          (", b + 1", (ca, cb + 1, cc, ps)), (", signal %d + 1" % (k % 5), (ca, cb, cc, _bump(ps, k % 5))),
                          (", last signal + 1", (ca, cb, cc, _bump(ps, 4)))):
            names.append(name + tag)
            cases.append(case)
    return ks, names, cases


@pytest.fixture(scope="module")
def branches():
    ks, names, cases = _branch_cases()
    key, _ = ve.make_key(*ks)
    return ks, key, names, cases


def test_accept_through_every_branch_and_reject_one_step_away(amd, branches):
    """Valid proofs whose C, vk_x, A, B (and pairs of them) are the point at infinity -- the branches of
    verify_load_kernel's flags 2 and 4 and of verify_miller_kernel that put f12_one() in place of a Miller value --
    are ACCEPTED, and each neighbour is rejected.  (With A or B at infinity the product a b stays 0 when the other
    factor moves: those neighbours stay accepted, as the congruence says.)  What the accept cases pin is the VALUE
    put in place: one.  Running miller_loop_pre on the all-zero point instead would pass too -- every line then lies
    in Fq2, which the final exponentiation sends to one -- so those two skips are shortcuts; a branch that dropped a
    factor that is not one (C ignored, or (A, B) skipped because C is infinity) fails here."""
    ks, key, names, cases = branches
    ver = amd.Verifier(key, 5, montgomery=True, device=0)
    exp = _check(ver, ks, cases, names)
    ver.close()
    by_name = dict(zip(names, exp))
    for kind in ("generic", "C = inf", "vk_x = inf", "A = inf", "B = inf", "A = inf, C = inf", "B = inf, C = inf",
                 "C = inf, vk_x = inf"):
        assert by_name[kind] is True
        assert by_name[kind + ", c + 1"] is False and by_name[kind + ", last signal + 1"] is False
    for kind in ("generic", "C = inf", "vk_x = inf"):
        assert by_name[kind + ", a + 1"] is False and by_name[kind + ", b + 1"] is False
    assert by_name["A = inf, a + 1"] is False and by_name["B = inf, b + 1"] is False
    assert by_name["A = inf, b + 1"] is True and by_name["B = inf, a + 1"] is True


def test_standard_form_key_and_json_route_give_the_same_verdicts(amd, branches):
    """Verifier(bytes, montgomery=False) and Verifier(verification_key.json object) on the n_public = 5 key."""
    ks, key, names, cases = branches
    vk_json = amd.vkey_json(key, 5)
    std, n_public = amd.vkey_from_json(vk_json)
    assert n_public == 5 and len(std) == len(key) and std != key
    exp = _expect(ks, cases)
    items = _items(cases)
    for ver in (amd.Verifier(key, 5, montgomery=True, device=0), amd.Verifier(std, 5, montgomery=False, device=0),
                amd.Verifier(vk_json, device=0)):
        assert ver.verify_batch(items) == exp
        ver.close()
    assert True in exp and False in exp


# ------------------------------------------------------------------ verify_vkx_kernel: lane stride and LDS tree
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_vkx_lane_stride_edges(amd, n):
    """256 lanes stride over the signals: one valid proof per width, and a rejection for signal j + 1 at the first and
    last lane of the first stride, the first lanes of the second and third (j = 0, 254, 255, 256, 257, n - 1) -- a
    kernel that drops one of them accepts exactly that case.  n = 0: no signals, vk_x = IC_0."""
    rng = random.Random(0x57 + n)
    ks = _key_scalars(rng, _scalars(rng, n + 1))
    key, _ = ve.make_key(*ks)
    a, bb = _scalars(rng, 2)
    pub = [rng.randrange(1 << 256) for _ in range(n)]
    c = ve.solve_c(ks, a, bb, pub)
    names, cases = ["valid", "c + 1"], [(a, bb, c, pub), (a, bb, c + 1, pub)]
    for j in sorted({j for j in (0, 254, 255, 256, 257, n - 1) if 0 <= j < n}):
        names.append("signal %d + 1" % j)
        cases.append((a, bb, c, _bump(pub, j)))
    cases.append((a, bb, c, pub))
    names.append("valid again")
    ver = amd.Verifier(key, n, montgomery=True, device=0)
    exp = _check(ver, ks, cases, names)
    ver.close()
    assert exp == [True] + [False] * (len(cases) - 2) + [True]


# ------------------------------------------------------------------ 4-bit windows of a signal
def test_vkx_window_digits_and_signals_at_and_above_r(amd):
    """n_public = 2, signal 0 = d 16^w for d in {1, 15}, w in {0, 1, 31, 32, 62, 63} (15 * 16^63 and its like are
    above r: the table entry d 16^w IC_j is right for any 256-bit signal, reduced or not): once with the proof solved
    for that value (accepted), once with the proof solved for the neighbouring digit d - 1 or d + 1 of the same window
    (rejected).  Then 0, r - 1, r, 2^256 - 1 and s + k r: a proof solved for s is a proof for s + k r."""
    rng = random.Random(0x316)
    ks = _key_scalars(rng, _scalars(rng, 3))
    key, _ = ve.make_key(*ks)
    a, bb = _scalars(rng, 2)
    s1 = rng.randrange(1 << 256)
    names, cases = [], []

    def add(name, solved_for, given):
        names.append(name)
        cases.append((a, bb, ve.solve_c(ks, a, bb, [solved_for, s1]), [given, s1]))

    for w in (0, 1, 31, 32, 62, 63):
        for d in (1, 15):
            v = d << (4 * w)
            add("%d * 16^%d" % (d, w), v, v)
            add("%d * 16^%d, proof for digit %d" % (d, w, d - 1), v - (1 << (4 * w)), v)
            if d < 15:
                add("%d * 16^%d, proof for digit %d" % (d, w, d + 1), v + (1 << (4 * w)), v)
    s = rng.randrange(R)
    for name, v in (("0", 0), ("r - 1", R - 1), ("r", R), ("2^256 - 1", TOP), ("s", s)):
        add(name, v, v)
        add(name + ", proof for the value reduced", v % R, v)
        add(name + ", proof for a neighbour", v + 1 if v < TOP else v - 1, v)
    for k in range(1, 5):
        assert s + k * R <= TOP and R - 1 + k * R <= TOP
        add("s + %d r, proof for s" % k, s, s + k * R)
        add("s + %d r, proof for s + 1" % k, s + 1, s + k * R)
        add("r - 1 + %d r, proof for r - 1" % k, R - 1, R - 1 + k * R)
    # the same edge values in the last signal, signal 0 random
    s0 = rng.randrange(1 << 256)
    for v in (0, R, TOP, 15 << 252):
        c = ve.solve_c(ks, a, bb, [s0, v])
        names += ["signal 1 = %d" % v, "signal 1 = %d, c + 1" % v]
        cases += [(a, bb, c, [s0, v]), (a, bb, c + 1, [s0, v])]
    ver = amd.Verifier(key, 2, montgomery=True, device=0)
    exp = _check(ver, ks, cases, names)
    ver.close()
    by_name = dict(zip(names, exp))
    assert by_name["15 * 16^63"] and by_name["1 * 16^63"] and not by_name["15 * 16^63, proof for digit 14"]
    assert by_name["r, proof for the value reduced"] and by_name["s + 4 r, proof for s"] and not by_name["s + 4 r, proof for s + 1"]
    assert exp.count(True) >= 12 + 10 + 8 + 4


# ------------------------------------------------------------------ doubling and cancellation inside the sum
@pytest.mark.parametrize("shape", ["equal", "opposite", "opposite, ic_0 = 0", "double"])
def test_vkx_exceptional_additions(amd, shape):
    """n_public = 512 (two strides of every lane).
    equal     ic_j the same for all j >= 1, all signals equal: both operands of every xyzz_add of the LDS tree are the
              same point (its doubling path), at every level.
    opposite  ic_{j+256} = -ic_j, all signals equal: each lane's sum cancels to infinity at its last madd, vk_x = IC_0;
              with ic_0 = 0 as well vk_x is infinity by cancellation.
    double    ic_{j+256} = ic_j and every signal the single digit d 16^w: the second madd of a lane adds the table entry
              its accumulator already holds (madd's doubling path)."""
    rng = random.Random(0xadd)
    ic0, e = _scalars(rng, 2)
    half = _scalars(rng, 256)
    ics = {"equal": [ic0] + [e] * 512, "opposite": [ic0] + half + [R - x for x in half],
           "opposite, ic_0 = 0": [0] + half + [R - x for x in half], "double": [ic0] + half + half}[shape]
    ks = _key_scalars(rng, ics)
    key, _ = ve.make_key(*ks)
    a, bb = _scalars(rng, 2)
    if shape == "double":
        signals = [1, 15 << 252, 7 << 124, 9 << 128]
    else:
        signals = [rng.randrange(1 << 256), 1, R - 1]
    names, cases = [], []
    for s in signals:
        pub = [s] * 512
        c = ve.solve_c(ks, a, bb, pub)
        if shape.startswith("opposite"):
            assert ve.vk_x(ks, pub) == ics[0]
        names += ["all signals %d" % s, "... c + 1", "... signal 0 + 1", "... signal 255 + 1", "... signal 256 + 1", "... signal 511 + 1"]
        cases += [(a, bb, c, pub), (a, bb, c + 1, pub)] + [(a, bb, c, _bump(pub, j)) for j in (0, 255, 256, 511)]
    ver = amd.Verifier(key, 512, montgomery=True, device=0)
    exp = _check(ver, ks, cases, names)
    ver.close()
    assert exp == [True, False, False, False, False, False] * len(signals)


def test_keys_with_ic_points_at_infinity(amd):
    """n_public = 4: IC_0 at infinity; some IC_j at infinity (their signals are free: changing them keeps an accepted
    proof accepted); every IC_j, j >= 1, at infinity (vk_x = IC_0 whatever the signals); every IC at infinity."""
    rng = random.Random(0x1c0)
    i0, i1, i2, i3, i4 = _scalars(rng, 5)
    tail = tuple(_scalars(rng, 4))
    a, bb = _scalars(rng, 2)
    pub = [rng.randrange(1 << 256) for _ in range(4)]
    other = [rng.randrange(1 << 256) for _ in range(4)]
    for ics, free in (([0, i1, i2, i3, i4], ()), ([i0, i1, 0, i3, 0], (1, 3)), ([i0, 0, i2, i3, i4], (0,)),
                      ([i0, 0, 0, 0, 0], (0, 1, 2, 3)), ([0, 0, 0, 0, 0], (0, 1, 2, 3))):
        ks = (ics,) + tail
        key, _ = ve.make_key(*ks)
        c = ve.solve_c(ks, a, bb, pub)
        cases = [(a, bb, c, pub), (a, bb, c + 1, pub), (ve.solve_a(ks, bb, pub), bb, 0, pub)]
        for j in range(4):
            cases.append((a, bb, c, _bump(pub, j)))
            cases.append((a, bb, c, pub[:j] + [other[j]] + pub[j + 1:]))
        cases.append((a, bb, c + 1, other))
        ver = amd.Verifier(key, 4, montgomery=True, device=0)
        exp = _check(ver, ks, cases)
        ver.close()
        assert exp[:3] == [True, False, True]
        for j in range(4):
            assert exp[3 + 2 * j] is (j in free) and exp[4 + 2 * j] is (j in free)


# ------------------------------------------------------------------ tails of the four launches, scratch regrowth
def test_batch_tails_and_scratch_regrowth_on_one_handle(amd):
    """One handle, n_public = 3, batches of 1, 63, 64, 65, 130 and then 2: a partial wavefront alone, beside full ones,
    every regrowth of ensure_scratch, and after the 130-batch a batch of 2 that must not see the stale d_ok / d_flags
    of the larger one.  Valid and invalid proofs (of all kinds: flags 0, 1, 2 and 4) mixed by a seeded pattern; the
    sequence runs twice with complementary patterns, so the first and last slot of every batch are on both sides."""
    rng = random.Random(0x7a11)
    ks = _key_scalars(rng, _scalars(rng, 4))
    key, _ = ve.make_key(*ks)
    a, bb = _scalars(rng, 2)
    pubs = [[rng.randrange(1 << 256) for _ in range(3)] for _ in range(3)]
    good, bad = [], []
    for pub in pubs:
        c = ve.solve_c(ks, a, bb, pub)
        good += [(a, bb, c, pub), (ve.solve_a(ks, bb, pub), bb, 0, pub), (0, bb, ve.solve_c(ks, 0, bb, pub), pub)]
        bad += [(a, bb, c + 1, pub), (a, bb, c, _bump(pub, 2)), (a, bb, 0, pub), (0, bb, c, pub)]
    assert _expect(ks, good) == [True] * len(good) and _expect(ks, bad) == [False] * len(bad)
    good, bad = _items(good), _items(bad)
    # rejected by the encoding rules (flag 1: verify_final_kernel answers without a pairing): a coordinate + q, C off its curve
    for k, (key_, i) in enumerate((("pi_a", 0), ("pi_c", 1))):
        pub_s, po = copy.deepcopy(good[3 * k])
        po[key_][i] = str(int(po[key_][i]) + (Q if key_ == "pi_a" else 1))
        bad.append((pub_s, po))
    ver = amd.Verifier(key, 3, montgomery=True, device=0)
    seen = []
    first, last = set(), set()
    for flip in (False, True):
        for count in (1, 63, 64, 65, 130, 2):
            exp = [rng.random() < 0.6 for _ in range(count)]
            exp[0], exp[-1] = True, count == 1
            if flip:
                exp[0], exp[-1] = False, count != 1
            got = ver.verify_batch([rng.choice(good) if ok else rng.choice(bad) for ok in exp])
            assert got == exp, "batch of %d: %r" % (count, [i for i in range(count) if got[i] != exp[i]])
            first.add((count, exp[0]))
            last.add((count, exp[-1]))
            seen += exp
    ver.close()
    assert True in seen and False in seen
    for count in (1, 63, 64, 65, 130, 2):
        assert {(count, True), (count, False)} <= first and {(count, True), (count, False)} <= last


# ------------------------------------------------------------------ encoding rules
def test_noncanonical_and_off_curve_points_are_rejected_between_valid_ones(amd):
    """A coordinate at or above q is rejected (no reduction), and so is a point off its curve: each of the 8 coordinate
    words of a valid proof as value + q and as q itself, an off-curve A, B (c1 of x only) and C -- every one between
    two valid proofs of the same batch, which stay accepted."""
    rng = random.Random(0xe1c)
    ks = _key_scalars(rng, _scalars(rng, 3))
    key, _ = ve.make_key(*ks)
    pub = [rng.randrange(1 << 256) for _ in range(2)]
    valid = []
    for _ in range(2):
        a, bb = _scalars(rng, 2)
        valid.append((a, bb, ve.solve_c(ks, a, bb, pub), pub))
    assert _expect(ks, valid) == [True, True]
    (pub_s, base), (_, other) = _items(valid)
    words = [("pi_a", 0), ("pi_a", 1), ("pi_b", 0, 0), ("pi_b", 0, 1), ("pi_b", 1, 0), ("pi_b", 1, 1), ("pi_c", 0), ("pi_c", 1)]

    def put(path, fn):
        t = copy.deepcopy(base)
        box = t
        for k in path[:-1]:
            box = box[k]
        value = fn(int(box[path[-1]]))
        assert 0 <= value <= TOP
        box[path[-1]] = str(value)
        return t

    tampered = []
    for path in words:
        tampered.append(put(path, lambda v: v + Q))
        tampered.append(put(path, lambda v: Q))
    off = [put(("pi_a", 1), lambda v: (v + 1) % Q), put(("pi_b", 0, 1), lambda v: (v + 1) % Q), put(("pi_c", 0), lambda v: (v + 1) % Q)]
    assert not b.G1.on_curve((int(off[0]["pi_a"][0]), int(off[0]["pi_a"][1])))
    assert not b.G2.on_curve(((int(off[1]["pi_b"][0][0]), int(off[1]["pi_b"][0][1])), (int(off[1]["pi_b"][1][0]), int(off[1]["pi_b"][1][1]))))
    assert not b.G1.on_curve((int(off[2]["pi_c"][0]), int(off[2]["pi_c"][1])))
    tampered += off
    items, exp = [(pub_s, base)], [True]
    for k, t in enumerate(tampered):
        items += [(pub_s, t), (pub_s, other if k % 2 == 0 else base)]
        exp += [False, True]
    assert len(tampered) == 19
    ver = amd.Verifier(key, 2, montgomery=True, device=0)
    got = ver.verify_batch(items)
    ver.close()
    assert got == exp, [i for i in range(len(exp)) if got[i] != exp[i]]
    assert True in got and False in got
