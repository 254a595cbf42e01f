"""the Groth16 batch verifier on the device (csrc/verify.hip, pairing.cuh) through the C ABI
(g16_verifier_create / g16_verify_batch) against oracle/groth16.py::verify (oracle/bn254.py's pairing) -- the
acceptance check snarkjs `groth16.verify` performs.  Every verdict, accepted or rejected, must be the
oracle's verdict; the pairing VALUE the kernels compute is compared with the oracle's as well."""
import copy
import random

import pytest

import bn254 as b
import formats as f
import groth16 as g
import synth
import verify_exponent_ref as ve
from test_cpu_pairing import oracle_value, tower_to_poly

pytestmark = pytest.mark.gpu


def _vk(vkey, p):
    return {"alpha1": f.g1_from_lem(vkey[0:64]), "beta2": f.g2_from_lem(vkey[64:192]),
            "gamma2": f.g2_from_lem(vkey[192:320]), "delta2": f.g2_from_lem(vkey[320:448]),
            "IC": [f.g1_from_lem(vkey[448 + 64 * i:512 + 64 * i]) for i in range(p + 1)]}


def _oracle_verdict(vk, pub, proof):
    try:
        pts = (f.g1_from_obj(proof["pi_a"]), f.g2_from_obj(proof["pi_b"]), f.g1_from_obj(proof["pi_c"]))
    except Exception:
        return False
    for P, curve in ((pts[0], b.G1), (pts[1], b.G2), (pts[2], b.G1)):
        if P is not None and not curve.on_curve(P):
            return False
    return g.verify(vk, [int(x) for x in pub], pts)


def test_pairing_value_on_device_equals_oracle(amd):
    rng = random.Random(17)
    pairs = [(b.G1_GEN, b.G2_GEN)]
    for _ in range(5):
        pairs.append((b.G1.mul(b.G1_GEN, rng.randrange(1, b.R)), b.G2.mul(b.G2_GEN, rng.randrange(1, b.R))))
    got = amd.pairing_op(pairs)
    for (P, Qp), vals in zip(pairs, got):
        assert tower_to_poly(vals) == oracle_value(P, Qp)
    # bilinearity on the device alone, 64 pairs (one full wavefront)
    a, c = rng.randrange(1, b.R), rng.randrange(1, b.R)
    v = amd.pairing_op([(b.G1.mul(b.G1_GEN, a), b.G2.mul(b.G2_GEN, c)), (b.G1.mul(b.G1_GEN, a * c % b.R), b.G2_GEN)] * 32)
    assert all(x == v[0] for x in v)


def test_pairing_identities_between_device_values(amd):
    """Identities every pairing satisfies, between values the device computed (compared through tower_to_poly with
    oracle/bn254.py's Fq12 product; no Python Miller loop): e(-P, Q) e(P, Q) = 1, additivity in either argument,
    e(P, Q)^r = 1 and e(P, Q) != 1."""
    rng = random.Random(0x9a1)
    p1, p2, q1, q2 = (rng.randrange(1, b.R) for _ in range(4))
    P1, P2, P12 = ve.g1_points([p1, p2, p1 + p2])
    Q1, Q2, Q12 = ve.g2_points([q1, q2, q1 + q2])
    pairs = [(P1, Q1), (b.G1.neg(P1), Q1), (P2, Q1), (P12, Q1), (P1, Q2), (P1, Q12)]
    e, e_neg, e_p2, e_p12, e_q2, e_q12 = (tower_to_poly(v) for v in amd.pairing_op(pairs))
    assert e != b.F12_ONE and e_neg != e
    assert b.f12_mul(e_neg, e) == b.F12_ONE
    assert b.f12_mul(e, e_p2) == e_p12
    assert b.f12_mul(e, e_q2) == e_q12
    assert b.f12_pow(e, b.R) == b.F12_ONE
    assert b.f12_pow(e_q12, b.R) == b.F12_ONE


def test_pairing_op_grid_tails(amd):
    """1, 63, 65 and 130 pairs drawn from 5 distinct ones: a partial wavefront alone, beside one and two full ones; every
    output is the value the same pair has in a 5-pair call."""
    rng = random.Random(0x7a1)
    five = list(zip(ve.g1_points([rng.randrange(1, b.R) for _ in range(5)]), ve.g2_points([rng.randrange(1, b.R) for _ in range(5)])))
    ref = amd.pairing_op(five)
    assert len({tuple(v) for v in ref}) == 5
    for count in (1, 63, 65, 130):
        pick = [rng.randrange(5) for _ in range(count)]
        pick[0], pick[-1] = count % 5, (count + 3) % 5
        got = amd.pairing_op([five[k] for k in pick])
        assert len(got) == count
        assert [i for i in range(count) if got[i] != ref[pick[i]]] == []


def test_precomputed_line_miller_loop_agrees_with_the_on_the_fly_loop(amd):
    """g2_precompute + miller_loop_pre (gamma2, delta2) have no operator: they are pinned by verdict, beside the
    on-the-fly miller_loop, on one G2 point Q = g G2 and a known k, B = k Q, A = a G1.
      key "gamma"  gamma2 = Q; the signals are solved so that vk_x = k A, and C so that e(C, delta2) e(alpha1, beta2) = 1.
                   What is left of the product is  miller_loop(-A, k Q) [factor 0] * miller_loop_pre(k A, Q) [factor 1],
                   one after the final exponentiation iff the two loops agree.
      key "delta"  delta2 = Q; C = k A, and the signals are solved so that e(vk_x, gamma2) e(alpha1, beta2) = 1.
                   What is left is  miller_loop(-A, k Q) [factor 0] * miller_loop_pre(k A, Q) [factor 2].
    k = 1 (B = Q itself), 2, r - 1 (B = -Q) and random; the neighbours B = (k + 1) Q are rejected.  Expected verdicts
    are verify_exponent_ref.accepts()."""
    rng = random.Random(0x11e)
    ics = [rng.randrange(1, b.R) for _ in range(3)]
    alpha, beta, g, other, a = (rng.randrange(1, b.R) for _ in range(5))
    head = [rng.randrange(1 << 256)]
    for which in ("gamma", "delta"):
        ks = (ics, alpha, beta, g, other) if which == "gamma" else (ics, alpha, beta, other, g)
        key, _ = ve.make_key(*ks)
        cases = []
        for k in (1, 2, b.R - 1, rng.randrange(1, b.R)):
            if which == "gamma":
                pub = head + [ve.solve_last_signal(ks, head, k * a % b.R)]
                c = -alpha * beta * pow(other, -1, b.R) % b.R
            else:
                pub = head + [ve.solve_last_signal(ks, head, ve.x_without_a_and_c(ks))]
                c = k * a % b.R
            assert c == ve.solve_c(ks, a, k * g % b.R, pub)
            cases += [(a, k * g % b.R, c, pub), (a, (k + 1) * g % b.R, c, pub)]
        exp = [ve.accepts(ks, *case) for case in cases]
        assert exp == [True, False] * 4
        ve.g1_points([x for ca, _, cc, _ in cases for x in (ca, cc)])
        ve.g2_points([cb for _, cb, _, _ in cases])
        ver = amd.Verifier(key, 2, montgomery=True, device=0)
        got = ver.verify_batch([([str(x) for x in pub], ve.proof_obj(ca, cb, cc)) for ca, cb, cc, pub in cases])
        ver.close()
        assert got == exp, which


@pytest.mark.parametrize("n,p,m,seed", [(150, 6, 120, 2), (900, 513, 380, 24)])
def test_verdicts_equal_oracle(amd, n, p, m, seed):
    zkey, wtns, vkey = amd.synth_setup(n, p, m, seed, 4)
    vk = _vk(vkey, p)
    prover = amd.Prover(zkey, device=0)
    proof, pub = prover.prove(wtns)
    wt2 = amd.synth_witness(n, p, m, seed, 999)
    proof2, pub2 = prover.prove(wt2)
    prover.close()
    ver = amd.Verifier(vkey, p, montgomery=True, device=0)
    cases = [(pub, proof), (pub2, proof2)]
    # wrong statement / wrong proof
    cases.append((pub2, proof))
    cases.append((pub, proof2))
    bad_pub = list(pub)
    bad_pub[p // 2] = str((int(bad_pub[p // 2]) + 1) % b.R)
    cases.append((bad_pub, proof))
    # a public signal given as value + r: snarkjs reduces modulo r, the verdict stays "accepted"
    wrap = list(pub)
    if int(wrap[0]) + b.R < (1 << 256):
        wrap[0] = str(int(wrap[0]) + b.R)
        cases.append((wrap, proof))
    # tampered points: still on the curve (negated A, C := A), off the curve, coordinate >= q, infinity
    t = copy.deepcopy(proof)
    t["pi_a"][1] = str(b.Q - int(t["pi_a"][1]))
    cases.append((pub, t))
    t = copy.deepcopy(proof)
    t["pi_c"] = list(proof["pi_a"])
    cases.append((pub, t))
    t = copy.deepcopy(proof)
    t["pi_c"][0] = str((int(t["pi_c"][0]) + 1) % b.Q)
    cases.append((pub, t))
    t = copy.deepcopy(proof)
    t["pi_b"][0][0] = str((int(t["pi_b"][0][0]) + 1) % b.Q)
    cases.append((pub, t))
    t = copy.deepcopy(proof)
    t["pi_a"][0] = str(int(t["pi_a"][0]) + b.Q)
    cases.append((pub, t))
    t = copy.deepcopy(proof)
    t["pi_a"] = ["0", "1", "0"]
    cases.append((pub, t))
    t = copy.deepcopy(proof)
    t["pi_b"] = [["0", "0"], ["1", "0"], ["0", "0"]]
    cases.append((pub, t))
    got = ver.verify_batch(cases)
    exp = []
    for ps, pr in cases:
        if any(int(pr[k][i]) >= b.Q for k in ("pi_a", "pi_c") for i in range(2)):
            exp.append(False)       # the oracle's big-int arithmetic would reduce it; snarkjs / the product reject the encoding
        else:
            exp.append(_oracle_verdict(vk, [int(x) % b.R for x in ps], pr))
    assert got == exp
    assert got[0] and got[1] and not got[4]
    if pub2 != pub:      # (a redrawn witness may keep the public wires: then both cross pairs are valid statements)
        assert not got[2] and not got[3]
    # one at a time == batch; too few signals = rejected
    assert [ver.verify(ps, pr) for ps, pr in cases[:4]] == got[:4]
    assert ver.verify(pub[:-1], proof) is False
    # the verification_key.json route (standard-form points) gives the same handle behaviour
    ver2 = amd.Verifier(amd.vkey_json(vkey, p), device=0)
    assert ver2.verify_batch(cases) == got
    ver.close()
    ver2.close()


def test_batch_of_256_with_known_bad_indices(amd):
    n, p, m, seed = 600, 20, 500, 31
    zkey, wtns, vkey = amd.synth_setup(n, p, m, seed, 4)
    prover = amd.Prover(zkey, device=0)
    base = []
    for k in range(8):
        w = wtns if k == 0 else amd.synth_witness(n, p, m, seed, 100 + k)
        proof, pub = prover.prove(w)
        base.append((pub, proof))
    prover.close()
    amd.Verifier(vkey, p, device=0).close()   # a handle that never ran a batch
    ver = amd.Verifier(vkey, p, device=0)
    rng = random.Random(3)
    bad = set(rng.sample(range(256), 23))
    items = []
    for i in range(256):
        pub, proof = base[i % 8]
        if i in bad:
            pub = list(pub)
            pub[i % p] = str((int(pub[i % p]) + 1 + i) % b.R)
        items.append((pub, proof))
    got = ver.verify_batch(items)
    assert got == [i not in bad for i in range(256)]
    assert len(ver.timings()) == 3
    # the same handle again: across a 64-lane block edge on the grown scratch, one proof, the whole batch
    assert ver.verify_batch(items[3:68]) == got[3:68]
    assert ver.verify_batch(items[:1]) == got[:1]
    assert ver.verify_batch(items) == got
    ver.close()


def test_verifier_key_errors(amd):
    zkey, _, vkey = amd.synth_setup(150, 6, 120, 2, 2)
    with pytest.raises(amd.G16Error) as e:
        amd.Verifier(vkey[:-1], 6)
    assert e.value.code == -2
    broken = bytearray(vkey)
    broken[0] ^= 1                       # alpha1.x: off the curve
    with pytest.raises(amd.G16Error) as e:
        amd.Verifier(bytes(broken), 6)
    assert e.value.code == -2 and "curve" in str(e.value)
