"""tests/verify_exponent_ref.py (the Groth16 verdict as one congruence between known exponents) against
oracle/groth16.py::verify (oracle/bn254.py's pairing), before tests/test_gpu_verify_exponent.py takes every expected
verdict of the device verifier from it.  Eight oracle verdicts: each costs two to four Python Miller loops."""
import random

import groth16 as g
from bn254 import R

import verify_exponent_ref as ve


def test_congruence_equals_the_oracles_pairing_check():
    rng = random.Random(0xe49)
    ks = ([rng.randrange(1, R) for _ in range(4)],) + tuple(rng.randrange(1, R) for _ in range(4))
    key, vk = ve.make_key(*ks)
    assert len(key) == 64 + 3 * 128 + 4 * 64 and len(vk["IC"]) == 4
    a, b_ = rng.randrange(1, R), rng.randrange(1, R)
    pub = [rng.randrange(R) for _ in range(3)]
    while pub[1] + R >= 1 << 256:
        pub[1] = rng.randrange(R)
    c = ve.solve_c(ks, a, b_, pub)
    wrapped = [pub[0], pub[1] + R, pub[2]]
    pub_x0 = pub[:2] + [ve.solve_last_signal(ks, pub[:2])]
    c_a0 = ve.solve_c(ks, 0, b_, pub)
    cases = [                                                       # (name, a, b, c, signals, verdict)
        ("generic", a, b_, c, pub, True),
        ("c + 1", a, b_, c + 1, pub, False),
        ("C = infinity", ve.solve_a(ks, b_, pub), b_, 0, pub, True),
        ("vk_x = infinity", a, b_, ve.solve_c(ks, a, b_, pub_x0), pub_x0, True),
        ("A = infinity", 0, b_, c_a0, pub, True),
        ("A = infinity, c + 1", 0, b_, c_a0 + 1, pub, False),
        ("signal + r", a, b_, c, wrapped, True),
        ("B = infinity", a, 0, ve.solve_c(ks, a, 0, pub), pub, True),
    ]
    assert ve.vk_x(ks, pub_x0) == 0 and c_a0 == ve.solve_c(ks, a, 0, pub)
    for name, ca, cb, cc, ps, verdict in cases:
        assert ve.accepts(ks, ca, cb, cc, ps) is verdict, name
        assert g.verify(vk, ps, ve.proof_points(ca, cb, cc)) is verdict, name


def test_solvers_and_encodings():
    rng = random.Random(3)
    ks = ([rng.randrange(1, R) for _ in range(6)],) + tuple(rng.randrange(1, R) for _ in range(4))
    b_ = rng.randrange(1, R)
    head = [rng.randrange(1 << 256) for _ in range(4)]
    pub = head + [ve.solve_last_signal(ks, head, ve.x_without_a_and_c(ks))]
    assert ve.accepts(ks, 0, b_, 0, pub) and ve.accepts(ks, 5, 0, 0, pub) and not ve.accepts(ks, 1, b_, 0, pub)
    assert ve.accepts(ks, ve.solve_a(ks, b_, head + [7]), b_, 0, head + [7])
    assert not ve.accepts(ks, ve.solve_a(ks, b_, head + [7]), b_, 0, head + [8])
    # a key with points at infinity: zeros in the byte image, None in the oracle's dict; signals of such an IC_j are free
    ks0 = ([0, 5, 0, 9],) + tuple(ks[1:])
    key, vk = ve.make_key(*ks0)
    assert key[448:512] == bytes(64) and key[576:640] == bytes(64) and key[512:576] != bytes(64)
    assert vk["IC"][0] is None and vk["IC"][2] is None and vk["IC"][1] is not None
    c = ve.solve_c(ks0, 3, b_, [1, 2, 3])
    assert ve.accepts(ks0, 3, b_, c, [1, 12345, 3]) and not ve.accepts(ks0, 3, b_, c, [2, 2, 3])
    po = ve.proof_obj(0, 0, c)
    assert po["pi_a"] == ["0", "1", "0"] and po["pi_b"] == [["0", "0"], ["1", "0"], ["0", "0"]] and po["pi_c"][2] == "1"
    assert ve.proof_obj(3, b_, 0)["pi_c"] == ["0", "1", "0"]
