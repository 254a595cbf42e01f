"""The ES256 verification schedule pinned "in the exponent" (tests/es256_exponent_ref.py: a valid signature for any chosen
u1, u2; tests/es256_cases.py: the families): every table entry, the exceptional additions at every key position of a
lane and every slot of the tree, the compare's branches, the scalar edges.  Here the construction's verdicts are pinned
to the big-int reference p256_ref.verify, and the families run on the host route (device -1: the code the kernels run).
No GPU needed."""
import pytest

import es256_cases as cases
import es256_exponent_ref as ex
import p256_ref as ref


def _int(b):
    return int.from_bytes(b, "big")


def test_tables_and_roots():
    rows = ex.table(ref.G)
    assert len(rows) == 64 and all(len(r) == 15 for r in rows)
    for w, dg in ((0, 1), (0, 15), (1, 1), (17, 9), (63, 15)):
        assert rows[w][dg - 1] == ref.mul(dg << (4 * w), ref.G)
    k = 0x8F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF0 % ref.N
    assert ex.mul_g(k) == ref.mul(k, ref.G) and ex.mul_g(0) is None and ex.mul_g(ref.N) is None
    for lo, step in ((ref.N, 1), (1, 1), (ref.P - 1, -1)):
        x, pt = ex.find_x(lo, step)
        assert ref.on_curve(pt) and pt[0] == x
        between = range(lo, x, step)
        assert len(between) < 16 and not any(pow((t**3 - 3 * t + ref.B) % ref.P, (ref.P - 1) // 2, ref.P) == 1 for t in between)


def test_both_builders_give_valid_signatures():
    d, u2 = 0xD00D, 0x89ABCDE << 100
    for u1, add in ((0x1234567 << 200, 0), (0, ref.N)):   # (n is added where the sum fits 256 bits: here to the digest 0)
        key, digest, sig = ex.signature_for(u1, u2, d, digest_add=add)
        q = ref.mul(d, ref.G)
        assert key == ref.point_bytes(q) and _int(digest) >= add
        assert ref.verify(q, _int(digest), _int(sig[:32]), _int(sig[32:]))
        assert ex.accepts(d, _int(digest), _int(sig[:32]), _int(sig[32:]))
        # the verifier's scalars are the chosen ones
        w = pow(_int(sig[32:]), -1, ref.N)
        assert (_int(digest) * w % ref.N, _int(sig[:32]) * w % ref.N) == (u1, u2)
    R = ref.mul(0xABCDEF, ref.G)
    u1 = 0x1234567 << 200
    key, digest, sig = ex.signature_for_point(u1, u2, R)
    q = (_int(key[:32]), _int(key[32:]))
    assert ref.add(ref.mul(u1, ref.G), ref.mul(u2, q)) == R
    assert ref.verify(q, _int(digest), _int(sig[:32]), _int(sig[32:]))
    assert not ex.accepts(d, _int(digest), 0, _int(sig[32:])) and not ex.accepts(d, _int(digest), _int(sig[:32]), ref.N)


@pytest.mark.parametrize("family", "abcde")
def test_constructions_against_the_reference(family):
    """every case of families b to e, every 7th of family a (7 is coprime to 15 and to 64: every digit and every window
    of both tables is sampled)"""
    every = cases.EXPONENT_FAMILIES[family]()
    sample = every[::7] if family == "a" else every
    assert len(sample) >= 12
    for name, key, d, digest, sig, want in sample:
        q = (_int(key[:32]), _int(key[32:]))
        e, r, s = _int(digest), _int(sig[:32]), _int(sig[32:])
        assert ref.verify(q, e, r, s) == want, name
        if d is not None:
            assert key == ref.point_bytes(ex.key_point(d)), name
            assert ex.accepts(d, e, r, s) == want, name


def test_family_a_reaches_every_table_entry():
    """digit by digit from the signatures themselves: u2 (u1 with u2 = 1) has one non-zero digit, and all 960 occur"""
    seen = {"key": set(), "G": set()}
    for name, _, _, digest, sig, want in cases.family_a():
        if not want:
            continue
        w = pow(_int(sig[32:]), -1, ref.N)
        u1, u2 = _int(digest) * w % ref.N, _int(sig[:32]) * w % ref.N
        u, which = (u2, "key") if u1 == 0 else (u1, "G")
        assert which == "G" or _int(digest) in (0, ref.N), name
        assert which == "key" or u2 == 1, name
        digits = [(win, (u >> (4 * win)) & 15) for win in range(64) if (u >> (4 * win)) & 15]
        assert len(digits) == 1, name
        seen[which].add(digits[0])
    assert len(seen["key"]) == len(seen["G"]) == 960
    assert {_int(c[3]) for c in cases.family_a() if c[0].startswith("a: key entry") and c[5]} == {0, ref.N}


@pytest.mark.parametrize("family", "abcde")
def test_host_route_every_family(amd, family):
    every = cases.EXPONENT_FAMILIES[family]()
    assert {c[5] for c in every} == {True, False}
    cases.run_exponent_batches(amd, -1, cases.exponent_batches(every))


def test_host_route_every_group_position(amd):
    batches = cases.exponent_batches(cases.exponent_cases())
    assert all(len(keys) <= 16 and len(items) % 4 for keys, items in batches)
    assert sum(c[0].startswith("dead group") for _, items in batches for c in items) > 400
    cases.run_exponent_batches(amd, -1, batches, rotations=(1, 2, 3))
