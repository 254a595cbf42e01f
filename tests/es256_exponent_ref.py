"""Python twin of the ES256 verdict "in the exponent", written from the ECDSA equation and not from the C++: the verifier
computes u1 = e / s, u2 = r / s (mod n), R = u1 G + u2 Q, and accepts iff R is not infinity and x(R) mod n = r.  With
the key a KNOWN multiple Q = d G,

  R = k G,  k = u1 + u2 d  (mod n),

one congruence and one multiple of G (accepts()).  And the equation can be turned round: a verifier takes digests, not
messages, so for ANY chosen pair (u1, u2) there is a valid signature --

  key of known d    R = (u1 + u2 d) G,  r = x(R) mod n,  s = r / u2,  digest = u1 s          (signature_for)
  chosen point R    Q = u2^-1 (R - u1 G),  r, s, digest as above                              (signature_for_point)

-- which puts an ACCEPTED signature on any table entry, lane, tree slot or compare branch one wants, with a rejected
neighbour one step away (the same u1, u2 claiming another r).  Nothing here calls the library; the arithmetic is
p256_ref's affine big-int addition.  tests/test_cpu_es256_exponent.py checks the rule against p256_ref.verify.

  a signature   (key bytes x | y, digest (32 bytes), r | s (64 bytes))"""
import functools

import p256_ref as ref
from p256_ref import N, P

WINDOWS, DIGITS = 64, 15


@functools.lru_cache(None)
def table(pt):
    """rows[w][dg - 1] = dg * 16^w * pt (dg = 1..15, w < 64): the window table of csrc/p256.cuh, by additions alone --
    one ref.add per entry, the sixteenth multiple of a row is the base of the next."""
    rows, base = [], pt
    for _ in range(WINDOWS):
        row = [base]
        for _ in range(DIGITS - 1):
            row.append(ref.add(row[-1], base))
        rows.append(row)
        base = ref.add(row[-1], base)
    return rows


def mul_g(k):
    """k G from G's table: at most 64 additions."""
    rows, acc, k = table(ref.G), None, k % N
    for w in range(WINDOWS):
        dg = (k >> (4 * w)) & 15
        if dg:
            acc = ref.add(acc, rows[w][dg - 1])
    return acc


@functools.lru_cache(None)
def key_point(d):
    assert d % N
    return mul_g(d)


def _signature(q, u1, u2, R, r, digest_add):
    """The signature under the key point q whose verification computes the scalars u1, u2 (hence R = u1 G + u2 q) and
    claims r (None: x(R) mod n, the valid one)."""
    assert 0 <= u1 < N and 0 < u2 < N and digest_add in (0, N)
    if r is None:
        assert R is not None
        r = R[0] % N
    assert 0 <= r < 1 << 256
    s = r * pow(u2, -1, N) % N        # (r = 0, r >= n: the signatures the range check must stop)
    digest = u1 * s % N + digest_add
    assert digest < 1 << 256
    return ref.point_bytes(q), ref.be(digest), ref.be(r) + ref.be(s)


def signature_for(u1, u2, d, digest_add=0, R=None, r=None):
    """Under the key d G.  R: the point (u1 + u2 d) G where the caller has it already (from a table); r: see _signature."""
    if R is None and r is None:
        R = mul_g(u1 + u2 * d)
    return _signature(key_point(d), u1, u2, R, r, digest_add)


def signature_for_point(u1, u2, R, digest_add=0, r=None):
    """Under the key Q = u2^-1 (R - u1 G), whose discrete log nobody knows when R comes from find_x."""
    q = ref.mul(pow(u2, -1, N), ref.add(R, ref.neg(mul_g(u1))))
    assert ref.on_curve(q)
    return _signature(q, u1, u2, R, r, digest_add)


def accepts(d, digest, r, s):
    """The verdict for the key d G: the range check, k = u1 + u2 d, k != 0, x(k G) mod n == r."""
    if not (1 <= r < N and 1 <= s < N):
        return False
    w = pow(s, -1, N)
    k = (digest * w + r * w * d) % N
    return k != 0 and mul_g(k)[0] % N == r


def find_x(lo, step):
    """The first x from lo in direction step (+1 / -1) that is the abscissa of a curve point, and that point (the root
    a^((p + 1) / 4), p = 3 mod 4)."""
    x = lo
    while True:
        assert 0 <= x < P
        a = (x * x * x - 3 * x + ref.B) % P
        y = pow(a, (P + 1) // 4, P)
        if y * y % P == a:
            return x, (x, y)
        x += step
