"""NIST P-256 and ECDSA in big-int affine arithmetic: the reference the ES256 tests compare the library against
(FIPS 186-4 D.1.2.3 for the curve, 6.4 for the signature).  Points are (x, y) tuples, None is infinity."""
P = 2**256 - 2**224 + 2**192 + 2**96 - 1
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
B = 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b
G = (0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
     0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5)


def on_curve(pt):
    return pt is not None and (pt[1] * pt[1] - pt[0] ** 3 + 3 * pt[0] - B) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], (-pt[1]) % P)


def add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = (3 * a[0] * a[0] - 3) * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def mul(k, pt):
    acc = None
    k %= N
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def sign(d, k, e):
    """(r, s) of the digest integer e (any size: reduced modulo n) under the private key d with the nonce k."""
    r = mul(k, G)[0] % N
    s = pow(k, -1, N) * (e + r * d) % N
    assert r and s
    return r, s


def verify(q, e, r, s):
    if not (1 <= r < N and 1 <= s < N):
        return False
    w = pow(s, -1, N)
    pt = add(mul(e * w % N, G), mul(r * w % N, q))
    return pt is not None and pt[0] % N == r


def be(x):
    return int(x).to_bytes(32, "big")


def point_bytes(pt):
    """x | y big-endian, (0, 0) for infinity: the key form and the layer operator's point form"""
    return bytes(64) if pt is None else be(pt[0]) + be(pt[1])
