"""Case builders shared by test_cpu_es256.py (device -1) and test_gpu_es256.py (device 0): inputs and the verdicts /
values of the big-int reference p256_ref, each built once per session."""
import base64
import functools
import hashlib
import json
import os
import random

import p256_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_DIGEST = "271ce33d671a2d3b816d788135f4343e14bc66802f8cd841faac939e8c11f3ee"


def _b64u(s):
    return base64.urlsafe_b64decode(s + "=" * (-len(s) % 4))


@functools.lru_cache(None)
def golden_key():
    """The NZCP specification's example issuer key as x | y."""
    doc = json.load(open(os.path.join(GOLDEN, "nzcp_example_issuer.json")))
    jwk = doc["keys"][doc["iss"] + "#" + doc["kid"]]
    return _b64u(jwk["x"]) + _b64u(jwk["y"])


def _bstr(buf, pos):
    """A CBOR byte string at pos -> (bytes, next position)."""
    major, n = buf[pos] >> 5, buf[pos] & 31
    assert major == 2
    pos += 1
    if n >= 24:
        size = 1 << (n - 24)
        n = int.from_bytes(buf[pos:pos + size], "big")
        pos += size
    return buf[pos:pos + n], pos + n


@functools.lru_cache(None)
def golden_pass():
    """(SHA-256 of ToBeSigned, r | s, ToBeSigned) of the specification's example pass."""
    uri = open(os.path.join(GOLDEN, "example_pass_uri.txt")).read().strip()
    b32 = uri.split("/")[-1]
    cose = base64.b32decode(b32 + "=" * (-len(b32) % 8))
    assert cose[0] == 0xD2 and cose[1] == 0x84   # tag 18, array of 4
    protected, pos = _bstr(cose, 2)
    assert cose[pos] == 0xA0                     # empty unprotected map
    payload, pos = _bstr(cose, pos + 1)
    sig, pos = _bstr(cose, pos)
    assert len(sig) == 64 and pos == len(cose)

    def bstr(b):
        return (bytes([0x40 + len(b)]) if len(b) < 24 else bytes([0x58, len(b)]) if len(b) < 256 else
                bytes([0x59]) + len(b).to_bytes(2, "big")) + b
    tbs = bytes([0x84, 0x6A]) + b"Signature1" + bstr(protected) + bstr(b"") + bstr(payload)
    digest = hashlib.sha256(tbs).digest()
    assert digest.hex() == GOLDEN_DIGEST
    return digest, sig, tbs


def specials(m):
    return [0, 1, m - 1, m - 2, (2**256 - 1) % m]


@functools.lru_cache(None)
def field_cases(m, seed):
    """(a, b) operand lists: every pair of the special values (sums and Montgomery running values at and past 2^256),
    then 64 random pairs."""
    rng = random.Random(seed)
    sp = specials(m)
    a = [x for x in sp for _ in sp] + [rng.randrange(m) for _ in range(64)]
    b = [y for _ in sp for y in sp] + [rng.randrange(m) for _ in range(64)]
    return a, b


def pack(values):
    return b"".join(ref.be(v) for v in values)


def unpack(buf):
    return [int.from_bytes(buf[i:i + 32], "big") for i in range(0, len(buf), 32)]


def _tile(items, count):
    """The case list cut or repeated to `count` items (None: as it is)."""
    return list(items) if count is None else (list(items) * (count // len(items) + 1))[:count]


def run_field_ops(amd, device, count=None):
    """Both fields' add, sub, mul and inverse through p256_op against Python ints (`count` items: see _tile)."""
    for name, m, seed in (("fp", ref.P, 1), ("fn", ref.N, 2)):
        a, b = field_cases(m, seed)
        a, b = _tile(a, count), _tile(b, count)
        for op, fn in (("add", lambda x, y: (x + y) % m), ("sub", lambda x, y: (x - y) % m), ("mul", lambda x, y: x * y % m)):
            got = unpack(amd.p256_op(f"{name}_{op}", pack(a), pack(b), device=device))
            assert got == [fn(x, y) for x, y in zip(a, b)], (name, op)
        inv_in = _tile([1, m - 1, 0] + field_cases(m, seed)[0][-8:], count)
        got = unpack(amd.p256_op(f"{name}_inv", pack(inv_in), device=device))
        assert got == [pow(x, -1, m) if x else 0 for x in inv_in], (name, "inv")


@functools.lru_cache(None)
def point_cases():
    """(a, b, a + b) affine triples: P+Q, P+P, P+(-P), inf+P, P+inf, inf+inf for P = G and random points."""
    rng = random.Random(3)
    pts = [ref.G] + [ref.mul(rng.randrange(1, ref.N), ref.G) for _ in range(3)]
    qs = [ref.mul(rng.randrange(1, ref.N), ref.G) for _ in range(4)]
    cases = [(None, None)]
    for p, q in zip(pts, qs):
        cases += [(p, q), (p, p), (p, ref.neg(p)), (None, p), (p, None)]
    return [(a, b, ref.add(a, b)) for a, b in cases]


def run_point_adds(amd, device, count=None):
    cases = _tile(point_cases(), count)
    a = b"".join(ref.point_bytes(c[0]) for c in cases)
    b = b"".join(ref.point_bytes(c[1]) for c in cases)
    want = b"".join(ref.point_bytes(c[2]) for c in cases)
    assert amd.p256_op("madd", a, b, device=device) == want
    assert amd.p256_op("add", a, b, device=device) == want


@functools.lru_cache(None)
def xcmp_cases():
    """(X, Z, r, expected) of the projective comparison x(X : Z) mod n == r."""
    rng = random.Random(4)
    gap = ref.P - ref.N
    out = []
    for _ in range(4):
        z = rng.randrange(1, ref.P)
        zz = z * z % ref.P
        r = rng.randrange(gap, ref.N)        # r + n >= p: only r itself can match
        small = rng.randrange(1, gap)        # r + n < p: both r and r + n match
        out += [(r * zz % ref.P, z, r, 1), ((r + 1) * zz % ref.P, z, r, 0), ((r + ref.N) * zz % ref.P, z, r, 0),
                (small * zz % ref.P, z, small, 1), ((small + ref.N) * zz % ref.P, z, small, 1),
                ((small + 1) * zz % ref.P, z, small, 0), (r * zz % ref.P, 0, r, 0)]
    out += [((gap - 1 + ref.N) * 9 % ref.P, 3, gap - 1, 1), ((gap + ref.N) * 9 % ref.P, 3, gap, 0)]   # the boundary r = p - n
    return out


def run_xcmp(amd, device, count=None):
    cases = _tile(xcmp_cases(), count)
    got = amd.p256_op("xcmp", b"".join(ref.be(c[0]) + ref.be(c[1]) for c in cases), pack([c[2] for c in cases]), device=device)
    assert list(got) == [c[3] for c in cases]


def _flip(b, bit):
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


D2 = 0x1F2E3D4C5B6A79881726354453627180A1B2C3D4E5F60718293A4B5C6D7E8F90   # the second, unrelated key
D5_16 = 5 * pow(16, -1, ref.N) % ref.N                                      # 16 Q = 5 G


@functools.lru_cache(None)
def signature_cases():
    """keys (x | y each) and [(name, digest, r | s, key index, expected verdict)]; every expectation is also the
    reference's verdict (asserted here)."""
    q2 = ref.mul(D2, ref.G)
    q5 = ref.mul(D5_16, ref.G)
    points = [None, q2, ref.G, ref.neg(ref.G), q5, ref.neg(q5)]
    keys = [golden_key()] + [ref.point_bytes(p) for p in points[1:]]
    points[0] = (int.from_bytes(keys[0][:32], "big"), int.from_bytes(keys[0][32:], "big"))
    digest, sig, _ = golden_pass()
    cases = [("golden", digest, sig, 0, True),
             ("digest bit", _flip(digest, 77), sig, 0, False),
             ("r bit", digest, _flip(sig, 13), 0, False),
             ("s bit", digest, _flip(sig, 256 + 200), 0, False),
             ("other key", digest, sig, 1, False)]
    r, s = sig[:32], sig[32:]
    for name, rr, ss in (("r = 0", bytes(32), s), ("s = 0", r, bytes(32)), ("r = n", ref.be(ref.N), s),
                         ("s = n", r, ref.be(ref.N)), ("r = 2^256 - 1", b"\xff" * 32, s)):
        cases.append((name, digest, rr + ss, 0, False))
    for name, e, k in (("e = n + 5", ref.N + 5, 0xC0FFEE), ("e = 2^256 - 1", 2**256 - 1, 0xBEEF01)):
        rr, ss = ref.sign(D2, k, e)
        cases.append((name, ref.be(e), ref.be(rr) + ref.be(ss), 1, True))
    # u1 = u2 = 5 under Q = G: the same table entry twice on one lane (the mixed addition doubles); under Q = -G the sum
    # is infinity
    r10 = ref.mul(10, ref.G)[0] % ref.N
    s5 = r10 * pow(5, -1, ref.N) % ref.N
    assert ref.be(r10).hex().startswith("cef66d6b") and ref.be(r10).hex().endswith("04c5723f")
    assert ref.be(s5).hex().startswith("5c97af7b") and ref.be(s5).hex().endswith("cd081e50")
    cases.append(("5 G + 5 G, one lane", ref.be(r10), ref.be(r10) + ref.be(s5), 2, True))
    cases.append(("5 G - 5 G, one lane", ref.be(r10), ref.be(r10) + ref.be(s5), 3, False))
    # u1 = 5, u2 = 16 under 16 Q = 5 G: two lanes' sums are equal (the full addition of the tree doubles); under -Q
    # they are opposite
    s16 = r10 * pow(16, -1, ref.N) % ref.N
    e5 = 5 * s16 % ref.N
    cases.append(("5 G + 5 G, two lanes", ref.be(e5), ref.be(r10) + ref.be(s16), 4, True))
    cases.append(("5 G - 5 G, two lanes", ref.be(e5), ref.be(r10) + ref.be(s16), 5, False))
    for name, dg, sg, k, want in cases:
        got = ref.verify(points[k], int.from_bytes(dg, "big"), int.from_bytes(sg[:32], "big"), int.from_bytes(sg[32:], "big"))
        assert got == want, name
    return keys, cases


def run_signature_cases(amd, device):
    keys, cases = signature_cases()
    v = amd.Es256Verifier(keys, device=device)
    try:
        got = v.verify_batch([c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases])
        assert [(c[0], g) for c, g in zip(cases, got)] == [(c[0], c[4]) for c in cases]
        # one at a time, and the default key
        assert v.verify_batch([cases[0][1]], [cases[0][2]]) == [True]
        assert v.verify_batch([cases[1][1]], [cases[1][2]]) == [False]
        assert v.verify_batch([], []) == []
        assert len(v.timings()) == 2
    finally:
        v.close()


BATCH_BAD = (0, 63, 64, 129)


@functools.lru_cache(None)
def batch130():
    """keys, digests, sigs, key_idx, expected: 130 signatures over 3 keys made by the reference, items BATCH_BAD spoiled
    (digest, r, s, key in turn); expected = the reference's verdicts."""
    rng = random.Random(5)
    ds = [rng.randrange(1, ref.N) for _ in range(3)]
    qs = [ref.mul(d, ref.G) for d in ds]
    digests, sigs, idx = [], [], []
    for i in range(130):
        k = i % 3
        e = rng.randrange(2**256)
        r, s = ref.sign(ds[k], rng.randrange(1, 2**40), e)   # (a short nonce keeps the reference quick)
        digests.append(ref.be(e))
        sigs.append(ref.be(r) + ref.be(s))
        idx.append(k)
    digests[0] = _flip(digests[0], 3)
    sigs[63] = _flip(sigs[63], 100)
    sigs[64] = _flip(sigs[64], 300)
    idx[129] = (idx[129] + 1) % 3
    want = [ref.verify(qs[k], int.from_bytes(d, "big"), int.from_bytes(s[:32], "big"), int.from_bytes(s[32:], "big"))
            for d, s, k in zip(digests, sigs, idx)]
    assert [i for i, w in enumerate(want) if not w] == list(BATCH_BAD)
    return [ref.point_bytes(q) for q in qs], digests, sigs, idx, want


@functools.lru_cache(None)
def mixed_wave():
    """One wavefront's worth of signatures (64) in which the crafted doubling and infinity cases sit among ordinary
    ones: keys, digests, sigs, key_idx, expected."""
    keys3, digests, sigs, idx, want = batch130()
    keys, cases = signature_cases()
    crafted = [c for c in cases if "lane" in c[0]]
    allkeys = keys3 + keys
    d, s, k, w = list(digests[:64]), list(sigs[:64]), list(idx[:64]), list(want[:64])
    for slot, c in zip((1, 2, 17, 33, 34, 62), crafted + crafted[:2]):
        d[slot], s[slot], k[slot], w[slot] = c[1], c[2], 3 + c[3], c[4]
    return allkeys, d, s, k, w


# ------------------------------------------------------------------ a 513-signal circuit for the combined verdict (GPU)
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N_PUB = 513
EXP, EXP_EARLY, NOW = 2000000000, 1600000000, 1700000000
_circuit = []


def _bits(digest):
    return [(byte >> (7 - k)) & 1 for byte in digest for k in range(8)]


def _witness(pub):
    """wire 0 = 1, wires 1..513 the public signals, then a, b = a^2, c = exp + signal 300 + a, d = b c"""
    a = 3
    c = (pub[512] + pub[300] + a) % R
    return [1] + pub + [a, a * a, c, a * a * c % R]


def pass_circuit(amd):
    """(vkey bytes, public signals, proofs) of a three-row circuit with NZCPPubIdentity's 513 public signals, set up with
    the trapdoor setup and proved on device 0, once per session: "a" the golden pass's digest bits with a credSubj digest
    and exp = EXP, "c" the same with signal 300 = 2, "d" the same as "a" with exp = EXP_EARLY (before NOW)."""
    if _circuit:
        return _circuit[0]
    import formats as f
    one, a, b, c, d = 0, N_PUB + 1, N_PUB + 2, N_PUB + 3, N_PUB + 4
    rows = [([(a, 1)], [(a, 1)], [(b, 1)]),
            ([(513, 1), (301, 1), (a, 1)], [(one, 1)], [(c, 1)]),
            ([(b, 1)], [(c, 1)], [(d, 1)])]
    zkey, vkey = amd.r1cs_setup(f.write_r1cs(N_PUB + 5, N_PUB, 0, rows), 41, 2)
    digest, _, _ = golden_pass()
    cred = _bits(bytes(range(32)))
    pubs = {"a": cred + _bits(digest) + [EXP], "d": cred + _bits(digest) + [EXP_EARLY]}
    pubs["c"] = list(pubs["a"])
    pubs["c"][300] = 2
    prover = amd.Prover(zkey, device=0)
    proofs = {}
    for name, pub in pubs.items():
        proofs[name], got = prover.prove(f.write_wtns(_witness(pub)))
        assert [int(x) for x in got] == pub
    prover.close()
    _circuit.append((vkey, pubs, proofs))
    return _circuit[0]
