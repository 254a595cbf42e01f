"""Case builders shared by test_cpu_es256.py (device -1) and test_gpu_es256.py (device 0): inputs and the verdicts /
values of the big-int reference p256_ref, each built once per session; and the families that pin the verification
schedule in the exponent (es256_exponent_ref), with the verdicts their construction gives."""
import base64
import functools
import hashlib
import json
import os
import random

import es256_exponent_ref as ex
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


# ------------------------------------------------------------------ the verification schedule, pinned in the exponent
# Signatures built by es256_exponent_ref for chosen (u1, u2): an accepted one on every table entry, lane position, tree
# slot and compare branch, a rejected neighbour beside it.  A case is (name, key bytes, d or None, digest, r | s,
# expected verdict): d the key's discrete log where it is known, the verdict the one the construction gives
# (tests/test_cpu_es256_exponent.py pins it to p256_ref.verify).
def _case(name, signature, want, d=None):
    key, digest, sig = signature
    return (name, key, d, digest, sig, want)


def _r_of(signature):
    return int.from_bytes(signature[2][:32], "big")


@functools.lru_cache(None)
def family_a():
    """Every table entry: u2 = dg 16^w alone (the key's table; digests 0 and n in turn, so u1 = 0), then u1 = dg 16^w
    with u2 = 1 (G's table), R read from the Python tables; then per window two rejects: a G-entry signature under the
    digest of the next digit, and the key entry dg + 1 claiming the r of entry dg."""
    d = random.Random(6).randrange(1, ref.N)
    q = ex.key_point(d)
    tg, tq = ex.table(ref.G), ex.table(q)
    entries = [(w, dg) for w in range(ex.WINDOWS) for dg in range(1, 16) if dg << (4 * w) < ref.N]
    out = [_case(f"a: key entry, window {w} digit {dg}",
                 ex.signature_for(0, dg << (4 * w), d, digest_add=ref.N * ((w + dg) & 1), R=tq[w][dg - 1]), True, d)
           for w, dg in entries]
    g_sigs = {(w, dg): ex.signature_for(dg << (4 * w), 1, d, R=ref.add(tg[w][dg - 1], q)) for w, dg in entries}
    out += [_case(f"a: G entry, window {w} digit {dg}", g_sigs[w, dg], True, d) for w, dg in entries]
    for w in range(ex.WINDOWS):
        dg = 1 + w % 14
        if (w, dg + 1) not in g_sigs:
            dg = 1
        this, nxt = g_sigs[w, dg], g_sigs[w, dg + 1]
        out.append(_case(f"a: G entry, window {w} digit {dg}, under the digest of digit {dg + 1}", (this[0], nxt[1], this[2]), False, d))
        out.append(_case(f"a: key entry, window {w} digit {dg + 1}, claiming the r of digit {dg}",
                         ex.signature_for(0, (dg + 1) << (4 * w), d, r=tq[w][dg - 1][0] % ref.N), False, d))
    return out


@functools.lru_cache(None)
def family_b():
    """Exceptional additions inside a lane.  Lane l adds G windows l, l + 16, l + 32, l + 48, then key windows l, l + 16,
    l + 32, l + 48; two G entries never meet, so the places are the key positions j = 0..3.  Under 16^(16 j) Q = c G,
    u1 = c 16^l and u2 = 16^(l + 16 j) make the key entry equal the accumulator (doubling, R = 2 c 16^l G); under -Q it
    opposes it (infinity; the signature claims the doubling's r, so a verifier that doubled there would accept).
    c = 5: the accumulator is one entry, Z = 1; c = 5 + 3 16^16: two entries, Z != 1.  Then, for j < 3: the lane
    cancels at position j and adds a further key entry -- the accumulator restarts from an affine point."""
    out = []
    for j in range(4):
        for c, what in ((5, "one-entry"), (5 + 3 * 16**16, "two-entry")):
            d = c * pow(16, -16 * j, ref.N) % ref.N
            for lane in (0, 7, 15):
                u1, u2 = c << (4 * lane), 1 << (4 * (lane + 16 * j))
                assert (u1 + u2 * d) % ref.N == 2 * u1 and (u1 - u2 * d) % ref.N == 0
                tag = f"b: lane {lane}, key position {j}, {what} accumulator"
                equal = ex.signature_for(u1, u2, d)
                out.append(_case(f"{tag}: equal", equal, True, d))
                out.append(_case(f"{tag}: opposite", ex.signature_for(u1, u2, ref.N - d, r=_r_of(equal)), False, ref.N - d))
                if j < 3:
                    more = u2 + (2 << (4 * (lane + 16 * (j + 1))))
                    out.append(_case(f"{tag}: opposite, then a further key entry", ex.signature_for(u1, more, ref.N - d), True, ref.N - d))
    return out


@functools.lru_cache(None)
def family_c():
    """Exceptional operands at every slot of the tree: step s = 8, 4, 2, 1 adds slot l + s into slot l < s, and before
    step s slot m holds the lanes congruent to m modulo 2 s.  Under 16^s Q = 5 G (one key per step, and its negative)
    lane l's G entries and lane l + s's key entries have equal sums, every other lane idle: one-entry sums (Z = 1)
    5 16^l G = 16^(l + s) Q, two-entry sums (5 + 15 16^16) 16^l G = (1 + 3 16^16) 16^(l + s) Q."""
    out = []
    for s in (8, 4, 2, 1):
        d = 5 * pow(16, -s, ref.N) % ref.N
        for slot in range(s):
            for g_digits, k_digits, what in ((5, 1, "one-entry"), (5 + (15 << 64), 1 + (3 << 64), "two-entry")):
                left, right = g_digits << (4 * slot), k_digits << (4 * (slot + s))
                assert (left - right * d) % ref.N == 0
                tag = f"c: step {s} slot {slot}, {what} sums"
                two = what == "two-entry"

                def lone(lane):   # (u1, u2) of a sum that sits in this lane alone: a key entry, or a G and a key entry
                    return (5 << (4 * lane) if two else 0), (3 if two else 1) << (4 * lane)
                equal = ex.signature_for(left, right, d)
                out.append(_case(f"{tag}: equal", equal, True, d))
                out.append(_case(f"{tag}: opposite", ex.signature_for(left, right, ref.N - d, r=_r_of(equal)), False, ref.N - d))
                out.append(_case(f"{tag}: left idle", ex.signature_for(*lone(slot + s), d), True, d))
                out.append(_case(f"{tag}: right idle", ex.signature_for(*lone(slot), d), True, d))
                if s > 1:   # (at step 1 every lane has been folded into slots 0 and 1: no third party is left)
                    # the infinity of slot `slot` meets lane m's sum at step s / 2, from the left or from the right
                    m = slot + s // 2 if slot < s // 2 else slot - s // 2
                    out.append(_case(f"{tag}: opposite, lane {m} finite", ex.signature_for(left + (7 << (4 * m)), right, ref.N - d),
                                     True, ref.N - d))
                    m = (slot + s + 1) % 16
                    assert m % s != slot % s
                    out.append(_case(f"{tag}: both idle, lane {m} finite", ex.signature_for(*lone(m), d), True, d))
    return out


@functools.lru_cache(None)
def family_d():
    """The compare x(R) mod n == r in a whole verification, R chosen by its abscissa (p - n is a 127-bit number)."""
    rng = random.Random(8)
    gap = ref.P - ref.N
    out = []

    def at(tag, lo, step, variants):
        x, R = ex.find_x(lo, step)
        u1, u2 = rng.randrange(1, ref.N), rng.randrange(1, ref.N)
        for name, r, want in variants(x):
            out.append(_case(f"d: x(R) {tag}: {name}", ex.signature_for_point(u1, u2, R, r=r), want))
        return x
    x = at("the first at or above n", ref.N, 1, lambda x: (("r = x - n", x - ref.N, True), ("r = x - n + 1", x - ref.N + 1, False)))
    assert ref.N <= x < ref.P
    x = at("the last below p", ref.P - 1, -1, lambda x: (("r = x - n", x - ref.N, True), ("r = x - n - 1", x - ref.N - 1, False)))
    assert ref.N <= x < ref.P
    x = at("the first at or above 1", 1, 1, lambda x: (("r = x", x, True), ("r = x + n", x + ref.N, False)))
    assert x < gap
    x = at("the last below p - n", gap - 1, -1, lambda x: (("r = x", x, True), ("r = x + 1", x + 1, False)))
    assert x < gap
    x = at("the first at or above p - n", gap, 1, lambda x: (("r = x", x, True), ("r = x - (p - n)", x - gap, False)))
    assert gap <= x < ref.N
    x = at("the last at or below n - 1", ref.N - 1, -1, lambda x: (("r = x", x, True), ("r = x - 1", x - 1, False)))
    assert gap <= x < ref.N
    return out


@functools.lru_cache(None)
def family_e():
    """Scalar edges: u1 = u2 = n - 1 (every digit but a few is 15), s = 1 and s = n - 1, the digests n - 1 and n + 1, u2
    with its top window alone beside a full u1."""
    rng = random.Random(9)
    d = rng.randrange(1, ref.N)
    top = ex.signature_for(ref.N - 1, ref.N - 1, d)
    out = [_case("e: u1 = u2 = n - 1", top, True, d),
           _case("e: u1 = u2 = n - 1, claiming r + 1", ex.signature_for(ref.N - 1, ref.N - 1, d, r=_r_of(top) + 1), False, d)]
    for s in (1, ref.N - 1):
        k = rng.randrange(1, ref.N)
        R = ex.mul_g(k)
        u2 = R[0] % ref.N * pow(s, -1, ref.N) % ref.N
        sig = ex.signature_for((k - u2 * d) % ref.N, u2, d, R=R)
        assert int.from_bytes(sig[2][32:], "big") == s
        out.append(_case("e: s = 1" if s == 1 else "e: s = n - 1", sig, True, d))
    for e in (ref.N - 1, ref.N + 1):
        r, s = ref.sign(d, rng.randrange(1, 2**40), e)
        sig = ref.be(r) + ref.be(s)
        name = "n - 1" if e < ref.N else "n + 1"
        out.append(_case(f"e: digest {name}", (ref.point_bytes(ex.key_point(d)), ref.be(e), sig), True, d))
        out.append(_case(f"e: the signature of digest {name} under digest n", (ref.point_bytes(ex.key_point(d)), ref.be(ref.N), sig), False, d))
    u1 = rng.randrange(1, ref.N)
    digits = [dg for dg in range(1, 16) if dg << 252 < ref.N]
    sigs = {dg: ex.signature_for(u1, dg << 252, d) for dg in digits}
    out += [_case(f"e: u2 = {dg} 16^63 beside a full u1", sigs[dg], True, d) for dg in digits]
    out.append(_case(f"e: u2 = {digits[-1]} 16^63 claiming the r of digit {digits[-2]}",
                     ex.signature_for(u1, digits[-1] << 252, d, r=_r_of(sigs[digits[-2]])), False, d))
    return out


EXPONENT_FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}


def exponent_cases(names="abcde"):
    return [c for n in names for c in EXPONENT_FAMILIES[n]()]


def exponent_batches(cases):
    """[(keys, [(name, digest, r | s, key index, expected)])]: the cases in order, cut where a 17th key would be needed
    (a verifier takes 16); after every fifth item a range-check reject of signature_cases() -- on the device a group of
    lanes that sums nothing but takes part in the shuffles -- and no batch's count a multiple of 4, so the last
    wavefront is partial."""
    dead = [(f"dead group, {c[0]}", c[1], c[2]) for c in signature_cases()[1] if c[0] in ("r = 0", "s = 0", "r = n", "s = n", "r = 2^256 - 1")]
    assert len(dead) == 5
    batches = []
    for n, (name, key, _, digest, sig, want) in enumerate(cases):
        if not batches or (key not in batches[-1][0] and len(batches[-1][0]) == 16):
            batches.append(([], []))
        keys, items = batches[-1]
        if key not in keys:
            keys.append(key)
        items.append((name, digest, sig, keys.index(key), want))
        if n % 5 == 4:
            items.append(dead[n // 5 % 5] + (len(keys) - 1, False))
    for keys, items in batches:
        if len(items) % 4 == 0:
            items.append(dead[0] + (0, False))
    return batches


def run_exponent_batches(amd, device, batches, rotations=(0,), against=None):
    """Every batch through a verifier on `device`, as it is and rotated left by each of `rotations` items (a wavefront
    holds four signatures: every item meets every group position): verdicts against the expectations, position by
    position, and against the route `against` (a device ordinal) where given."""
    for keys, items in batches:
        v = amd.Es256Verifier(keys, device=device)
        other = amd.Es256Verifier(keys, device=against) if against is not None else None
        try:
            for rot in rotations:
                it = items[rot:] + items[:rot]
                args = [c[1] for c in it], [c[2] for c in it], [c[3] for c in it]
                got = v.verify_batch(*args)
                wrong = [(c[0], g) for c, g in zip(it, got) if g != c[4]]
                assert not wrong, (f"rotation {rot}: {len(wrong)} of {len(it)} verdicts differ from the construction's", wrong[:12])
                if other is not None:
                    theirs = other.verify_batch(*args)
                    assert got == theirs, (rot, [c[0] for c, g, t in zip(it, got, theirs) if g != t][:12])
        finally:
            v.close()
            if other is not None:
                other.close()


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
