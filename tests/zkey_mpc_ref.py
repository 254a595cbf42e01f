"""Python twin of the phase-2 contribution pieces (csrc/zkey_mpc.cpp), written from their description and not from the
C++: the section-10 codec, the transcript and contribution hashes (hashlib.blake2b), ChaCha20 and the transcript's point
on G2 over oracle/bn254.py, the same-ratio check through the oracle's pairing, and contribute_ref, which builds the
header and section 10 a contribution must produce.  The G2 derivation restates ffjavascript's as far as that is possible
without the package; it is NOT cross-checked against snarkjs."""
import hashlib
import struct

import bn254 as b
import formats as f
from bn254 import Q, R, RQ

RQ_INV = pow(RQ, -1, Q)
HDR_DELTA1, HDR_DELTA2 = 468, 532          # offsets in section 2
REC_FIXED = 64 + 64 + 64 + 128 + 64 + 4 + 4


def blake2b(data):
    return hashlib.blake2b(data, digest_size=64).digest()


# ------------------------------------------------------------------ section 10
def parse_section10(s10):
    """-> (csHash, [record dict]); ValueError on a section shorter than its records say or with trailing bytes."""
    if len(s10) < 68:
        raise ValueError("zkey: Invalid File format")
    cs, n = s10[:64], struct.unpack_from("<I", s10, 64)[0]
    pos, recs = 68, []
    for _ in range(n):
        if len(s10) - pos < REC_FIXED:
            raise ValueError("zkey: Invalid File format")
        typ, plen = struct.unpack_from("<II", s10, pos + 384)
        if len(s10) - pos - REC_FIXED < plen:
            raise ValueError("zkey: Invalid File format")
        r = s10[pos:pos + REC_FIXED + plen]
        recs.append({"deltaAfter": r[:64], "g1_s": r[64:128], "g1_sx": r[128:192], "g2_spx": r[192:320],
                     "transcript": r[320:384], "type": typ, "params": r[392:], "raw": r})
        pos += REC_FIXED + plen
    if pos != len(s10):
        raise ValueError("zkey: Invalid File format")
    return cs, recs


def name_params(name):
    if not name:
        return b""
    cut = name[:64]
    while len(cut.encode("utf-8")) > 255:
        cut = cut[:-1]
    enc = cut.encode("utf-8")
    return bytes([1, len(enc)]) + enc


def write_record(delta_after, g1_s, g1_sx, g2_spx, transcript, name=None, typ=0):
    params = name_params(name)
    return delta_after + g1_s + g1_sx + g2_spx + transcript + struct.pack("<II", typ, len(params)) + params


# ------------------------------------------------------------------ hashing
def _be(x):
    return int(x).to_bytes(32, "big")


def g1_uncompressed(lem):
    P = f.g1_from_lem(lem)
    if P is None:
        return bytes([0x40]) + bytes(63)
    return _be(P[0]) + _be(P[1])


def g2_uncompressed(lem):
    P = f.g2_from_lem(lem)
    if P is None:
        return bytes([0x40]) + bytes(127)
    (x0, x1), (y0, y1) = P
    return _be(x1) + _be(x0) + _be(y1) + _be(y0)


def hash_pubkey_feed(rec):
    return (g1_uncompressed(rec["deltaAfter"]) + g1_uncompressed(rec["g1_s"]) + g1_uncompressed(rec["g1_sx"]) +
            g2_uncompressed(rec["g2_spx"]) + rec["transcript"])


def transcript_hash(cs_hash, earlier, g1_s, g1_sx):
    return blake2b(cs_hash + b"".join(hash_pubkey_feed(r) for r in earlier) + g1_uncompressed(g1_s) + g1_uncompressed(g1_sx))


def contribution_hash(rec):
    return blake2b(hash_pubkey_feed(rec))


# ------------------------------------------------------------------ ChaCha20 and the point on G2
class ChaCha:
    def __init__(self, key_words):
        self.key, self.counter, self.buf = list(key_words), 0, []

    def _block(self):
        M = 0xffffffff
        s = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574] + self.key + \
            [self.counter & M, (self.counter >> 32) & M, 0, 0]
        x = list(s)

        def rotl(v, n):
            return ((v << n) | (v >> (32 - n))) & M

        def qr(a, bb, c, d):
            x[a] = (x[a] + x[bb]) & M; x[d] = rotl(x[d] ^ x[a], 16)
            x[c] = (x[c] + x[d]) & M; x[bb] = rotl(x[bb] ^ x[c], 12)
            x[a] = (x[a] + x[bb]) & M; x[d] = rotl(x[d] ^ x[a], 8)
            x[c] = (x[c] + x[d]) & M; x[bb] = rotl(x[bb] ^ x[c], 7)
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        self.counter += 1
        self.buf = [(u + v) & M for u, v in zip(x, s)]

    def u32(self):
        if not self.buf:
            self._block()
        return self.buf.pop(0)

    def u64(self):
        hi = self.u32()
        return (hi << 32) + self.u32()

    def field(self, modulus):
        while True:
            v = sum(self.u64() << (64 * i) for i in range(4)) & ((1 << 254) - 1)
            if v < modulus:
                return v


def _fq_sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def f2_sqrt(a):
    a0, a1 = a
    if a1 == 0:
        r = _fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        r = _fq_sqrt(-a0 % Q)
        return None if r is None else (0, r)
    n = _fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if n is None:
        return None
    inv2 = pow(2, -1, Q)
    for cand in ((a0 + n) * inv2 % Q, (a0 - n) * inv2 % Q):
        x0 = _fq_sqrt(cand)
        if x0 is not None:
            root = (x0, a1 * pow(2 * x0, -1, Q) % Q)
            return root if b.f2_sqr(root) == (a0 % Q, a1 % Q) else None
    return None


def f2_negative(a):
    v = a[1] if a[1] != 0 else a[0]
    return v > (Q - 1) // 2


def hash_to_g2_trace(transcript):
    """-> (point, number of x draws): the x draws beyond the first are the rejected ones."""
    rng = ChaCha(struct.unpack(">8I", transcript[:32]))
    draws = 0
    while True:
        c0 = rng.field(Q) * RQ_INV % Q        # the drawn value is the Montgomery image
        c1 = rng.field(Q) * RQ_INV % Q
        greatest = rng.u32() & 1
        draws += 1
        x = (c0, c1)
        y = f2_sqrt(b.f2_add(b.f2_mul(b.f2_sqr(x), x), b.G2_B))
        if y is None:
            continue
        if f2_negative(y) != bool(greatest):
            y = b.f2_neg(y)
        break
    # (Curve.mul reduces its scalar mod r: the cofactor goes through jmul)
    return b.G2.to_affine(b.G2.jmul((x, y), 2 * Q - R)), draws


def hash_to_g2(transcript):
    return hash_to_g2_trace(transcript)[0]


# ------------------------------------------------------------------ checks
def same_ratio(g1a, g1b, g2c, g2d):
    """e(a, d) = e(b, c); infinity operands are refused."""
    if None in (g1a, g1b, g2c, g2d):
        return False
    return b.pairing_product_is_one([(g1a, g2d), (b.G1.neg(g1b), g2c)])


def verify_chain(init_zkey, zkey):
    """The record walk of the verifier (header delta included), sections 8 / 9 left out."""
    def parts(buf):
        secs = f.read_binfile(buf, "zkey", 2)
        return f.section(buf, secs, 2), parse_section10(f.section(buf, secs, 10))
    h0, (cs0, recs0) = parts(init_zkey)
    h1, (cs1, recs1) = parts(zkey)
    if cs0 != cs1 or [r["raw"] for r in recs1[:len(recs0)]] != [r["raw"] for r in recs0]:
        return False
    cur = f.g1_from_lem(h0[HDR_DELTA1:HDR_DELTA1 + 64])
    for i in range(len(recs0), len(recs1)):
        r = recs1[i]
        if transcript_hash(cs1, recs1[:i], r["g1_s"], r["g1_sx"]) != r["transcript"]:
            return False
        sp = hash_to_g2(r["transcript"])
        spx = f.g2_from_lem(r["g2_spx"])
        after = f.g1_from_lem(r["deltaAfter"])
        if not same_ratio(f.g1_from_lem(r["g1_s"]), f.g1_from_lem(r["g1_sx"]), sp, spx):
            return False
        if not same_ratio(cur, after, sp, spx):
            return False
        cur = after
    if cur != f.g1_from_lem(h1[HDR_DELTA1:HDR_DELTA1 + 64]):
        return False
    return same_ratio(f.g1_from_lem(h0[HDR_DELTA1:HDR_DELTA1 + 64]), cur,
                      f.g2_from_lem(h0[HDR_DELTA2:HDR_DELTA2 + 128]), f.g2_from_lem(h1[HDR_DELTA2:HDR_DELTA2 + 128]))


# ------------------------------------------------------------------ the contribution
def contribute_ref(zkey_bytes, name, d, s):
    """-> (section 2, section 10, contribution hash) of the key `zkey contribute` must write for secrets d, s."""
    secs = f.read_binfile(zkey_bytes, "zkey", 2)
    h = f.section(zkey_bytes, secs, 2)
    s10 = f.section(zkey_bytes, secs, 10)
    cs, recs = parse_section10(s10)
    g1_s = b.G1.mul(b.G1_GEN, s)
    g1_sx = b.G1.mul(g1_s, d)
    g1_s_b, g1_sx_b = f.g1_to_lem(g1_s), f.g1_to_lem(g1_sx)
    tr = transcript_hash(cs, recs, g1_s_b, g1_sx_b)
    g2_spx = b.G2.mul(hash_to_g2(tr), d)
    delta1 = b.G1.mul(f.g1_from_lem(h[HDR_DELTA1:HDR_DELTA1 + 64]), d)
    delta2 = b.G2.mul(f.g2_from_lem(h[HDR_DELTA2:HDR_DELTA2 + 128]), d)
    rec = write_record(f.g1_to_lem(delta1), g1_s_b, g1_sx_b, f.g2_to_lem(g2_spx), tr, name)
    new_h = h[:HDR_DELTA1] + f.g1_to_lem(delta1) + f.g2_to_lem(delta2) + h[HDR_DELTA2 + 128:]
    new_s10 = cs + struct.pack("<I", len(recs) + 1) + s10[68:] + rec
    _, new_recs = parse_section10(new_s10)
    return new_h, new_s10, contribution_hash(new_recs[-1])
