"""The reference of the pass tests: the contract of include/g16_prover.h ("NZCP pass verification from URIs") restated in
plain Python -- base32, a minimal recursive CBOR reader, hashlib, p256_ref for the signature.  Records are dicts with the
fields of g16_pass_result."""
import hashlib

import p256_ref

URI_MAX = 2048
CBOR_DEPTH = 16
HAS_SUBJECT = 1
OK, MALFORMED, ALG, KEY, SIGNATURE, NOT_YET, EXPIRED, TOO_LONG = range(8)
B32 = "ABCDEFGHIJKLMNOPQRSTUVWXYZ234567"


class Malformed(Exception):
    pass


def base32_decode(text):
    """bytes of A-Z2-7 characters with optional trailing '=', or None"""
    body = text.rstrip(b"=")
    acc = nbits = 0
    out = bytearray()
    for ch in body:
        v = B32.find(chr(ch))
        if v < 0:
            return None
        acc = (acc << 5 | v) & 0xFFF
        nbits += 5
        if nbits >= 8:
            nbits -= 8
            out.append(acc >> nbits & 0xFF)
    return bytes(out)


def base32_encode(data):
    bits = "".join(f"{b:08b}" for b in data)
    bits += "0" * (-len(bits) % 5)
    return "".join(B32[int(bits[i:i + 5], 2)] for i in range(0, len(bits), 5))


class Item:
    """One CBOR item: major, arg, and for strings .data, arrays .items, maps .pairs (in order), tags .inner"""

    def __init__(self, major, arg):
        self.major, self.arg = major, arg
        self.data = self.items = self.pairs = self.inner = None

    def is_text(self, s=None):
        return self.major == 3 and (s is None or self.data == s.encode())

    def is_int(self):
        return self.major in (0, 1)

    def int_value(self):
        return self.arg if self.major == 0 else -1 - self.arg


def read_item(buf, pos, depth):
    """(Item, next position); depth = containers open around this item inside the item being skipped, or None where the
    item is one the walk reads itself (the cap does not count those)."""
    if pos >= len(buf):
        raise Malformed("truncated")
    major, info = buf[pos] >> 5, buf[pos] & 31
    pos += 1
    if major == 7 or info > 27:
        raise Malformed("major type 7 or info 28..31")
    arg = info
    if info >= 24:
        n = 1 << (info - 24)
        if pos + n > len(buf):
            raise Malformed("truncated head")
        arg = int.from_bytes(buf[pos:pos + n], "big")
        pos += n
    it = Item(major, arg)
    if major in (2, 3):
        if arg > len(buf) - pos:
            raise Malformed("truncated string")
        it.data = bytes(buf[pos:pos + arg])
        return it, pos + arg
    if major in (4, 5, 6):
        count = arg if major == 4 else 2 * arg if major == 5 else 1
        if count > len(buf) - pos:
            raise Malformed("more items than bytes")
        inner = None
        if depth is not None and count:
            inner = depth + 1
            if inner > CBOR_DEPTH:
                raise Malformed("nesting")
        kids = []
        for _ in range(count):
            kid, pos = read_item(buf, pos, inner)
            kids.append(kid)
        if major == 4:
            it.items = kids
        elif major == 5:
            it.pairs = list(zip(kids[0::2], kids[1::2]))
        else:
            it.inner = kids[0]
    return it, pos


def read_walked_map(buf, walked):
    """The map at the start of buf with its entries read as skipped items (the cap counts from each of them), except the
    values of the keys `walked` names -- {key predicate: reader of the value's bytes from its position}"""
    if not buf:
        raise Malformed("empty")
    head, body = read_item_head(buf, 0)
    if head.major != 5 or 2 * head.arg > len(buf) - body:
        raise Malformed("not a map")
    pos, pairs = body, []
    for _ in range(head.arg):
        key, pos = read_item(buf, pos, 0)
        reader = next((r for pred, r in walked if pred(key)), None)
        if pos < len(buf) and reader and buf[pos] >> 5 == 5:
            value, pos = reader(buf, pos)
        else:
            value, pos = read_item(buf, pos, 0)
        pairs.append((key, value))
    return pairs, pos


def read_item_head(buf, pos):
    if pos >= len(buf):
        raise Malformed("truncated")
    major, info = buf[pos] >> 5, buf[pos] & 31
    pos += 1
    if major == 7 or info > 27:
        raise Malformed("head")
    arg = info
    if info >= 24:
        n = 1 << (info - 24)
        if pos + n > len(buf):
            raise Malformed("truncated head")
        arg = int.from_bytes(buf[pos:pos + n], "big")
        pos += n
    return Item(major, arg), pos


def last(pairs, pred):
    """the value of the last pair whose key satisfies pred, or None (a later duplicate overrides)"""
    found = None
    for k, v in pairs:
        if pred(k):
            found = v
    return found


class WalkedMap(Item):
    def __init__(self, pairs):
        super().__init__(5, len(pairs))
        self.pairs = pairs


def _subject_reader(buf, pos):
    pairs, end = read_walked_map(buf[pos:], [])
    return WalkedMap(pairs), pos + end


def _vc_reader(buf, pos):
    pairs, end = read_walked_map(buf[pos:], [(lambda k: k.is_text("credentialSubject"), _subject_reader)])
    return WalkedMap(pairs), pos + end


def bstr(b):
    n = len(b)
    return (bytes([0x40 + n]) if n < 24 else bytes([0x58, n]) if n < 256 else bytes([0x59]) + n.to_bytes(2, "big")) + b


def blank(verdict):
    return {"verdict": verdict, "key_idx": 0, "tbs_len": 0, "flags": 0, "nbf": 0, "exp": 0,
            "tbs_sha256": bytes(32), "cred_subj_sha256": bytes(32)}


def front(uri, names):
    """(record with verdict 0 / 1 / 2 / 3 / 7, signature or None): everything before the signature check.  names: the
    "<iss>#<kid>" of the keys in order."""
    text = uri.encode("utf-8") if isinstance(uri, str) else bytes(uri)
    if len(text) > URI_MAX:
        return blank(TOO_LONG), None
    try:
        text = text.strip(b" \t\r\n")
        if not text.startswith(b"NZCP:/1/"):
            raise Malformed("prefix")
        if not text[8:].rstrip(b"="):
            raise Malformed("no base32 characters")
        cose = base32_decode(text[8:])
        if cose is None:
            raise Malformed("base32")
        head, pos = read_item_head(cose, 0)
        if head.major != 6 or head.arg != 18:
            raise Malformed("not tag 18")
        head, pos = read_item_head(cose, pos)
        if head.major != 4 or head.arg != 4:
            raise Malformed("not an array of 4")
        parts = []
        for _ in range(4):
            it, pos = read_item(cose, pos, 0)
            parts.append(it)
        protected, _, payload, sig = parts
        if protected.major != 2 or payload.major != 2 or sig.major != 2:
            raise Malformed("not byte strings")
        hdr, _ = read_walked_map(protected.data, [])
        claims, _ = read_walked_map(payload.data, [(lambda k: k.is_text("vc"), _vc_reader)])
        iss = last(claims, lambda k: k.major == 0 and k.arg == 1)
        exp = last(claims, lambda k: k.major == 0 and k.arg == 4)
        nbf = last(claims, lambda k: k.major == 0 and k.arg == 5)
        if iss is None or not iss.is_text():
            raise Malformed("iss")
        for v in (exp, nbf):
            if v is None or not v.is_int() or not -2**63 <= v.int_value() < 2**63:
                raise Malformed("exp / nbf")
        vc = last(claims, lambda k: k.is_text("vc"))
        if vc is None or vc.major != 5:
            raise Malformed("vc")
        subj = last(vc.pairs, lambda k: k.is_text("credentialSubject"))
        if subj is None or subj.major != 5:
            raise Malformed("credentialSubject")
        if len(sig.data) != 64:
            raise Malformed("signature length")
    except Malformed:
        return blank(MALFORMED), None
    rec = blank(OK)
    tbs = bytes([0x84, 0x6A]) + b"Signature1" + bstr(protected.data) + bstr(b"") + bstr(payload.data)
    rec.update(tbs_len=len(tbs), tbs_sha256=hashlib.sha256(tbs).digest(), nbf=nbf.int_value(), exp=exp.int_value())
    fields = [last(subj.pairs, lambda k, n=n: k.is_text(n)) for n in ("givenName", "familyName", "dob")]
    if all(f is not None and f.is_text() for f in fields):
        rec["flags"] = HAS_SUBJECT
        rec["cred_subj_sha256"] = hashlib.sha256(b",".join(f.data for f in fields)).digest()
    alg = last(hdr, lambda k: k.major == 0 and k.arg == 1)
    kid = last(hdr, lambda k: k.major == 0 and k.arg == 4)
    key = None
    if kid is not None and kid.major in (2, 3):
        name = iss.data + b"#" + kid.data
        key = next((j for j, n in enumerate(names) if n.encode("utf-8") == name), None)
    if alg is None or alg.major != 1 or alg.arg != 6:
        rec["verdict"] = ALG
    elif key is None:
        rec["verdict"] = KEY
    rec["key_idx"] = key or 0
    return rec, sig.data


def verify(uri, names, points, now):
    """the record of g16_pass_verify_batch: points[j] = the affine (x, y) of key j"""
    rec, sig = front(uri, names)
    if rec["verdict"] != OK:
        return rec
    ok = p256_ref.verify(points[rec["key_idx"]], int.from_bytes(rec["tbs_sha256"], "big"), int.from_bytes(sig[:32], "big"),
                         int.from_bytes(sig[32:], "big"))
    rec["verdict"] = SIGNATURE if not ok else NOT_YET if now < rec["nbf"] else EXPIRED if now >= rec["exp"] else OK
    return rec
