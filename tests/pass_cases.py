"""Case builders shared by test_cpu_pass.py (device -1), test_gpu_pass.py (device 0) and test_node_pass.py: a Python port
of js/nzcpInput.js::syntheticPass that signs with p256_ref under two test keys, the edge cases of the contract in
include/g16_prover.h, and a seeded corpus; every expectation is pass_ref's record (asserted here, on the CPU), each
built once per session."""
import base64
import functools
import hashlib
import json
import os
import random

import p256_ref as ref
import pass_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOW = 1700000000
NBF, EXP = 1635883530, 1951416330
D_A = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE
D_B = 0x1F2E3D4C5B6A79881726354453627180A1B2C3D4E5F60718293A4B5C6D7E8F90
ISS_LIVE = "did:web:nzcp.identity.health.nz"
KID_A, KID_B = "z12Kf7UQ", "key-b"
KID_23, KID_24 = "k" * 23, "K" * 24


def _b64u(b):
    return base64.urlsafe_b64encode(b).decode().rstrip("=")


def _jwk(pt):
    return {"kty": "EC", "crv": "P-256", "x": _b64u(ref.be(pt[0])), "y": _b64u(ref.be(pt[1]))}


@functools.lru_cache(None)
def example_uri():
    return open(os.path.join(GOLDEN, "example_pass_uri.txt")).read().strip()


@functools.lru_cache(None)
def key_set():
    """(keys object {"<iss>#<kid>": jwk} in order, names, affine points, private keys or None): the specification's
    example issuer, then test keys A and B, then A again under a 23- and a 24-byte kid"""
    doc = json.load(open(os.path.join(GOLDEN, "nzcp_example_issuer.json")))
    keys = dict(doc["keys"])
    qa, qb = ref.mul(D_A, ref.G), ref.mul(D_B, ref.G)
    keys[f"{ISS_LIVE}#{KID_A}"] = _jwk(qa)
    keys[f"{ISS_LIVE}#{KID_B}"] = _jwk(qb)
    keys[f"{ISS_LIVE}#{KID_23}"] = _jwk(qa)
    keys[f"{ISS_LIVE}#{KID_24}"] = _jwk(qa)
    names = list(keys)

    def point(j):
        d = lambda v: int.from_bytes(base64.urlsafe_b64decode(v + "=" * (-len(v) % 4)), "big")
        return (d(j["x"]), d(j["y"]))
    return keys, names, [point(keys[n]) for n in names], {KID_A: D_A, KID_B: D_B, KID_23: D_A, KID_24: D_A}


@functools.lru_cache(None)
def expected(uri, now=NOW):
    """pass_ref's record of the pass under key_set() (shared: do not change it)"""
    _, names, points, _ = key_set()
    return pass_ref.verify(uri, names, points, now)


# ------------------------------------------------------------------ CBOR writers
def head(major, n):
    if n < 24:
        return bytes([major << 5 | n])
    if n < 256:
        return bytes([major << 5 | 24, n])
    if n < 65536:
        return bytes([major << 5 | 25]) + n.to_bytes(2, "big")
    return bytes([major << 5 | 26]) + n.to_bytes(4, "big")


def text(s):
    b = s.encode("utf-8") if isinstance(s, str) else s
    return head(3, len(b)) + b


def bstr(b):
    return head(2, len(b)) + b


def u32(v):
    return b"\x1a" + v.to_bytes(4, "big")


def cmap(pairs):
    return head(5, len(pairs)) + b"".join(k + v for k, v in pairs)


def nested(depth):
    """`depth` arrays of one element around the integer 0"""
    return head(4, 1) * depth + b"\x00"


# ------------------------------------------------------------------ the synthetic pass
def protected_header(kid=KID_A, alg=b"\x26", kid_text=False, pairs=None):
    if pairs is None:
        k = kid.encode() if isinstance(kid, str) else kid
        pairs = [(b"\x04", text(k) if kid_text else bstr(k)), (b"\x01", alg)]
    return cmap(pairs)


def subject(given="Jack", family="Sparrow", dob="1960-04-16"):
    pairs = []
    if given is not None:
        pairs.append((text("givenName"), text(given)))
    pairs += [(text("familyName"), text(family)), (text("dob"), text(dob))]
    return cmap(pairs)


def payload_claims(iss=ISS_LIVE, nbf=NBF, exp=EXP, subj=None, iss_item=None, exp_item=None, nbf_item=None, vc_pairs=None, cti=None):
    subj = subject() if subj is None else subj
    if vc_pairs is None:
        vc_pairs = [(text("@context"), head(4, 2) + text("https://www.w3.org/2018/credentials/v1") + text("https://nzcp.covid19.health.nz/contexts/v1")),
                    (text("version"), text("1.0.0")),
                    (text("type"), head(4, 2) + text("VerifiableCredential") + text("PublicCovidPass")),
                    (text("credentialSubject"), subj)]
    cti = hashlib.sha256(subj).digest()[:16] if cti is None else cti
    return cmap([(b"\x01", iss_item or text(iss)), (b"\x05", nbf_item or u32(nbf)), (b"\x04", exp_item or u32(exp)),
                 (text("vc"), cmap(vc_pairs)), (b"\x07", bstr(cti))])


def to_be_signed(protected, payload):
    return bytes([0x84, 0x6A]) + b"Signature1" + pass_ref.bstr(protected) + b"\x40" + pass_ref.bstr(payload)


def sign(d, protected, payload):
    tbs = to_be_signed(protected, payload)
    nonce = int.from_bytes(hashlib.sha256(b"nonce" + tbs).digest()[:5], "big") + 1   # (a short nonce keeps the reference quick)
    r, s = ref.sign(d, nonce, int.from_bytes(hashlib.sha256(tbs).digest(), "big"))
    return ref.be(r) + ref.be(s)


def uri_of(cose):
    return "NZCP:/1/" + pass_ref.base32_encode(cose)


def make(kid=KID_A, d=None, protected=None, payload=None, unprotected=b"\xa0", tag=b"\xd2", sig=None, sig_item=None, cose_only=False, **claims):
    """A pass URI: the protected header of `kid`, the claims of payload_claims(**claims), signed by the private key `d`
    (default: the key of `kid`), or with the given signature bytes / signature item"""
    protected = protected_header(kid) if protected is None else protected
    payload = payload_claims(**claims) if payload is None else payload
    if sig is None:
        sig = sign(key_set()[3].get(kid, D_A) if d is None else d, protected, payload)
    cose = tag + head(4, 4) + bstr(protected) + unprotected + bstr(payload) + (sig_item or bstr(sig))
    return cose if cose_only else uri_of(cose)


def _family_for(pred, **kw):
    """the shortest familyName for which pred(protected, payload) holds"""
    for n in range(1, 200):
        family = ("Sparrow" * 30)[:n]
        protected, payload = protected_header(kw.get("kid", KID_A)), payload_claims(subj=subject(family=family))
        if pred(protected, payload):
            return family
    raise AssertionError("no familyName length fits")


def spoil_sig(uri):
    """the same pass with one bit of s flipped"""
    cose = bytearray(pass_ref.base32_decode(uri[8:].encode()))
    cose[-3] ^= 0x10
    return uri_of(bytes(cose))


# ------------------------------------------------------------------ the edge cases: (name, uri, expected verdict at NOW)
@functools.lru_cache(None)
def padding_cases():
    """ToBeSigned lengths 55, 56, 63, 0, 1 mod 64 and credSubj strings of 55, 56, 63, 64 bytes: all valid passes"""
    out = []
    for res in (55, 56, 63, 0, 1):
        family = _family_for(lambda p, q: len(to_be_signed(p, q)) % 64 == res)
        out.append((f"tbs {res} mod 64", make(subj=subject(family=family)), 0))
    for n in (55, 56, 63, 64):
        family = "F" * (n - len("Jack,") - len(",1960-04-16"))
        out.append((f"credSubj {n} bytes", make(subj=subject(family=family)), 0))
    return out


@functools.lru_cache(None)
def cbor_cases():
    out = []
    for n in (255, 256):   # the 58 / 59 head of the payload in ToBeSigned
        for k in range(1, 200):
            vc_pairs = [(text("credentialSubject"), subject(family="S" * k))]
            if len(payload_claims(vc_pairs=vc_pairs, cti=bytes(4))) == n:
                break
        out.append((f"payload {n} bytes", make(vc_pairs=vc_pairs, cti=bytes(4)), 0))
    out.append(("kid 23 bytes", make(kid=KID_23), 0))
    out.append(("kid 24 bytes", make(kid=KID_24), 0))
    out.append(("kid as text", make(protected=protected_header(KID_A, kid_text=True)), 0))
    out.append(("tag d8 12", make(tag=b"\xd8\x12"), 0))
    out.append(("nesting 16", make(unprotected=cmap([(b"\x00", nested(15))])), 0))
    out.append(("nesting 17", make(unprotected=cmap([(b"\x00", nested(16))])), 1))
    out.append(("indefinite length", make(unprotected=b"\xbf\xff"), 1))
    out.append(("indefinite byte string", make(unprotected=b"\x5f\x41\x00\xff"), 1))
    out.append(("float", make(unprotected=cmap([(b"\x01", b"\xf9\x3c\x00")])), 1))
    sig = bytes(range(64))
    out.append(("length one past the end", make(sig_item=b"\x58\x41" + sig), 1))
    out.append(("signature 63 bytes", make(sig=sig[:63]), 1))
    out.append(("signature 65 bytes", make(sig=sig + b"\x00"), 1))
    kid = bstr(KID_A.encode())
    out.append(("duplicate alg, ES256 last", make(protected=cmap([(b"\x01", b"\x27"), (b"\x04", kid), (b"\x01", b"\x26")])), 0))
    out.append(("duplicate alg, ES256 first", make(protected=cmap([(b"\x01", b"\x26"), (b"\x04", kid), (b"\x01", b"\x27")])), 2))
    out.append(("alg absent", make(protected=cmap([(b"\x04", kid)])), 2))
    out.append(("iss a byte string", make(iss_item=bstr(ISS_LIVE.encode())), 1))
    out.append(("exp a text string", make(exp_item=text("1951416330")), 1))
    out.append(("nbf above int64", make(nbf_item=b"\x1b" + (2**63).to_bytes(8, "big")), 1))
    out.append(("exp 8 bytes wide", make(exp_item=b"\x1b" + EXP.to_bytes(8, "big")), 0))
    out.append(("no credentialSubject", make(vc_pairs=[(text("version"), text("1.0.0"))]), 1))
    out.append(("vc an array", make(payload=cmap([(b"\x01", text(ISS_LIVE)), (b"\x05", u32(NBF)), (b"\x04", u32(EXP)), (text("vc"), head(4, 0))])), 1))
    out.append(("givenName missing", make(subj=subject(given=None)), 0))
    out.append(("bytes after the first item", uri_of(make(cose_only=True) + b"\xff\xff\xff"), 0))
    out.append(("surrounding space", " \t" + make() + "\r\n", 0))
    out.append(("version 2", make().replace("NZCP:/1/", "NZCP:/2/"), 1))
    out.append(("padding kept", make() + "==", 0))
    out.append(("nothing but padding", "NZCP:/1/====", 1))
    out.append(("empty", "", 1))
    return out


@functools.lru_cache(None)
def precedence_cases():
    """(name, uri, now, expected verdict)"""
    valid = make()
    wrong_alg = protected_header("nobody", alg=b"\x27")
    out = [("wrong alg, unknown key", make(protected=wrong_alg, d=D_A), NOW, 2),
           ("unknown key, bad signature", make(kid="nobody", sig=bytes(range(1, 65))), NOW, 3),
           ("bad signature, expired", spoil_sig(make(exp=NOW - 5)), NOW, 4),
           ("expired", make(exp=NOW - 5), NOW, 6),
           ("nbf - 1", valid, NBF - 1, 5), ("nbf", valid, NBF, 0), ("exp - 1", valid, EXP - 1, 0), ("exp", valid, EXP, 6)]
    return out


@functools.lru_cache(None)
def cap_cases():
    """URI text of exactly 2048 bytes (valid) and of 2049 (too long): padding inside item 1"""
    want = (pass_ref.URI_MAX - 8) * 5 // 8   # decoded bytes of 2040 characters
    n = 700
    n += want - len(make(unprotected=cmap([(b"\x01", bstr(bytes(n)))]), cose_only=True))
    uri = make(unprotected=cmap([(b"\x01", bstr(bytes(n)))]))
    assert len(uri) == pass_ref.URI_MAX
    return [("2048 bytes", uri, 0), ("2049 bytes", uri + "=", 7)]


def check_expectations(cases):
    """every stated verdict is the reference's"""
    for c in cases:
        name, uri, now, want = (c[0], c[1], NOW, c[2]) if len(c) == 3 else c
        assert expected(uri, now)["verdict"] == want, (name, expected(uri, now)["verdict"], want)


# ------------------------------------------------------------------ the corpus
@functools.lru_cache(None)
def corpus():
    """(uris, pass_ref's records at NOW): 140 seeded passes over three keys; at least half reach verdict 0 and every
    verdict occurs at least twice (asserted).  Everything in it but the verdict-7 items is in the domain on which the
    one-pass JS reader and the contract agree."""
    rng = random.Random(20240607)
    names = ["Jack", "Aroha", "Wiremu", "Mere", "Oliver", "Charlotte-Anne", "Te Rangi"]
    families = ["Sparrow", "Ngata", "Smith", "O'Connor", "Van der Merwe", "Li"]
    uris = [example_uri()]
    while len(uris) < 140:
        kid = rng.choice((KID_A, KID_B))
        subj = subject(rng.choice(names), rng.choice(families), f"{rng.randrange(1930, 2015)}-{rng.randrange(1, 13):02d}-{rng.randrange(1, 29):02d}")
        kind = rng.random()
        if kind < 0.58:
            uri = make(kid=kid, subj=subj)
        elif kind < 0.64:
            uri = spoil_sig(make(kid=kid, subj=subj))
        elif kind < 0.70:
            uri = make(kid=kid, subj=subj, nbf=NOW + rng.randrange(1, 10**6))
        elif kind < 0.76:
            uri = make(kid=kid, subj=subj, exp=NOW - rng.randrange(0, 10**6))
        elif kind < 0.81:
            uri = make(kid="retired", subj=subj, d=D_B)
        elif kind < 0.86:
            uri = make(protected=protected_header(kid, alg=b"\x38\x22"), subj=subj, d=D_A)
        elif kind < 0.90:
            uri = make(kid=kid, subj=subj, unprotected=cmap([(b"\x01", bstr(bytes(1100)))]))   # above 2048 characters
        else:
            cose = make(kid=kid, subj=subj, cose_only=True)
            how = rng.randrange(4)
            if how == 0:
                uri = uri_of(cose[:rng.randrange(1, len(cose))])
            elif how == 1:
                spot = rng.randrange(0, 24)
                uri = uri_of(cose[:spot] + b"\xff" + cose[spot + 1:])
            elif how == 2:
                uri = uri_of(cose)
                spot = rng.randrange(8, len(uri) - 1)
                uri = uri[:spot] + rng.choice("=a189") + uri[spot + 1:]
            else:
                uri = uri_of(cose).replace("NZCP:/1/", rng.choice(("NZCP:/2/", "nzcp:/1/", "NZCP:/1")))
        uris.append(uri)
    records = [expected(u) for u in uris]
    verdicts = [r["verdict"] for r in records]
    assert 2 * verdicts.count(0) >= len(uris), verdicts.count(0)
    assert all(verdicts.count(v) >= 2 for v in range(8)), [verdicts.count(v) for v in range(8)]
    assert len(set(verdicts[:64])) >= 5 and len({r["key_idx"] for r in records[:64]}) >= 3   # mixed inside one wavefront
    return uris, records


def run_batch(amd, device, uris, now=NOW):
    keys = key_set()[0]
    v = amd.PassVerifier(keys, device=device)
    try:
        return v.verify_batch(uris, now)
    finally:
        v.close()


def run_cases(amd, device, cases):
    """one batch per distinct `now`; every record equals the reference's"""
    check_expectations(cases)
    cases = [(c[0], c[1], NOW, c[2]) if len(c) == 3 else c for c in cases]
    for now in sorted({c[2] for c in cases}):
        group = [c for c in cases if c[2] == now]
        got = run_batch(amd, device, [c[1] for c in group], now)
        for c, g in zip(group, got):
            assert g == expected(c[1], now), (c[0], g, expected(c[1], now))


# ------------------------------------------------------------------ the checks both routes run
EXAMPLE_TBS_SHA256 = "271ce33d671a2d3b816d788135f4343e14bc66802f8cd841faac939e8c11f3ee"


def run_example(amd, device):
    """the specification's example pass: 600 characters -> 370 bytes -> ToBeSigned of 314 bytes"""
    uri = example_uri()
    assert len(uri) == 600
    assert len(amd.pass_op("base32", [uri[8:]], device=device)[0]) == 370
    (rec,) = run_batch(amd, device, [uri], NOW)
    assert rec["verdict"] == 0 and rec["key_idx"] == 0 and rec["tbs_len"] == 314 and rec["flags"] == amd.PASS_HAS_SUBJECT
    assert rec["tbs_sha256"].hex() == EXAMPLE_TBS_SHA256
    assert rec["cred_subj_sha256"] == hashlib.sha256(b"Jack,Sparrow,1960-04-16").digest()
    assert (rec["nbf"], rec["exp"]) == (1635883530, 1951416330)
    assert rec == expected(uri)


SHA_LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 128)


def run_sha256_edges(amd, device):
    msgs = [bytes((7 * i + n) & 0xFF for i in range(n)) for n in SHA_LENGTHS]
    assert amd.pass_op("sha256", msgs, device=device) == [hashlib.sha256(m).digest() for m in msgs]


def run_base32_tails(amd, device):
    rng = random.Random(7)
    plain = [bytes(rng.randrange(256) for _ in range(n)) for n in range(1, 11)]   # every residue mod 5, twice
    enc = [pass_ref.base32_encode(p) for p in plain]
    padded = [e + "=" * (-len(e) % 8) for e in enc]
    bad = [enc[6][:4] + "=" + enc[6][5:], enc[7][:3] + enc[7][3].lower() + enc[7][4:]] + [enc[9][:5] + c + enc[9][6:] for c in "0189"]
    bad += ["A" * (PASS_CHARS_MAX + 1)]
    items = enc + padded + bad + ["", "A" * PASS_CHARS_MAX]
    want = plain + plain + [None] * len(bad) + [b"", bytes(PASS_CHARS_MAX * 5 // 8)]
    assert [pass_ref.base32_decode(i.encode()) if len(i) <= PASS_CHARS_MAX else None for i in items] == want
    assert amd.pass_op("base32", items, device=device) == want


PASS_CHARS_MAX = pass_ref.URI_MAX


def run_front_op(amd, device):
    """op 2: the front end alone, no key table: the reference's record with no names"""
    uris = [c[1] for c in cbor_cases()] + [c[1] for c in cap_cases()]
    got = amd.pass_op("front", uris, device=device)
    want = [pass_ref.front(u, [])[0] for u in uris]
    assert got == want
    assert {r["verdict"] for r in got} == {1, 2, 3, 7}


GRID_TAILS = (1, 63, 64, 65, 130, 33)   # (33 after the largest: a smaller batch on scratch that has grown)


def run_grid_tails(amd, device):
    uris, records = corpus()
    amd.PassVerifier(key_set()[0], device=device).close()   # a handle that never ran a batch
    v = amd.PassVerifier(key_set()[0], device=device)
    try:
        for n in GRID_TAILS:
            assert v.verify_batch(uris[:n], NOW) == records[:n], n
        assert v.verify_batch([], NOW) == []
        assert len(v.timings()) == 3
    finally:
        v.close()


def run_corpus(amd, device):
    uris, records = corpus()
    got = run_batch(amd, device, uris, NOW)
    for i, (g, w) in enumerate(zip(got, records)):
        assert g == w, (i, uris[i][:60], g, w)


def run_errors(amd, device):
    import ctypes as C
    import pytest
    keys, names, _, _ = key_set()
    lib = amd.load()
    h = C.c_void_p()
    one = (C.c_char_p * 1)(b"did:web:x")
    packed = bytes(64)
    for args in ((None, one, one), (packed, None, one), (packed, one, None)):
        assert lib.g16_pass_verifier_create(args[0], args[1], args[2], 1, device, C.byref(h)) == -1
        assert b"NULL argument" in lib.g16_last_error()
    assert lib.g16_pass_verifier_create(packed, one, one, 1, device, None) == -1
    many = {f"did:web:x#{i}": keys[names[1]] for i in range(17)}
    with pytest.raises(amd.G16Error) as e:
        amd.PassVerifier(many, device=device)
    assert e.value.code == -1 and "1 to 16 keys" in str(e.value)
    off = dict(keys[names[1]])
    off["y"] = _b64u(ref.be(ref.mul(D_A, ref.G)[1] ^ 1))
    with pytest.raises(amd.G16Error) as e:
        amd.PassVerifier({names[0]: keys[names[0]], names[1]: off}, device=device)
    assert e.value.code == -2 and "key 1 is not on the curve" in str(e.value)
    with pytest.raises(amd.G16Error) as e:
        amd.PassVerifier({"did:web:x#" + "k" * 129: keys[names[1]]}, device=device)
    assert e.value.code == -1 and "kid must be 1 to 128 bytes" in str(e.value)
    v = amd.PassVerifier(keys, device=device)
    try:
        out = (amd.PassResult * 1)()
        offsets = (C.c_uint64 * 2)(0, 4)
        assert lib.g16_pass_verify_batch(None, b"NZCP", offsets, 1, NOW, out) == -1
        assert lib.g16_pass_verify_batch(v._h, None, offsets, 1, NOW, out) == -1
        assert lib.g16_pass_verify_batch(v._h, b"NZCP", None, 1, NOW, out) == -1
        assert lib.g16_pass_verify_batch(v._h, b"NZCP", offsets, 1, NOW, None) == -1
        assert b"NULL argument" in lib.g16_last_error()
        assert lib.g16_pass_verify_batch(v._h, None, None, 0, NOW, None) == 0   # count = 0 is accepted
        offsets = (C.c_uint64 * 2)(4, 0)
        assert lib.g16_pass_verify_batch(v._h, b"NZCP", offsets, 1, NOW, out) == -1
        assert b"offsets do not ascend" in lib.g16_last_error()
    finally:
        v.close()
    with pytest.raises(amd.G16Error) as e:
        amd.pass_op(3, ["A"], device=device)
    assert "unknown op" in str(e.value)
    assert amd.pass_op("sha256", [], device=device) == []
