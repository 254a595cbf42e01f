"""Crafted circuits and passes for the pass-prove tests (g16_pass_inputs, g16_pass_fullprove_batch and its PLONK twin): a
witness program (wtns_prog_ref.py writes it) and its twin .r1cs (formats.py), so that keys can be set up from the .r1cs
and witnesses computed from the program; the passes come from pass_cases.make.  Nothing here calls the library.

    pack(M)   inputs  toBeSigned[8 M] (a bit a word, MSB first per byte), toBeSignedLen
              public  ceil(8 M / 248) words, word j = the input bits [248 j, 248 j + 248) as one big-endian integer (a
                      short last word holds the bits that are left), then the length
              check 0 "the last bit of the base pass is set": input bit K = 0, K = 8 * (the base pass's tbs_len - 1) + 7
A program's coefficients are int64, so 248 bits are packed in Horner steps of 62 bits: u1 = A0 * 2^62 + A1,
u2 = u1 * 2^62 + A2, word = u2 * 2^62 + A3, every A a linear form over 62 input bits; the R1CS rows are the same
products.  Every public word depends linearly on its bits alone, so the expected signals are computed from the
ToBeSigned bytes with Python integers.

    constant(n)   the same inputs, n public outputs that are the constant 7 whatever the input: what MATCH_PUBLIC must
                  refuse (n = 513)."""
import functools

import formats as f
import pass_cases as pc
import pass_ref
import wtns_prog_ref as ref

TEXT = "the last bit of the base pass is set"
M_MAIN, M_ODD = 320, 299
STEP, WORD = 62, 248


def base_pass(odd=False, **kw):
    """The base pass (cti chosen, so that the last byte of ToBeSigned is ours): its last bit clear, or set with odd=True
    -- the same length, and the circuit's check refuses it."""
    return pc.make(cti=bytes(15) + (b"\x0f" if odd else b"\x0e"), **kw)


@functools.lru_cache(None)
def tbs_of(uri):
    """ToBeSigned bytes of a well-formed pass, through pass_ref's reader"""
    cose = pass_ref.base32_decode(uri.strip().encode()[8:])
    head, pos = pass_ref.read_item_head(cose, 0)
    head, pos = pass_ref.read_item_head(cose, pos)
    parts = []
    for _ in range(4):
        it, pos = pass_ref.read_item(cose, pos, 0)
        parts.append(it)
    tbs = bytes([0x84, 0x6A]) + b"Signature1" + pass_ref.bstr(parts[0].data) + b"\x40" + pass_ref.bstr(parts[2].data)
    assert len(tbs) == pass_ref.front(uri, [])[0]["tbs_len"]
    return tbs


@functools.lru_cache(None)
def check_bit():
    return 8 * (len(tbs_of(base_pass())) - 1) + 7


def bits_of(tbs, m):
    return [(tbs[k >> 3] >> (7 - (k & 7))) & 1 if (k >> 3) < len(tbs) else 0 for k in range(8 * m)]


def input_words(tbs, m):
    """The image g16_nzcp_inputs writes, from Python integers"""
    return ref.words(bits_of(tbs, m) + [len(tbs)])


def n_words(m):
    return (8 * m + WORD - 1) // WORD


def public_values(tbs, m):
    """pack(m)'s public signals for a ToBeSigned of at most m bytes"""
    bits = bits_of(tbs, m)
    out = []
    for j in range(n_words(m)):
        v = 0
        for b in bits[WORD * j:WORD * (j + 1)]:
            v = v << 1 | b
        out.append(v)
    return out + [len(tbs)]


def violates(tbs, m):
    k = check_bit()
    return k < 8 * m and bits_of(tbs, m)[k] == 1


def _program(m, n_public, outputs_of):
    """The shared frame: wire 0 = 1, wires 1..n_public the outputs, then the 8 m + 1 inputs; outputs_of(next free wire,
    wire of input bit k, wire of the length) -> (ops, rows, next free wire)"""
    first_in = 1 + n_public
    bit = lambda k: first_in + k
    length = first_in + 8 * m
    ops = [("input", first_in + k, k) for k in range(8 * m + 1)]
    more, rows, n_wires = outputs_of(length + 1, bit, length)
    ops += more
    k = check_bit()
    checks = []
    if k < 8 * m:
        ops.append(("check", [(bit(k), 1)], 0))
        rows.append(([(bit(k), 1)], [(0, 1)], []))
        checks = [TEXT]
    return {"n_wires": n_wires, "n_public": n_public, "ops": ops, "checks": checks, "m": m,
            "prog": ref.write(n_wires, ops, checks, n_public=n_public,
                              inputs=[("toBeSigned", 0, 8 * m), ("toBeSignedLen", 8 * m, 1)], outputs=list(range(1, n_public + 1))),
            "r1cs": f.write_r1cs(n_wires, n_public, 0, rows)}


@functools.lru_cache(None)
def pack(m):
    """-> dict(name, m, n_wires, n_public, ops, checks, prog, r1cs)"""
    nw = n_words(m)

    def outputs_of(free, bit, length):
        ops, rows = [], []
        for j in range(nw):
            ks = list(range(WORD * j, min(WORD * (j + 1), 8 * m)))
            groups = [ks[g:g + STEP] for g in range(0, len(ks), STEP)]
            forms = [[(bit(k), 1 << (len(g) - 1 - i)) for i, k in enumerate(g)] for g in groups]
            acc = forms[0]   # (a linear form; a wire from the first Horner step on)
            for s in range(1, len(forms)):
                shift = 1 << len(groups[s])
                dst = 1 + j if s == len(forms) - 1 else free
                ops.append(("quad", dst, acc, [(0, shift)], forms[s]))
                rows.append((acc, [(0, shift)], [(dst, 1)] + [(w, ref.R - c) for w, c in forms[s]]))
                if dst == free:
                    free += 1
                acc = [(dst, 1)]
            if len(forms) == 1:
                ops.append(("quad", 1 + j, acc, [(0, 1)], []))
                rows.append((acc, [(0, 1)], [(1 + j, 1)]))
        ops.append(("quad", 1 + nw, [(length, 1)], [(0, 1)], []))
        rows.append(([(length, 1)], [(0, 1)], [(1 + nw, 1)]))
        return ops, rows, free
    c = _program(m, nw + 1, outputs_of)
    c["name"] = f"pack{m}"
    return c


@functools.lru_cache(None)
def constant(n_public, m=M_MAIN):
    """n_public outputs that are 7 whatever the pass; the inputs are read and ignored"""
    def outputs_of(free, bit, length):
        ops = [("quad", 1 + j, [(0, 7)], [(0, 1)], []) for j in range(n_public)]
        rows = [([(0, 7)], [(0, 1)], [(1 + j, 1)]) for j in range(n_public)]
        return ops, rows, free
    c = _program(m, n_public, outputs_of)
    c["name"] = f"constant{n_public}"
    return c


def public_bytes(tbs, m):
    return ref.words(public_values(tbs, m))


@functools.lru_cache(None)
def good_passes(count, m=M_MAIN):
    """`count` distinct valid passes of mixed lengths that pack(m) accepts (ToBeSigned at most m bytes, bit K clear): the
    base pass first (where it fits), then family names of growing length under both test keys; below the base pass's
    length the passes carry a "vc" of the credentialSubject alone"""
    small = m < len(tbs_of(base_pass()))
    out = [] if small else [base_pass()]
    n = 1
    while len(out) < count:
        subj = pc.subject(family=("Ngata-Sparrow" * 8)[:n])
        extra = {"vc_pairs": [(pc.text("credentialSubject"), subj)]} if small else {}
        uri = pc.make(kid=(pc.KID_A, pc.KID_B)[n & 1], subj=subj, cti=bytes(16), **extra)
        n += 1
        tbs = tbs_of(uri)
        if len(tbs) <= m and not violates(tbs, m):
            out.append(uri)
        assert n < 100
    return tuple(out)


def pass_with_tbs_len(want, **kw):
    """A valid pass whose ToBeSigned has exactly `want` bytes (the family name takes up the slack)"""
    for n in range(1, 400):
        uri = pc.make(subj=pc.subject(family="F" * n), cti=bytes(16), **kw)
        if len(tbs_of(uri)) == want:
            return uri
    raise AssertionError("no family name fits")
