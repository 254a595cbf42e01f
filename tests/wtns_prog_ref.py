"""Reference for the witness calculator (csrc/witness_program.h): a writer and a reader of the program format and a
big-integer evaluator over oracle/bn254.R -- the oracle for crafted programs, in the role wtns_check_ref.py plays for the
checker.  Nothing here calls the library.

A program is described by a list of ops IN ANY ORDER; write() computes the levels (1 + the highest level read), sorts by
(level, kind) and lays the sections out as the C++ recorder does.  Ops (forms are lists of (wire, coefficient)):
    ("input", wire, j)          ("quad", wire, a, b, c)        ("bits", [wires], a, check or None)
    ("inv0", wire, a)           ("isz", wire, a)               ("check", a, k)
checks = the list of texts, one per check index."""
import struct

import bn254

R = bn254.R
NO_CHECK = 0xFFFFFFFF
INPUT, QUAD, BITS, INV0, ISZ, CHECK = range(6)
KIND = {"input": INPUT, "quad": QUAD, "bits": BITS, "inv0": INV0, "isz": ISZ, "check": CHECK}


def _forms(op):
    k = op[0]
    if k == "input":
        return [], [], []
    if k == "quad":
        return op[2], op[3], op[4]
    if k == "bits":
        return op[2], [], []
    if k == "check":
        return op[1], [], []
    return op[2], [], []


def _defs(op):
    k = op[0]
    if k == "check":
        return []
    return list(op[1]) if k == "bits" else [op[1]]


def levels_of(ops):
    """Level per op, by fixpoint over the definitions (ops may come in any order)."""
    wire_level = {0: 0}
    lv = [None] * len(ops)
    left = set(range(len(ops)))
    while left:
        done = set()
        for i in sorted(left):
            reads = [w for form in _forms(ops[i]) for w, _ in form]
            if all(w in wire_level for w in reads):
                lv[i] = 1 + max([wire_level[w] for w in reads], default=0)
                done.add(i)
                for w in _defs(ops[i]):
                    wire_level[w] = lv[i]
        assert done, "the ops do not form a program (a cycle, or a wire nobody defines)"
        left -= done
    return lv


def _container(magic, sections):
    out = magic + struct.pack("<II", 1, len(sections))
    for sid, data in sections:
        out += struct.pack("<IQ", sid, len(data)) + data
    return out


def write(n_wires, ops, checks=(), n_public=0, n_inputs=None, inputs=(), outputs=(), levels=None, raw=None):
    """-> the file image.  levels: override the computed level per op (for malformed programs); raw: a function that
    may edit the dict of sections before framing."""
    lv = levels if levels is not None else levels_of(ops)
    order = sorted(range(len(ops)), key=lambda i: (lv[i], KIND[ops[i][0]]))
    n_levels = max(lv, default=0)
    if n_inputs is None:
        n_inputs = 1 + max([op[2] for op in ops if op[0] == "input"], default=-1)
    recs, terms, targets = b"", b"", []
    t_at = 0
    for i in order:
        op = ops[i]
        a, b, c = _forms(op)
        kind, dst, n, chk = KIND[op[0]], 0, 0, NO_CHECK
        if op[0] == "input":
            dst, n = op[1], op[2]
        elif op[0] == "bits":
            dst, n = len(targets), len(op[1])
            targets += list(op[1])
            chk = NO_CHECK if op[3] is None else op[3]
        elif op[0] == "check":
            chk = op[2]
        else:
            dst = op[1]
        recs += struct.pack("<8I", kind, dst, n, chk, t_at, len(a), len(b), len(c))
        for w, cf in list(a) + list(b) + list(c):
            terms += struct.pack("<Iq", w, cf)
        t_at += len(a) + len(b) + len(c)
    index = [sum(1 for x in lv if x <= l) for l in range(n_levels + 1)]
    texts = []
    ids = []
    for t in checks:
        if t not in texts:
            texts.append(t)
        ids.append(texts.index(t))
    sec6 = struct.pack(f"<{len(ids)}I", *ids) + b"".join(struct.pack("<I", len(t.encode())) + t.encode() for t in texts)
    sec7 = b"".join(struct.pack("<III", first, count, len(name.encode())) + name.encode() for name, first, count in inputs)
    secs = {
        1: struct.pack("<11I", n_wires, n_public, n_inputs, len(ops), n_levels, t_at, len(targets), len(ids), len(texts),
                       len(inputs), len(outputs)),
        2: recs, 3: terms, 4: struct.pack(f"<{len(index)}I", *index), 5: struct.pack(f"<{len(targets)}I", *targets),
        6: sec6, 7: sec7, 8: struct.pack(f"<{len(outputs)}I", *outputs)}
    if raw:
        raw(secs)
    return _container(b"wprg", sorted(secs.items()))


def read(img):
    """The file image -> dict(n_wires, n_public, n_inputs, ops (in file order, the shapes above), levels (per op), checks,
    inputs, outputs)."""
    assert img[:4] == b"wprg"
    _, nsec = struct.unpack_from("<II", img, 4)
    pos, sec = 12, {}
    for _ in range(nsec):
        sid, size = struct.unpack_from("<IQ", img, pos)
        sec[sid] = img[pos + 12:pos + 12 + size]
        pos += 12 + size
    h = struct.unpack("<11I", sec[1])
    n_ops, n_levels, n_checks, n_texts, n_names = h[3], h[4], h[7], h[8], h[9]
    targets = struct.unpack(f"<{h[6]}I", sec[5])
    index = struct.unpack(f"<{n_levels + 1}I", sec[4])
    ops, lv, level = [], [], 0
    for k in range(n_ops):
        while level < n_levels and k >= index[level]:
            level += 1
        kind, dst, n, chk, t_off, na, nb, nc = struct.unpack_from("<8I", sec[2], 32 * k)
        ts = [struct.unpack_from("<Iq", sec[3], 12 * i) for i in range(t_off, t_off + na + nb + nc)]
        a, b, c = ts[:na], ts[na:na + nb], ts[na + nb:]
        if kind == INPUT:
            ops.append(("input", dst, n))
        elif kind == QUAD:
            ops.append(("quad", dst, a, b, c))
        elif kind == BITS:
            ops.append(("bits", list(targets[dst:dst + n]), a, None if chk == NO_CHECK else chk))
        elif kind == INV0:
            ops.append(("inv0", dst, a))
        elif kind == ISZ:
            ops.append(("isz", dst, a))
        else:
            ops.append(("check", a, chk))
        lv.append(level)
    ids = struct.unpack_from(f"<{n_checks}I", sec[6])
    pos, texts = 4 * n_checks, []
    for _ in range(n_texts):
        (ln,) = struct.unpack_from("<I", sec[6], pos)
        texts.append(sec[6][pos + 4:pos + 4 + ln].decode())
        pos += 4 + ln
    pos, inputs = 0, []
    for _ in range(n_names):
        first, count, ln = struct.unpack_from("<III", sec[7], pos)
        inputs.append((sec[7][pos + 12:pos + 12 + ln].decode(), first, count))
        pos += 12 + ln
    return {"n_wires": h[0], "n_public": h[1], "n_inputs": h[2], "ops": ops, "levels": lv, "checks": [texts[i] for i in ids],
            "inputs": inputs, "outputs": list(struct.unpack(f"<{h[10]}I", sec[8]))}


def evaluate(n_wires, ops, inputs):
    """Big-integer evaluation in any valid order -> (wire values, status)."""
    lv = levels_of(ops)
    w = [None] * n_wires
    w[0] = 1
    status = NO_CHECK

    def lin(form):
        return sum(cf * w[x] for x, cf in form) % R

    for i in sorted(range(len(ops)), key=lambda i: lv[i]):
        op = ops[i]
        k = op[0]
        if k == "input":
            w[op[1]] = inputs[op[2]] % R
        elif k == "quad":
            w[op[1]] = (lin(op[2]) * lin(op[3]) + lin(op[4])) % R
        elif k == "bits":
            v, n = lin(op[2]), len(op[1])
            if v >> n:
                if op[3] is not None:
                    status = min(status, op[3])
                v = 0
            for j, t in enumerate(op[1]):
                w[t] = (v >> j) & 1
        elif k == "inv0":
            v = lin(op[2])
            w[op[1]] = pow(v, R - 2, R) if v else 0
        elif k == "isz":
            w[op[1]] = 1 if lin(op[2]) == 0 else 0
        else:
            if lin(op[1]) != 0:
                status = min(status, op[2])
    return w, status


def words(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


# ------------------------------------------------------------------ crafted programs (shared by the CPU and GPU tests)
def _rand(seed):
    import random
    return random.Random(seed)


def crafted_cases():
    """-> [dict(name, n_wires, ops, checks, inputs = [input vector, ...])]: each op kind alone and at its edges."""
    rng = _rand(20261020)
    cases = []

    def case(name, n_wires, ops, inputs, checks=()):
        cases.append({"name": name, "n_wires": n_wires, "ops": ops, "checks": list(checks), "inputs": inputs})

    rnd = [rng.randrange(R) for _ in range(4)]
    case("input", 2, [("input", 1, 0)], [[0], [1], [R - 1], [rnd[0]]])
    # QUAD: (w1 + 2)(w2 - 3) + (5 w1 - 7 w2), negative coefficients; then 0, 1 and 300 terms
    case("quad", 4, [("input", 1, 0), ("input", 2, 1), ("quad", 3, [(1, 1), (0, 2)], [(2, 1), (0, -3)], [(1, 5), (2, -7)])],
         [[0, 0], [1, 1], [R - 1, R - 2], rnd[:2], [3, 2 ** 200]])
    case("quad_0_terms", 2, [("quad", 1, [], [], [])], [[]])
    case("quad_1_term", 3, [("input", 1, 0), ("quad", 2, [], [], [(1, -(2 ** 62))])], [[1], [R - 1], [rnd[1]]])
    wide = [("input", 1 + i, i) for i in range(300)]
    coefs = [rng.choice([1, -1, 2, -2 ** 40, 2 ** 31, rng.randrange(-2 ** 63, 2 ** 63)]) for _ in range(300)]
    wide.append(("quad", 301, [(1 + i, coefs[i]) for i in range(300)], [(1, 1), (300, -1)], [(1 + i, coefs[299 - i]) for i in range(300)]))
    case("quad_300_terms", 302, wide, [[rng.randrange(R) for _ in range(300)], [i for i in range(300)]])
    # BITS n: 2^n - 1 fits, 2^n raises its check and gives zero bits
    for n in (1, 32, 64, 253):
        ops = [("input", 1, 0), ("bits", list(range(2, 2 + n)), [(1, 1)], 0)]
        case(f"bits_{n}", 2 + n, ops, [[0], [1], [2 ** n - 1], [2 ** n], [rng.randrange(2 ** n)], [R - 1]], ["does not fit"])
    # INV0 / ISZ on 0, 1, r - 1 and a random element
    # ... and around 4096, where the evaluators' table of small inverses ends (kWpInvSmall), on both sides of zero
    case("inv0_isz", 4, [("input", 1, 0), ("inv0", 2, [(1, 1)]), ("isz", 3, [(1, 1)])],
         [[0], [1], [R - 1], [rnd[2]], [4095], [4096], [R - 4095], [R - 4096], [2 ** 32 + 5], [2 ** 64]])
    # a CHECK that holds and one that does not; two violated checks: the lower index is reported although the
    # higher one sits at an earlier level
    case("check", 3, [("input", 1, 0), ("input", 2, 1), ("check", [(1, 1), (2, -1)], 0)], [[5, 5], [5, 6], [0, R - 1]], ["a === b"])
    case("two_checks", 4, [("input", 1, 0), ("quad", 2, [], [], [(1, 1)]), ("quad", 3, [], [], [(2, 1)]),
                           ("check", [(3, 1)], 0), ("check", [(3, 1), (0, -1)], 1), ("check", [(1, 1), (0, -2)], 2)],
         [[0], [1], [2], [3]], ["w3 is 0", "w3 is 1", "w1 is 2"])
    return cases


def width_program(width):
    """One level of exactly `width` ops over one input level: op i = QUAD (in0 + i)(in1 - i) + i."""
    ops = [("input", 1, 0), ("input", 2, 1)]
    ops += [("quad", 3 + i, [(1, 1), (0, i)], [(2, 1), (0, -i)], [(0, i)]) for i in range(width)]
    return 3 + width, ops


def chain_program(depth):
    """`depth` levels of one op each: w[i + 1] = w[i] * w[i] + w[i] + 1."""
    ops = [("input", 1, 0)]
    ops += [("quad", 2 + i, [(1 + i, 1)], [(1 + i, 1)], [(1 + i, 1), (0, 1)]) for i in range(depth - 1)]
    return 1 + depth, ops


def scattered_bits_program():
    """A BITS op with 35 scattered targets (the add_mod32 shape: five 32-bit operands, 3 carry bits), read back by a
    QUAD that recombines them."""
    n = 35
    targets = [3 + ((i * 37) % 101) for i in range(n)]           # distinct, not contiguous, not ascending
    free = [w for w in range(3, 3 + 101) if w not in targets]
    ops = [("input", 1, 0), ("input", 2, 1), ("bits", targets, [(1, 1), (2, 4)], None)]
    ops += [("quad", w, [], [], [(0, w)]) for w in free]
    ops.append(("quad", 104, [], [], [(targets[i], 1 << i) for i in range(n)]))
    return 105, ops
