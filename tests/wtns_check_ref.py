"""Big-integer twin of g16_wtns_check and builders for the small R1CS the witness-check tests use.

verdict(rows, w) restates the check with Python integers: per row a = A.w, b = B.w, c = C.w mod r, the row holds when
a * b = c mod r; the verdict names the lowest failing row, counts the failing rows and carries that row's a, b, c.
"""
import formats as f
from bn254 import R

FIELDS = ("ok", "constraint", "n_failed", "a", "b", "c")


def lc(terms, w):
    return sum(cf * w[s] for s, cf in terms) % R


def verdict(rows, w):
    first, n_failed = -1, 0
    for i, (A, B, Cc) in enumerate(rows):
        if (lc(A, w) * lc(B, w) - lc(Cc, w)) % R:
            n_failed += 1
            if first < 0:
                first = i
    if first < 0:
        return {"ok": True, "constraint": -1, "n_failed": 0, "a": 0, "b": 0, "c": 0}
    A, B, Cc = rows[first]
    return {"ok": False, "constraint": first, "n_failed": n_failed, "a": lc(A, w), "b": lc(B, w), "c": lc(Cc, w)}


def as_dict(v):
    """The library's verdict object as the twin's dict."""
    return {k: getattr(v, k) for k in FIELDS}


def text(v):
    return f"wtns check: constraint {v['constraint']} is not satisfied ({v['n_failed']} in all)"


class Lcg:
    """A small deterministic generator of field elements (the tests need no quality, only fixed values)."""

    def __init__(self, seed):
        self.x = seed

    def fr(self):
        out = 0
        for _ in range(4):
            self.x = (self.x * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            out = (out << 64) | self.x
        return out % R


class Builder:
    """Rows and a witness grown together: wire 0 is the constant 1, every row solves its own target wire."""

    def __init__(self, seed=1):
        self.w = [1]
        self.rows = []
        self.target = []       # per row: the wire whose value makes the row hold
        self.rng = Lcg(seed)

    def wire(self, value):
        self.w.append(value % R)
        return len(self.w) - 1

    def short_row(self):
        """(x + 3 y) * (k z) = t with fresh wires: three terms at most on a side."""
        x, y, z = (self.wire(self.rng.fr()) for _ in range(3))
        k = self.rng.fr()
        A, B = [(x, 1), (y, 3)], [(z, k)]
        t = self.wire(lc(A, self.w) * lc(B, self.w))
        self.rows.append((A, B, [(t, 1)]))
        self.target.append(t)
        return len(self.rows) - 1

    def long_row(self, which, length, coef=None, value=None):
        """One side (which = 0, 1, 2: A, B, C) of `length` terms over fresh wires, the two others one term each.
        coef(j) / value(j) give term j's coefficient and wire value; by default the coefficients cycle through +1, -1 and
        a general value, and the LAST term is general and non-zero, so it is also the last record of the row in the
        library's order (the +-1 records first): the last lane of the last stride owns it."""
        terms = []
        for j in range(length):
            cf = coef(j) if coef else (1, R - 1, self.rng.fr() | 2)[2 if j == length - 1 else j % 3]
            v = value(j) if value else (self.rng.fr() | 1)
            terms.append((self.wire(v), cf % R))
        s = lc(terms, self.w)
        one = [(0, 1)]
        if which == 2:       # 1 * t = C.w
            t = self.wire(s)
            row = ([(t, 1)], one, terms)
        else:                # (A.w) * 1 = t, or 1 * (B.w) = t
            t = self.wire(s)
            row = (terms, one, [(t, 1)]) if which == 0 else (one, terms, [(t, 1)])
        self.rows.append(row)
        self.target.append(t)
        return len(self.rows) - 1

    def r1cs(self, rows=None):
        return f.write_r1cs(len(self.w), 0, 0, self.rows if rows is None else rows)

    def wtns(self, w=None):
        return f.write_wtns(self.w if w is None else w)

    def broken(self, *rows):
        """The witness with the target wire of every given row raised by one: exactly those rows fail."""
        w = list(self.w)
        for r in rows:
            w[self.target[r]] = (w[self.target[r]] + 1) % R
        return w
