"""Representative-exact twin of the Fr NTT (csrc/ntt.hip over csrc/fr29.cuh).

test_cpu_ntt_plan.py models the pass plan and the tile index math on residues mod r.  This module runs the same
plan on the INTEGERS the kernels hold: a lazy element is its value sum l[i] 2^(29 i), Montgomery radix 2^261, never
reduced below r except by fr29_weak_reduce.  Every function returns the integer its device twin returns (pinned
integer for integer against a host build of fr29.cuh by test_cpu_ntt_lazy.py), so the twin can say how large a value
gets at every stage, and it raises BoundBreach where a kernel precondition fails:

  subtrahend of fr29_sub<K> <= K r;  product input < 16 r;  weak-reduce input < 16 r (and quotient <= 16: the NEGQ
  table has 17 rows);  fr29_to_fr / fr29_to_plain input < 16 r.

The index math (plan, tile_gidx) is imported from test_cpu_ntt_plan.py; the reduce cadence (the K of every DIF phase,
the stages after which a tile is weak-reduced, the reduce on load) is read from ntt.hip's own text (kernel_cadence),
so a change of the kernels' cadence is a change of the twin's.

MAINTAINERS: kernel_cadence matches the exact spelling of the subtraction, reduce_now and tile-load lines of ntt.hip.
Reformatting those lines makes this module raise RuntimeError at import, which fails every lazy-NTT test, CPU and GPU;
the fix is to update the patterns in kernel_cadence, not the kernel."""
import os
import re
from functools import lru_cache

from bn254 import R, RR, fr_root
from test_cpu_ntt_plan import bitrev, plan, tile_gidx

BITS = 261
RAD = 1 << BITS
MASK = RAD - 1
NINV = (-pow(R, -1, RAD)) & MASK        # -r^-1 mod 2^261: the nine per-limb INV steps of f29_mul taken together
ONE = RAD % R                           # G16_FR29_ONE
TO = (RAD * RAD // (1 << 256)) % R      # G16_FR29_TO   (2^266 mod r): Mont256 -> Mont261
FROM = (1 << 256) % R                   # G16_FR29_FROM: Mont261 -> Mont256
R16 = 16 * R
RINV = pow(RAD, -1, R)

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nzcp-circom_amd", "csrc")
with open(os.path.join(_CSRC, "bn254_consts.h")) as _f:
    RECIP = int(re.search(r"#define\s+G16_FR29_RECIP\s+(\d+)u", _f.read()).group(1))


def kernel_cadence(path=os.path.join(_CSRC, "ntt.hip")):
    """The reduce cadence as ntt.hip states it, read from its text so that the twin follows the kernels and not a copy
    of them: the K of fr29_sub per DIF phase (product branch and the stage on index bit 0), the DIF phase and the DIT
    stage after which the tile is weak-reduced, and which kernels weak-reduce on load.  The patterns are tied to the
    spelling of five lines of ntt.hip; a line that reads as neither form raises here, and the patterns are then
    brought up to date with the kernel."""
    with open(path) as fh:
        src = fh.read()
    sub3 = r"phase == 0 \? fr29_sub<(\d)>\(u, v\) : \(phase == 1 \? fr29_sub<(\d)>\(u, v\) : fr29_sub<(\d)>\(u, v\)\)"
    k0 = re.search(r"tile\[e1\] = dif \? \(" + sub3 + r"\)\s*: fr29_sub<2>\(u, v\);", src)
    kp = re.search(r"const F29 d = " + sub3 + ";", src)
    red = re.search(r"reduce_now = dif \? \(phase == (\d) && k \+ 1 < S\) : \(k == (\d+) && S > (\d+)\);", src)
    if not (k0 and kp and red):
        raise RuntimeError("ntt.hip: ntt_tile_stages no longer reads as the twin expects")
    bounds = [src.index("void ntt_pass_kernel"), src.index("void ntt_mid_pass_kernel"),
              src.index("void ntt_last_pass_join_kernel"), src.index("void ntt_pow_table_kernel")]
    load = {}
    for i, name in enumerate(("pass", "mid", "join")):
        m = re.search(r"tile\[e\] = (fr29_weak_reduce\()?x\[(gidx\(e\)|base \+ e)\]\)?;", src[bounds[i]:bounds[i + 1]])
        if not m:
            raise RuntimeError(f"ntt.hip: the tile load of the {name} kernel no longer reads as the twin expects")
        load[name] = m.group(1) is not None
    return {
        "dif_k": tuple(int(x) for x in kp.groups()),
        "dif_k0": tuple(int(x) for x in k0.groups()),
        "dif_reduce_phase": int(red.group(1)),
        "dit_reduce_k": int(red.group(2)),
        "dit_reduce_S": int(red.group(3)),
        "load_reduce": load,
    }


CADENCE = kernel_cadence()

# the field element whose lazy image is the representative r - 1: e 2^261 = -1 (mod r)
E = (-RINV) % R
E_MONT256 = E * RR % R                  # what fr_fft takes


class BoundBreach(AssertionError):
    """a precondition of the kernels' lazy arithmetic does not hold"""


# ------------------------------------------------------------------ arithmetic (fr29.cuh / fq29.cuh)
def mont(a, b):
    """(a b + m r) / 2^261 with m = -a b / r mod 2^261: what f29_mul's 162 multiply-adds compute"""
    t = a * b
    return (t + (((t & MASK) * NINV) & MASK) * R) >> BITS


def fr29_mul(a, b):
    if a >= R16 or b >= R16:
        raise BoundBreach(f"product input {max(a, b) / R:.4f} r")
    return mont(a, b)


def fr29_add(a, b):
    return a + b


def fr29_sub(K, a, b):
    if b > K * R:
        raise BoundBreach(f"subtrahend {b / R:.4f} r against K = {K}")
    return a + K * R - b


def fr29_weak_reduce(x):
    if x >= R16:
        raise BoundBreach(f"weak-reduce input {x / R:.4f} r")
    q = ((x >> 232) * RECIP) >> 40
    if q > 16:
        raise BoundBreach(f"weak-reduce quotient {q}")
    return (x + ((-q * R) & MASK)) & MASK          # + NEGQ[q], carry, top limb & (2^29 - 1)


def _cond_sub(t):
    return t - R if t >= R else t


def fr29_from_fr(v):
    return mont(v, TO)


def fr29_to_fr(a):
    if a >= R16:
        raise BoundBreach(f"to_fr input {a / R:.4f} r")
    return _cond_sub(mont(a, FROM)) & ((1 << 256) - 1)


def fr29_to_plain(a):
    if a >= R16:
        raise BoundBreach(f"to_plain input {a / R:.4f} r")
    return _cond_sub(mont(a, 1)) & ((1 << 256) - 1)


# fr29_pow_u64 runs 64 square(-and-multiply) steps from ONE.  The leading squarings of ONE reach a fixed point
# at once, so the state after the bits of a prefix p depends on p alone: pow(a, 2 p + b) follows from pow(a, p).
_ONE_FIX = ONE
for _ in range(8):
    _ONE_FIX = mont(_ONE_FIX, _ONE_FIX)
assert mont(_ONE_FIX, _ONE_FIX) == _ONE_FIX


def fr29_pow_u64(a, e):
    r = ONE
    for i in range(63, -1, -1):
        r = mont(r, r)
        if (e >> i) & 1:
            r = mont(r, a)
    return r


def pow_table(a, n):
    """[fr29_pow_u64(a, i) for i in range(n)] in ~1.5 products per entry (n <= 2^27: >= 8 leading squarings)"""
    out = [_ONE_FIX] * n
    for i in range(1, n):
        s = out[i >> 1]
        s = mont(s, s)
        out[i] = mont(s, a) if i & 1 else s
    return out


# ------------------------------------------------------------------ tables (ntt_tables_create)
class Tables:
    def __init__(self, L):
        N = 1 << L
        half = max(1, N // 2)
        wc = fr_root(L)
        w = fr29_from_fr(wc * RR % R)
        winv = fr29_from_fr(pow(wc, -1, R) * RR % R)
        inc = fr29_from_fr(fr_root(L + 1) * RR % R)
        self.ninv = fr29_from_fr(pow(N, -1, R) * RR % R)
        self.tw_fwd = pow_table(w, half)
        self.tw_inv = pow_table(winv, half)
        pw = pow_table(inc, N)
        self.coset = [mont(self.ninv, pw[bitrev(j, L)]) for j in range(N)]
        self.bitrev = [bitrev(j, L) for j in range(N)]
        self.cache = {}     # index lists and per-stage twiddle lists of the tiles: the same for every vector


@lru_cache(maxsize=4)
def tables(L):
    return Tables(L)


@lru_cache(maxsize=None)
def _pairs(n, bit):
    """the butterflies of a stage on tile bit `bit`: (elements e0, elements e1 = e0 | 1 << bit)"""
    low = (1 << bit) - 1
    e0s = [((bf >> bit) << (bit + 1)) | (bf & low) for bf in range(n >> 1)]
    return e0s, [e | (1 << bit) for e in e0s]


NEGQ = [(-q * R) & MASK for q in range(17)]          # G16_FR29_NEGQ


def kernel_plan(L, tile_log=9, min_tb=2):
    """ntt_tables_create: G16_NTT_TILE_LOG / G16_NTT_MIN_TB with their clamps, then the pass plan"""
    tile_max = min(max(tile_log, 3), 11)
    min_tb = min(max(min_tb, 0), tile_max - 1)
    return plan(L, tile_max, min_tb)


# ------------------------------------------------------------------ the passes
class Twin:
    """One NttTables worth of transforms.  rec[(tag, k, branch)] = largest representative seen on that branch of
    stage k of the pass `tag`; sub[(tag, k)] = (largest subtrahend, K); low[(tag, k)] = smallest difference.
    Branches: 'sum', 'diff' (before the DIF product / the DIT difference), 'prod'; stage 'load' / 'store' / 'post'."""

    def __init__(self, L, tile_log=9, min_tb=2):
        self.L, self.N = L, 1 << L
        self.tl, self.passes = kernel_plan(L, tile_log, min_tb)
        self.t = tables(L)
        self.rec, self.sub, self.low = {}, {}, {}
        self.c = CADENCE

    # -- records
    def _hi(self, key, vals):
        m = max(vals)
        if m > self.rec.get(key, -1):
            self.rec[key] = m

    # -- ntt_tile_stages
    def stages(self, tile, tw, g, lo_bits, S, tb, dif, tag):
        L, n = self.L, len(tile)
        for k in range(S):
            st = S - 1 - k if dif else k
            bit, beta = tb + st, lo_bits + st
            hmask, sh, phase = (1 << beta) - 1, L - 1 - beta, k % 3
            e0s, e1s = _pairs(n, bit)
            us = [tile[e] for e in e0s]
            vs = [tile[e] for e in e1s]
            if beta:
                # the twiddles depend on the tile through the low bits of its base alone
                key = (dif, n, lo_bits, tb, st, g[0] & ((1 << lo_bits) - 1))
                ws = self.t.cache.get(key)
                if ws is None:
                    ws = self.t.cache[key] = [tw[(g[e] & hmask) << sh] for e in e0s]
            if dif:
                K = (self.c["dif_k"] if beta else self.c["dif_k0"])[phase]
                KR = K * R
                sums = [u + v for u, v in zip(us, vs)]
                mv = max(vs)
                if mv > self.sub.get((tag, k), (-1, K))[0]:
                    self.sub[(tag, k)] = (mv, K)
                if mv > KR:
                    raise BoundBreach(f"{tag} stage {k}: subtrahend {mv / R:.4f} r against K = {K}")
                ds = [u + KR - v for u, v in zip(us, vs)]
                self._hi((tag, k, "diff"), ds)
                self.low[(tag, k)] = min(min(ds), self.low.get((tag, k), R16))
                if beta:
                    if max(ds) >= R16:
                        raise BoundBreach(f"{tag} stage {k}: product input {max(ds) / R:.4f} r")
                    ds = [((t := d * w) + (((t & MASK) * NINV) & MASK) * R) >> BITS for d, w in zip(ds, ws)]
                    self._hi((tag, k, "prod"), ds)
            else:
                K, KR = 2, 2 * R
                if beta:
                    if max(vs) >= R16:
                        raise BoundBreach(f"{tag} stage {k}: product input {max(vs) / R:.4f} r")
                    vs = [((t := v * w) + (((t & MASK) * NINV) & MASK) * R) >> BITS for v, w in zip(vs, ws)]
                    self._hi((tag, k, "prod"), vs)
                mv = max(vs)
                if mv > self.sub.get((tag, k), (-1, K))[0]:
                    self.sub[(tag, k)] = (mv, K)
                if mv > KR:
                    raise BoundBreach(f"{tag} stage {k}: subtrahend {mv / R:.4f} r against K = 2")
                sums = [u + v for u, v in zip(us, vs)]
                ds = [u + KR - v for u, v in zip(us, vs)]
                self._hi((tag, k, "diff"), ds)
            self._hi((tag, k, "sum"), sums)
            for e, s in zip(e0s, sums):
                tile[e] = s
            for e, d in zip(e1s, ds):
                tile[e] = d
            c = self.c
            if (phase == c["dif_reduce_phase"] and k + 1 < S) if dif else (k == c["dit_reduce_k"] and S > c["dit_reduce_S"]):
                self._reduce(tile, tag)

    def _reduce(self, tile, tag):
        m = max(tile)
        if m >= R16:
            raise BoundBreach(f"{tag}: weak-reduce input {m / R:.4f} r")
        # (below 16 r the quotient estimate is at most 15: inside the table)
        tile[:] = [(x + NEGQ[((x >> 232) * RECIP) >> 40]) & MASK for x in tile]

    def _tile_idx(self, t, lo_bits, S, tb):
        key = ("g", self.tl, lo_bits, S, tb, t)
        g = self.t.cache.get(key)
        if g is None:
            gi = tile_gidx(t, self.tl, lo_bits, S, tb)
            g = self.t.cache[key] = [gi(e) for e in range(1 << self.tl)]
        return g

    def _load(self, x, g, tag, kernel="pass"):
        tile = [x[i] for i in g]
        self._hi((tag, "load", "in"), tile)
        if self.c["load_reduce"][kernel]:
            self._reduce(tile, tag)
        return tile

    def _mul_all(self, tile, tab, tag):
        m = max(tile)
        if m >= R16:
            raise BoundBreach(f"{tag}: product input {m / R:.4f} r")
        self._hi((tag, "post", "in"), tile)
        return [((t := a * c) + (((t & MASK) * NINV) & MASK) * R) >> BITS for a, c in zip(tile, tab)]

    def run_pass(self, x, p, dif, post=None):
        """ntt_pass_kernel over the whole vector, in place"""
        lo_bits, S, tb = self.passes[p]
        tag = ("dif" if dif else "dit", p)
        tw = self.t.tw_inv if dif else self.t.tw_fwd
        for t in range(self.N >> self.tl):
            g = self._tile_idx(t, lo_bits, S, tb)
            tile = self._load(x, g, tag)
            self.stages(tile, tw, g, lo_bits, S, tb, dif, tag)
            self._hi((tag, "store", "out"), tile)
            if post is not None:
                tile = self._mul_all(tile, [post[i] for i in g], tag)
            for i, v in zip(g, tile):
                x[i] = v

    def mid_pass(self, x):
        """ntt_mid_pass_kernel: last inverse pass, coset table, first forward pass on the tile"""
        tl = self.tl
        for t in range(self.N >> tl):
            g = list(range(t << tl, (t + 1) << tl))
            tile = self._load(x, g, ("dif", 0), "mid")
            self.stages(tile, self.t.tw_inv, g, 0, tl, 0, True, ("dif", 0))
            tile = self._mul_all(tile, self.t.coset[t << tl:(t + 1) << tl], ("dif", 0))
            self._hi((("dit", 0), "load", "in"), tile)
            self.stages(tile, self.t.tw_fwd, g, 0, tl, 0, False, ("dit", 0))
            self._hi((("dit", 0), "store", "out"), tile)
            x[t << tl:(t + 1) << tl] = tile

    def join_pass(self, a, b, c, p):
        """ntt_last_pass_join_kernel: the last forward pass of a, b, c and P = plain(a' b' - c')"""
        lo_bits, S, tb = self.passes[p]
        tag = ("dit", p)
        out = [0] * self.N
        for t in range(self.N >> self.tl):
            g = self._tile_idx(t, lo_bits, S, tb)
            tiles = []
            for x in (a, b, c):
                tile = self._load(x, g, tag, "join")
                self.stages(tile, self.t.tw_fwd, g, lo_bits, S, tb, False, tag)
                self._hi((tag, "store", "out"), tile)
                tiles.append(tile)
            for i, ta, tb_, tc in zip(g, *tiles):
                out[i] = fr29_to_plain(fr29_sub(2, fr29_mul(ta, tb_), fr29_weak_reduce(tc)))
        return out

    # -- ops.hip fft_impl
    def _import(self, vals, rev):
        br = self.t.bitrev
        return [mont(vals[br[j]], TO) for j in range(self.N)] if rev else [mont(v, TO) for v in vals]

    def _export(self, z, rev, scale=None):
        if scale is not None:
            z = self._mul_all(z, [scale] * self.N, ("export", 0))
        m = max(z)
        if m >= R16:
            raise BoundBreach(f"to_fr input {m / R:.4f} r")
        out = [_cond_sub(mont(v, FROM)) & ((1 << 256) - 1) for v in z]
        br = self.t.bitrev
        return [out[br[i]] for i in range(self.N)] if rev else out

    def fft(self, vals, inverse=False):
        """fr_fft / fr_fft(inverse=True) on canonical Montgomery(2^256) images"""
        np_ = len(self.passes)
        z = self._import(vals, rev=not inverse)
        if self.L:
            for p in (reversed(range(np_)) if inverse else range(np_)):
                self.run_pass(z, p, inverse)
        return self._export(z, rev=inverse, scale=self.t.ninv if inverse else None)

    # -- zkey_verify_h.hip: import (bit-reversed), coset table, forward passes, export
    def coset_forward(self, vals):
        z = self._mul_all(self._import(vals, rev=True), self.t.coset, ("dit", "scale"))
        for p in range(len(self.passes)):
            self.run_pass(z, p, False)
        return self._export(z, rev=False)

    # -- ntt_coset_roundtrip
    def coset_roundtrip(self, vecs, join=False):
        """Odd-coset evaluation of lazy vectors in place; join (three vectors): returns P = plain(a' b' - c')."""
        np_ = len(self.passes)
        if self.L == 0:
            raise NotImplementedError("L = 0 is a table product alone")
        if np_ < 2:                                   # one pass: the unfused route
            for x in vecs:
                self.run_pass(x, 0, True, post=self.t.coset)
            if join:
                return self.join_pass(*vecs, 0)
            for x in vecs:
                self.run_pass(x, 0, False)
            return None
        for x in vecs:
            for p in range(np_ - 1, 0, -1):
                self.run_pass(x, p, True)
            self.mid_pass(x)
            for p in range(1, np_ - 1 if join else np_):
                self.run_pass(x, p, False)
        return self.join_pass(*vecs, np_ - 1) if join else None


def lazy(v):
    """field element -> the canonical lazy representative (what a load's weak reduction leaves of a generic value)"""
    return v * RAD % R


def residues(xs):
    return [x * RINV % R for x in xs]


# ------------------------------------------------------------------ the input families
def constant_e(L):
    return [E] * (1 << L)


def square_wave(L, beta):
    return [E if (i >> beta) & 1 else 0 for i in range(1 << L)]


def wave_bits(passes):
    """one index bit in each DIF phase of each pass: [(pass, stage k, beta)]"""
    out = []
    for p, (lo, S, tb) in enumerate(passes):
        for phase in range(min(3, S)):
            out.append((p, phase, lo + S - 1 - phase))
    return out


def worst_path_tile(tw, L, lo_bits, S, tb, gidx, col, behind_product=False):
    """Field values (residues of the lazy words, as field elements) of one DIT tile that drive its all-ones row up by
    2 r per stage: c = e in row 0 of column `col`, and one value in row 2^k, k < min(S, 7), chosen so that the
    product v w of stage k on the path is the residue rho_k itself and not rho_k + r.  A product (V W + m r) / 2^261,
    m < 2^261, is the smallest integer of its class that is >= V W / 2^261, and V < (2 k + 1.1) r at stage k (a loaded
    word below 1.1 r, +2 r per stage), so rho_k = ceil((2 k + 1.1) r W / 2^261) for the table word W of the path is
    the smallest residue that returns as itself whatever representative the load left of the tile's zeros (chosen from
    this bound and not by search: it holds for every pass and route alike).  The stage on index bit 0 has no product:
    its word is the loaded one, unique below 1.0001 r from r / 2^13 on -- or, where the tile comes out of the coset
    product (behind_product: the fused mid pass, zkey_h_scalars), from 16 r W / 2^261 < 0.1 r on.
    Returns {tile element: field value}."""
    out = {col: E}
    for k in range(min(S, 7)):
        beta = lo_bits + k
        e0 = (((1 << k) - 1) << tb) | col                  # the path's partner row 2^k - 1
        if beta == 0:
            rho = R // 10 if behind_product else (R >> 13) + 1
            wres = 1
        else:
            W = tw[(gidx(e0) & ((1 << beta) - 1)) << (L - 1 - beta)]
            rho = (20 * k + 11) * R // 10 * W // RAD + 1
            wres = W * RINV % R
        # rows [2^k, 2^(k+1)) hold the transform of a delta: every row of the block carries the value of row 2^k
        out[((1 << k) << tb) | col] = rho * RINV % R * pow(wres, -1, R) % R
    return out


def _undo_dit_pass(y, twi, L, tl, lo_bits, S, tb):
    """The inverse of one forward pass on residues, in place: the DIF butterflies of test_cpu_ntt_plan.run_pass with
    inverse twiddles, then 2^-S, on the tiles that hold anything (a zero tile stays zero)."""
    sc = pow(2, -S, R)
    for t in range((1 << L) >> tl):
        gi = tile_gidx(t, tl, lo_bits, S, tb)
        g = [gi(e) for e in range(1 << tl)]
        if not any(y[i] for i in g):
            continue
        for k in range(S):
            st = S - 1 - k
            beta = lo_bits + st
            for e0, e1 in zip(*_pairs(len(g), tb + st)):
                i0, i1 = g[e0], g[e1]
                u, v = y[i0], y[i1]
                y[i0], y[i1] = (u + v) % R, (u - v) * twi[(i0 & ((1 << beta) - 1)) << (L - 1 - beta)] % R
        for i in g:
            y[i] = y[i] * sc % R


def worst_path_vector(L, p, tile_log=9, min_tb=2, tile=None, col=None):
    """Input of fr_fft (natural order, field values) whose vector before forward pass p holds worst_path_tile in one
    tile and zeros elsewhere: the sparse vector mapped back through passes 0 .. p-1 (each DIT pass undone by the DIF
    pass with inverse twiddles and 2^-S) and the bit reversal.  Returns (vector, (tile, path element))."""
    tl, passes = kernel_plan(L, tile_log, min_tb)
    lo_bits, S, tb = passes[p]
    N = 1 << L
    ntiles = N >> tl
    tile = ntiles - 1 if tile is None else tile
    col = (1 << tb) - 1 if col is None else col
    gidx = tile_gidx(tile, tl, lo_bits, S, tb)
    y = [0] * N
    for e, v in worst_path_tile(tables(L).tw_fwd, L, lo_bits, S, tb, gidx, col).items():
        y[gidx(e)] = v
    if p:
        w = fr_root(L)
        twi = [pow(w, -i, R) for i in range(max(1, N // 2))]
        for q in range(p - 1, -1, -1):
            _undo_dit_pass(y, twi, L, tl, *passes[q])
    path = (((1 << min(S, 7)) - 1) << tb) | col
    return [y[bitrev(i, L)] for i in range(N)], (tile, path)


def coset_preimage(y, L):
    """The evaluations A_T on the domain whose coefficient vector times the coset table is y at the input of the
    first forward pass (bit-reversed order, as the fused mid pass holds it): coef[i] = y[bitrev(i)] / w_2N^i."""
    from groth16 import ntt
    N = 1 << L
    iinv = pow(fr_root(L + 1), -1, R)
    coef, t = [0] * N, 1
    for i in range(N):
        coef[i] = y[bitrev(i, L)] * t % R
        t = t * iinv % R
    return ntt(coef), coef


def chain_vectors(L, tile_log=9, min_tb=2):
    """A_T of the two witnesses of the Groth16 chain (rows w_i * 1 = w_i: B_T = 1 but for the binding row, C_T =
    A_T o B_T): (i) constant e, (ii) the worst-path vector of the first forward pass behind the coset table, with one
    coefficient that only another tile reads spent on the binding row's A_T[N - 1] = 1."""
    from groth16 import ntt
    N = 1 << L
    const = [E] * (N - 1) + [1]
    tl, passes = kernel_plan(L, tile_log, min_tb)
    gidx = tile_gidx(0, tl, 0, tl, 0)
    y = [0] * N
    for e, v in worst_path_tile(tables(L).tw_fwd, L, 0, tl, 0, gidx, 0, behind_product=True).items():
        y[gidx(e)] = v
    a, coef = coset_preimage(y, L)
    if N > (1 << tl):
        # A_T[N - 1] = sum coef[i] w^-i: move it to 1 with the coefficient the last tile's element 0 reads
        i0 = bitrev(N - (1 << tl), L)
        coef[i0] = (coef[i0] + (1 - a[N - 1]) * pow(fr_root(L), i0, R)) % R
        a = ntt(coef)
        assert a[N - 1] == 1
    return const, a


def h_scalar_vectors(L):
    """u of zkey_h_scalars (u[N - 1] = 0; its words are imported as Montgomery(2^256) images, then multiplied by the
    coset table): constant e, and the u whose twisted vector is the worst-path vector of the first forward pass."""
    N = 1 << L
    tl, passes = kernel_plan(L)
    gidx = tile_gidx(0, tl, 0, tl, 0)
    iinv = pow(fr_root(L + 1), -1, R)
    y = [0] * N
    for e, v in worst_path_tile(tables(L).tw_fwd, L, 0, tl, 0, gidx, 0, behind_product=True).items():
        y[gidx(e)] = v
    assert y[N - 1] == 0
    u, t = [0] * N, N * RR % R
    for i in range(N):
        u[i] = y[bitrev(i, L)] * t % R
        t = t * iinv % R
    return [E_MONT256] * (N - 1) + [0], u


def family_names(L, tile_log=9, min_tb=2):
    """(a) const, (b) wave-p<pass>-ph<phase>: one square wave per DIF phase of each pass, (c) path-p<pass>: the
    worst-path vector of each forward pass"""
    tl, passes = kernel_plan(L, tile_log, min_tb)
    waves = [f"wave-p{p}-ph{ph}" for p, ph, _ in wave_bits(passes)]
    return ["const"] + waves + [f"path-p{p}" for p in range(len(passes))]


def family_vector(L, tile_log, min_tb, name):
    """the vector of field values a family name stands for"""
    if name == "const":
        return constant_e(L)
    kind, p, *rest = name.split("-")
    p = int(p[1:])
    if kind == "path":
        return worst_path_vector(L, p, tile_log, min_tb)[0]
    lo, S, tb = kernel_plan(L, tile_log, min_tb)[1][p]
    return square_wave(L, lo + S - 1 - int(rest[0][2:]))


def primitive_cases():
    """(op, a, b) for the host build of fr29.cuh and the device's f29_op: a few hundred, the edges first"""
    import random
    rng = random.Random(2929)
    edge = [0, 1, R - 1, R, R + 1, 16 * R - 1] + [k * R for k in range(2, 16)] + [k * R - 1 for k in (2, 8, 15)]

    def lz(kmax):
        return rng.randrange(R) + rng.randrange(kmax + 1) * R
    cases = []
    cases += [("from_fr", v, 0) for v in [0, 1, R - 1, E_MONT256, RR] + [rng.randrange(R) for _ in range(40)]]
    cases += [("mul", x, y) for x, y in zip(edge, reversed(edge))] + [("mul", x, x) for x in edge]
    cases += [("mul", lz(15), lz(15)) for _ in range(120)]
    cases += [("weak", x, 0) for x in edge] + [("weak", lz(15), 0) for _ in range(80)]
    for K in (2, 3, 5):
        subs = [0, 1, R - 1, R, K * R, K * (R - 1)] + [rng.randrange(K * R + 1) for _ in range(24)]
        cases += [(f"sub{K}", a, s) for s in subs for a in (0, lz(9))]
    cases += [("to_fr", x, 0) for x in edge] + [("to_fr", lz(15), 0) for _ in range(40)]
    return cases


def twin_value(op, a, b):
    if op == "from_fr":
        return fr29_from_fr(a)
    if op == "mul":
        return fr29_mul(a, b)
    if op == "weak":
        return fr29_weak_reduce(a)
    if op == "to_fr":
        return fr29_to_fr(a)
    return fr29_sub(int(op[3:]), a, b)
