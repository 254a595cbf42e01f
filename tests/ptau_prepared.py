"""Test helper: a .ptau v1 image for a KNOWN (tau, alpha, beta), prepared for phase 2 when asked -- the Python
restatement that g16_ptau_synth must equal byte for byte.  Used at powers <= 9 only (pure Python points).

Layout (snarkjs powersoftau_utils.js / powersoftau_preparephase2.js): section 1 = n8, q, power, ceremonyPower;
2 = [tau^i]G1, i < 2^(power+1) - 1; 3 = [tau^i]G2, 4 = [alpha tau^i]G1, 5 = [beta tau^i]G1, i < 2^power;
6 = [beta]G2; 7 = contributions (none).  Prepared: 12 = [L_i(tau)]G1, 13 = [L_i(tau)]G2, 14 = [alpha L_i(tau)]G1,
15 = [beta L_i(tau)]G1, each as blocks k = 0, 1, ... of the 2^k Lagrange points of the size-2^k domain, block k from
point 2^k - 1: section 12 through block power + 1, sections 13-15 through block power."""
import struct

import groth16 as g
from bn254 import G1, G2, G2_GEN, Q, R
from formats import N8, g1_to_lem, g2_to_lem, le, read_binfile, write_binfile


def _g1s(ks):
    return b"".join(g1_to_lem(P) for P in G1.gen_mul_many(ks))


def _g2s(ks):
    return b"".join(g2_to_lem(P) for P in G2.gen_mul_many(ks))


def lagrange_blocks(tau, last_block):
    out = []
    for k in range(last_block + 1):
        out += g.lagrange_at(1 << k, tau)
    return out


def write_ptau_prepared(power, tau, alpha, beta, prepared=True):
    n = 1 << power
    s1 = struct.pack("<I", N8) + le(Q) + struct.pack("<II", power, power)
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    secs = [(1, s1), (2, _g1s(pw)), (3, _g2s(pw[:n])), (4, _g1s([alpha * x % R for x in pw[:n]])),
            (5, _g1s([beta * x % R for x in pw[:n]])), (6, g2_to_lem(G2.mul(G2_GEN, beta))), (7, struct.pack("<I", 0))]
    if prepared:
        lag = lagrange_blocks(tau, power + 1)
        m = 2 * n - 1
        secs += [(12, _g1s(lag)), (13, _g2s(lag[:m])), (14, _g1s([alpha * x % R for x in lag[:m]])),
                 (15, _g1s([beta * x % R for x in lag[:m]]))]
    return write_binfile("ptau", 1, secs)


def sections(buf):
    """-> [(id, payload)] in file order."""
    secs = read_binfile(buf, "ptau", 1, "ptau")
    order = sorted(((pos, sid, size) for sid, lst in secs.items() for pos, size in lst))
    return [(sid, buf[pos:pos + size]) for pos, sid, size in order]


def rewrite(buf, edit):
    """The image with edit(id, payload) -> payload (or None: drop the section) applied to every section."""
    out = []
    for sid, data in sections(buf):
        d = edit(sid, data)
        if d is not None:
            out.append((sid, d))
    return write_binfile("ptau", 1, out)
