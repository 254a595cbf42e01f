"""Test helper: the Python restatement of `powersoftau prepare phase2` (g16_ptau_prepare) for a ceremony of KNOWN
scalars.  A section whose point i is [x_i]G gives block k = [y_j]G with y = the inverse DFT of size 2^k of x_0 ..
x_{2^k - 1} over Fr (a plain transform of scalars, w_k = fr_root(k)), then one generator multiplication per point.
Section 12 has the extra block power + 1, whose last input (section 2 stops one point short) is zero.

For x_i = tau^i the blocks are the Lagrange basis L_j(tau) of the size-2^k domain (groth16.lagrange_at), except the
padded top block of section 12: y_j = L_j(tau) - w^j tau^(M-1) / M, M = 2^(power+1) (top_block_scalar)."""
import struct

from bn254 import G1, G1_GEN, G2, G2_GEN, R, fr_root
from formats import g1_to_lem, g2_to_lem

from ptau_prepared import sections


def idft(xs):
    """y_j = (1/N) sum_i w_N^(-ij) x_i, N = len(xs) a power of two (recursive radix 2)."""
    n = len(xs)
    k = n.bit_length() - 1
    assert 1 << k == n

    def rec(v, winv):
        if len(v) == 1:
            return v
        ev, od = rec(v[0::2], winv * winv % R), rec(v[1::2], winv * winv % R)
        h = len(v) // 2
        out = [0] * len(v)
        t = 1
        for j in range(h):
            u = t * od[j] % R
            out[j] = (ev[j] + u) % R
            out[j + h] = (ev[j] - u) % R
            t = t * winv % R
        return out
    ninv = pow(n, -1, R)
    return [y * ninv % R for y in rec(list(xs), pow(fr_root(k), -1, R))]


def block_scalars(xs, last_block):
    """Blocks 0 .. last_block of the source scalars xs (zero from index len(xs) on), concatenated in file order."""
    out = []
    for k in range(last_block + 1):
        n = 1 << k
        out += idft([xs[i] if i < len(xs) else 0 for i in range(n)])
    return out


def lagrange_scalar(M, j, tau):
    """L_j(tau) over the size-M domain, tau not in the domain."""
    w = pow(fr_root(M.bit_length() - 1), j, R)
    return (pow(tau, M, R) - 1) * pow(M, -1, R) % R * w % R * pow((tau - w) % R, -1, R) % R


def top_block_scalar(power, j, tau):
    """Point j of block power + 1 of section 12 as a multiple of G1: the Lagrange value minus the share of the missing
    input tau^(M-1)."""
    M = 2 << power
    w = pow(fr_root(power + 1), j, R)
    return (lagrange_scalar(M, j, tau) - w * pow(tau, M - 1, R) % R * pow(M, -1, R)) % R


def g1_bytes(ks):
    return b"".join(g1_to_lem(P) for P in G1.gen_mul_many(ks))


def g2_bytes(ks):
    return b"".join(g2_to_lem(P) for P in G2.gen_mul_many(ks))


def g1_point_bytes(k):
    k %= R
    return g1_to_lem(G1.mul(G1_GEN, k) if k else None)


def expected_sections(power, x2, x3, x4, x5):
    """{12..15: bytes} for source sections whose points are [x2_i]G1, [x3_i]G2, [x4_i]G1, [x5_i]G1."""
    return {12: g1_bytes(block_scalars(x2, power + 1)), 13: g2_bytes(block_scalars(x3, power)),
            14: g1_bytes(block_scalars(x4, power)), 15: g1_bytes(block_scalars(x5, power))}


def ceremony_scalars(power, tau, alpha, beta):
    n = 1 << power
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    return pw, pw[:n], [alpha * x % R for x in pw[:n]], [beta * x % R for x in pw[:n]]


def split(buf):
    """-> ([ids in file order], {id: payload})."""
    secs = sections(buf)
    return [sid for sid, _ in secs], dict(secs)


def power_of(buf):
    return struct.unpack_from("<I", split(buf)[1][1], 36)[0]
