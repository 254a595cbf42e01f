"""Python twin of the phase-2 MPCParams exchange (csrc/zkey_bellman_host.cpp, csrc/zkey_bellman.hip), written from the
description of the file and of the basis change, not from the C++: the MPCParams codec over a key's sections, the
closed form of H, and the basis change as a plain O(N^2) sum IN THE EXPONENT -- the tests' points are known multiples
of the generator, so a point is its scalar (0 = infinity) and the sum shares no transform, no window and no curve
formula with the code under test; the points come from the oracle's fixed-base multiplication afterwards."""
import struct

import bn254 as b
import formats as f
import zkey_mpc_ref as mref
from bn254 import Q, R

HEADER = 576
DELTA1, DELTA2 = 384, 448                   # offsets in the MPCParams header
RECORD = 384
RUNS = ("IC", "H", "L", "A", "B1", "B2")
RUN_POINT = {"IC": 64, "H": 64, "L": 64, "A": 64, "B1": 64, "B2": 128}
RUN_SECTION = {"IC": 3, "L": 8, "A": 5, "B1": 6, "B2": 7}
HDR_ALPHA1 = 84                              # section 2: alpha1, beta1, beta2, gamma2, delta1, delta2 from here
G1_INF_BE = bytes([0x40]) + bytes(63)


# ------------------------------------------------------------------ the basis change, in the exponent
def basis_forward(a, L):
    """a[i] = the scalar of section 9's point i -> T[k] = -2 w^k sum_i w^(2ik) a[i], ALL N values."""
    N, w = 1 << L, b.fr_root(L + 1)
    pw = [pow(w, j, R) for j in range(2 * N)]
    return [(-2 * pw[k]) * sum(pw[2 * i * k % (2 * N)] * a[i] for i in range(N)) % R for k in range(N)]


def basis_inverse(t, L):
    """t[k] -> (1 / N) sum_k w^(-2ik) (-(1/2) w^(-k)) t[k]."""
    N, w = 1 << L, b.fr_root(L + 1)
    pw = [pow(w, -j, R) for j in range(2 * N)]
    half = pow(-2, -1, R)
    x = [half * pw[k] * t[k] % R for k in range(N)]
    ninv = pow(N, -1, R)
    return [ninv * sum(pw[2 * i * k % (2 * N)] * x[k] for k in range(N)) % R for i in range(N)]


def project(a, L):
    """What import(export(.)) makes of section 9: T[N-1] dropped."""
    t = basis_forward(a, L)
    t[-1] = 0
    return basis_inverse(t, L)


def h_closed_form(tau, N, delta=1):
    """The MPCParams H run in the exponent: tau^k (tau^N - 1) / delta, k < N - 1."""
    z = (pow(tau, N, R) - 1) * pow(delta, -1, R) % R
    return [pow(tau, k, R) * z % R for k in range(N - 1)]


def points(scalars):
    """[a] G for every a, file form (0 -> infinity = zero bytes), concatenated."""
    nz = [a % R for a in scalars if a % R]
    it = iter(b.G1.gen_mul_many(nz))
    return b"".join(f.g1_to_lem(next(it)) if a % R else bytes(64) for a in scalars)


# ------------------------------------------------------------------ the file
def _be(x):
    return int(x).to_bytes(32, "big")


def g1_be(lem):
    return mref.g1_uncompressed(lem)


def g2_be(lem):
    return mref.g2_uncompressed(lem)


def g1_from_be(be):
    """-> file form; ValueError for what the format refuses (flags, a coordinate >= q, off the curve)."""
    if be[0] & 0xc0:
        if be != G1_INF_BE:
            raise ValueError("mpcparams: Invalid File format")
        return bytes(64)
    x, y = int.from_bytes(be[:32], "big"), int.from_bytes(be[32:], "big")
    if x >= Q or y >= Q or not b.G1.on_curve((x, y)):
        raise ValueError("mpcparams: Invalid File format")
    return f.g1_to_lem((x, y))


def run_be(data, psz):
    conv = g1_be if psz == 64 else g2_be
    return b"".join(conv(data[i:i + psz]) for i in range(0, len(data), psz))


def key_sections(zkey):
    secs = f.read_binfile(zkey, "zkey", 2)
    return {sid: f.section(zkey, secs, sid) for sid in secs}


def record_be(rec):
    return mref.hash_pubkey_feed(rec)


def write_mpcparams(sec, h_be):
    """The image of a key's sections with the given H run (big-endian images, N - 1 of them)."""
    h = sec[2]
    at = HDR_ALPHA1
    out = [g1_be(h[at:at + 64]), g1_be(h[at + 64:at + 128]), g2_be(h[at + 128:at + 256]), g2_be(h[at + 256:at + 384]),
           g1_be(h[mref.HDR_DELTA1:mref.HDR_DELTA1 + 64]), g2_be(h[mref.HDR_DELTA2:mref.HDR_DELTA2 + 128])]
    for name in RUNS:
        data = h_be if name == "H" else run_be(sec[RUN_SECTION[name]], RUN_POINT[name])
        out.append(struct.pack(">I", len(data) // RUN_POINT[name]) + data)
    cs, recs = mref.parse_section10(sec[10])
    out.append(cs + struct.pack(">I", len(recs)) + b"".join(record_be(r) for r in recs))
    return b"".join(out)


def parse_mpcparams(buf):
    """-> dict: header (576 bytes), the six runs (bytes), csHash, records (384 bytes each), and `at`: name -> offset."""
    out = {"header": buf[:HEADER], "at": {}}
    pos = HEADER
    for name in RUNS:
        n = struct.unpack_from(">I", buf, pos)[0]
        out["at"][name] = pos
        out[name] = buf[pos + 4:pos + 4 + n * RUN_POINT[name]]
        pos += 4 + n * RUN_POINT[name]
    out["csHash"] = buf[pos:pos + 64]
    out["at"]["csHash"] = pos
    c = struct.unpack_from(">I", buf, pos + 64)[0]
    pos += 68
    out["at"]["records"] = pos
    out["records"] = [buf[pos + i * RECORD:pos + (i + 1) * RECORD] for i in range(c)]
    assert pos + c * RECORD == len(buf)
    return out
