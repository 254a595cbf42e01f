"""Python twin of the beacon pieces (csrc/beacon.h, mpc_beacon_scalars in csrc/zkey_mpc.cpp), written from their
description and not from the C++: the delay function over hashlib.sha256, the secret scalars over the ChaCha of
tests/zkey_mpc_ref.py, and the builder and the walker of a beacon record's params.  The derivation of the scalars is
this library's own rule, as the CLI's `-e` rule is: it is NOT snarkjs's."""
import hashlib
import struct

from bn254 import R
from zkey_mpc_ref import ChaCha, name_params

EXP_MIN, EXP_MAX = 10, 63


def chain(beacon, exp):
    """h_0 = beacon, h_(i+1) = SHA-256(h_i) -> h at i = 2^exp (32 bytes)."""
    h = bytes(beacon)
    for _ in range(1 << exp):
        h = hashlib.sha256(h).digest()
    return h


def scalars(beacon, exp, count):
    """count draws below r of ONE ChaCha20 stream keyed with the seed as eight big-endian words; zero maps to 1.
    6: (tau, alpha, beta, s_tau, s_alpha, s_beta); 2: (d, s)."""
    rng = ChaCha(struct.unpack(">8I", chain(beacon, exp)))
    return tuple(rng.field(R) or 1 for _ in range(count))


def params(name, beacon, exp):
    """ids ascending: the name's block if any, then 2 | e, then 3 | len | beacon."""
    return name_params(name) + bytes([2, exp, 3, len(beacon)]) + bytes(beacon)


def walk(p):
    """snarkjs's reader: ids 1 (len, name), 2 (e), 3 (len, hash), strictly ascending, nothing else, nothing cut short.
    -> (exp, beacon) when the block states a beacon (both found, e in range, the hash not empty), else None."""
    found, last, i = {}, 0, 0
    while i < len(p):
        pid = p[i]
        if pid <= last or pid > 3 or len(p) - i < 2:
            return None
        last = pid
        if pid == 2:
            found[2] = p[i + 1]
            i += 2
            continue
        n = p[i + 1]
        if len(p) - i - 2 < n:
            return None
        found[pid] = bytes(p[i + 2:i + 2 + n])
        i += 2 + n
    if 2 not in found or 3 not in found or not found[3] or not EXP_MIN <= found[2] <= EXP_MAX:
        return None
    return found[2], found[3]
