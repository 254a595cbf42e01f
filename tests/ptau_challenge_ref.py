"""Python twin of the phase-1 challenge / response exchange (csrc/ptau_mpc.cpp, csrc/ptau_points.hip), written from the
description of the file formats and not from the C++: the compressed and uncompressed point codecs, and export /
contribute / import built on ptau_mpc_ref and the oracle (pure-Python points, small powers only).

  challenge file  prev (64) | every point of sections 2-6, uncompressed big-endian            384 n + 128 bytes
  response file   challenge hash (64) | the same points compressed | nine key points uncompressed   192 n + 864 bytes
  compressed      x big-endian (G2: c1 | c0); 0x40 of byte 0 = infinity, 0x80 = y "negative" (f2_negative's rule)"""
import struct

import bn254 as b
import formats as f
from bn254 import Q
from ptau_mpc_ref import (KEYS, PSZ, challenge_hash, first_challenge, generator_sections, key_points, parse_section7, points_feed,
                          response_hash, scaled_sections, write_record)
from ptau_prepared import sections
from zkey_mpc_ref import _fq_sqrt, blake2b, f2_negative, f2_sqrt, g1_uncompressed, g2_uncompressed

KEYS_BYTES = 6 * 64 + 3 * 128


def _be(x):
    return int(x).to_bytes(32, "big")


def rhs_g1(x):
    return (x * x * x + 3) % Q


def rhs_g2(x):
    return b.f2_add(b.f2_mul(b.f2_sqr(x), x), b.G2_B)


# ------------------------------------------------------------------ point codecs (file image <-> the files' forms)
def compress(lem):
    """File image (64 / 128 bytes) -> compressed (32 / 64 bytes)."""
    if len(lem) == 64:
        P = f.g1_from_lem(lem)
        if P is None:
            return bytes([0x40]) + bytes(31)
        out, neg = bytearray(_be(P[0])), P[1] > (Q - 1) // 2
    else:
        P = f.g2_from_lem(lem)
        if P is None:
            return bytes([0x40]) + bytes(63)
        out, neg = bytearray(_be(P[0][1]) + _be(P[0][0])), f2_negative(P[1])
    if neg:
        out[0] |= 0x80
    return bytes(out)


def decompress(c):
    """Compressed (32 / 64 bytes) -> file image, or None when the image is not a point: a 0x40 flag with anything else
    set, x >= q, x^3 + b without a root."""
    flags, body = c[0] & 0xc0, bytes([c[0] & 0x3f]) + c[1:]
    if flags & 0x40:
        return bytes(2 * len(c)) if flags == 0x40 and not any(body) else None
    neg = bool(flags & 0x80)
    if len(c) == 32:
        x = int.from_bytes(body, "big")
        y = None if x >= Q else _fq_sqrt(rhs_g1(x))
        if y is None:
            return None
        return f.g1_to_lem((x, -y % Q if (y > (Q - 1) // 2) != neg else y))
    x = (int.from_bytes(body[32:], "big"), int.from_bytes(body[:32], "big"))
    y = None if max(x) >= Q else f2_sqrt(rhs_g2(x))
    if y is None:
        return None
    return f.g2_to_lem((x, b.f2_neg(y) if f2_negative(y) != neg else y))


def from_be(u):
    """Uncompressed big-endian (64 / 128 bytes) -> file image, or None: a set 0x80, a 0x40 flag with anything else set,
    a coordinate >= q, a point off its curve."""
    if u[0] & 0xc0:
        return bytes(len(u)) if u[0] == 0x40 and not any(u[1:]) else None
    w = [int.from_bytes(u[i:i + 32], "big") for i in range(0, len(u), 32)]
    if max(w) >= Q:
        return None
    if len(u) == 64:
        return f.g1_to_lem((w[0], w[1])) if w[1] * w[1] % Q == rhs_g1(w[0]) else None
    x, y = (w[1], w[0]), (w[3], w[2])
    return f.g2_to_lem((x, y)) if b.f2_sqr(y) == rhs_g2(x) else None


def _run(data, psz, fn):
    out = [fn(data[i:i + psz]) for i in range(0, len(data), psz)]
    if None in out:
        raise ValueError("point %d is not a point of the curve" % out.index(None))
    return b"".join(out)


def keys_uncompressed(rec):
    return (b"".join(g1_uncompressed(rec[k + ".g1_s"]) + g1_uncompressed(rec[k + ".g1_sx"]) for k in KEYS) +
            b"".join(g2_uncompressed(rec[k + ".g2_spx"]) for k in KEYS))


def _counts(n):
    return {2: 2 * n - 1, 3: n, 4: n, 5: n, 6: 1}


# ------------------------------------------------------------------ the three commands
def export_challenge_ref(ptau):
    """-> the challenge file; its Blake2b-512 is the challenge the next contribution answers."""
    secs = dict(sections(ptau))
    power = struct.unpack_from("<I", secs[1], 36)[0]
    recs = parse_section7(secs[7]) if 7 in secs else []
    if not recs:
        prev = blake2b(b"")
    else:
        answered = recs[-2]["nextChallenge"] if len(recs) > 1 else first_challenge(generator_sections(power))
        prev = response_hash(answered, recs[-1])
    return prev + points_feed(secs)


def challenge_contribute_ref(challenge_file, secret):
    """-> (the response file, the contribution hash).  secret = (tau, alpha, beta, s_tau, s_alpha, s_beta)."""
    n = (len(challenge_file) - 128) // 384
    if n < 2 or n & (n - 1) or len(challenge_file) != 384 * n + 128:
        raise ValueError("ptau challenge: Invalid File format")
    power, secs, at = n.bit_length() - 1, {}, 64
    for sid, cnt in _counts(n).items():
        secs[sid] = _run(challenge_file[at:at + cnt * PSZ[sid]], PSZ[sid], from_be)
        at += cnt * PSZ[sid]
    challenge = blake2b(challenge_file)
    rec = key_points(challenge, secret)
    new = scaled_sections(secs, power, secret[0], secret[1], secret[2])
    body = b"".join(_run(new[sid], PSZ[sid], compress) for sid in (2, 3, 4, 5, 6))
    return challenge + body + keys_uncompressed(rec), response_hash(challenge, rec)


def import_response_ref(ptau, response, name):
    """-> (the file `powersoftau import response` must write, the contribution hash); the record's pairing checks are
    left to ptau_mpc_ref.verify_ref."""
    secs = dict(sections(ptau))
    power = struct.unpack_from("<I", secs[1], 36)[0]
    n = 1 << power
    recs = parse_section7(secs[7]) if 7 in secs else []
    old7 = secs.get(7, struct.pack("<I", 0))
    if power < 1 or len(response) != 192 * n + 864:
        raise ValueError("ptau import response: Invalid File format")
    challenge = recs[-1]["nextChallenge"] if recs else first_challenge(secs)
    if response[:64] != challenge:
        raise ValueError("ptau import response: the response does not answer this file's challenge")
    new, at = {}, 64
    for sid, cnt in _counts(n).items():
        new[sid] = _run(response[at:at + cnt * PSZ[sid] // 2], PSZ[sid] // 2, decompress)
        at += cnt * PSZ[sid] // 2
    rec, tail = {}, response[-KEYS_BYTES:]
    for x, k in enumerate(KEYS):
        rec[k + ".g1_s"], rec[k + ".g1_sx"] = from_be(tail[128 * x:128 * x + 64]), from_be(tail[128 * x + 64:128 * x + 128])
        rec[k + ".g2_spx"] = from_be(tail[384 + 128 * x:512 + 128 * x])
    if None in rec.values():
        raise ValueError("ptau import response: a key point is not a valid image")
    rec["tauG1"], rec["tauG2"] = new[2][64:128], new[3][128:256]
    rec["alphaG1"], rec["betaG1"], rec["betaG2"] = new[4][:64], new[5][:64], new[6]
    resp_hash = response_hash(challenge, rec)
    rec["nextChallenge"] = challenge_hash(new, resp_hash)
    s7 = struct.pack("<I", len(recs) + 1) + old7[4:] + write_record(rec, name)
    out = f.write_binfile("ptau", 1, [(1, secs[1])] + [(sid, new[sid]) for sid in (2, 3, 4, 5, 6)] + [(7, s7)])
    return out, resp_hash
