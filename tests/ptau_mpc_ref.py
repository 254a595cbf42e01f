"""Python twin of the phase-1 ceremony pieces (csrc/ptau_mpc.cpp), written from their description and not from the C++:
the section-7 record codec, the challenge and response hashes (hashlib.blake2b), contribute_ref -- the whole file a
contribution must produce, pure-Python points, small powers only -- and verify_ref, the record walk of the verifier
through the oracle's pairing.  hash_to_g2, same_ratio and the uncompressed images come from zkey_mpc_ref."""
import struct

import bn254 as b
import formats as f
from bn254 import R
from ptau_prepared import sections
from zkey_mpc_ref import blake2b, g1_uncompressed, g2_uncompressed, hash_to_g2, name_params, same_ratio

REC_FIXED = 1432 + 64 + 4 + 4
STATE = [("tauG1", 64), ("tauG2", 128), ("alphaG1", 64), ("betaG1", 64), ("betaG2", 128)]
KEYS = ("tau", "alpha", "beta")
G1_LEM, G2_LEM = f.g1_to_lem(b.G1_GEN), f.g2_to_lem(b.G2_GEN)
PSZ = {2: 64, 3: 128, 4: 64, 5: 64, 6: 128}


# ------------------------------------------------------------------ section 7
def parse_section7(s7):
    """-> [record dict]; ValueError on a section shorter than its records say or with trailing bytes."""
    if len(s7) < 4:
        raise ValueError("ptau: Invalid File format")
    n = struct.unpack_from("<I", s7, 0)[0]
    pos, recs = 4, []
    for _ in range(n):
        if len(s7) - pos < REC_FIXED:
            raise ValueError("ptau: Invalid File format")
        typ, plen = struct.unpack_from("<II", s7, pos + 1496)
        if len(s7) - pos - REC_FIXED < plen:
            raise ValueError("ptau: Invalid File format")
        r = s7[pos:pos + REC_FIXED + plen]
        rec, at = {"raw": r, "type": typ, "params": r[REC_FIXED:]}, 0
        for name, size in STATE:
            rec[name] = r[at:at + size]
            at += size
        for k in KEYS:
            rec[k + ".g1_s"], rec[k + ".g1_sx"] = r[at:at + 64], r[at + 64:at + 128]
            at += 128
        for k in KEYS:
            rec[k + ".g2_spx"] = r[at:at + 128]
            at += 128
        rec["partialHash"], rec["nextChallenge"] = r[at:at + 216], r[at + 216:at + 280]
        recs.append(rec)
        pos += REC_FIXED + plen
    if pos != len(s7):
        raise ValueError("ptau: Invalid File format")
    return recs


def write_record(rec, name=None, typ=0):
    params = name_params(name)
    out = b"".join(rec[n] for n, _ in STATE)
    out += b"".join(rec[k + ".g1_s"] + rec[k + ".g1_sx"] for k in KEYS)
    out += b"".join(rec[k + ".g2_spx"] for k in KEYS)
    return out + bytes(216) + rec["nextChallenge"] + struct.pack("<II", typ, len(params)) + params


# ------------------------------------------------------------------ hashing
def points_feed(secs):
    """Every point of sections 2, 3, 4, 5, 6 in that order, uncompressed big-endian standard form."""
    out = []
    for sid in (2, 3, 4, 5, 6):
        d, psz = secs[sid], PSZ[sid]
        unc = g1_uncompressed if psz == 64 else g2_uncompressed
        out += [unc(d[i:i + psz]) for i in range(0, len(d), psz)]
    return b"".join(out)


def challenge_hash(secs, prev):
    return blake2b(prev + points_feed(secs))


def first_challenge(secs):
    return challenge_hash(secs, blake2b(b""))


def generator_sections(power):
    n = 1 << power
    return {2: G1_LEM * (2 * n - 1), 3: G2_LEM * n, 4: G1_LEM * n, 5: G1_LEM * n, 6: G2_LEM}


def key_g2_sp(challenge, x, g1_s, g1_sx):
    return hash_to_g2(blake2b(challenge + bytes([x]) + g1_uncompressed(g1_s) + g1_uncompressed(g1_sx)))


def response_hash(challenge, rec):
    return blake2b(challenge + b"".join(g1_uncompressed(rec[k + ".g1_s"]) + g1_uncompressed(rec[k + ".g1_sx"]) for k in KEYS) +
                   b"".join(g2_uncompressed(rec[k + ".g2_spx"]) for k in KEYS))


# ------------------------------------------------------------------ the contribution
def _scale(data, psz, scalars):
    grp, dec, enc = (b.G1, f.g1_from_lem, f.g1_to_lem) if psz == 64 else (b.G2, f.g2_from_lem, f.g2_to_lem)
    out = []
    for i, k in enumerate(scalars):
        P = dec(data[i * psz:(i + 1) * psz])
        out.append(enc(None if P is None or k % R == 0 else grp.mul(P, k % R)))
    return b"".join(out)


def scaled_sections(secs, power, tau, alpha, beta):
    """Sections 2-6 after a contribution (tau, alpha, beta), by one multiplication per point."""
    n = 1 << power
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    return {2: _scale(secs[2], 64, pw), 3: _scale(secs[3], 128, pw[:n]), 4: _scale(secs[4], 64, [alpha * x % R for x in pw[:n]]),
            5: _scale(secs[5], 64, [beta * x % R for x in pw[:n]]), 6: _scale(secs[6], 128, [beta])}


def key_points(challenge, secret):
    """The nine key points of a record (file form) for secret = (tau, alpha, beta, s_tau, s_alpha, s_beta)."""
    rec = {}
    for x, k in enumerate(KEYS):
        g1_s = b.G1.mul(b.G1_GEN, secret[3 + x])
        g1_sx = b.G1.mul(g1_s, secret[x])
        rec[k + ".g1_s"], rec[k + ".g1_sx"] = f.g1_to_lem(g1_s), f.g1_to_lem(g1_sx)
        rec[k + ".g2_spx"] = f.g2_to_lem(b.G2.mul(key_g2_sp(challenge, x, rec[k + ".g1_s"], rec[k + ".g1_sx"]), secret[x]))
    return rec


def contribute_ref(ptau, name, secret):
    """-> (the file `powersoftau contribute` must write, the contribution hash).  secret = (tau, alpha, beta, s_tau,
    s_alpha, s_beta)."""
    secs = dict(sections(ptau))
    power = struct.unpack_from("<I", secs[1], 36)[0]
    recs = parse_section7(secs[7]) if 7 in secs else []
    old7 = secs.get(7, struct.pack("<I", 0))
    challenge = recs[-1]["nextChallenge"] if recs else first_challenge(secs)
    rec = key_points(challenge, secret)
    new = scaled_sections(secs, power, secret[0], secret[1], secret[2])
    if power >= 1:
        rec["tauG1"], rec["tauG2"] = new[2][64:128], new[3][128:256]
    else:
        rec["tauG1"] = _scale(recs[-1]["tauG1"] if recs else G1_LEM, 64, [secret[0]])
        rec["tauG2"] = _scale(recs[-1]["tauG2"] if recs else G2_LEM, 128, [secret[0]])
    rec["alphaG1"], rec["betaG1"], rec["betaG2"] = new[4][:64], new[5][:64], new[6]
    response = response_hash(challenge, rec)
    rec["nextChallenge"] = challenge_hash(new, response)
    s7 = struct.pack("<I", len(recs) + 1) + old7[4:] + write_record(rec, name)
    out = f.write_binfile("ptau", 1, [(1, secs[1])] + [(sid, new[sid]) for sid in (2, 3, 4, 5, 6)] + [(7, s7)])
    return out, response


# ------------------------------------------------------------------ the record walk
def verify_ref(ptau):
    """Checks 1 to 4 of the verifier: the first powers, the record walk, the file's points against the last record and
    its challenge hash.  The powers (check 5) and the prepared sections (check 6) are left out."""
    secs = dict(sections(ptau))
    power = struct.unpack_from("<I", secs[1], 36)[0]
    recs = parse_section7(secs[7]) if 7 in secs else []
    if secs[2][:64] != G1_LEM or secs[3][:128] != G2_LEM:
        return False
    cur = {"tau": b.G1_GEN, "alpha": b.G1_GEN, "beta": b.G1_GEN}
    challenge = None
    for i, r in enumerate(recs):
        challenge = first_challenge(generator_sections(power)) if i == 0 else recs[i - 1]["nextChallenge"]
        for x, k in enumerate(KEYS):
            sp = key_g2_sp(challenge, x, r[k + ".g1_s"], r[k + ".g1_sx"])
            spx = f.g2_from_lem(r[k + ".g2_spx"])
            now = f.g1_from_lem(r[k + "G1"])
            if not same_ratio(f.g1_from_lem(r[k + ".g1_s"]), f.g1_from_lem(r[k + ".g1_sx"]), sp, spx):
                return False
            if not same_ratio(cur[k], now, sp, spx):
                return False
            cur[k] = now
        for k in ("tau", "beta"):
            if not same_ratio(b.G1_GEN, f.g1_from_lem(r[k + "G1"]), b.G2_GEN, f.g2_from_lem(r[k + "G2"])):
                return False
    if not recs:
        return all(secs[sid] == d for sid, d in generator_sections(power).items())
    last = recs[-1]
    if (last["alphaG1"], last["betaG1"], last["betaG2"]) != (secs[4][:64], secs[5][:64], secs[6]):
        return False
    if power >= 1 and (last["tauG1"], last["tauG2"]) != (secs[2][64:128], secs[3][128:256]):
        return False
    return challenge_hash(secs, response_hash(challenge, last)) == last["nextChallenge"]
