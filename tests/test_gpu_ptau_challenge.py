"""The phase-1 challenge / response exchange on the device (csrc/ptau_points.hip, csrc/ptau_mpc.cpp).  Layer: the three
point kernels and the square-root routine against the Python twin (tests/ptau_challenge_ref.py), byte for byte, across
chunk and grid tails, with every kind of bad image reported at its index.  Commands: import(old, contribute(export(old),
secret), name) is ptau_contribute(old, name, secret) byte for byte; chained exchanges verify; a tampered response gets the
text of the check it fails and writes nothing."""
import random

import pytest

import bn254 as b
import formats as f
from bn254 import Q, R
from ptau_challenge_ref import (KEYS_BYTES, challenge_contribute_ref, compress, decompress, export_challenge_ref, from_be,
                                import_response_ref, rhs_g1, rhs_g2)
from ptau_prepare_ref import split
from ptau_prepared import rewrite
from zkey_mpc_ref import _fq_sqrt, f2_sqrt, g1_uncompressed, g2_uncompressed

pytestmark = pytest.mark.gpu

PSZ = {1: 64, 2: 128}


def _secret(seed):
    return tuple(pow(seed + 2 + i, 1000 + 7 * i + seed, R) for i in range(6))


# ------------------------------------------------------------------ layer: the point kernels
def _random_points(group, count, rng):
    """File images of `count` random points of the curve (G2: of the twist, not necessarily of the subgroup)."""
    out = []
    while len(out) < count:
        if group == 1:
            x = rng.randrange(Q)
            y = _fq_sqrt(rhs_g1(x))
            if y is not None:
                out.append(f.g1_to_lem((x, y)))
        else:
            x = (rng.randrange(Q), rng.randrange(Q))
            y = f2_sqrt(rhs_g2(x))
            if y is not None:
                out.append(f.g2_to_lem((x, y)))
    return out


def _negated(group, lem):
    if group == 1:
        x, y = f.g1_from_lem(lem)
        return f.g1_to_lem((x, -y % Q))
    x, y = f.g2_from_lem(lem)
    return f.g2_to_lem((x, b.f2_neg(y)))


@pytest.fixture(scope="module")
def points():
    """Per group: 300 random points and their opposites (both signs of every x), infinity first, in the middle and last;
    with the twin's compressed and uncompressed images."""
    out = {}
    for group in (1, 2):
        rng = random.Random(1000 + group)
        pos = _random_points(group, 300, rng)
        lem = [bytes(PSZ[group])] + pos[:150] + [_negated(group, p) for p in pos[:150]] + [bytes(PSZ[group])] + pos[150:] + \
              [_negated(group, p) for p in pos[150:]] + [bytes(PSZ[group])]
        unc = g1_uncompressed if group == 1 else g2_uncompressed
        out[group] = {"lem": lem, "comp": [compress(p) for p in lem], "be": [unc(p) for p in lem]}
        assert len(lem) == 603 and len({c[0] & 0x80 for c in out[group]["comp"]}) == 2
    return out


@pytest.mark.parametrize("env,count", [({}, 603), ({"G16_PTAU_CHUNK": "37", "G16_PTAU_LANES": "64"}, 603),
                                       ({"G16_PTAU_CHUNK": "603"}, 603), ({"G16_PTAU_CHUNK": "201"}, 603),
                                       ({"G16_PTAU_CHUNK": "302"}, 603), ({"G16_PTAU_CHUNK": "1"}, 5)],
                         ids=["default", "chunk37_lanes64", "chunk603", "chunk201", "chunk302", "first5_chunk1"])
@pytest.mark.parametrize("group", [1, 2])
def test_compress_then_decompress_is_the_identity_and_the_twin(amd, points, group, env, count, monkeypatch):
    """603 points: with chunks of 37 on 64 lanes, 16 full chunks and a tail of 11, every chunk ending mid-wavefront.  The
    chunk-count edges of the two buffer sets: chunks of 603, one full chunk on a single set; of 201, three full chunks
    without a tail, the first reuse of set 0; of 302, two chunks (302 + 301) and no reuse; the first five points one to
    a chunk, every set reused twice."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = {k: v[:count] for k, v in points[group].items()}
    lem = b"".join(p["lem"])
    comp, bad, _ = amd.ptau_points_compress(group, lem)
    assert bad == -1 and comp == b"".join(p["comp"])
    back, bad, _, be = amd.ptau_points_decompress(group, comp)
    assert bad == -1 and back == lem and be == b"".join(p["be"])
    assert amd.ptau_points_decompress(group, comp, want_be=False)[:2] == (lem, -1)
    again, bad, _ = amd.ptau_points_from_be(group, be)
    assert bad == -1 and again == lem


def _no_root(group, rng):
    while True:
        if group == 1:
            x = rng.randrange(Q)
            if _fq_sqrt(rhs_g1(x)) is None:
                return x.to_bytes(32, "big")
        else:
            x = (rng.randrange(Q), rng.randrange(Q))
            if f2_sqrt(rhs_g2(x)) is None:
                return x[1].to_bytes(32, "big") + x[0].to_bytes(32, "big")


@pytest.mark.parametrize("group", [1, 2])
def test_decompress_at_the_largest_x(amd, points, group):
    """x = q - 1, the last value below the range check (G2: c0 = c1 = q - 1).  On G1 x^3 + 3 = 2 there, and 2 IS a square
    (q = 7 mod 8): the image is a point and must come out as the twin's, for both flags; x = q right above it is
    refused.  On G2 the twin says which it is."""
    half, comp = PSZ[group] // 2, points[group]["comp"]
    img = (Q - 1).to_bytes(32, "big") * group
    want = decompress(img)
    assert group == 2 or want is not None
    for flag in (0, 0x80):
        flagged = bytes([img[0] | flag]) + img[1:]
        out, bad, _, _ = amd.ptau_points_decompress(group, b"".join(comp[:36] + [flagged] + comp[37:]), want_be=False)
        if want is None:
            assert bad == 36
        else:
            assert bad == -1 and out[36 * 2 * half:37 * 2 * half] == decompress(flagged) and compress(decompress(flagged)) == flagged
    over = bytes(half - 32) + Q.to_bytes(32, "big")
    assert amd.ptau_points_decompress(group, b"".join(comp[:36] + [over] + comp[37:]), want_be=False)[1] == 36


@pytest.mark.parametrize("small", [False, True], ids=["default", "chunk37_lanes64"])
@pytest.mark.parametrize("group", [1, 2])
def test_decompress_rejects_bad_images_at_their_index(amd, points, group, small, monkeypatch):
    if small:
        monkeypatch.setenv("G16_PTAU_CHUNK", "37")
        monkeypatch.setenv("G16_PTAU_LANES", "64")
    half, comp = PSZ[group] // 2, points[group]["comp"]
    bads = {"x = q": bytes(half - 32) + Q.to_bytes(32, "big"),
            "no root": _no_root(group, random.Random(3)),
            "0x40 with a stray byte": bytes([0x40]) + bytes(half - 2) + b"\1",
            "0x40 and 0x80": bytes([0xc0]) + bytes(half - 1)}
    if group == 2:
        bads["x.c1 = q"] = Q.to_bytes(32, "big") + comp[5][32:]
    for k, (name, img) in enumerate(bads.items()):
        assert decompress(img) is None, name
        at = (0, 36, 37, 300, 591, 602)[k % 6]
        got = amd.ptau_points_decompress(group, b"".join(comp[:at] + [img] + comp[at + 1:]), want_be=False)
        assert got[1] == at, (name, at, got[1])
    # the smallest index wins, whichever chunk finishes first
    two = list(comp)
    two[590], two[75] = bads["x = q"], bads["no root"]
    assert amd.ptau_points_decompress(group, b"".join(two), want_be=False)[1] == 75
    two[3] = bads["0x40 with a stray byte"]
    assert amd.ptau_points_decompress(group, b"".join(two), want_be=False)[1] == 3


@pytest.mark.parametrize("group", [1, 2])
def test_from_be_rejects_bad_images_at_their_index(amd, points, group, monkeypatch):
    monkeypatch.setenv("G16_PTAU_CHUNK", "37")
    monkeypatch.setenv("G16_PTAU_LANES", "64")
    size, be = PSZ[group], points[group]["be"]
    good = be[7]
    bads = {"y >= q": good[:size - 32] + Q.to_bytes(32, "big"),
            "x >= q": (Q + 2).to_bytes(32, "big") + good[32:],
            "off the curve": good[:-1] + bytes([good[-1] ^ 1]),
            "a set 0x80": bytes([good[0] | 0x80]) + good[1:],
            "0x40 with a stray byte": bytes([0x40]) + bytes(size - 2) + b"\1",
            "zeros without the flag": bytes(size)}
    for k, (name, img) in enumerate(bads.items()):
        assert from_be(img) is None, name
        at = (0, 36, 37, 299, 591, 602)[k]
        assert amd.ptau_points_from_be(group, b"".join(be[:at] + [img] + be[at + 1:]))[1] == at, name
    two = list(be)
    two[400], two[41] = bads["y >= q"], bads["off the curve"]
    assert amd.ptau_points_from_be(group, b"".join(two))[1] == 41


# ------------------------------------------------------------------ layer: the square roots
def test_fq_sqrt_batch(amd):
    rng = random.Random(11)
    squares = [pow(rng.randrange(1, Q), 2, Q) for _ in range(200)]
    others = []
    while len(others) < 200:
        v = rng.randrange(1, Q)
        if _fq_sqrt(v) is None:
            others.append(v)
    values = [0, 1, Q - 1] + squares + others
    got = amd.fq_sqrt_batch(0, values)
    for v, r in zip(values, got):
        assert (r is not None) == (_fq_sqrt(v) is not None), v
        assert r is None or r * r % Q == v
    assert got[0] == 0 and got[2] is None and all(r is not None for r in got[3:203]) and not any(got[203:])


def test_fq2_sqrt_batch(amd, monkeypatch):
    """The cases a curve point cannot reach: c1 = 0 (with c0 a residue: root (r, 0); a non-residue: root (0, r)), squares
    of (0, c1), zero -- beside general squares and non-residues; over several chunks."""
    monkeypatch.setenv("G16_PTAU_CHUNK", "37")
    monkeypatch.setenv("G16_PTAU_LANES", "64")
    rng = random.Random(12)
    values = [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1)]
    values += [b.f2_sqr((rng.randrange(1, Q), 0)) for _ in range(20)]
    values += [b.f2_sqr((0, rng.randrange(1, Q))) for _ in range(20)]
    values += [b.f2_sqr((rng.randrange(Q), rng.randrange(1, Q))) for _ in range(60)]
    non_residues = [v for v in (rng.randrange(1, Q) for _ in range(60)) if _fq_sqrt(v) is None][:20]
    assert len(non_residues) == 20
    squares = len(values)
    values += [(v, 0) for v in non_residues]                      # a0 a non-residue of Fq: the root is (0, r)
    values += [(rng.randrange(Q), rng.randrange(1, Q)) for _ in range(80)]
    got = amd.fq_sqrt_batch(1, values)
    for v, r in zip(values, got):
        assert (r is not None) == (f2_sqrt(v) is not None), v
        assert r is None or b.f2_sqr(r) == v, v
    assert squares == 105 and all(r is not None for r in got[:squares + 20])
    assert all(r[0] == 0 and r[1] != 0 for r in got[squares:squares + 20])
    assert 0 < sum(r is None for r in got[-80:]) < 80
    with pytest.raises(amd.G16Error) as e:
        amd.fq_sqrt_batch(1, [(1, Q)])
    assert e.value.code == -1


# ------------------------------------------------------------------ commands: the defining property
def _exchange(amd, old, name, secret):
    challenge = amd.ptau_export_challenge(old)
    response, h = amd.ptau_challenge_contribute(challenge, secret, device=0)
    new, h2 = amd.ptau_import_response(old, response, name, device=0)
    return new, h, h2, response


def _cases(amd, power):
    n = 1 << power
    p0 = amd.ptau_new(power)
    one = amd.ptau_contribute(p0, "before", _secret(200 + power), device=0)[0]

    def holes(sid, d):        # infinity inputs, away from the points a record is made of
        at = {2: 2 * n - 2, 4: n - 1, 5: n - 1}.get(sid)
        return d if at is None else d[:at * 64] + bytes(64) + d[(at + 1) * 64:]
    return {"generator": p0, "one_record": one, "prepared": amd.ptau_prepare(one, device=0), "infinity_inputs": rewrite(p0, holes)}


@pytest.mark.parametrize("case", ["generator", "one_record", "prepared", "infinity_inputs"])
@pytest.mark.parametrize("power", [1, 2, 3])
def test_exchange_equals_contribute_byte_for_byte(amd, power, case):
    old, s = _cases(amd, power)[case], _secret(210 + power)
    want, wh = amd.ptau_contribute(old, "exchanged", s, device=0)
    got, h, h2, _ = _exchange(amd, old, "exchanged", s)
    assert got == want and h == wh and h2 == wh
    assert split(got)[0] == [1, 2, 3, 4, 5, 6, 7]


def test_exchange_equals_contribute_at_power_12_across_chunks(amd, monkeypatch):
    old, s = amd.ptau_contribute(amd.ptau_new(12), "before", _secret(231), device=0)[0], _secret(232)
    want = amd.ptau_contribute(old, None, s, device=0)
    monkeypatch.setenv("G16_PTAU_CHUNK", "1000")
    got, h, h2, _ = _exchange(amd, old, None, s)
    assert (got, h) == want and h2 == h


@pytest.mark.parametrize("power", [1, 2, 3])
def test_response_and_import_equal_the_twin(amd, power):
    s = _secret(240 + power)
    old = amd.ptau_contribute(amd.ptau_new(power), "before", _secret(250), device=0)[0]
    challenge = amd.ptau_export_challenge(old)
    assert challenge == export_challenge_ref(old)
    response, h = amd.ptau_challenge_contribute(challenge, s, device=0)
    assert (response, h) == challenge_contribute_ref(challenge, s)
    assert amd.ptau_import_response(old, response, "twin", device=0) == import_response_ref(old, response, "twin")


def test_two_chained_exchanges_verify_and_prepare(amd):
    p = amd.ptau_new(4)
    for k in range(2):
        p = _exchange(amd, p, "contributor %d" % k, _secret(260 + k))[0]
    assert amd.ptau_verify(p, device=0) == (True, "")
    prep = amd.ptau_prepare(p, device=0)
    assert split(prep)[0] == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    assert amd.ptau_verify(prep, device=0) == (True, "")
    # the OS CSPRNG gives another response, and that one imports too
    r1 = amd.ptau_challenge_contribute(amd.ptau_export_challenge(p), None, device=0)[0]
    r2 = amd.ptau_challenge_contribute(amd.ptau_export_challenge(p), None, device=0)[0]
    assert r1 != r2 and amd.ptau_verify(amd.ptau_import_response(p, r1, None, device=0)[0], device=0) == (True, "")


def test_challenge_contribute_names_the_first_bad_point(amd):
    challenge = amd.ptau_export_challenge(amd.ptau_new(3))
    at = 64 + 15 * 64 + 5 * 128                       # point 5 of section 3
    bad = challenge[:at + 127] + bytes([challenge[at + 127] ^ 1]) + challenge[at + 128:]
    at4 = 64 + 15 * 64 + 8 * 128 + 2 * 64            # and point 2 of section 4: the earlier section is named
    bad = bad[:at4] + bytes([bad[at4] | 0x80]) + bad[at4 + 1:]
    with pytest.raises(amd.G16Error) as e:
        amd.ptau_challenge_contribute(bad, _secret(270), device=0)
    assert e.value.code == -2 and str(e.value) == "ptau challenge contribute: point 5 of section 3 is not a point of the curve"


# ------------------------------------------------------------------ commands: tampered responses
@pytest.fixture(scope="module")
def honest(amd):
    """Power 3 on top of one record: the old file, an honest response, and one to the same challenge with another tau."""
    old = amd.ptau_contribute(amd.ptau_new(3), "before", _secret(280), device=0)[0]
    s = _secret(281)
    challenge = amd.ptau_export_challenge(old)
    response = amd.ptau_challenge_contribute(challenge, s, device=0)[0]
    other = amd.ptau_challenge_contribute(challenge, (s[0] + 1,) + s[1:], device=0)[0]
    return old, response, other


def _refused(amd, tmp_path, old, response, text):
    """The verdict through the buffer form, then through the file form: no output file, the old file's bytes as they were."""
    import ctypes
    with pytest.raises(amd.G16Error) as e:
        amd.ptau_import_response(old, response, "tampered", device=0)
    assert e.value.code == 0 and str(e.value) == "ptau import response: " + text, str(e.value)
    lib = amd.load()
    (tmp_path / "old.ptau").write_bytes(old)
    (tmp_path / "response").write_bytes(response)
    ok, out = ctypes.c_int(7), tmp_path / "new.ptau"
    rc = lib.g16_ptau_import_response_files(str(tmp_path / "old.ptau").encode(), str(tmp_path / "response").encode(), str(out).encode(),
                                            b"tampered", 0, None, ctypes.byref(ok))
    assert rc == 0 and ok.value == 0 and lib.g16_last_error().decode() == "ptau import response: " + text
    assert not out.exists() and (tmp_path / "old.ptau").read_bytes() == old


def test_import_accepts_a_flipped_sign_and_verify_names_the_section(amd, honest):
    old, response, _ = honest
    at = 64 + 4 * 32                                   # point 4 of section 2: y -> -y
    flipped = response[:at] + bytes([response[at] ^ 0x80]) + response[at + 1:]
    new, _ = amd.ptau_import_response(old, flipped, "flipped", device=0)
    assert amd.ptau_verify(new, device=0) == (False, "ptau verify: section 2 is not the powers of tau")
    assert amd.ptau_verify(amd.ptau_import_response(old, response, "honest", device=0)[0], device=0) == (True, "")


def test_import_refuses_tampered_responses(amd, honest, tmp_path):
    old, response, other = honest
    keys_at = len(response) - KEYS_BYTES
    # tau.g1_s <-> tau.g1_sx
    swapped = response[:keys_at] + response[keys_at + 64:keys_at + 128] + response[keys_at:keys_at + 64] + response[keys_at + 128:]
    _refused(amd, tmp_path, old, swapped, "a contribution's public key is not consistent")
    # section 2 scaled by another tau than the key's
    run2 = slice(64, 64 + 15 * 32)
    _refused(amd, tmp_path, old, response[:64] + other[run2] + response[run2.stop:], "a contribution's tauG1 does not continue the chain")
    # point 1 of section 3 replaced
    at = 64 + 15 * 32 + 64
    _refused(amd, tmp_path, old, response[:at] + other[at:at + 64] + response[at + 64:], "a contribution's tauG2 does not match its tauG1")
    # a key point at infinity
    inf = response[:keys_at + 384] + bytes([0x40]) + bytes(127) + response[keys_at + 512:]
    _refused(amd, tmp_path, old, inf, "a contribution holds the point at infinity")
    # a point that is none: a format error naming it, not a verdict
    at = 64 + 15 * 32 + 8 * 64 + 3 * 32                # point 3 of section 4
    with pytest.raises(amd.G16Error) as e:
        amd.ptau_import_response(old, response[:at] + Q.to_bytes(32, "big") + response[at + 32:], None, device=0)
    assert e.value.code == -2 and str(e.value) == "ptau import response: point 3 of section 4 is not a point of the curve"
    # the file form with the honest response writes what the buffer form returns
    import ctypes
    lib = amd.load()
    ok, out = ctypes.c_int(7), tmp_path / "new.ptau"
    (tmp_path / "response").write_bytes(response)
    h = ctypes.create_string_buffer(64)
    rc = lib.g16_ptau_import_response_files(str(tmp_path / "old.ptau").encode(), str(tmp_path / "response").encode(), str(out).encode(),
                                            b"tampered", 0, h, ctypes.byref(ok))
    assert rc == 0 and ok.value == 1 and (out.read_bytes(), h.raw) == amd.ptau_import_response(old, response, "tampered", device=0)
