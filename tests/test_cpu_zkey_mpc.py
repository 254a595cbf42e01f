"""CPU side of `zkey contribute` / `zkey verify frominit` (csrc/zkey_mpc.cpp): Blake2b-512 against hashlib, the
transcript's point on G2 against the Python twin (tests/zkey_mpc_ref.py) and the oracle's curve arithmetic, every
refusal of g16_zkey_contribute before the device (and before G16_E_NOGPU), and the twin's own chain check on the twin's
own record."""
import hashlib
import struct

import pytest

import bn254 as b
import formats as f
import groth16 as g
import synth
import zkey_mpc_ref as ref
from bn254 import R
from conftest import golden_path

TD = {"tau": 0x1234567 ** 5 % R, "alpha": 0xabcdef ** 7 % R, "beta": 0x55aa ** 11 % R, "gamma": 1, "delta": 1}
D, S = 0x1f2e3d4c5b6a7988 ** 3 % R, 0x0123456789abcdef ** 3 % R


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def _transcript(i):
    return hashlib.blake2b(b"zkey mpc transcript %d" % i, digest_size=64).digest()


@pytest.fixture(scope="module")
def key(amd):
    n, p, m, seed = 24, 2, 12, 1
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    zkey, _ = amd.r1cs_setup_trapdoor(f.write_r1cs(n, p, 0, rows), TD, 2)
    return zkey


@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, 255, 256, 1000])
def test_blake2b512_equals_hashlib(amd, n):
    data = bytes((7 * i + 3) & 0xff for i in range(n))
    assert amd.blake2b512(data) == hashlib.blake2b(data, digest_size=64).digest()


@pytest.fixture(scope="module")
def g2_cases():
    """Ten transcripts and the twin's points; the first one found whose first x draw is rejected is among them."""
    out = []
    redraw = None
    i = 0
    while len(out) < 9 or redraw is None:
        t = _transcript(i)
        P, draws = ref.hash_to_g2_trace(t)
        if draws > 1 and redraw is None:
            redraw = (t, P, draws)
        elif len(out) < 9:
            out.append((t, P, draws))
        i += 1
    return out + [redraw]


def test_hash_to_g2_equals_twin(amd, g2_cases):
    assert len(g2_cases) == 10
    for t, P, _ in g2_cases:
        assert amd.zkey_hash_to_g2(t) == f.g2_to_lem(P)
        assert P is not None and b.G2.on_curve(P)
        assert b.G2.to_affine(b.G2.jmul(P, R)) is None      # killed by r


def test_hash_to_g2_redraw_loop(amd, g2_cases):
    t, P, draws = g2_cases[-1]
    assert draws > 1
    assert amd.zkey_hash_to_g2(t) == f.g2_to_lem(P)


def _refused(amd, zkey, code, text=None, d=D, s=S):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_contribute(zkey, "x", d, s, device=0)
    assert e.value.code == code, str(e.value)
    if text:
        assert text in str(e.value)


def test_contribute_refuses_a_plonk_key(amd):
    _refused(amd, open(golden_path("plonk_small.zkey"), "rb").read(), -2, "zkey file is not groth16")


def test_contribute_refuses_truncated_images(amd, key):
    for cut in (0, 5, 12, 100, len(key) // 2, len(key) - 1):
        _refused(amd, key[:cut], -2, "Invalid File format")


def test_contribute_refuses_bad_scalars(amd, key):
    _refused(amd, key, -1, d=0)
    _refused(amd, key, -1, d=R)
    _refused(amd, key, -1, s=0)
    _refused(amd, key, -1, s=R)


def _with_section10(key, s10):
    secs = f.read_binfile(key, "zkey", 2)
    out = [(sid, s10 if sid == 10 else f.section(key, secs, sid)) for sid in sorted(secs)]
    return f.write_binfile("zkey", 1, out)


def test_contribute_refuses_a_cut_section_10(amd, key):
    new_h, new_s10, _ = ref.contribute_ref(key, "first", D, S)
    assert _with_section10(key, f.section(key, f.read_binfile(key, "zkey", 2), 10)) == key
    good = _with_section10(key, new_s10)
    _refused(amd, _with_section10(key, new_s10[:-1]), -2, "zkey: Invalid File format")
    _refused(amd, _with_section10(key, new_s10 + b"\0"), -2, "zkey: Invalid File format")
    # a coordinate >= q and a point off its curve in a record
    s = bytearray(new_s10)
    s[68 + 64:68 + 96] = b"\xff" * 32
    _refused(amd, _with_section10(key, bytes(s)), -2, "zkey: Invalid File format")
    s = bytearray(new_s10)
    s[68 + 64] ^= 1
    _refused(amd, _with_section10(key, bytes(s)), -2, "zkey: Invalid File format")
    if not _gpu_present():
        _refused(amd, good, -4)


def test_a_beacon_record_is_read_and_carried(amd, key):
    """A type-1 record (params: id 2 + 32-byte beacon hash length-prefixed, id 3 + iterations) parses like any other."""
    _, s10, _ = ref.contribute_ref(key, None, D, S)
    _, recs = ref.parse_section10(s10)
    params = bytes([2, 4]) + b"\x01\x02\x03\x04" + bytes([3, 10])
    beacon = recs[0]["raw"][:384] + struct.pack("<II", 1, len(params)) + params
    with_beacon = _with_section10(key, s10[:64] + struct.pack("<I", 1) + beacon)
    cs, got = ref.parse_section10(f.section(with_beacon, f.read_binfile(with_beacon, "zkey", 2), 10))
    assert got[0]["type"] == 1 and got[0]["params"] == params
    if not _gpu_present():
        _refused(amd, with_beacon, -4)
    else:
        new, _ = amd.zkey_contribute(with_beacon, "x", D, S, device=0)
        _, recs2 = ref.parse_section10(f.section(new, f.read_binfile(new, "zkey", 2), 10))
        assert len(recs2) == 2 and recs2[0]["raw"] == beacon and recs2[1]["type"] == 0


def test_no_cpu_path(amd, key):
    if _gpu_present():
        pytest.skip("GPU present")
    _refused(amd, key, -4)
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_verify_from_init(key, key, device=0)
    assert e.value.code == -4


def test_verify_malformed_is_format_error(amd, key):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_verify_from_init(key, key[:len(key) - 1], device=0)
    assert e.value.code == -2


def test_twin_accepts_its_own_record(amd, key):
    new_h, new_s10, chash = ref.contribute_ref(key, "first", D, S)
    assert amd.blake2b512(ref.hash_pubkey_feed(ref.parse_section10(new_s10)[1][0])) == chash
    secs = f.read_binfile(key, "zkey", 2)
    out = [(sid, new_h if sid == 2 else new_s10 if sid == 10 else f.section(key, secs, sid)) for sid in sorted(secs)]
    contributed = f.write_binfile("zkey", 1, out)
    assert ref.verify_chain(key, contributed)
    assert ref.verify_chain(key, key)
    cs, recs = ref.parse_section10(new_s10)
    assert cs == bytes(64) and len(recs) == 1 and recs[0]["params"] == b"\x01\x05first" and recs[0]["type"] == 0
    assert chash == ref.contribution_hash(recs[0]) and len(chash) == 64
    # a flipped transcript byte or another d in g2_spx breaks the chain
    bad = bytearray(new_s10)
    bad[68 + 320] ^= 1
    assert not ref.verify_chain(key, f.write_binfile("zkey", 1, [(sid, bytes(bad) if sid == 10 else x) for sid, x in out]))
    _, other, _ = ref.contribute_ref(key, "first", D + 1, S)
    mixed = new_s10[:68 + 192] + other[68 + 192:68 + 320] + new_s10[68 + 320:]
    assert not ref.verify_chain(key, f.write_binfile("zkey", 1, [(sid, mixed if sid == 10 else x) for sid, x in out]))
