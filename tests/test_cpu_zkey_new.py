"""CPU side of `zkey new` with the circuit hash (csrc/zkey_cshash_host.cpp, the streaming Blake2b-512 of
csrc/zkey_mpc.cpp): the streaming hasher against hashlib for every way of cutting the feed around its 128-byte blocks,
and every argument and format error of g16_zkey_new, g16_zkey_new_files and g16_zkey_cs_hash, which must come out
before the device is asked for -- on a machine without one a valid input ends in G16_E_NOGPU (-4), with one it
succeeds."""
import hashlib

import pytest

import formats as f
import synth
import zkey_mpc_ref as mref
from bn254 import Q, R
from ptau_prepared import rewrite

TD = {"tau": 0x1234567 ** 5 % R, "alpha": 0xabcdef ** 7 % R, "beta": 0x55aa ** 11 % R, "gamma": 1, "delta": 1}
N, P, M, SEED = 24, 2, 12, 1          # m + p + 1 = 15: domain 2^4, 2N - 1 = 31 points of section 2 are read


# ------------------------------------------------------------------ the streaming hasher
LENGTHS = [0, 1, 127, 128, 129, 255, 256, 257, 576 + 4 + 64 * 3]


def _cut_sets(n):
    blocks = list(range(128, n + 1, 128))
    sets = {"none": [], "every_byte": list(range(1, n)), "at_128k": blocks,
            "at_128k_minus_1": [k - 1 for k in blocks], "at_128k_plus_1": [k + 1 for k in blocks if k + 1 <= n],
            "at_128k_pm_1": sorted({c for k in blocks for c in (k - 1, k + 1) if 0 <= c <= n}),
            "at_the_very_end": [n], "empty_parts": [0, 0] + [c for k in blocks for c in (k, k)] + [n, n],
            "header_then_counts": [c for c in (576, 580, 580 + 64, 580 + 128) if c <= n]}
    return sets


@pytest.mark.parametrize("n", LENGTHS)
def test_streaming_blake2b_equals_hashlib(amd, n):
    data = bytes((7 * i + 3) & 0xff for i in range(n))
    want = hashlib.blake2b(data, digest_size=64).digest()
    assert amd.blake2b512(data) == want                      # the one-shot form is a call of the streaming one
    for what, cuts in _cut_sets(n).items():
        assert amd.blake2b512_parts(data, cuts) == want, (n, what)


def test_streaming_blake2b_refuses_bad_cuts(amd):
    for cuts in ([5, 4], [11]):
        with pytest.raises(amd.G16Error) as e:
            amd.blake2b512_parts(bytes(10), cuts)
        assert e.value.code == -1 and "cuts must ascend" in str(e.value)


# ------------------------------------------------------------------ errors ahead of the device
@pytest.fixture(scope="module")
def r1cs():
    _, rows, _ = synth.gen_circuit(N, P, M, SEED)
    return f.write_r1cs(N, P, 0, rows)


@pytest.fixture(scope="module")
def init(amd, r1cs):
    """the initial key of this circuit for TD (gamma = delta = 1), made on the host: what zkey new writes up to csHash"""
    zkey, _ = amd.r1cs_setup_trapdoor(r1cs, TD, 2)
    assert f.read_zkey(zkey)["domainSize"] == 16
    return zkey


@pytest.fixture(scope="module")
def ptau4(amd):
    return amd.ptau_synth(4, TD["tau"], TD["alpha"], TD["beta"], prepared=True, device=-1)


def _new_err(amd, r1cs, ptau):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_new(r1cs, ptau, device=0)
    return e.value


def _hash_err(amd, key, ptau):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_cs_hash(key, ptau, device=0)
    return e.value


def _both(amd, r1cs, init, ptau):
    return [_new_err(amd, r1cs, ptau), _hash_err(amd, init, ptau)]


def test_valid_inputs_reach_the_device_check(amd, r1cs, init, ptau4):
    """without a device both entries end in G16_E_NOGPU after every check; with one they give the same hash"""
    got = []
    for call in (lambda: amd.zkey_new(r1cs, ptau4, device=0)[1], lambda: amd.zkey_cs_hash(init, ptau4, device=0)):
        try:
            got.append(call())
        except amd.G16Error as e:
            assert e.code == -4 and "no HIP device" in str(e), str(e)
    assert len(got) in (0, 2) and len(set(got)) <= 1


def test_malformed_r1cs(amd, r1cs, ptau4):
    for bad in (r1cs[:40], b"r1cx" + r1cs[4:], r1cs[:-1]):
        e = _new_err(amd, bad, ptau4)
        assert e.code == -2 and "r1cs" in str(e), str(e)


def test_unprepared_ptau(amd, r1cs, init):
    raw = amd.ptau_synth(4, TD["tau"], TD["alpha"], TD["beta"], prepared=False, device=-1)
    e = _new_err(amd, r1cs, raw)
    assert e.code == -2 and str(e) == "Powers of tau is not prepared."
    # the hash alone reads section 2 only: an unprepared file passes every check
    try:
        amd.zkey_cs_hash(init, raw, device=0)
    except amd.G16Error as e2:
        assert e2.code == -4, str(e2)


def test_ptau_of_too_small_a_power(amd, r1cs, init):
    ptau3 = amd.ptau_synth(3, TD["tau"], TD["alpha"], TD["beta"], prepared=True, device=-1)
    e = _new_err(amd, r1cs, ptau3)             # the setup's own text comes first
    assert e.code == -2 and str(e) == "circuit too big for this power of tau ceremony. 15 > 2**3"
    e = _hash_err(amd, init, ptau3)
    assert e.code == -1 and str(e) == "zkey new: the ptau is too small for this key"


def test_truncated_and_wrong_curve_ptau(amd, r1cs, init, ptau4):
    for cut in (0, 12, 100):
        for e in _both(amd, r1cs, init, ptau4[:cut]):
            assert e.code == -2 and "ptau: Invalid File format" in str(e), (cut, str(e))
    other = rewrite(ptau4, lambda sid, d: d[:4] + (Q - 2).to_bytes(32, "little") + d[36:] if sid == 1 else d)
    for e in _both(amd, r1cs, init, other):
        assert e.code == -2 and "ptau: Invalid File format (bn128 powers of tau expected)" in str(e)


def test_not_an_initial_key(amd, r1cs, init, ptau4):
    # a key with one contribution record, fabricated on the host from the initial key
    hdr, s10, _ = mref.contribute_ref(init, "x", 5, 7)
    secs = f.read_binfile(init, "zkey", 2)
    order = sorted(secs, key=lambda sid: secs[sid][0][0])
    with_record = f.write_binfile("zkey", 1, [(sid, {10: s10}.get(sid, f.section(init, secs, sid))) for sid in order])
    e = _hash_err(amd, with_record, ptau4)
    assert e.code == -1 and str(e) == "zkey cs hash: not an initial key"
    # ... and its header's delta without the record
    other_delta = f.write_binfile("zkey", 1, [(sid, {2: hdr}.get(sid, f.section(init, secs, sid))) for sid in order])
    e = _hash_err(amd, other_delta, ptau4)
    assert e.code == -1 and str(e) == "zkey cs hash: not an initial key"
    # a trapdoor key with delta = 3
    key3, _ = amd.r1cs_setup_trapdoor(r1cs, dict(TD, delta=3), 2)
    e = _hash_err(amd, key3, ptau4)
    assert e.code == -1 and str(e) == "zkey cs hash: not an initial key"
    # a malformed key is a format error, ahead of everything about the ptau
    e = _hash_err(amd, init[:-1], ptau4[:40])
    assert e.code == -2 and "zkey: Invalid File format" in str(e)


def test_section_2_cut_short(amd, r1cs, init, ptau4):
    for edit in (lambda sid, d: d[:30 * 64] if sid == 2 else d, lambda sid, d: None if sid == 2 else d):
        for e in _both(amd, r1cs, init, rewrite(ptau4, edit)):
            assert e.code == -2 and str(e) == "ptau: Invalid File format", str(e)


@pytest.mark.parametrize("at", [0, 16, 30])
def test_section_2_coordinate_not_below_q(amd, r1cs, init, ptau4, at):
    def edit(sid, d):
        return d[:at * 64] + Q.to_bytes(32, "little") + d[at * 64 + 32:] if sid == 2 else d
    for e in _both(amd, r1cs, init, rewrite(ptau4, edit)):
        assert e.code == -2 and str(e) == "ptau: Invalid File format", str(e)


@pytest.mark.parametrize("at", [0, 17, 30])
def test_section_2_point_off_the_curve(amd, r1cs, init, ptau4, at):
    def edit(sid, d):
        if sid != 2:
            return d
        b = bytearray(d)
        b[at * 64 + 32] ^= 1      # y of point `at`
        return bytes(b)
    for e in _both(amd, r1cs, init, rewrite(ptau4, edit)):
        assert e.code == -2 and str(e) == "ptau: Invalid File format", str(e)


def test_a_point_past_the_ones_the_hash_reads_is_not_looked_at(amd, r1cs, init):
    ptau5 = amd.ptau_synth(5, TD["tau"], TD["alpha"], TD["beta"], prepared=True, device=-1)

    def edit(sid, d):
        if sid != 2:
            return d
        b = bytearray(d)
        b[31 * 64 + 32] ^= 1
        return bytes(b)
    bad = rewrite(ptau5, edit)
    for call in (lambda: amd.zkey_new(r1cs, bad, device=0), lambda: amd.zkey_cs_hash(init, bad, device=0)):
        try:
            call()
        except amd.G16Error as e:
            assert e.code == -4, str(e)


def test_files_forms(amd, r1cs, init, ptau4, tmp_path):
    import ctypes as C
    lib = amd.load()
    short = rewrite(ptau4, lambda sid, d: d[:30 * 64] if sid == 2 else d)
    paths = {}
    for name, data in (("c.r1cs", r1cs), ("init.zkey", init), ("ok.ptau", ptau4), ("short.ptau", short), ("cut.r1cs", r1cs[:40])):
        paths[name] = str(tmp_path / name).encode()
        (tmp_path / name).write_bytes(data)
    out = str(tmp_path / "new.zkey").encode()
    h = C.create_string_buffer(64)
    assert lib.g16_zkey_new_files(paths["cut.r1cs"], paths["ok.ptau"], out, 0, h) == -2 and b"r1cs" in lib.g16_last_error()
    assert lib.g16_zkey_new_files(paths["c.r1cs"], paths["short.ptau"], out, 0, h) == -2
    assert lib.g16_last_error() == b"ptau: Invalid File format"
    assert lib.g16_zkey_cs_hash_files(paths["init.zkey"], paths["short.ptau"], 0, h) == -2
    assert lib.g16_last_error() == b"ptau: Invalid File format"
    assert lib.g16_zkey_new_files(paths["c.r1cs"], str(tmp_path / "none.ptau").encode(), out, 0, h) == -1
    assert not (tmp_path / "new.zkey").exists()
    rc = lib.g16_zkey_new_files(paths["c.r1cs"], paths["ok.ptau"], out, 0, None)
    assert rc in (0, -4) and (rc == 0) == (tmp_path / "new.zkey").exists()


def test_null_arguments_and_layer_entry(amd):
    lib = amd.load()
    assert lib.g16_zkey_new(None, 0, None, 0, 0, None, None, None) == -1
    assert lib.g16_zkey_cs_hash(None, 0, None, 0, 0, None) == -1
    import ctypes as C
    out = C.create_string_buffer(64)
    assert lib.g16_zkey_h_monomial(0, bytes(64), 25, out) == -1 and b"log_n out of range" in lib.g16_last_error()
    with pytest.raises(ValueError):
        amd.zkey_h_monomial(bytes(64 * 2), 1)
