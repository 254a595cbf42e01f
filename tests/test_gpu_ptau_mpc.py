"""`powersoftau contribute` and `powersoftau verify` on the device (csrc/ptau_scale.hip, csrc/ptau_mpc.cpp).  A contribution
(tau, alpha, beta) to the generator file gives the sections g16_ptau_synth writes for those scalars, byte for byte, and
the whole file and the contribution hash of the Python twin (tests/ptau_mpc_ref.py); the chunk, lane and window
overrides change no byte; the verifier accepts honest chains and names the check that a tampered file fails."""
import hashlib
import struct

import pytest

import bn254 as b
import formats as f
import groth16 as g
from bn254 import Q, R, fr_root
from ptau_mpc_ref import (challenge_hash, contribute_ref, first_challenge, generator_sections, key_points, parse_section7,
                          response_hash)
from ptau_prepare_ref import split
from ptau_prepared import rewrite, write_ptau_prepared

pytestmark = pytest.mark.gpu

ORDER = [1, 2, 3, 4, 5, 6, 7]


def _secret(seed):
    return tuple(pow(seed + 2 + i, 1000 + 7 * i + seed, R) for i in range(6))


def _sections_equal(got, want):
    ids, gs = split(got)
    _, ws = split(want)
    assert ids == ORDER
    for sid in range(1, 7):
        assert gs[sid] == ws[sid], sid


# ------------------------------------------------------------------ exact
@pytest.mark.parametrize("seed", [41, 42])
@pytest.mark.parametrize("power", range(10))
def test_contribution_to_the_generator_file_exact(amd, power, seed):
    s = _secret(seed)
    p0 = amd.ptau_new(power)
    got, h = amd.ptau_contribute(p0, "first", s, device=0)
    _sections_equal(got, amd.ptau_synth(power, s[0], s[1], s[2], prepared=False, device=0))
    challenge = first_challenge(generator_sections(power))
    assert h == response_hash(challenge, key_points(challenge, s))
    assert parse_section7(split(got)[1][7])[0]["partialHash"] == bytes(216)
    if power <= 4:
        want, wh = contribute_ref(p0, "first", s)
        assert got == want and h == wh


def test_second_contribution_is_the_product(amd):
    power, s1, s2 = 3, _secret(51), _secret(52)
    c1, _ = amd.ptau_contribute(amd.ptau_new(power), "one", s1, device=0)
    c2, h2 = amd.ptau_contribute(c1, None, s2, device=0)
    _sections_equal(c2, amd.ptau_synth(power, s1[0] * s2[0] % R, s1[1] * s2[1] % R, s1[2] * s2[2] % R, prepared=False, device=0))
    want, wh = contribute_ref(c1, None, s2)
    assert c2 == want and h2 == wh
    assert amd.ptau_contribute(c1, None, s2, device=0) == (c2, h2)      # the same inputs give the same bytes
    assert amd.ptau_contribute(c1, None, None, device=0)[0] != c2       # the OS CSPRNG does not


def test_contribution_on_top_of_non_generator_points(amd):
    power, s = 5, _secret(53)
    t = g.trapdoor(54)
    src = amd.ptau_synth(power, t["tau"], t["alpha"], t["beta"], prepared=False, device=0)
    got, _ = amd.ptau_contribute(src, None, s, device=0)
    _sections_equal(got, amd.ptau_synth(power, t["tau"] * s[0] % R, t["alpha"] * s[1] % R, t["beta"] * s[2] % R,
                                        prepared=False, device=0))


# ------------------------------------------------------------------ chunks, offsets, grid-stride, windows
@pytest.fixture(scope="module")
def default_runs(amd):
    return {p: amd.ptau_contribute(amd.ptau_new(p), "x", _secret(60 + p), device=0) for p in (6, 12)}


@pytest.mark.parametrize("window,chunk", [(3, 37), (4, 37), (5, 37), (5, 64), (5, 32)], ids=["3", "4", "5", "5-chunk64", "5-chunk32"])
def test_small_chunks_and_grids_change_no_byte(amd, default_runs, monkeypatch, window, chunk):
    """Power 6, chunks of 37 points on 64 lanes: section 2's 127 points end a chunk mid-wavefront (127 = 3 x 37 + 16).
    Chunks of 64 and of 32: the 64 points of sections 3-5 are exactly one and exactly two full chunks, section 2 is
    64 + 63 and 3 x 32 + 31."""
    monkeypatch.setenv("G16_PTAU_CHUNK", str(chunk))
    monkeypatch.setenv("G16_PTAU_LANES", "64")
    monkeypatch.setenv("G16_PTAU_WINDOW", str(window))
    assert amd.ptau_contribute(amd.ptau_new(6), "x", _secret(66), device=0) == default_runs[6]


def test_grid_stride_passes_change_no_byte(amd, default_runs, monkeypatch):
    """One chunk of 127 / 64 points over 64 lanes: two grid-stride passes, the second half empty."""
    monkeypatch.setenv("G16_PTAU_LANES", "64")
    assert amd.ptau_contribute(amd.ptau_new(6), "x", _secret(66), device=0) == default_runs[6]


def test_first_across_many_chunk_boundaries(amd, default_runs, monkeypatch):
    monkeypatch.setenv("G16_PTAU_CHUNK", "1000")
    assert amd.ptau_contribute(amd.ptau_new(12), "x", _secret(72), device=0) == default_runs[12]


def test_default_run_at_power_12_is_exact(amd, default_runs):
    s = _secret(72)
    _sections_equal(default_runs[12][0], amd.ptau_synth(12, s[0], s[1], s[2], prepared=False, device=0))


def test_exponent_range_power_16(amd, capfd, monkeypatch):
    """Exponents up to 2^17 - 2; sections compared by SHA-256; prints the trace line."""
    power, s = 16, _secret(16)
    monkeypatch.setenv("G16_TRACE_HOST", "1")
    capfd.readouterr()
    got, _ = amd.ptau_contribute(amd.ptau_new(power), None, s, device=0)
    trace = capfd.readouterr().err
    monkeypatch.delenv("G16_TRACE_HOST")
    line = [x for x in trace.splitlines() if "[g16] ptau contribute" in x]
    with capfd.disabled():
        print("\n" + (line[0] if line else trace))
    assert line
    want = amd.ptau_synth(power, s[0], s[1], s[2], prepared=False, device=0)
    ids, gs = split(got)
    _, ws = split(want)
    assert ids == ORDER
    for sid in range(1, 7):
        assert hashlib.sha256(gs[sid]).digest() == hashlib.sha256(ws[sid]).digest(), sid


# ------------------------------------------------------------------ degenerate scalars and points
@pytest.mark.parametrize("name", ["tau_one", "tau_minus_one", "tau_root", "alpha_beta_one", "one_infinity", "all_infinity"])
def test_degenerate_scalars_and_points(amd, name):
    power, s = 5, list(_secret(80))
    if name == "tau_one":
        s[0] = 1
    if name == "tau_minus_one":
        s[0] = R - 1
    if name == "tau_root":
        s[0] = fr_root(3)          # the powers cycle with period 8
    if name == "alpha_beta_one":
        s[1] = s[2] = 1
    src = amd.ptau_new(power)
    want = split(write_ptau_prepared(power, s[0], s[1], s[2], prepared=False))[1]
    if name == "one_infinity":
        src = rewrite(src, lambda sid, d: d[:3 * 64] + bytes(64) + d[4 * 64:] if sid == 4 else d)
        want[4] = want[4][:3 * 64] + bytes(64) + want[4][4 * 64:]
    if name == "all_infinity":
        src = rewrite(src, lambda sid, d: bytes(len(d)) if sid == 5 else d)
        want[5] = bytes(len(want[5]))
    ids, gs = split(amd.ptau_contribute(src, None, tuple(s), device=0)[0])
    assert ids == ORDER
    for sid in range(2, 7):
        assert gs[sid] == want[sid], sid
    if name == "tau_root":
        assert gs[2][:64] == gs[2][8 * 64:9 * 64] and gs[3][128:256] == gs[3][9 * 128:10 * 128]


# ------------------------------------------------------------------ prepared input, and on to a key
def test_prepared_input_is_dropped_and_the_result_feeds_the_setup(amd):
    msg = hashlib.sha256(b"a ceremony of our own").digest()
    out = amd.sha256_chain_setup(1, msg, 5, want_zkey=False, want_r1cs=True)
    s = _secret(90)
    td = {"tau": s[0], "alpha": s[1], "beta": s[2], "gamma": 1, "delta": 1}
    amd.setup_device(0)
    try:
        trap, vkey = amd.r1cs_setup_trapdoor(out["r1cs"], td, 0)
    finally:
        amd.setup_device(-1)
    L = f.read_zkey(trap)["domainSize"].bit_length() - 1
    src = amd.ptau_prepare(amd.ptau_new(L), device=0)
    assert split(src)[0] == ORDER + [12, 13, 14, 15]
    got, _ = amd.ptau_contribute(src, "prepared in", s, device=0)
    assert split(got)[0] == ORDER
    prep = amd.ptau_prepare(got, device=0)
    want = amd.ptau_synth(L, s[0], s[1], s[2], prepared=True, device=0)
    ids, gs = split(prep)
    _, ws = split(want)
    assert ids == ORDER + [12, 13, 14, 15]
    for sid in (2, 3, 4, 5, 6, 13, 14, 15):
        assert gs[sid] == ws[sid], sid
    M = 2 << L
    assert len(gs[12]) == (2 * M - 1) * 64 and gs[12][:(M - 1) * 64] == ws[12][:(M - 1) * 64]
    key = amd.groth16_setup_ptau(out["r1cs"], prep, device=0)
    rs = g.trapdoor(9)
    prover = amd.Prover(key, device=0)
    proof = prover.prove(out["wtns"], f.le(rs["tau"]), f.le(rs["alpha"]))
    prover.close()
    v = amd.Verifier(vkey, n_public=256, device=0)
    assert v.verify(proof[1], proof[0])
    v.close()
    assert amd.ptau_verify(prep, device=0) == (True, "")


# ------------------------------------------------------------------ verify
@pytest.fixture(scope="module")
def chain(amd):
    """Power 3: the files after one, two and three contributions."""
    out = [amd.ptau_new(3)]
    for k in range(3):
        out.append(amd.ptau_contribute(out[-1], f"contributor {k}", _secret(100 + k), device=0)[0])
    return out


def test_verify_accepts_honest_files(amd, chain):
    for power in (0, 1, 3, 7):
        assert amd.ptau_verify(amd.ptau_new(power), device=0) == (True, ""), power
    assert amd.ptau_verify(chain[1], device=0) == (True, "")
    assert amd.ptau_verify(chain[3], device=0) == (True, "")
    assert amd.ptau_verify(amd.ptau_prepare(chain[3], device=0), device=0) == (True, "")
    p0 = amd.ptau_contribute(amd.ptau_new(0), "zero", _secret(110), device=0)[0]
    p0 = amd.ptau_contribute(p0, None, _secret(111), device=0)[0]
    assert amd.ptau_verify(p0, device=0) == (True, "")
    assert amd.ptau_verify(amd.ptau_contribute(amd.ptau_new(9), None, None, device=0)[0], device=0) == (True, "")


def _reject(amd, ptau, text):
    ok, why = amd.ptau_verify(ptau, device=0)
    assert not ok and why == "ptau verify: " + text, why


def _edit7(ptau, rec_index, at, new):
    """Bytes [at, at + len(new)) of record rec_index replaced."""
    recs = parse_section7(split(ptau)[1][7])
    pos = 4 + sum(len(r["raw"]) for r in recs[:rec_index]) + at
    return rewrite(ptau, lambda sid, d: d[:pos] + new + d[pos + len(new):] if sid == 7 else d)


def _reseal(ptau):
    """The last record's nextChallenge recomputed for the file's points as they stand (so that a tampered point gets past
    the hash check to the check under test)."""
    secs = split(ptau)[1]
    recs = parse_section7(secs[7])
    power = struct.unpack_from("<I", secs[1], 36)[0]
    challenge = recs[-2]["nextChallenge"] if len(recs) > 1 else first_challenge(generator_sections(power))
    return _edit7(ptau, len(recs) - 1, 1432, challenge_hash(secs, response_hash(challenge, recs[-1])))


def _double(lem):
    if len(lem) == 64:
        return f.g1_to_lem(b.G1.mul(f.g1_from_lem(lem), 2))
    return f.g2_to_lem(b.G2.mul(f.g2_from_lem(lem), 2))


def test_verify_rejects_a_file_of_known_scalars_without_records(amd):
    _reject(amd, amd.ptau_synth(3, 5, 6, 7, prepared=False, device=0), "a file without contributions is not the generator file")


WRONG_POWER = {2: "section 2 is not the powers of tau", 3: "section 3 is not the powers of tau",
               4: "section 4 is not alpha times the powers of tau", 5: "section 5 is not beta times the powers of tau"}


@pytest.mark.parametrize("where", ["interior", "last"])
@pytest.mark.parametrize("sid", [2, 3, 4, 5])
def test_verify_rejects_one_wrong_power(amd, chain, sid, where):
    psz = 128 if sid == 3 else 64
    n = len(split(chain[2])[1][sid]) // psz
    i = 3 if where == "interior" else n - 1
    bad = rewrite(chain[2], lambda s, d: d[:i * psz] + _double(d[i * psz:(i + 1) * psz]) + d[(i + 1) * psz:] if s == sid else d)
    _reject(amd, bad, "the last contribution's challenge hash does not match the file")
    _reject(amd, _reseal(bad), WRONG_POWER[sid])


def test_verify_rejects_tampered_records(amd, chain):
    last = parse_section7(split(chain[3])[1][7])[-1]
    # tauG1 <-> alphaG1 of the last record
    bad = _edit7(_edit7(chain[3], 2, 0, last["alphaG1"]), 2, 192, last["tauG1"])
    _reject(amd, bad, "a contribution's tauG1 does not continue the chain")
    # g1_sx of the beta key doubled, in the middle record
    mid = parse_section7(split(chain[3])[1][7])[1]
    _reject(amd, _edit7(chain[3], 1, 448 + 2 * 128 + 64, _double(mid["beta.g1_sx"])), "a contribution's public key is not consistent")
    # tauG2 of the first record doubled
    first = parse_section7(split(chain[3])[1][7])[0]
    _reject(amd, _edit7(chain[3], 0, 64, _double(first["tauG2"])), "a contribution's tauG2 does not match its tauG1")
    # one byte of the last nextChallenge; of an earlier one (the next record's keys hang on it)
    flip = bytes([last["nextChallenge"][9] ^ 1])
    _reject(amd, _edit7(chain[3], 2, 1432 + 9, flip), "the last contribution's challenge hash does not match the file")
    _reject(amd, _edit7(chain[3], 1, 1432 + 9, bytes([mid["nextChallenge"][9] ^ 1])), "a contribution's public key is not consistent")
    # a record point at infinity
    _reject(amd, _edit7(chain[3], 1, 192, bytes(64)), "a contribution holds the point at infinity")
    _reject(amd, _edit7(chain[3], 2, 832, bytes(128)), "a contribution holds the point at infinity")
    # the records of another file
    other = amd.ptau_contribute(chain[2], "someone else", _secret(120), device=0)[0]
    s7 = split(other)[1][7]
    _reject(amd, rewrite(chain[3], lambda sid, d: s7 if sid == 7 else d), "the file's points are not the last contribution's")
    # the first power
    g2 = f.g2_to_lem(b.G2.mul(b.G2_GEN, 2))
    _reject(amd, rewrite(chain[3], lambda sid, d: g2 + d[128:] if sid == 3 else d), "the first point of section 2 or 3 is not the generator")


def test_verify_reports_a_pairing_failure_before_a_host_failure(amd, chain):
    """Two failures in one file: the middle record's beta key fails its pairing check, and the last record's challenge
    hash does not match the file.  The verdicts of the pairing checks come first; the host checks' follow them."""
    recs = parse_section7(split(chain[3])[1][7])
    bad_key = _edit7(chain[3], 1, 448 + 2 * 128 + 64, _double(recs[1]["beta.g1_sx"]))
    flip = bytes([recs[2]["nextChallenge"][9] ^ 1])
    _reject(amd, bad_key, "a contribution's public key is not consistent")                                     # each alone
    _reject(amd, _edit7(chain[3], 2, 1432 + 9, flip), "the last contribution's challenge hash does not match the file")
    _reject(amd, _edit7(bad_key, 2, 1432 + 9, flip), "a contribution's public key is not consistent")          # together


def test_verify_rejects_wrong_prepared_sections(amd, chain):
    prep = amd.ptau_prepare(chain[1], device=0)
    swapped = rewrite(prep, lambda sid, d: d[:5 * 64] + d[6 * 64:7 * 64] + d[5 * 64:6 * 64] + d[7 * 64:] if sid == 14 else d)
    assert swapped != prep
    _reject(amd, swapped, "the prepared sections are not the transform of sections 2 to 5")
    _reject(amd, rewrite(prep, lambda sid, d: None if sid == 15 else d), "the prepared sections 12 to 15 are not all present")
    _reject(amd, rewrite(prep, lambda sid, d: d[:-64] if sid == 15 else d), "the prepared sections are not the transform of sections 2 to 5")


def test_verify_reports_malformed_points_as_format_errors(amd, chain):
    def off_curve(sid, d):
        return d[:2 * 64] + bytes([d[2 * 64] ^ 1]) + d[2 * 64 + 1:] if sid == 4 else d

    def coordinate_q(sid, d):
        return d[:5 * 128 + 32] + Q.to_bytes(32, "little") + d[5 * 128 + 64:] if sid == 3 else d
    for edit in (off_curve, coordinate_q):
        with pytest.raises(amd.G16Error) as e:
            amd.ptau_verify(rewrite(chain[2], edit), device=0)
        assert e.value.code == -2 and str(e.value).endswith("ptau: Invalid File format")
