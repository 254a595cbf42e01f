"""`powersoftau prepare phase2` on the device (csrc/ptau_prepare.hip via g16_ptau_prepare).  For a ceremony of a KNOWN
(tau, alpha, beta) the prepared sections are the Lagrange points g16_ptau_synth(prepared=1) writes, byte for byte --
except block power + 1 of section 12, whose last input snarkjs pads with infinity: that block is checked against the
Python restatement (tests/ptau_prepare_ref.py).  The prepared file then feeds g16_groth16_setup_ptau."""
import hashlib
import os
import random
import time

import pytest

import formats as f
import groth16 as g
from bn254 import fr_root
from conftest import ROOT
from ptau_prepare_ref import (ceremony_scalars, expected_sections, g1_bytes, g1_point_bytes, split, top_block_scalar)
from ptau_prepared import rewrite

pytestmark = pytest.mark.gpu

ORDER = [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]


def _td(seed):
    t = g.trapdoor(seed)
    return {"tau": t["tau"], "alpha": t["alpha"], "beta": t["beta"], "gamma": 1, "delta": 1}


def _check_against_generator(got, want, power):
    """Order 1..7, 12..15; sections 1-7, 13-15 and blocks 0..power of section 12 equal the generator's prepared file.
    -> the top block of section 12."""
    ids, gs = split(got)
    wids, ws = split(want)
    assert ids == ORDER and wids == ORDER
    for sid in (1, 2, 3, 4, 5, 6, 7, 13, 14, 15):
        assert gs[sid] == ws[sid], sid
    M = 2 << power
    assert len(gs[12]) == (2 * M - 1) * 64
    assert gs[12][:(M - 1) * 64] == ws[12][:(M - 1) * 64]
    return gs[12][(M - 1) * 64:]


def _check_top_block_sampled(top, power, tau, seed, count=64):
    """Seeded positions of the padded top block (always 0, 1, M - 1): the generator's Lagrange point minus
    [w^j / M][tau^(M-1)]G1, as one multiple of the generator.  A cost cap, not a tolerance: every compared point is exact."""
    M = 2 << power
    rng = random.Random(seed)
    pos = {0, 1, M - 1}
    while len(pos) < min(count, M):
        pos.add(rng.randrange(M))
    for j in sorted(pos):
        assert top[j * 64:(j + 1) * 64] == g1_point_bytes(top_block_scalar(power, j, tau)), j


@pytest.mark.parametrize("seed", [31, 32])
@pytest.mark.parametrize("power", range(10))
def test_small_powers_exact(amd, power, seed):
    td = _td(seed)
    src = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    want = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=True, device=0)
    got = amd.ptau_prepare(src, device=0)
    top = _check_against_generator(got, want, power)
    M = 2 << power
    assert top == g1_bytes([top_block_scalar(power, j, td["tau"]) for j in range(M)])
    assert top != split(want)[1][12][(M - 1) * 64:]


@pytest.mark.parametrize("power", [12, 16, 18])
def test_every_stage_count_exact(amd, power):
    td = _td(power + 100)
    src = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    want = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=True, device=0)
    got = amd.ptau_prepare(src, device=0)
    top = _check_against_generator(got, want, power)
    _check_top_block_sampled(top, power, td["tau"], power)


def _degenerate(amd, name):
    power = 5
    td = _td(55)
    tau = {"tau_one": 1, "tau_root": fr_root(3)}.get(name, td["tau"])
    src = amd.ptau_synth(power, tau, td["alpha"], td["beta"], prepared=False, device=0)
    x2, x3, x4, x5 = ceremony_scalars(power, tau, td["alpha"], td["beta"])
    if name == "one_infinity":
        src = rewrite(src, lambda sid, d: d[:3 * 64] + bytes(64) + d[4 * 64:] if sid == 4 else d)
        x4[3] = 0
    if name == "all_infinity":
        src = rewrite(src, lambda sid, d: bytes(len(d)) if sid == 5 else d)
        x5 = [0] * len(x5)
    return power, src, expected_sections(power, x2, x3, x4, x5)


@pytest.mark.parametrize("name", ["tau_one", "tau_root", "one_infinity", "all_infinity"])
def test_degenerate_inputs(amd, name):
    """tau = 1 makes every butterfly a doubling or a cancellation, tau = w_8 puts the source on the domain; infinity
    inputs stay valid.  Expected values from the restatement by linearity; infinity comes out as zero bytes."""
    power, src, want = _degenerate(amd, name)
    ids, gs = split(amd.ptau_prepare(src, device=0))
    _, ss = split(src)
    assert ids == ORDER
    for sid in range(1, 8):
        assert gs[sid] == ss[sid]
    for sid in (12, 13, 14, 15):
        assert gs[sid] == want[sid], sid
    if name == "tau_one":
        # block k of all-equal inputs is (P, 0, ..., 0): section 14 holds one point per block
        zeros = sum(gs[14][i:i + 64] == bytes(64) for i in range(0, len(gs[14]), 64))
        assert zeros == (2 << power) - 1 - (power + 1)
        zeros2 = sum(gs[13][i:i + 128] == bytes(128) for i in range(0, len(gs[13]), 128))
        assert zeros2 == (2 << power) - 1 - (power + 1)
    if name == "tau_root":
        # tau = w_8^1: block 3 is the unit vector e_1, and larger blocks hold infinity off the multiples of 2^k / 8
        blk = gs[14][7 * 64:15 * 64]
        assert [blk[i * 64:(i + 1) * 64] == bytes(64) for i in range(8)] == [j != 1 for j in range(8)]
    if name == "all_infinity":
        assert gs[15] == bytes(len(gs[15]))


def test_idempotent(amd):
    td = _td(77)
    src = amd.ptau_synth(7, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    once = amd.ptau_prepare(src, device=0)
    assert amd.ptau_prepare(once, device=0) == once
    full = amd.ptau_synth(7, td["tau"], td["alpha"], td["beta"], prepared=True, device=0)
    assert amd.ptau_prepare(full, device=0) == once
    # other section ids are not carried over
    ids, secs = split(src)
    extra = f.write_binfile("ptau", 1, [(sid, secs[sid]) for sid in ids] + [(9, b"x" * 10)])
    assert amd.ptau_prepare(extra, device=0) == once


def _zkey_sections(buf):
    secs = f.read_binfile(buf, "zkey", 2, "zkey")
    return {sid: f.section(buf, secs, sid) for sid in secs}


def _same_but_h(key, want):
    a, b = _zkey_sections(key), _zkey_sections(want)
    assert sorted(a) == sorted(b)
    for sid in a:
        if sid != 9:
            assert a[sid] == b[sid], sid
    assert len(a[9]) == len(b[9])


def test_prepared_file_feeds_the_setup(amd):
    """SHA-256 chain circuit of domain 2^L.  A file of power exactly L: the H basis comes from the padded top block, so
    section 9 differs from the trapdoor key's while every other section and the proof are the same.  Power L + 1: the
    whole key is the trapdoor key."""
    msg = hashlib.sha256(b"prepare phase2 feeds the setup").digest()
    out = amd.sha256_chain_setup(1, msg, 5, want_zkey=False, want_r1cs=True)
    r1cs = out["r1cs"]
    td = _td(171)
    amd.setup_device(0)
    try:
        want, vkey = amd.r1cs_setup_trapdoor(r1cs, td, 0)
    finally:
        amd.setup_device(-1)
    L = f.read_zkey(want)["domainSize"].bit_length() - 1
    src = amd.ptau_synth(L, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    key = amd.groth16_setup_ptau(r1cs, amd.ptau_prepare(src, device=0), device=0)
    _same_but_h(key, want)
    assert _zkey_sections(key)[9] != _zkey_sections(want)[9]
    rs = g.trapdoor(9)
    r, s = f.le(rs["tau"]), f.le(rs["alpha"])
    proofs = []
    for k in (key, want):
        prover = amd.Prover(k, device=0)
        proofs.append(prover.prove(out["wtns"], r, s))
        prover.close()
    assert proofs[0] == proofs[1]
    v = amd.Verifier(vkey, n_public=256, device=0)
    assert v.verify(proofs[0][1], proofs[0][0])
    v.close()
    src = amd.ptau_synth(L + 1, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    assert amd.groth16_setup_ptau(r1cs, amd.ptau_prepare(src, device=0), device=0) == want


def test_full_size_power_20(amd, capfd, monkeypatch):
    """Power 20, one run: sections 13-15 and blocks <= 20 of section 12 hash to the generator's, the top block is
    sampled, and the native nzcp_live circuit's key from the prepared file is the trapdoor key apart from section 9.
    Prints the trace line and the wall time (no time is a pass condition).  Measured on one MI355X: the prepare call
    8.3 s, the whole test 16 s; run it under a limit of a few minutes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nzcp_pass
    power = 20
    td = _td(2021)
    src = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
    monkeypatch.setenv("G16_TRACE_HOST", "1")
    capfd.readouterr()
    t0 = time.time()
    got = amd.ptau_prepare(src, device=0)
    wall = time.time() - t0
    trace = capfd.readouterr().err
    monkeypatch.delenv("G16_TRACE_HOST")
    line = [x for x in trace.splitlines() if "[g16] ptau prepare" in x]
    with capfd.disabled():
        print(f"\nptau prepare, power {power}: {wall:.2f} s wall")
        print(line[0] if line else trace)
    assert line
    want = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=True, device=0)
    ids, gs = split(got)
    _, ws = split(want)
    del want
    assert ids == ORDER
    M = 2 << power
    sha = lambda b: hashlib.sha256(b).digest()   # noqa: E731
    for sid in (1, 2, 3, 4, 5, 6, 7, 13, 14, 15):
        assert sha(gs[sid]) == sha(ws[sid]), sid
    assert sha(gs[12][:(M - 1) * 64]) == sha(ws[12][:(M - 1) * 64])
    assert len(gs[12]) == (2 * M - 1) * 64
    _check_top_block_sampled(gs[12][(M - 1) * 64:], power, td["tau"], power)
    del gs, ws
    tbs = nzcp_pass.to_be_signed("Anne-Marie", "Te Whare", "1987-11-30", live=True, exp=1700000000)
    out = amd.nzcp_circuit_setup(amd.NZCP_LIVE_PARAMS, tbs, 77, want_zkey=False, want_r1cs=True)
    amd.setup_device(0)
    try:
        trap, _ = amd.r1cs_setup_trapdoor(out["r1cs"], td, 0)
    finally:
        amd.setup_device(-1)
    key = amd.groth16_setup_ptau(out["r1cs"], got, device=0)
    _same_but_h(key, trap)
