"""`snarkjs powersoftau prepare phase2` (alias `pt2`) through the Node CLI on files: an unprepared power-6 ceremony is
prepared, compared with the Python writers, and then carries `groth16 setup`, `prove` and `verify` -- OK!"""
import json
import os
import shutil
import subprocess

import pytest

import formats as f
import synth
import groth16 as g
from conftest import ROOT
from ptau_prepare_ref import g1_bytes, split, top_block_scalar
from ptau_prepared import write_ptau_prepared

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@needs_node
@pytest.mark.gpu
def test_node_prepare_phase2_then_setup_prove_verify(addon, tmp_path):
    n, p, m, seed = 60, 5, 40, 3
    power = 6
    rows, w = synth.make(n, p, m, seed)
    t = g.trapdoor(seed + 7)
    rf, pf, qf, zf, wf = (tmp_path / x for x in ("c.r1cs", "pot.ptau", "pot_prepared.ptau", "c_0000.zkey", "w.wtns"))
    rf.write_bytes(f.write_r1cs(n, p, 0, rows))
    pf.write_bytes(write_ptau_prepared(power, t["tau"], t["alpha"], t["beta"], prepared=False))
    wf.write_bytes(f.write_wtns(w))
    cli = os.path.join(JS, "cli.js")

    def run(*args):
        return subprocess.run(["node", cli, *map(str, args)], capture_output=True, text=True, timeout=300)
    r = run("powersoftau", "prepare", "phase2", pf, qf)
    assert r.returncode == 0, r.stderr
    ids, gs = split(qf.read_bytes())
    _, ws = split(write_ptau_prepared(power, t["tau"], t["alpha"], t["beta"], prepared=True))
    assert ids == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    for sid in (1, 2, 3, 4, 5, 6, 7, 13, 14, 15):
        assert gs[sid] == ws[sid], sid
    M = 2 << power
    assert gs[12][:(M - 1) * 64] == ws[12][:(M - 1) * 64]
    assert gs[12][(M - 1) * 64:] == g1_bytes([top_block_scalar(power, j, t["tau"]) for j in range(M)])
    # the prepared file carries the rest of the flow
    r = run("groth16", "setup", rf, qf, zf)
    assert r.returncode == 0, r.stderr
    vkf, prf, puf = tmp_path / "vk.json", tmp_path / "proof.json", tmp_path / "public.json"
    assert run("zkey", "export", "verificationkey", zf, vkf).returncode == 0
    r = run("groth16", "prove", zf, wf, prf, puf)
    assert r.returncode == 0, r.stderr
    r = run("groth16", "verify", vkf, puf, prf)
    assert r.returncode == 0 and "snarkJS: OK!" in r.stdout, r.stderr
    assert json.loads(puf.read_text()) == [str(x) for x in w[1:p + 1]]
    # `pt2` is the same command
    qf2 = tmp_path / "again.ptau"
    r = run("pt2", pf, qf2)
    assert r.returncode == 0, r.stderr
    assert qf2.read_bytes() == qf.read_bytes()
    # a missing input: exit 1 with snarkjs's error prefix
    r = run("powersoftau", "prepare", "phase2", tmp_path / "missing.ptau", tmp_path / "x.ptau")
    err = [x for x in r.stderr.splitlines() if x.startswith("[ERROR] snarkJS:")]
    assert r.returncode == 1 and err and "cannot open" in err[0], r.stderr
