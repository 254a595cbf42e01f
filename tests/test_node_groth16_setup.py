"""`snarkjs groth16 setup` (alias `zkey new`) through the Node CLI on files: setup from a prepared ptau, then
`zkey export verificationkey`, `groth16 prove` and `groth16 verify` -- OK!, and the key equals the oracle's."""
import json
import os
import shutil
import subprocess

import pytest

import formats as f
import groth16 as g
import synth
from conftest import ROOT
from ptau_prepared import write_ptau_prepared

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@needs_node
@pytest.mark.gpu
def test_node_groth16_setup_prove_verify(addon, tmp_path):
    n, p, m, seed = 60, 5, 40, 3
    rows, w = synth.make(n, p, m, seed)
    t = g.trapdoor(seed + 7)
    td = {"tau": t["tau"], "alpha": t["alpha"], "beta": t["beta"], "gamma": 1, "delta": 1}
    zk, _ = g.setup(n, p, rows, td)
    rf, pf, zf, wf = tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "c_0000.zkey", tmp_path / "w.wtns"
    rf.write_bytes(f.write_r1cs(n, p, 0, rows))
    pf.write_bytes(write_ptau_prepared(6, td["tau"], td["alpha"], td["beta"]))
    wf.write_bytes(f.write_wtns(w))
    cli = os.path.join(JS, "cli.js")

    def run(*args):
        return subprocess.run(["node", cli, *map(str, args)], capture_output=True, text=True, timeout=300)
    r = run("groth16", "setup", rf, pf, zf)
    assert r.returncode == 0, r.stderr
    assert zf.read_bytes() == f.write_zkey(zk)
    vkf, prf, puf = tmp_path / "vk.json", tmp_path / "proof.json", tmp_path / "public.json"
    assert run("zkey", "export", "verificationkey", zf, vkf).returncode == 0
    r = run("groth16", "prove", zf, wf, prf, puf)
    assert r.returncode == 0, r.stderr
    r = run("groth16", "verify", vkf, puf, prf)
    assert r.returncode == 0 and "snarkJS: OK!" in r.stdout, r.stderr
    assert json.loads(puf.read_text()) == [str(x) for x in w[1:p + 1]]
    # `zkey new` is the same command
    zf2 = tmp_path / "again.zkey"
    r = run("zkey", "new", rf, pf, zf2)
    assert r.returncode == 0, r.stderr
    assert zf2.read_bytes() == zf.read_bytes()
    # a missing ceremony file: exit 1 with snarkjs's error prefix
    r = run("groth16", "setup", rf, tmp_path / "missing.ptau", tmp_path / "x.zkey")
    err = [x for x in r.stderr.splitlines() if x.startswith("[ERROR] snarkJS:")]
    assert r.returncode == 1 and err and "cannot open" in err[0], r.stderr
