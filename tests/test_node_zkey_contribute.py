"""`zkey contribute` and `zkey verify` through the Node CLI on files: setup from a prepared ptau, a contribution, the
chain check, then `zkey export verificationkey`, `groth16 prove` and `groth16 verify` with the contributed key."""
import hashlib
import os
import shutil
import subprocess

import pytest

import formats as f
import groth16 as g
import synth
import zkey_mpc_ref as ref
from bn254 import R
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
def test_node_contribute_verify_prove(addon, tmp_path):
    n, p, m, seed = 60, 5, 40, 3
    rows, w = synth.make(n, p, m, seed)
    t = g.trapdoor(seed + 7)
    rf, pf, wf = tmp_path / "c.r1cs", tmp_path / "pot.ptau", tmp_path / "w.wtns"
    z0, z1, z1b = tmp_path / "c_0000.zkey", tmp_path / "c_0001.zkey", tmp_path / "c_0001_again.zkey"
    rf.write_bytes(f.write_r1cs(n, p, 0, rows))
    pf.write_bytes(write_ptau_prepared(6, t["tau"], t["alpha"], t["beta"]))
    wf.write_bytes(f.write_wtns(w))
    cli = os.path.join(JS, "cli.js")

    def run(*args):
        return subprocess.run(["node", cli, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert run("groth16", "setup", rf, pf, z0).returncode == 0
    r = run("zkey", "contribute", z0, z1, "--name=first", "-e=abc")
    assert r.returncode == 0, r.stderr
    # the secret as the CLI documents it, the key and the printed hash as the twin computes them
    h = hashlib.blake2b(b"abc", digest_size=64).digest()
    d, s = (int.from_bytes(h[k:k + 32], "little") % R or 1 for k in (0, 32))
    want_h, want_s10, want_hash = ref.contribute_ref(z0.read_bytes(), "first", d, s)
    new = z1.read_bytes()
    secs = f.read_binfile(new, "zkey", 2)
    assert f.section(new, secs, 2) == want_h and f.section(new, secs, 10) == want_s10
    block = "\n".join("\t\t" + " ".join(want_hash[16 * i + 4 * j:16 * i + 4 * j + 4].hex() for j in range(4)) for i in range(4))
    assert "Contribution Hash: \n" + block in r.stdout, r.stdout
    # the same entropy: the same file (alias zkc)
    assert run("zkc", z0, z1b, "--name=first", "-e=abc").returncode == 0
    assert z1b.read_bytes() == new
    r = run("zkey", "verify", "frominit", z0, pf, z1)
    assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr
    r = run("zkey", "verify", rf, pf, z1)
    assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr
    assert sorted(x.name for x in tmp_path.iterdir()) == sorted(x.name for x in (rf, pf, wf, z0, z1, z1b))
    vkf, prf, puf = tmp_path / "vk.json", tmp_path / "proof.json", tmp_path / "public.json"
    assert run("zkey", "export", "verificationkey", z1, vkf).returncode == 0
    r = run("groth16", "prove", z1, wf, prf, puf)
    assert r.returncode == 0, r.stderr
    r = run("groth16", "verify", vkf, puf, prf)
    assert r.returncode == 0 and "snarkJS: OK!" in r.stdout, r.stderr
    # a tampered key: two points of section 9 swapped
    pos, size = secs[9][0]
    bad = bytearray(new)
    bad[pos:pos + 64], bad[pos + 64:pos + 128] = new[pos + 64:pos + 128], new[pos:pos + 64]
    assert bytes(bad) != new
    zb = tmp_path / "bad.zkey"
    zb.write_bytes(bytes(bad))
    r = run("zkvi", z0, pf, zb)
    err = [x for x in r.stderr.splitlines() if x.startswith("[ERROR] snarkJS:")]
    assert r.returncode == 1 and err and "zkey verify:" in err[0], r.stderr
