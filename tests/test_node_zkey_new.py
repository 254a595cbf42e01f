"""`zkey new --cshash` through the Node CLI on files: the key of test_gpu_zkey_new's closed-form test (the legacy key
with the circuit hash at the head of section 10, the hash = hashlib's Blake2b-512 over the twin's MPCParams image with
the closed-form H run), `zKey.csHash` of the legacy key gives the same bytes, and without the flag the command writes
what it always wrote."""
import os
import shutil
import subprocess

import pytest

import formats as f
import groth16 as g
import synth
import zkey_bellman_ref as ref
import zkey_mpc_ref as mref
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
def test_node_zkey_new_with_and_without_the_circuit_hash(addon, tmp_path):
    n, p, m, seed = 24, 2, 12, 1          # domain 2^4
    rows, _ = synth.make(n, p, m, seed)
    t = g.trapdoor(seed + 7)
    td = {"tau": t["tau"], "alpha": t["alpha"], "beta": t["beta"], "gamma": 1, "delta": 1}
    zk, _ = g.setup(n, p, rows, td)
    legacy = f.write_zkey(zk)
    rf, pf = tmp_path / "c.r1cs", tmp_path / "pot.ptau"
    rf.write_bytes(f.write_r1cs(n, p, 0, rows))
    pf.write_bytes(write_ptau_prepared(4, td["tau"], td["alpha"], td["beta"]))
    cli = os.path.join(JS, "cli.js")

    def run(*args):
        return subprocess.run(["node", cli, *map(str, args)], capture_output=True, text=True, timeout=300)

    sections = ref.key_sections(legacy)
    image = ref.write_mpcparams(sections, ref.run_be(ref.points(ref.h_closed_form(td["tau"], 16, 1)), 64))
    want = mref.blake2b(image[:ref.parse_mpcparams(image)["at"]["csHash"]])

    zf = tmp_path / "c_0000.zkey"
    r = run("zkey", "new", rf, pf, zf, "--cshash")
    assert r.returncode == 0, r.stderr
    got = ref.key_sections(zf.read_bytes())
    for sid in range(1, 10):
        assert got[sid] == sections[sid], f"section {sid}"
    assert got[10] == want + bytes(4)
    assert "Circuit Hash" in r.stdout and "%08x" % int.from_bytes(want[:4], "big") in r.stdout
    r = run("groth16", "setup", rf, pf, tmp_path / "again.zkey", "--cshash")
    assert r.returncode == 0 and (tmp_path / "again.zkey").read_bytes() == zf.read_bytes()

    # without the flag: the legacy key, and nothing printed
    for cmd in (("zkey", "new"), ("groth16", "setup")):
        out = tmp_path / ("plain_%s.zkey" % cmd[0])
        r = run(*cmd, rf, pf, out)
        assert r.returncode == 0, r.stderr
        assert out.read_bytes() == legacy and r.stdout == ""

    # the library entry, the hash of the legacy key alone, and the verifier on both keys
    lf = tmp_path / "plain_zkey.zkey"
    script = ("const { zKey } = require(%r); (async () => { const h = await zKey.csHash(%r, %r); "
              "const h2 = await zKey.newZKey(%r, %r, %r, { csHash: true }); "
              "console.log(Buffer.from(h).toString('hex')); console.log(Buffer.from(h2).toString('hex')); })()"
              % (os.path.join(JS, "index.js"), str(lf), str(pf), str(rf), str(pf), str(tmp_path / "lib.zkey")))
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [want.hex(), want.hex()]
    assert (tmp_path / "lib.zkey").read_bytes() == zf.read_bytes()
    for key in (zf, lf):
        r = run("zkey", "verify", rf, pf, key)
        assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr
