"""The ptau leg of `zkey verify` through the Node CLI and API on files: `zkvi` opens the ptau it is given and rejects a
ceremony of another tau, `--skip-ptau` restores the check without the leg, `zkv` sets the initial key up in memory and
leaves no file behind, and zKey.verifyFromR1cs tells an honest key from one with a forged H basis."""
import json
import os
import shutil
import subprocess

import pytest

import formats as f
import groth16 as g
import synth
from bn254 import R
from conftest import ROOT

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
H_TEXT = "zkey verify: section 9 is not the ceremony's H basis scaled by 1 / delta"


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@needs_node
@pytest.mark.gpu
def test_node_zkey_verify_with_the_ptau(amd, addon, tmp_path):
    n, p, m, seed = 24, 2, 12, 1          # domain 2^4
    rows, _ = synth.make(n, p, m, seed)
    t = g.trapdoor(seed + 7)
    ptau = amd.ptau_synth(4, t["tau"], t["alpha"], t["beta"], device=0)
    r1cs = f.write_r1cs(n, p, 0, rows)
    init = amd.groth16_setup_ptau(r1cs, ptau, device=0)
    one, _ = amd.zkey_contribute(init, "first", 0x1f2e3d4c5b6a7988 ** 3 % R, 0x0123456789abcdef ** 3 % R, device=0)
    secs = f.read_binfile(one, "zkey", 2)
    pos, _ = secs[9][0]
    forged = one[:pos] + one[pos + 64:pos + 128] + one[pos:pos + 64] + one[pos + 128:]
    assert forged != one
    files = {"c.r1cs": r1cs, "pot.ptau": ptau, "c_0000.zkey": init, "c_0001.zkey": one, "forged.zkey": forged,
             "other.ptau": amd.ptau_synth(4, (t["tau"] + 1) % R, t["alpha"], t["beta"], prepared=False, device=0)}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    path = {name: str(tmp_path / name) for name in files}
    cli = os.path.join(JS, "cli.js")

    def run(*args):
        return subprocess.run(["node", cli, *args], capture_output=True, text=True, timeout=300)
    # the ptau is opened: a ceremony of another tau
    r = run("zkvi", path["c_0000.zkey"], path["other.ptau"], path["c_0001.zkey"])
    err = [x for x in r.stderr.splitlines() if x.startswith("[ERROR] snarkJS:")]
    assert r.returncode == 1 and err and H_TEXT in err[0], r.stderr
    r = run("zkvi", path["c_0000.zkey"], path["other.ptau"], path["c_0001.zkey"], "--skip-ptau")
    assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr
    r = run("zkey", "verify", "frominit", path["c_0000.zkey"], path["pot.ptau"], path["c_0001.zkey"])
    assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr
    # from the .r1cs: in memory
    r = run("zkv", path["c.r1cs"], path["pot.ptau"], path["c_0001.zkey"])
    assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr
    assert sorted(x.name for x in tmp_path.iterdir()) == sorted(files)
    script = ("const { zKey } = require(%s); (async () => { const out = [];"
              " for (const z of %s) out.push(await zKey.verifyFromR1cs(%s, %s, z));"
              " console.log(JSON.stringify(out)); })().catch((e) => { console.error(e); process.exit(1); });"
              % (json.dumps(os.path.join(JS, "index.js")), json.dumps([path["c_0001.zkey"], path["forged.zkey"]]),
                 json.dumps(path["c.r1cs"]), json.dumps(path["pot.ptau"])))
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [True, False]
    assert sorted(x.name for x in tmp_path.iterdir()) == sorted(files)
