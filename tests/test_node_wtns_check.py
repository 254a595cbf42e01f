"""`wtns check` through the Node.js host (nzcp-circom_amd/js): the CLI command and its alias `wchk`, `prove --check`
and `wtns.check`.  The CPU part runs the host route (--device -1); the GPU part the device route and the prover.  The
texts are modelled on later snarkjs releases and are not compared with snarkjs (the pinned 0.4.12 has no such command)."""
import json
import os
import shutil
import subprocess

import pytest

import formats as f
import wtns_check_ref as ref
from conftest import ROOT

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A small circuit with rows of all three length classes: paths of its .r1cs, a good and a bad witness."""
    d = tmp_path_factory.mktemp("wchk")
    b = ref.Builder(seed=11)
    for _ in range(5):
        b.short_row()
    b.long_row(2, 30)
    b.long_row(0, 80)
    bad = b.broken(6, 3)
    paths = {k: str(d / k) for k in ("c.r1cs", "good.wtns", "bad.wtns")}
    for k, data in zip(paths, (b.r1cs(), b.wtns(), b.wtns(bad))):
        with open(paths[k], "wb") as fh:
            fh.write(data)
    return paths, ref.verdict(b.rows, bad)


def cli(*args):
    return subprocess.run(["node", CLI, *args], capture_output=True, text=True, timeout=300)


def failure_text(v):
    return ("[ERROR] snarkJS: WITNESS CHECKING FAILED\n"
            f"constraint {v['constraint']} is not satisfied ({v['n_failed']} in all)\n"
            f"a = {v['a']}\nb = {v['b']}\nc = {v['c']}\n")


def check_cli(files, device):
    paths, want = files
    for cmd in (["wtns", "check"], ["wchk"]):
        r = cli(*cmd, paths["c.r1cs"], paths["good.wtns"], "--device", device)
        assert (r.returncode, r.stdout, r.stderr) == (0, "WITNESS IS CORRECT\n", "")
        r = cli(*cmd, paths["c.r1cs"], paths["bad.wtns"], "--device", device)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", failure_text(want))
    r = cli("wtns", "check", paths["c.r1cs"], paths["c.r1cs"], "--device", device)
    assert (r.returncode, r.stderr) == (1, "[ERROR] snarkJS: wtns: Invalid File format\n")
    r = cli("wtns", "check", paths["c.r1cs"])
    assert r.returncode == 2 and r.stderr.startswith("usage: cli.js wtns check")


def check_api(files, device):
    paths, want = files
    script = f"""
    const {{ wtns }} = require({json.dumps(JS)});
    (async () => {{
      const out = [];
      for (const w of [{json.dumps(paths["good.wtns"])}, {json.dumps(paths["bad.wtns"])}])
        out.push(await wtns.check({json.dumps(paths["c.r1cs"])}, w, {{device: {device}}}));
      try {{ await wtns.check({json.dumps(paths["c.r1cs"])}, {json.dumps(paths["c.r1cs"])}, {{device: {device}}}); }}
      catch (e) {{ out.push(e.message); }}
      console.log(JSON.stringify(out));
    }})();
    """
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    good, bad, err = json.loads(r.stdout)
    assert good == {"ok": True, "constraint": -1, "nFailed": 0, "a": "0", "b": "0", "c": "0"}
    assert bad == {"ok": False, "constraint": want["constraint"], "nFailed": want["n_failed"],
                   "a": str(want["a"]), "b": str(want["b"]), "c": str(want["c"])}
    assert err == "wtns: Invalid File format"


@needs_node
def test_cli_wtns_check_host_route(addon, files):
    check_cli(files, "-1")


@needs_node
def test_node_wtns_check_host_route(addon, files, amd):
    check_api(files, -1)
    # the same fields as Python
    paths, want = files
    assert ref.as_dict(amd.wtns_check(paths["c.r1cs"], paths["bad.wtns"], device=-1)) == want


@needs_node
@pytest.mark.gpu
def test_cli_wtns_check_device(addon, files):
    check_cli(files, "0")


@needs_node
@pytest.mark.gpu
def test_node_wtns_check_device(addon, files, amd):
    check_api(files, 0)
    paths, want = files
    assert ref.as_dict(amd.wtns_check(paths["c.r1cs"], paths["bad.wtns"], device=0)) == want


@needs_node
@pytest.mark.gpu
def test_cli_prove_check(addon, amd, tmp_path):
    """`prove --check circuit.r1cs` stops on a bad witness with the report of `wtns check`, exit status 1 and no proof
    file; a good witness is proved as without the flag."""
    out = amd.sha256_message_setup(b"abc", 7, want_zkey=True, want_r1cs=True)
    rows = f.read_r1cs(out["r1cs"])["rows"]
    w = f.read_wtns(out["wtns"])["w"]
    bad = list(w)
    bad[300] ^= 1   # a message bit
    want = ref.verdict(rows, bad)
    assert not want["ok"]
    for name, data in (("c.zkey", out["zkey"]), ("c.r1cs", out["r1cs"]), ("good.wtns", out["wtns"]), ("bad.wtns", f.write_wtns(bad))):
        (tmp_path / name).write_bytes(data)
    pj, uj = tmp_path / "proof.json", tmp_path / "public.json"
    common = ["--r", "5", "--s", "7"]
    r = cli("groth16", "prove", str(tmp_path / "c.zkey"), str(tmp_path / "bad.wtns"), str(pj), str(uj), "--check",
            str(tmp_path / "c.r1cs"), *common)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", failure_text(want))
    assert not pj.exists() and not uj.exists()
    r = cli("prove", str(tmp_path / "c.zkey"), str(tmp_path / "good.wtns"), str(pj), str(uj), "--check", str(tmp_path / "c.r1cs"), *common)
    assert r.returncode == 0, r.stderr
    checked = (pj.read_text(), uj.read_text())
    pj.unlink(); uj.unlink()
    r = cli("prove", str(tmp_path / "c.zkey"), str(tmp_path / "good.wtns"), str(pj), str(uj), *common)
    assert r.returncode == 0, r.stderr
    assert (pj.read_text(), uj.read_text()) == checked
