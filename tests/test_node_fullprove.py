"""`plonk fullprove` (alias `pkf`), plonk.fullProve and groth16.fullProveBatch through the Node.js host (nzcp-circom_amd/js):
the witness computed on the card and proved from where it lies.  The circuit is fullprove_circuits.tiny()."""
import json
import os
import shutil
import subprocess

import pytest

import fullprove_circuits as fc
from conftest import ROOT

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
pytestmark = pytest.mark.gpu
BLINDING = ",".join(str(1000 + 7 * k) for k in range(9))


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@pytest.fixture(scope="module")
def small(tmp_path_factory, amd):
    d = tmp_path_factory.mktemp("fullprove")
    c = fc.tiny()
    files = {"c.prog": c["prog"], "c.r1cs": c["r1cs"], "plonk.zkey": amd.plonk_setup(c["r1cs"], 9, device=0),
             "g16.zkey": amd.r1cs_setup(c["r1cs"], 5)[0],
             "good.json": json.dumps({"x": "7", "y": 6}).encode(), "bad.json": json.dumps({"x": 7, "y": 7}).encode(),
             "good2.json": json.dumps({"y": 2, "x": 3}).encode()}
    paths = {}
    for k, data in files.items():
        paths[k] = str(d / k)
        with open(paths[k], "wb") as fh:
            fh.write(data)
    return paths, d


def cli(*args):
    return subprocess.run(["node", CLI, *args], capture_output=True, text=True, timeout=300)


@needs_node
def test_cli_plonk_fullprove(addon, small):
    """fullprove == wtns calculate + plonk prove: the same public.json, a proof `plonk verify` accepts -- and, with the
    blinding fixed, the proof plonk.prove gives for the same witness and scalars.  A violating input writes nothing."""
    paths, d = small
    pj, uj, wt, vk = d / "proof.json", d / "public.json", d / "w.wtns", d / "vk.json"
    assert cli("zkey", "export", "verificationkey", paths["plonk.zkey"], str(vk)).returncode == 0
    assert cli("wc", paths["c.prog"], paths["good.json"], str(wt)).returncode == 0
    r = cli("plonk", "prove", paths["plonk.zkey"], str(wt), str(pj), str(uj))
    assert r.returncode == 0, r.stderr
    ref_public = uj.read_text()
    assert json.loads(ref_public) == ["42"]
    pj.unlink(), uj.unlink()
    for cmd in (["plonk", "fullprove"], ["pkf"]):
        r = cli(*cmd, paths["good.json"], paths["c.prog"], paths["plonk.zkey"], str(pj), str(uj))
        assert (r.returncode, r.stdout, r.stderr) == (0, "", "")
        assert uj.read_text() == ref_public
        r = cli("plonk", "verify", str(vk), str(uj), str(pj))
        assert (r.returncode, r.stdout) == (0, "[INFO]  snarkJS: OK!\n"), r.stderr
        pj.unlink(), uj.unlink()
    # the blinding fixed: the proof file equals plonk.prove's with the same nine scalars
    r = cli("pkf", paths["good.json"], paths["c.prog"], paths["plonk.zkey"], str(pj), str(uj), "--blinding", BLINDING)
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "")
    script = f"""
    const {{ plonk }} = require({json.dumps(JS)});
    (async () => {{
      const p = await plonk.createProver({json.dumps(paths["plonk.zkey"])});
      const res = await p.prove({json.dumps(str(wt))}, {{blinding: {json.dumps(BLINDING.split(","))}}});
      await p.close();
      console.log(JSON.stringify(res.proof, null, 1));
    }})();
    """
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == pj.read_text() + "\n" and uj.read_text() == ref_public
    pj.unlink(), uj.unlink()
    # a violating input: the check's text, exit status 1, no file; a usage error: exit status 2
    for cmd in (["plonk", "fullprove"], ["pkf"]):
        r = cli(*cmd, paths["bad.json"], paths["c.prog"], paths["plonk.zkey"], str(pj), str(uj))
        assert (r.returncode, r.stdout, r.stderr) == (1, "", f"[ERROR] snarkJS: {fc.TEXT}\n")
        assert not pj.exists() and not uj.exists()
    r = cli("plonk", "fullprove", paths["good.json"], paths["c.prog"])
    assert r.returncode == 2 and r.stderr.startswith("usage: cli.js plonk fullprove")


@needs_node
def test_api_fullprove_batch(addon, small):
    """groth16.fullProveBatch on three inputs, the middle one violating: the CLI's `g16f` outputs for the two good ones
    and {error} for the third; plonk.fullProveBatch likewise, its proofs accepted by plonk.verify."""
    paths, d = small
    common = ["--r", "5", "--s", "7"]
    exp = []
    for k in ("good.json", "good2.json"):
        pj, uj = d / f"{k}.proof", d / f"{k}.public"
        r = cli("g16f", paths[k], paths["c.prog"], paths["g16.zkey"], str(pj), str(uj), *common)
        assert r.returncode == 0, r.stderr
        exp.append({"proof": json.loads(pj.read_text()), "publicSignals": json.loads(uj.read_text())})
    inputs = [paths["good.json"], paths["bad.json"], paths["good2.json"]]
    script = f"""
    const {{ groth16, plonk, exportVerificationKey }} = require({json.dumps(JS)});
    (async () => {{
      const inputs = {json.dumps(inputs)};
      const g = await groth16.fullProveBatch(inputs, {json.dumps(paths["c.prog"])}, {json.dumps(paths["g16.zkey"])}, {{r: "5", s: "7"}});
      const p = await plonk.fullProveBatch(inputs, {json.dumps(paths["c.prog"])}, {json.dumps(paths["plonk.zkey"])});
      const vk = exportVerificationKey({json.dumps(paths["plonk.zkey"])});
      const ok = [];
      for (const x of p) ok.push(x.error !== undefined ? x.error : await plonk.verify(vk, x.publicSignals, x.proof));
      let rejected = null;
      try {{ await plonk.fullProve(inputs[1], {json.dumps(paths["c.prog"])}, {json.dumps(paths["plonk.zkey"])}); }} catch (e) {{ rejected = e.message; }}
      console.log(JSON.stringify({{g, ok, pubs: p.map((x) => x.publicSignals || null), rejected}}));
    }})();
    """
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert got["g"] == [exp[0], {"error": fc.TEXT}, exp[1]]
    assert got["ok"] == [True, fc.TEXT, True] and got["pubs"] == [["42"], None, ["6"]]
    assert got["rejected"] == fc.TEXT
