"""nzcp.provePasses and `nzcp prove` through the Node.js host (nzcp-circom_amd/js): pass URIs in, Groth16 proofs out in one
native call (g16_pass_fullprove_batch).  The circuit is pass_prove_circuits.pack(320); the proofs are checked with
groth16.verify, the public signals against Python's packing of the ToBeSigned bytes."""
import json
import os
import shutil
import subprocess

import pytest

import pass_cases as pc
import pass_prove_circuits as ppc
from conftest import ROOT

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@pytest.fixture(scope="module")
def files(tmp_path_factory, amd):
    d = tmp_path_factory.mktemp("passprove")
    c = ppc.pack(ppc.M_MAIN)
    good = ppc.good_passes(2)
    uris = [good[0], ppc.base_pass(odd=True), good[1], pc.make(exp=pc.NOW - 5, cti=bytes(16))]
    data = {"c.prog": c["prog"], "g16.zkey": amd.r1cs_setup(c["r1cs"], 5)[0], "keys.json": json.dumps(pc.key_set()[0]).encode(),
            "passes.txt": ("\n".join(uris) + "\n").encode()}
    paths = {}
    for k, b in data.items():
        paths[k] = str(d / k)
        with open(paths[k], "wb") as fh:
            fh.write(b)
    return paths, d, uris


@needs_node
def test_prove_passes(addon, files):
    """two good passes, one the circuit refuses and one that has expired: outcomes, texts, and proofs that verify"""
    paths, d, uris = files
    vk = d / "vk.json"
    r = subprocess.run(["node", CLI, "zkey", "export", "verificationkey", paths["g16.zkey"], str(vk)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    script = f"""
    const {{ nzcp, groth16 }} = require({json.dumps(JS)});
    const fs = require("fs");
    (async () => {{
      const opts = {{ program: {json.dumps(paths["c.prog"])}, zkey: fs.readFileSync({json.dumps(paths["g16.zkey"])}),
                     keys: JSON.parse(fs.readFileSync({json.dumps(paths["keys.json"])}, "utf-8")), now: {pc.NOW} }};
      const uris = fs.readFileSync({json.dumps(paths["passes.txt"])}, "utf-8").split("\\n").filter((x) => x);
      const res = await nzcp.provePasses(uris, opts);
      const vk = JSON.parse(fs.readFileSync({json.dumps(str(vk))}, "utf-8"));
      const ok = [];
      for (const r of res) ok.push(r.proof ? await groth16.verify(vk, r.publicSignals, r.proof) : null);
      const unsigned = await nzcp.provePasses(uris.slice(3), Object.assign({{ unsigned: true }}, opts));
      console.log(JSON.stringify({{ res, ok, unsigned, outcomes: nzcp.PROVE_OUTCOMES, reasons: nzcp.PASS_REASONS }}));
    }})();
    """
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["outcomes"] == ["done", "pass", "tooLong", "check", "mismatch"]
    assert [x["outcome"] for x in out["res"]] == ["done", "check", "done", "pass"]
    assert out["ok"] == [True, None, True, None]
    assert [x["text"] for x in out["res"]] == [None, ppc.TEXT, None, out["reasons"]["expired"]]
    for x, u in zip(out["res"], uris):
        if x["outcome"] == "done":
            assert [int(s) for s in x["publicSignals"]] == ppc.public_values(ppc.tbs_of(u), ppc.M_MAIN)
        else:
            assert x["proof"] is None and x["publicSignals"] is None
    assert [x["pass"]["ok"] for x in out["res"]] == [True, True, True, False]
    assert out["res"][3]["pass"]["exp"] == pc.NOW - 5
    # unsigned: the expired pass is proved, its verdict still recorded
    (u,) = out["unsigned"]
    assert u["outcome"] == "done" and u["pass"]["reason"] == out["reasons"]["expired"] and u["proof"] is not None


@needs_node
def test_cli_prove(addon, files):
    paths, d, uris = files
    out_dir = d / "out"
    out_dir.mkdir()
    r = subprocess.run(["node", CLI, "nzcp", "prove", paths["passes.txt"], paths["c.prog"], paths["g16.zkey"], "--keys", paths["keys.json"],
                        "--now", str(pc.NOW), "--out", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["pass 0: PROVED", f"pass 1: NOT PROVED (check) {ppc.TEXT}", "pass 2: PROVED",
                                     "pass 3: NOT PROVED (pass) the pass has expired (exp)"]
    assert sorted(os.listdir(out_dir)) == ["proof_0.json", "proof_2.json", "public_0.json", "public_2.json"]
    assert [int(s) for s in json.loads((out_dir / "public_2.json").read_text())] == ppc.public_values(ppc.tbs_of(uris[2]), ppc.M_MAIN)
    r = subprocess.run(["node", CLI, "nzcp", "prove", uris[0], paths["c.prog"], paths["g16.zkey"], "--keys", paths["keys.json"],
                        "--now", str(pc.NOW)], capture_output=True, text=True, timeout=300)
    assert (r.returncode, r.stdout) == (0, "pass 0: PROVED\n"), r.stderr
