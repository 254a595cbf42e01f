"""`nzcp program`, `wtns calculate` and `groth16 fullprove` through the Node.js host (nzcp-circom_amd/js), the witness on
the host route.  The small circuit is crafted here (wtns_prog_ref.py writes its witness program, formats.py its .r1cs):
    wires 1 = out (public), 2 = x, 3 = y;   out = x * y;   x - y - 1 = 0 (check 0: "x is not y + 1")
so an input with x != y + 1 violates a constraint.  `fullprove` needs the prover, hence a card."""
import json
import os
import shutil
import subprocess

import pytest

import formats as f
import wtns_prog_ref as ref
from conftest import ROOT

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
TEXT = "x is not y + 1"


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("wcalc")
    ops = [("input", 2, 0), ("input", 3, 1), ("quad", 1, [(2, 1)], [(3, 1)], []), ("check", [(2, 1), (3, -1), (0, -1)], 0)]
    prog = ref.write(4, ops, [TEXT], n_public=1, inputs=[("x", 0, 1), ("y", 1, 1)], outputs=[1])
    rows = [([(2, 1)], [(3, 1)], [(1, 1)]), ([(2, 1), (3, ref.R - 1), (0, ref.R - 1)], [(0, 1)], [])]
    paths = {k: str(d / k) for k in ("c.prog", "c.r1cs", "good.json", "bad.json")}
    for k, data in (("c.prog", prog), ("c.r1cs", f.write_r1cs(4, 1, 0, rows)),
                    ("good.json", json.dumps({"x": "7", "y": 6}).encode()), ("bad.json", json.dumps({"x": 7, "y": 7}).encode())):
        with open(paths[k], "wb") as fh:
            fh.write(data)
    return paths, d


def cli(*args):
    return subprocess.run(["node", CLI, *args], capture_output=True, text=True, timeout=300)


@needs_node
def test_cli_wtns_calculate(addon, small, amd):
    paths, d = small
    for n, cmd in enumerate((["wtns", "calculate"], ["wc"])):
        out = str(d / f"w{n}.wtns")
        r = cli(*cmd, paths["c.prog"], paths["good.json"], out)
        assert (r.returncode, r.stdout, r.stderr) == (0, "", "")
        assert f.read_wtns(open(out, "rb").read())["w"] == [1, 42, 7, 6]
        assert amd.wtns_check(paths["c.r1cs"], out, device=-1).ok
        # a violating input: the check's text, exit status 1, no file
        bad = str(d / f"bad{n}.wtns")
        r = cli(*cmd, paths["c.prog"], paths["bad.json"], bad)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", f"[ERROR] snarkJS: {TEXT}\n")
        assert not os.path.exists(bad)
    # inputs that do not match the program's table, a file that is no program
    (d / "extra.json").write_text(json.dumps({"x": 1, "y": 0, "z": 3}))
    r = cli("wc", paths["c.prog"], str(d / "extra.json"), str(d / "no.wtns"))
    assert (r.returncode, r.stderr) == (1, "[ERROR] snarkJS: wtns calculate: the program has no input z\n")
    (d / "short.json").write_text(json.dumps({"x": 1}))
    r = cli("wc", paths["c.prog"], str(d / "short.json"), str(d / "no.wtns"))
    assert (r.returncode, r.stderr) == (1, "[ERROR] snarkJS: wtns calculate: input y is missing\n")
    r = cli("wc", paths["c.r1cs"], paths["good.json"], str(d / "no.wtns"))
    assert (r.returncode, r.stderr) == (1, "[ERROR] snarkJS: wprg: Invalid File format\n")
    assert not os.path.exists(d / "no.wtns")
    r = cli("wtns", "calculate", paths["c.prog"])
    assert r.returncode == 2 and r.stderr.startswith("usage: cli.js wtns calculate")


@needs_node
def test_cli_nzcp_program_and_api(addon, small, amd, tmp_path):
    """`nzcp program example` writes the image nzcp_witness_program gives; a template's program through the API computes
    what the Python binding computes."""
    out = tmp_path / "example.prog"
    r = cli("nzcp", "program", "example", str(out))
    assert (r.returncode, r.stdout, r.stderr) == (0, "", "")
    assert out.read_bytes() == amd.nzcp_witness_program(amd.NZCP_EXAMPLE_PARAMS)
    r = cli("nzcp", "program", "neither", str(tmp_path / "no.prog"))
    assert r.returncode == 1 and "nzcp program: expected" in r.stderr and not (tmp_path / "no.prog").exists()
    gp, gw = tmp_path / "quin.prog", tmp_path / "quin.wtns"
    script = f"""
    const {{ wtns, nzcp }} = require({json.dumps(JS)});
    (async () => {{
      await nzcp.gadgetProgram("quinSelector", [3], {json.dumps(str(gp))});
      await wtns.calculate({{in: [11, 22, 33, 2]}}, {json.dumps(str(gp))}, {json.dumps(str(gw))});
      try {{ await wtns.calculate({{in: [11, 22, 33, 200]}}, {json.dumps(str(gp))}, {json.dumps(str(gw))} + ".bad"); }}
      catch (e) {{ console.log(e.message); }}
    }})();
    """
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=300)
    assert (r.returncode, r.stdout) == (0, "QuinSelector: index out of range\n"), r.stderr
    assert gp.read_bytes() == amd.nzcp_gadget_program("quinSelector", [3])
    calc = amd.WitnessCalculator(str(gp), device=-1)
    assert gw.read_bytes() == calc.wtns([11, 22, 33, 2]) and not os.path.exists(str(gw) + ".bad")


@needs_node
@pytest.mark.gpu
def test_cli_groth16_fullprove(addon, small, amd):
    """fullprove == wtns calculate + prove with the same r, s; a violating input writes nothing."""
    paths, d = small
    zkey, _ = amd.r1cs_setup(open(paths["c.r1cs"], "rb").read(), 5)
    zk = d / "c.zkey"
    zk.write_bytes(zkey)
    pj, uj, wt = d / "proof.json", d / "public.json", d / "full.wtns"
    common = ["--r", "5", "--s", "7"]
    for cmd in (["groth16", "fullprove"], ["g16f"]):
        r = cli(*cmd, paths["good.json"], paths["c.prog"], str(zk), str(pj), str(uj), *common)
        assert (r.returncode, r.stdout, r.stderr) == (0, "", "")
        full = (pj.read_text(), uj.read_text())
        pj.unlink(), uj.unlink()
        assert json.loads(full[1]) == ["42"]
    assert cli("wc", paths["c.prog"], paths["good.json"], str(wt)).returncode == 0
    r = cli("groth16", "prove", str(zk), str(wt), str(pj), str(uj), *common)
    assert r.returncode == 0, r.stderr
    assert (pj.read_text(), uj.read_text()) == full
    pj.unlink(), uj.unlink()
    r = cli("groth16", "fullprove", paths["bad.json"], paths["c.prog"], str(zk), str(pj), str(uj), *common)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", f"[ERROR] snarkJS: {TEXT}\n")
    assert not pj.exists() and not uj.exists()
