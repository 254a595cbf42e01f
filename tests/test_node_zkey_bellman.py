"""The phase-2 MPCParams exchange through the Node CLI on files: `zkey export bellman`, `zkey bellman contribute`, `zkey
import bellman` and their aliases `zkeb`, `zkbc`, `zkib` -- the same key and printed hash as `zkey contribute` with the
same -e text, a refused response with exit status 1 and the verdict's text, usage errors with exit status 2."""
import hashlib
import os
import shutil
import subprocess

import pytest

import formats as f
import groth16 as g
import synth
import zkey_bellman_ref as ref
import zkey_mpc_ref as mref
from bn254 import R
from conftest import ROOT
from ptau_prepared import write_ptau_prepared

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


def _run(*args):
    return subprocess.run(["node", CLI, *map(str, args)], capture_output=True, text=True, timeout=300)


@needs_node
@pytest.mark.parametrize("args", [("zkey", "export", "bellman", "only.zkey"), ("zkeb",), ("zkey", "bellman", "contribute", "bn128", "c"),
                                  ("zkbc", "c", "r"), ("zkey", "import", "bellman", "old.zkey", "resp"), ("zkib", "--name=x")])
def test_usage_errors_exit_2(addon, args):
    r = _run(*args)
    assert r.returncode == 2 and r.stderr.startswith("usage: cli.js zkey "), r.stderr


@needs_node
def test_another_curve_is_refused(addon, tmp_path):
    r = _run("zkbc", "bls12381", tmp_path / "c", tmp_path / "r")
    assert r.returncode == 1 and "Curve not supported: bls12381" in r.stderr


@needs_node
@pytest.mark.gpu
def test_node_export_contribute_import(addon, tmp_path):
    n, p, m, seed = 24, 2, 12, 1   # the small case
    rows, _ = synth.make(n, p, m, seed)
    t = g.trapdoor(seed + 1000)
    rf, pf = tmp_path / "c.r1cs", tmp_path / "pot.ptau"
    z0, z1, z1p, z1q = (tmp_path / x for x in ("c_0000.zkey", "c_0001.zkey", "c_0001_imported.zkey", "c_0001_alias.zkey"))
    ch, resp, ch2, resp2 = (tmp_path / x for x in ("c.mpcparams", "c_response.mpcparams", "c_alias.mpcparams", "c_alias_response.mpcparams"))
    rf.write_bytes(f.write_r1cs(n, p, 0, rows))
    pf.write_bytes(write_ptau_prepared(4, t["tau"], t["alpha"], t["beta"]))
    assert _run("groth16", "setup", rf, pf, z0).returncode == 0
    r = _run("zkey", "contribute", z0, z1, "--name=first", "-e=abc")
    assert r.returncode == 0, r.stderr
    direct_out = r.stdout

    r = _run("zkey", "export", "bellman", z0, ch)
    assert r.returncode == 0, r.stderr
    N = 16
    sec = ref.key_sections(z0.read_bytes())
    assert ch.read_bytes() == ref.write_mpcparams(sec, ref.run_be(ref.points(ref.h_closed_form(t["tau"], N)), 64))
    r = _run("zkey", "bellman", "contribute", "bn128", ch, resp, "-e=abc")
    assert r.returncode == 0, r.stderr
    h = hashlib.blake2b(b"abc", digest_size=64).digest()
    d, s = (int.from_bytes(h[k:k + 32], "little") % R or 1 for k in (0, 32))
    _, _, want_hash = mref.contribute_ref(z0.read_bytes(), "first", d, s)
    block = "\n".join("\t\t" + " ".join(want_hash[16 * i + 4 * j:16 * i + 4 * j + 4].hex() for j in range(4)) for i in range(4))
    assert "Contribution Hash: \n" + block in r.stdout and block in direct_out, r.stdout
    r = _run("zkey", "import", "bellman", z0, resp, z1p, "--name=first")
    assert r.returncode == 0, r.stderr
    a, bb = ref.key_sections(z1.read_bytes()), ref.key_sections(z1p.read_bytes())
    for sid in (1, 2, 3, 4, 5, 6, 7, 8, 10):
        assert a[sid] == bb[sid], f"section {sid}"
    r = _run("zkey", "verify", "frominit", z0, pf, z1p)
    assert r.returncode == 0 and "ZKey Ok!" in r.stdout, r.stderr

    # the aliases: the same files
    assert _run("zkeb", z0, ch2).returncode == 0 and ch2.read_bytes() == ch.read_bytes()
    assert _run("zkbc", "bn128", ch2, resp2, "-e=abc").returncode == 0 and resp2.read_bytes() == resp.read_bytes()
    assert _run("zkib", z0, resp2, z1q, "--name=first").returncode == 0 and z1q.read_bytes() == z1p.read_bytes()

    # a response without a new record: the verdict, exit 1, nothing written
    out = tmp_path / "never.zkey"
    r = _run("zkey", "import", "bellman", z0, ch, out)
    assert r.returncode == 1 and "[ERROR] snarkJS: zkey import bellman: the response holds no new contribution" in r.stderr, r.stderr
    assert not out.exists()
    r = _run("zkib", z0, rf, out)
    assert r.returncode == 1 and "mpcparams: Invalid File format" in r.stderr and not out.exists()
