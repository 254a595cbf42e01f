"""`snarkjs powersoftau new`, `contribute` and `verify` (aliases `ptn`, `ptc`, `ptv`) through the Node CLI on files, at
power 4: the reproducible `-e` text gives the Python twin's bytes and contribution hash; exit codes and printed lines."""
import hashlib
import os
import shutil
import subprocess

import pytest

from bn254 import R
from conftest import ROOT
from ptau_mpc_ref import contribute_ref
from ptau_prepared import rewrite, sections, write_ptau_prepared

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


def _secret_from_text(text):
    """The CLI's own rule (not snarkjs's): Blake2b-512(text | byte j), halves reduced mod r, zero mapped to 1."""
    out = [0] * 6
    for j in range(3):
        h = hashlib.blake2b(text.encode() + bytes([j]), digest_size=64).digest()
        out[j] = int.from_bytes(h[:32], "little") % R or 1
        out[3 + j] = int.from_bytes(h[32:], "little") % R or 1
    return tuple(out)


def _format_hash(h):
    return "\n".join("\t\t" + " ".join(h[i * 16 + j * 4:i * 16 + j * 4 + 4].hex() for j in range(4)) for i in range(4))


def _run(*args):
    return subprocess.run(["node", os.path.join(JS, "cli.js"), *map(str, args)], capture_output=True, text=True, timeout=300)


def _error_line(r):
    err = [x for x in r.stderr.splitlines() if x.startswith("[ERROR] snarkJS:")]
    return err[0] if err else ""


@needs_node
def test_node_powersoftau_new(addon, tmp_path):
    """Host only: runs without a device."""
    p0 = tmp_path / "pot_0000.ptau"
    r = _run("powersoftau", "new", "bn128", 4, p0)
    assert r.returncode == 0, r.stderr
    assert p0.read_bytes() == write_ptau_prepared(4, 1, 1, 1, prepared=False)
    again = tmp_path / "again.ptau"
    assert _run("ptn", "bn128", 4, again).returncode == 0 and again.read_bytes() == p0.read_bytes()
    r = _run("powersoftau", "new", "bls12381", 4, tmp_path / "x.ptau")
    assert r.returncode == 1 and "Curve not supported" in _error_line(r), r.stderr
    r = _run("powersoftau", "new", "bn128", 25, tmp_path / "x.ptau")
    assert r.returncode == 1 and "limit of 24" in _error_line(r), r.stderr
    assert not (tmp_path / "x.ptau").exists()
    assert _run("powersoftau", "new", "bn128").returncode == 2


@needs_node
@pytest.mark.gpu
def test_node_new_contribute_verify(addon, tmp_path):
    p0, p1, p2 = (tmp_path / x for x in ("pot_0000.ptau", "pot_0001.ptau", "pot_0002.ptau"))
    assert _run("powersoftau", "new", "bn128", 4, p0).returncode == 0
    r = _run("powersoftau", "contribute", p0, p1, "--name=First contribution", "-e=some random text")
    assert r.returncode == 0, r.stderr
    want, wh = contribute_ref(p0.read_bytes(), "First contribution", _secret_from_text("some random text"))
    assert p1.read_bytes() == want
    assert r.stdout == "[INFO]  snarkJS: Contribution Hash: \n" + _format_hash(wh) + "\n"
    # `ptc` is the same command; without -e the secret is fresh
    r = _run("ptc", p1, p2, "-n=second", "-e=other text")
    assert r.returncode == 0, r.stderr
    want2, wh2 = contribute_ref(want, "second", _secret_from_text("other text"))
    assert p2.read_bytes() == want2 and _format_hash(wh2) in r.stdout
    p3 = tmp_path / "pot_0003.ptau"
    assert _run("ptc", p2, p3).returncode == 0 and _run("ptc", p2, tmp_path / "other.ptau").returncode == 0
    assert p3.read_bytes() != (tmp_path / "other.ptau").read_bytes()
    # verify: the printed line and the exit code
    for good in (p0, p1, p2, p3):
        r = _run("powersoftau", "verify", good)
        assert r.returncode == 0 and r.stdout == "[INFO]  snarkJS: Powers of tau Ok!\n", r.stderr
    assert _run("ptv", p3).returncode == 0
    bad = tmp_path / "bad.ptau"
    s7 = dict(sections(p1.read_bytes()))[7]
    bad.write_bytes(rewrite(p2.read_bytes(), lambda sid, d: s7 if sid == 7 else d))
    r = _run("powersoftau", "verify", bad)
    assert r.returncode == 1 and _error_line(r) == "[ERROR] snarkJS: ptau verify: the file's points are not the last contribution's", r.stderr
    # a missing input: exit 1 with snarkjs's error prefix, and no output file
    r = _run("powersoftau", "contribute", tmp_path / "missing.ptau", tmp_path / "x.ptau", "-e=x")
    assert r.returncode == 1 and "cannot open" in _error_line(r), r.stderr
    assert not (tmp_path / "x.ptau").exists()
    r = _run("powersoftau", "verify", tmp_path / "missing.ptau")
    assert r.returncode == 1 and "cannot open" in _error_line(r), r.stderr
    assert _run("powersoftau", "contribute", p0).returncode == 2
