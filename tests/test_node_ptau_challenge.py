"""`snarkjs powersoftau export challenge`, `challenge contribute` and `import response` (aliases `ptec`, `ptcc`, `ptir`)
through the Node CLI on files, at power 3: the round trip writes the file and prints the hash of `powersoftau contribute`
with the same `-e` text; exit codes and printed lines."""
import hashlib
import os
import shutil
import subprocess

import pytest

from bn254 import R
from conftest import ROOT
from ptau_challenge_ref import challenge_contribute_ref, export_challenge_ref
from ptau_mpc_ref import contribute_ref
from ptau_prepared import write_ptau_prepared
from zkey_mpc_ref import blake2b

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
def test_node_export_challenge(addon, tmp_path):
    """Host only: runs without a device."""
    p0, ch = tmp_path / "pot_0000.ptau", tmp_path / "challenge_0001"
    p0.write_bytes(write_ptau_prepared(3, 1, 1, 1, prepared=False))
    r = _run("powersoftau", "export", "challenge", p0, ch)
    assert r.returncode == 0, r.stderr
    assert ch.read_bytes() == export_challenge_ref(p0.read_bytes())
    assert r.stdout == "[INFO]  snarkJS: Challenge Hash: \n" + _format_hash(blake2b(ch.read_bytes())) + "\n"
    again = tmp_path / "again"
    assert _run("ptec", p0, again).returncode == 0 and again.read_bytes() == ch.read_bytes()
    r = _run("powersoftau", "export", "challenge", tmp_path / "missing.ptau", tmp_path / "x")
    assert r.returncode == 1 and "cannot open" in _error_line(r) and not (tmp_path / "x").exists()
    assert _run("powersoftau", "export", "challenge", p0).returncode == 2
    # the other two commands check their inputs before they look for a device
    r = _run("powersoftau", "challenge", "contribute", "bls12381", ch, tmp_path / "x")
    assert r.returncode == 1 and "Curve not supported" in _error_line(r)
    (tmp_path / "short").write_bytes(ch.read_bytes()[:-1])
    r = _run("ptcc", "bn128", tmp_path / "short", tmp_path / "x", "-e=x")
    assert r.returncode == 1 and _error_line(r) == "[ERROR] snarkJS: ptau challenge: Invalid File format"
    r = _run("ptir", p0, ch, tmp_path / "x")
    assert r.returncode == 1 and _error_line(r) == "[ERROR] snarkJS: ptau import response: Invalid File format"
    assert not (tmp_path / "x").exists()
    assert _run("powersoftau", "challenge", "contribute", "bn128", ch).returncode == 2
    assert _run("powersoftau", "import", "response", p0, ch).returncode == 2


@needs_node
@pytest.mark.gpu
def test_node_exchange_round_trip(addon, tmp_path):
    p0, ch, resp, p1 = (tmp_path / x for x in ("pot_0000.ptau", "challenge_0001", "response_0001", "pot_0001.ptau"))
    assert _run("ptn", "bn128", 3, p0).returncode == 0
    assert _run("powersoftau", "export", "challenge", p0, ch).returncode == 0
    r = _run("powersoftau", "challenge", "contribute", "bn128", ch, resp, "-e=some random text")
    assert r.returncode == 0, r.stderr
    secret = _secret_from_text("some random text")
    want_resp, wh = challenge_contribute_ref(ch.read_bytes(), secret)
    assert resp.read_bytes() == want_resp
    assert r.stdout == "[INFO]  snarkJS: Contribution Hash: \n" + _format_hash(wh) + "\n"
    r = _run("powersoftau", "import", "response", p0, resp, p1, "--name=First contribution")
    assert r.returncode == 0, r.stderr
    want, wh2 = contribute_ref(p0.read_bytes(), "First contribution", secret)
    assert p1.read_bytes() == want and wh2 == wh
    assert r.stdout == "[INFO]  snarkJS: Contribution Hash: \n" + _format_hash(wh) + "\n"
    # the same file as `powersoftau contribute` with the same text writes
    direct = tmp_path / "direct.ptau"
    assert _run("ptc", p0, direct, "--name=First contribution", "-e=some random text").returncode == 0
    assert direct.read_bytes() == p1.read_bytes()
    # the aliases, one round later, without -e; the result verifies
    ch2, resp2, p2 = (tmp_path / x for x in ("challenge_0002", "response_0002", "pot_0002.ptau"))
    assert _run("ptec", p1, ch2).returncode == 0
    assert _run("ptcc", "bn128", ch2, resp2).returncode == 0
    assert _run("ptir", p1, resp2, p2, "-n=second").returncode == 0
    r = _run("powersoftau", "verify", p2)
    assert r.returncode == 0 and r.stdout == "[INFO]  snarkJS: Powers of tau Ok!\n", r.stderr
    # a response to another challenge: the check's text, exit 1, nothing written
    r = _run("powersoftau", "import", "response", p1, resp, tmp_path / "x.ptau")
    assert r.returncode == 1, r.stdout
    assert _error_line(r) == "[ERROR] snarkJS: ptau import response: the response does not answer this file's challenge"
    assert not (tmp_path / "x.ptau").exists()
