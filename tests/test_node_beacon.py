"""`snarkjs powersoftau beacon` and `zkey beacon` (aliases `ptb`, `zkb`) through the Node CLI on files, at power 4 and on
tests/golden/tiny.zkey: the bytes and the printed contribution hash are the Python route's; a bad hex string is a usage
error (exit 2), a value out of range an error of the library (exit 1), and neither writes a file."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, golden_path

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
BEACON = bytes((37 * i + 11) & 0xff for i in range(32))
EXP = 10


@pytest.fixture(scope="module")
def addon():
    subprocess.check_call(["make", "-C", os.path.join(JS, "addon")], stdout=subprocess.DEVNULL)
    return os.path.join(JS, "addon", "g16_napi.node")


def _format_hash(h):
    return "\n".join("\t\t" + " ".join(h[i * 16 + j * 4:i * 16 + j * 4 + 4].hex() for j in range(4)) for i in range(4))


def _run(*args):
    return subprocess.run(["node", os.path.join(JS, "cli.js"), *map(str, args)], capture_output=True, text=True, timeout=300)


def _error_line(r):
    err = [x for x in r.stderr.splitlines() if x.startswith("[ERROR] snarkJS:")]
    return err[0] if err else ""


def _inputs(amd, tmp_path):
    old_ptau, old_zkey = tmp_path / "pot_0000.ptau", tmp_path / "circuit_0000.zkey"
    old_ptau.write_bytes(amd.ptau_new(4))
    shutil.copyfile(golden_path("tiny.zkey"), old_zkey)
    return [("powersoftau", "ptb", old_ptau, ".ptau"), ("zkey", "zkb", old_zkey, ".zkey")]


@needs_node
def test_node_beacon_usage_and_range_errors(amd, addon, tmp_path):
    """Everything here ends before the device is asked for: runs without one."""
    for group, alias, old, ext in _inputs(amd, tmp_path):
        out = tmp_path / ("x" + ext)
        for cmd in ([group, "beacon"], [alias]):
            for args in ([old, out, "abc", EXP], [old, out, "zz" + BEACON.hex()[2:], EXP], [old, out, BEACON.hex()], [old, out],
                         [old, out, BEACON.hex(), "ten"]):
                r = _run(*cmd, *args)
                assert r.returncode == 2 and r.stderr.startswith("usage: cli.js " + group + " beacon "), (args, r.stderr)
            for hexs, e, text in ((BEACON.hex(), 9, "beacon: numIterationsExp must be between 10 and 63"),
                                  (BEACON.hex(), 64, "beacon: numIterationsExp must be between 10 and 63"),
                                  ("", EXP, "beacon: the beacon hash must be 1 to 255 bytes"),
                                  ("ab" * 256, EXP, "beacon: the beacon hash must be 1 to 255 bytes")):
                r = _run(*cmd, old, out, hexs, e, "--name=x")
                assert r.returncode == 1 and _error_line(r) == "[ERROR] snarkJS: " + text, r.stderr
            r = _run(*cmd, tmp_path / "missing", out, BEACON.hex(), EXP)
            assert r.returncode == 1 and "cannot open" in _error_line(r), r.stderr
        assert not out.exists()


@needs_node
@pytest.mark.gpu
def test_node_beacon_equals_the_python_route(amd, addon, tmp_path):
    for group, alias, old, ext in _inputs(amd, tmp_path):
        call = amd.ptau_beacon if group == "powersoftau" else amd.zkey_beacon
        want, wh = call(old.read_bytes(), BEACON, EXP, "Final Beacon", device=0)
        new = tmp_path / ("beacon" + ext)
        r = _run(group, "beacon", old, new, BEACON.hex(), EXP, "--name=Final Beacon")
        assert r.returncode == 0, r.stderr
        assert new.read_bytes() == want
        assert r.stdout == "[INFO]  snarkJS: Contribution Hash: \n" + _format_hash(wh) + "\n"
        # the alias is the same command; "0x" and upper-case digits are the same bytes; -n= is --name=
        again = tmp_path / ("again" + ext)
        r = _run(alias, old, again, "0x" + BEACON.hex().upper(), EXP, "-n=Final Beacon")
        assert r.returncode == 0, r.stderr
        assert again.read_bytes() == want and _format_hash(wh) in r.stdout
        # without a name
        bare = tmp_path / ("bare" + ext)
        assert _run(alias, old, bare, BEACON.hex(), EXP).returncode == 0
        assert bare.read_bytes() == call(old.read_bytes(), BEACON, EXP, device=0)[0]
    r = _run("powersoftau", "verify", tmp_path / "beacon.ptau")
    assert r.returncode == 0 and r.stdout == "[INFO]  snarkJS: Powers of tau Ok!\n", r.stderr
