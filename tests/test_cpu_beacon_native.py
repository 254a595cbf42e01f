"""Memory safety of the beacon params walker and the delay function (csrc/beacon.h), as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/native/beacon_test.cpp runs beacon_params_walk on every prefix of
valid params blocks held in heap buffers of exactly that length, with hostile id and length bytes, and the SHA-256 chain
at e = 10 against constants of the Python twin.  Nothing is loaded into Python."""
import os
import subprocess
import warnings

from beacon_ref import chain
from conftest import ROOT


def test_params_walker_prefixes_and_the_chain(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "beacon_test.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "nzcp-circom_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        warnings.warn("no sanitizer runtime for g++ here: beacon_test runs without it")
        san = []
    exe = tmp_path / "beacon_test"
    subprocess.check_call(cmd + san + [src, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
    # the constants in the program are the twin's
    text = open(src).read()
    beacon = bytes((37 * i + 11) & 0xff for i in range(255))
    for b in (beacon[:32], b"\x01", beacon):
        assert chain(b, 10).hex() in text
