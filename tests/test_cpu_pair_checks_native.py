"""The batch of pairing checks the ceremony verifiers share (csrc/pair_checks.h) and the Blake2b unit (csrc/blake2b.cpp),
as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/native/pair_checks_test.cpp
stands in for g16_pairing_op with the host build of csrc/pairing.cuh and pins that all checks holding gives no verdict,
that the verdict is the FIRST failing check's, that an empty batch makes no device call, that images and standard-form
words lay out the same pairs, and that an error of the call comes back unchanged; then RFC 7693's "abc" vector and the
streaming hash over every split.  The program links blake2b.cpp with a plain g++: the unit needs no HIP header.  Nothing
is loaded into Python."""
import os
import subprocess
import warnings

from conftest import ROOT


def test_pair_checks_and_blake2b(tmp_path):
    csrc = os.path.join(ROOT, "nzcp-circom_amd", "csrc")
    src = [os.path.join(ROOT, "tests", "native", "pair_checks_test.cpp"), os.path.join(csrc, "blake2b.cpp")]
    # (-Wno-unknown-pragmas: the field headers carry `#pragma unroll` for the device compiler)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", csrc]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        warnings.warn("no sanitizer runtime for g++ here: pair_checks_test runs without it")
        san = []
    exe = tmp_path / "pair_checks_test"
    subprocess.check_call(cmd + san + src + ["-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
