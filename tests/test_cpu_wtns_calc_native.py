"""Memory safety of the host side of g16_wtns_calc (csrc/witness_program.cpp: the recorder's file image, the loader's
validation, the host route) as a stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/native/witness_program_test.cpp records a program, evaluates it against values worked out by hand, and feeds the
loader every prefix of the image and the image with every word overwritten by hostile values, from heap buffers of
exactly that length; whatever the loader accepts is evaluated.  Nothing is loaded into Python."""
import os
import subprocess
import warnings

from conftest import ROOT

CSRC = os.path.join(ROOT, "nzcp-circom_amd", "csrc")


def test_loader_and_host_route_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # (host code only: the compiler the library's .cpp units use)
    srcs = [os.path.join(ROOT, "tests", "native", "witness_program_test.cpp"), os.path.join(CSRC, "witness_program.cpp")]
    cmd = [hipcc, "--cuda-host-only", "-O2", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([hipcc, "--cuda-host-only", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        warnings.warn("no sanitizer runtime for the host compiler here: witness_program_test runs without it")
        san = []
    exe = tmp_path / "witness_program_test"
    subprocess.check_call(cmd + san + srcs + ["-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
