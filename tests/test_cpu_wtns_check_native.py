"""Memory safety of the host side of g16_wtns_check (csrc/wtns_check_host.cpp: the host route, the r1cs -> CSR builder of
the device route, the verdict plumbing) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/native/wtns_check_test.cpp drives it with device = -1, evaluates the builder's CSR
with the host forms of the kernel's arithmetic against the host route, and feeds the checker every prefix of a witness
and of an .r1cs from heap buffers of exactly that length.  Nothing is loaded into Python."""
import os
import subprocess
import warnings

from conftest import ROOT

CSRC = os.path.join(ROOT, "nzcp-circom_amd", "csrc")


def test_host_route_and_csr_builder_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # (host code only: the compiler the library's .cpp units use)
    srcs = [os.path.join(ROOT, "tests", "native", "wtns_check_test.cpp"), os.path.join(CSRC, "wtns_check_host.cpp"),
            os.path.join(CSRC, "circuit.cpp")]
    cmd = [hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([hipcc, "--cuda-host-only", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        warnings.warn("no sanitizer runtime for the host compiler here: wtns_check_test runs without it")
        san = []
    exe = tmp_path / "wtns_check_test"
    subprocess.check_call(cmd + san + srcs + ["-o", str(exe), "-lpthread"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
