"""Memory safety of the one container reader and layout helper (csrc/binfile.h), as a stand-alone host program under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/native/binfile_test.cpp runs bin_open on every prefix of a
three-section file held in a heap buffer of exactly that length, with every size field overwritten by hostile values,
reads bin_layout's image back, and drops, moves and hands out the owning Buf (the leak checker and the double-free check
are the asserts there).  Nothing is loaded into Python.  What the parsers built on it ANSWER is pinned by
tests/test_cpu_parser_errors.py."""
import os
import subprocess
import warnings

from conftest import ROOT


def test_bin_open_prefixes_and_hostile_sizes(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "binfile_test.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "nzcp-circom_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        warnings.warn("no sanitizer runtime for g++ here: binfile_test runs without it")
        san = []
    exe = tmp_path / "binfile_test"
    subprocess.check_call(cmd + san + [src, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
