"""The owners of csrc/device_job.h -- DeviceBuf, PinnedBuf, PhaseEvents, DeviceStream, StreamDrain, upload -- as a
stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer: tests/native/device_owners_test.cpp
defines the HIP entry points the header uses as recording fakes over malloc / free (the HIP runtime is not linked) and
reads the release order, the once-only release after every failing acquisition, growth and the drain guard from their
log.  Nothing is loaded into Python.  The handles built on these owners run in the GPU tests of their routes."""
import os
import subprocess
import warnings

import pytest

from conftest import ROOT

HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_owners_release_order_failures_growth_and_drain(tmp_path):
    if not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime.h")):
        pytest.fail("no HIP headers under " + HIP_INCLUDE + ": device_job.h cannot be compiled")
    src = os.path.join(ROOT, "tests", "native", "device_owners_test.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", HIP_INCLUDE,
           "-I", os.path.join(ROOT, "nzcp-circom_amd", "csrc")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        warnings.warn("no sanitizer runtime for g++ here: device_owners_test runs without it")
        san = []
    exe = tmp_path / "device_owners_test"
    subprocess.check_call(cmd + san + [src, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
