"""Replays the "gpu" table of tests/golden/setup_digests.json on the device: PLONK setup with and without the Lagrange
section, PLONK and Groth16 setup from a ceremony file, prepare phase2 at powers 0, 1 (where the block layout
degenerates) and 3, recorded in one run on an MI355X before the host setup code was split (cases and recorder:
tests/golden/make_setup_digests.py).  The cases of GPU_SAME_AS_CPU, run with the fixed-base multiplications on the
device, must reproduce the CPU table; the three file-path forms must write files with the digests of their buffer
forms."""
import importlib.util
import json

import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_setup_digests", golden_path("make_setup_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def table():
    return json.load(open(golden_path("setup_digests.json")))


@pytest.fixture(scope="module")
def inp():
    return gen.inputs()


@pytest.mark.parametrize("name", list(gen.GPU_CASES))
def test_recorded_digests(amd, table, inp, name):
    assert gen.run(amd, gen.GPU_CASES, name, inp, 0) == table["gpu"][name]


@pytest.mark.parametrize("name", gen.GPU_SAME_AS_CPU)
def test_device_reproduces_the_cpu_digests(amd, table, inp, name):
    assert gen.run(amd, gen.CPU_CASES, name, inp, 0) == table["cpu"][name]


@pytest.mark.parametrize("name", list(gen.GPU_FILES))
def test_file_forms_write_the_buffer_forms_bytes(amd, table, inp, name):
    same_as, got = gen.run_files(amd, inp, name, 0)
    assert got == table["gpu"][same_as]
