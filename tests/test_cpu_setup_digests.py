"""Replays the "cpu" table of tests/golden/setup_digests.json: SHA-256 and length of every output buffer of the setup-side
entry points on the host path (setup_device(-1)) -- the synthetic circuit and witness, the SHA-256 and NZCP circuit
builders' .r1cs and .wtns images (otherwise only checked for satisfiability: these pin the bytes and the row order),
every NZCP gadget's outputs and constraint count, the .r1cs trapdoor setups and the test ceremony writer.  The table was
recorded before the host setup code was split into circuit, setup and ptau units (cases and recorder:
tests/golden/make_setup_digests.py); an entry that differs means the code is wrong, not the table."""
import importlib.util
import json

import pytest

from conftest import golden_path

_spec = importlib.util.spec_from_file_location("make_setup_digests", golden_path("make_setup_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def table():
    return json.load(open(golden_path("setup_digests.json")))


@pytest.fixture(scope="module")
def inp():
    return gen.inputs()


def test_table_is_complete(table, inp):
    assert list(table["cpu"]) == list(gen.CPU_CASES) and list(table["gpu"]) == list(gen.GPU_CASES)
    assert set(gen.GPU_SAME_AS_CPU) <= set(gen.CPU_CASES)
    assert {v[0] for v in gen.GPU_FILES.values()} <= set(gen.GPU_CASES)
    for part in ("cpu", "gpu"):
        for name, outs in table[part].items():
            assert outs and ("error" in outs) == (name == "plonk_setup_ptau_too_big"), name
    assert table["cpu"]["sha256_chain_1"].keys() == {"zkey", "wtns", "vkey", "r1cs"}
    assert len(table["cpu"]["nzcp_gadgets"]) == len(gen.gadget_vectors(inp)) == 18


@pytest.mark.parametrize("name", list(gen.CPU_CASES))
def test_recorded_digests(amd, table, inp, name):
    assert gen.run(amd, gen.CPU_CASES, name, inp, -1) == table["cpu"][name]
