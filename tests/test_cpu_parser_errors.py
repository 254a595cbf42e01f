"""Replays tests/golden/parser_errors.json: every recorded mutant of a zkey, r1cs or ptau file must give the recorded
return code and g16_last_error text, byte for byte, at every entry point that parses before it touches a device.  The
table was recorded before csrc/binfile.h replaced the five hand-written section-table walkers (generator, mutation
kinds and hand-written cases: tests/golden/make_parser_errors.py); an entry that differs means the code is wrong, not
the table.
Every recorded answer comes before the device check, so the replay is the same with or without a GPU."""
import importlib.util
import json

import pytest

from conftest import golden_path

_spec = importlib.util.spec_from_file_location("make_parser_errors", golden_path("make_parser_errors.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def table():
    return json.load(open(golden_path("parser_errors.json")))


@pytest.fixture(scope="module")
def files():
    return gen.bases()


# Hand-written cases every entry point holds, by whole label, `%d` being the section that stands for "a required
# section other than the first": 2, except on the Groth16 .ptau route, which reads no section 2 or 3.
COMMON = ("cut inside the file header", "cut inside the first section record", "first section size 2^64 - 1",
          "first section size one byte past the end", "duplicated id: section %d renamed to 1, the first copy must win",
          "section %d renamed to id %d", "section 1 renamed to id 17", "version max + 1")
# The .ptau routes' missing-section cases.  A .ptau without section 2 or 3 passes the Groth16 route's parser, so those
# two plain cases are NOT in its table (they stop at the device check); sections 4 (renamed out of reach, id 20) and 12
# stand in for them there, and sections 2 and 3 appear only next to a bad power, which is what answers.
PTAU_MISSING = {
    "plonk_setup_ptau": ("section 1 missing", "section 2 missing", "section 3 missing", "section 2 missing and power 29"),
    "ptau_prepare": ("section 1 missing", "section 2 missing", "section 3 missing", "section 2 missing and power 29"),
    "groth16_setup_ptau": ("section 1 missing", "section 4 renamed to id 20", "section 12 missing",
                           "section 2 missing and power 29", "section 3 missing and power 29"),
}


def test_table_is_complete(table):
    assert set(table["entries"]) == set(gen.ENTRIES)
    for name, e in table["entries"].items():
        assert len(e["fuzz"]) == gen.FUZZ_CASES and e["seed"] == gen.ENTRIES[name][3]
        labels = {c[0] for c in e["hand"]}
        sid = 4 if name == "groth16_setup_ptau" else 2
        want = {w % ((sid, sid + 16) if w.count("%d") == 2 else sid) if "%d" in w else w for w in COMMON}
        want |= set(PTAU_MISSING.get(name, ()))
        assert want <= labels, (name, sorted(want - labels))
        assert all(c[2] in (gen.E_ARG, gen.E_FORMAT) for c in e["fuzz"] + e["hand"])
    for want in gen.MUST_APPEAR:
        assert any(t == want or (want.endswith("Missing section") and t.startswith(want + " ")) for t in table["texts"]), want


@pytest.mark.parametrize("name", list(gen.ENTRIES))
def test_recorded_code_and_text(amd, table, files, name):
    buf = files[gen.ENTRIES[name][0]]
    e = table["entries"][name]
    wrong = []
    for what, mut, rc, ti in e["fuzz"] + e["hand"]:
        got = gen.run(amd, name, files, gen.apply(buf, mut))
        if got != (rc, table["texts"][ti]):
            wrong.append((what, mut, (rc, table["texts"][ti]), got))
    assert not wrong, "%d of %d differ; first: %r" % (len(wrong), len(e["fuzz"]) + len(e["hand"]), wrong[:3])
