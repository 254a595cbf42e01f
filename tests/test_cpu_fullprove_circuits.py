"""The crafted circuits of the batched fullprove tests (fullprove_circuits.py), before any device test relies on them:
the program's witness (wtns_prog_ref.evaluate) satisfies the twin .r1cs under the host-route checker, a violating pass
fails the check row and raises check 0, and the host-route calculator computes the same words from the program image."""
import pytest

import formats as f
import fullprove_circuits as fc
import wtns_prog_ref as ref


@pytest.fixture(scope="module", params=[1, 2, fc.LADDER_K], ids=["tiny", "ladder2", "ladder300"])
def circuit(request):
    return fc.ladder(request.param)


def test_program_witness_satisfies_the_r1cs(amd, circuit):
    c = circuit
    k = c["n_public"]
    assert c["n_wires"] == k + 3 and len(f.read_r1cs(c["r1cs"])["rows"]) == k + 1
    for i in (0, 1, 6):
        w, status = fc.witness(c, i)
        assert status == ref.NO_CHECK and None not in w
        x, y = fc.inputs(i)
        assert (w[0], w[1], w[k + 1], w[k + 2]) == (1, x * y, x, y)
        if k > 1:
            assert w[k] == (w[k - 1] * x + y) % ref.R
        v = amd.wtns_check(c["r1cs"], f.write_wtns(w), device=-1)
        assert v.ok, v.reason
    # a violating pass: check 0, and exactly the check row fails
    w, status = fc.witness(c, 3, violate=True)
    assert status == 0
    v = amd.wtns_check(c["r1cs"], f.write_wtns(w), device=-1)
    assert not v.ok and v.constraint == k and v.n_failed == 1


def test_host_calculator_reads_the_program(amd, circuit):
    c = circuit
    calc = amd.WitnessCalculator(c["prog"], device=-1)
    assert (calc.n_wires, calc.n_public, calc.n_inputs, calc.n_levels) == (c["n_wires"], c["n_public"], 2, c["n_public"] + 1)
    assert calc.outputs == list(range(1, c["n_public"] + 1)) and calc.inputs == {"x": (0, 1), "y": (1, 1)}
    for i in (0, 5):
        words, status = calc.calculate(fc.inputs(i))
        assert status == amd.NO_CHECK and words == ref.words(fc.witness(c, i)[0])
        assert words[32:32 * (1 + c["n_public"])] == fc.public_bytes(c, i)
    _, status = calc.calculate({"x": 9, "y": 9}, want_words=False)
    assert status == 0 and calc.check_text(status) == fc.TEXT
    calc.close()
