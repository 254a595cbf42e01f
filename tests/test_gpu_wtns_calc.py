"""wtns calculate on the device (csrc/wtns_calc.hip): every result is compared word for word with the host route
(device = -1) and, for crafted programs, with the big-integer evaluator of wtns_prog_ref.py.

T = 256 is the workgroup size of the kernel (kWcalcThreads): one workgroup computes one witness, its threads stride over
the ops of a level and meet at a barrier per level.  The shapes below are the smallest at which that can go wrong: a
level of 1, 63, 64, 65 ops (a wavefront's edge), 255, 256, 257 (the workgroup's edge, a second trip of the stride loop)
and 1 025 (a fifth trip, one op); a chain of 2 000 levels of one op each (every barrier, every hand-over through
memory); a BITS op whose 35 targets are scattered."""
import pytest

import formats as f
import wtns_prog_ref as ref
from test_cpu_wtns_calc import CASES, TEMPLATES, check_template

pytestmark = pytest.mark.gpu

T = 256


def both(amd, img):
    return amd.WitnessCalculator(img, device=0), amd.WitnessCalculator(img, device=-1)


def agree(dev, host, n_wires, ops, inputs_list):
    """Device == host route == the Python evaluator, words and status, for every input vector."""
    want = []
    for inp in inputs_list:
        w, status = ref.evaluate(n_wires, ops, inp)
        want.append((ref.words(w), status))
    assert host.calculate_batch(inputs_list) == want
    assert dev.calculate_batch(inputs_list) == want
    for inp, one in zip(inputs_list, want):
        assert dev.calculate(inp) == one


# ------------------------------------------------------------------ crafted programs
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_program(amd, case):
    dev, host = both(amd, ref.write(case["n_wires"], case["ops"], case["checks"]))
    agree(dev, host, case["n_wires"], case["ops"], case["inputs"])
    dev.close(), host.close()


@pytest.mark.parametrize("width", [1, 63, 64, 65, T - 1, T, T + 1, 4 * T + 1])
def test_level_width(amd, width):
    n, ops = ref.width_program(width)
    dev, host = both(amd, ref.write(n, ops))
    assert dev.n_levels == 2
    agree(dev, host, n, ops, [[3, 5], [ref.R - 1, 2 ** 200 + width]])
    dev.close(), host.close()


def test_chain_of_2000_levels(amd):
    """A pure dependency chain: the barrier count (2 000 levels, one op each: thread 0 works, 255 only wait) and
    visibility (op i + 1 runs on the same thread or, in the second program, on another wavefront than op i)."""
    n, ops = ref.chain_program(2000)
    dev, host = both(amd, ref.write(n, ops))
    dev.close(), host.close()   # handles that never ran a batch
    dev, host = both(amd, ref.write(n, ops))
    assert dev.n_levels == 2000
    agree(dev, host, n, ops, [[2], [ref.R - 1]])
    dev.close(), host.close()
    # the same chain with 1 + (i * 67) % 200 idle ops ahead of the chain's op in level i: the chain's op moves from lane to
    # lane and wavefront to wavefront, so every level's value crosses wavefronts through memory
    depth, wire, chain = 300, 1, [("input", 1, 0)]
    ops2, n2 = list(chain), 2
    for i in range(depth):
        pad = 1 + (i * 67) % 200
        for _ in range(pad):   # idle ops of this level: they read the chain's current wire too
            ops2.append(("quad", n2, [], [], [(wire, 1), (0, n2)]))
            n2 += 1
        ops2.append(("quad", n2, [(wire, 1)], [(wire, 1)], [(wire, 3), (0, 1)]))
        wire, n2 = n2, n2 + 1
    dev, host = both(amd, ref.write(n2, ops2))
    assert dev.n_levels == depth + 1
    agree(dev, host, n2, ops2, [[7]])
    dev.close(), host.close()


def test_bits_with_35_scattered_targets(amd):
    n, ops = ref.scattered_bits_program()
    dev, host = both(amd, ref.write(n, ops))
    agree(dev, host, n, ops, [[2 ** 32 - 1, 2 ** 32 - 1], [0x12345678, 0x9ABCDEF0], [2 ** 35, 0], [0, 0]])
    dev.close(), host.close()


# ------------------------------------------------------------------ templates
@pytest.mark.parametrize("name,params,vectors", TEMPLATES, ids=[f"{t[0]}{i}" for i, t in enumerate(TEMPLATES)])
def test_template_program(amd, name, params, vectors):
    """The template vectors on the device: the builder's outputs and texts (check_template), and the WHOLE wire vector
    equal to the host route's."""
    dev, host = both(amd, amd.nzcp_gadget_program(name, params))
    got = check_template(amd, dev, name, params, vectors)
    assert got == host.calculate_batch([prog_in for _, prog_in in vectors])
    dev.close(), host.close()


# ------------------------------------------------------------------ batches and chunks
def _batch_inputs(count):
    # quinSelector(5): [1..5, index]; witness i selects index i % 5; the one in the middle violates (index 100)
    inputs = [[10 + i, 20 + i, 30 + i, 40 + i, 50 + i, i % 5] for i in range(count)]
    if count > 2:
        inputs[count // 2][5] = 100          # (100 + 8 - 5 does not fit LessThan(3)'s four bits)
    return inputs


@pytest.mark.parametrize("chunk", [None, 1, 2])
@pytest.mark.parametrize("count", [1, 2, 65])
def test_batches_and_forced_chunks(amd, monkeypatch, count, chunk):
    if chunk:
        monkeypatch.setenv("G16_WTNS_CALC_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("G16_WTNS_CALC_CHUNK", raising=False)
    dev, host = both(amd, amd.nzcp_gadget_program("quinSelector", [5]))
    inputs = _batch_inputs(count)
    got = dev.calculate_batch(inputs)
    assert got == host.calculate_batch(inputs)
    for i, (words, status) in enumerate(got):
        if count > 2 and i == count // 2:
            assert dev.check_text(status) == "QuinSelector: index out of range"
        else:   # the neighbours of the violating witness are untouched
            assert status == amd.NO_CHECK
            assert int.from_bytes(words[32 * dev.outputs[0]:32 * dev.outputs[0] + 32], "little") == 10 * (1 + i % 5) + i
    # the same calculator, another batch (shorter, other values; the status words of the last call are gone)
    again = [[7, 8, 9, 10, 11, 4 - i % 5] for i in range(max(1, count - 1))]
    assert dev.calculate_batch(again) == host.calculate_batch(again)
    assert all(status == amd.NO_CHECK for _, status in dev.calculate_batch(again, want_words=False))
    dev.close(), host.close()


# ------------------------------------------------------------------ the full size
@pytest.fixture(scope="module")
def example(amd):
    """The example-parameter circuit once: its program, and the builder's key, witness and .r1cs for the MoH pass."""
    from test_cpu_sha256_circuit import example_to_be_signed
    tbs = example_to_be_signed()
    out = amd.nzcp_circuit_setup(amd.NZCP_EXAMPLE_PARAMS, tbs, 77, want_zkey=True, want_r1cs=True)
    out["tbs"] = tbs
    out["prog"] = amd.nzcp_witness_program(amd.NZCP_EXAMPLE_PARAMS)
    return out


def test_full_size_example_pass(amd, example):
    tbs, max_bytes = example["tbs"], amd.NZCP_EXAMPLE_PARAMS[1]
    calc = amd.WitnessCalculator(example["prog"], device=0)
    inputs = amd.nzcp_inputs(tbs, max_bytes)
    body = example["wtns"][-calc.n_wires * 32:]
    # the device witness is the builder's, word for word, and its .wtns image the builder's file
    words, status = calc.calculate(inputs)
    assert status == amd.NO_CHECK and words == body
    assert calc.wtns(inputs) == example["wtns"]
    checker = amd.R1csChecker(example["r1cs"], device=0)
    assert checker.check(calc.wtns(inputs)).ok
    checker.close()
    # stage_inputs + prove_staged == stage_witness + prove_staged, with fixed r and s
    r, s = f.le(0x1234567890ABCDEF ** 3 % ref.R), f.le(0xFEDCBA0987654321 ** 3 % ref.R)
    prover = amd.Prover(example["zkey"])
    prover.stage(0, example["wtns"])
    want = prover.prove_staged(0, r, s)
    assert prover.stage_inputs(1, calc, inputs) == amd.NO_CHECK
    assert prover.prove_staged(1, r, s) == want
    # the refusals: counts that differ from the key's, a host-route calculator, a violating pass
    gadget = amd.WitnessCalculator(amd.nzcp_gadget_program("quinSelector", [3]), device=0)
    with pytest.raises(amd.G16Error, match=r"stage inputs: the program has 18 wires and 0 public signals, the key \d+ and 513"):
        prover.stage_inputs(2, gadget, [1, 2, 3, 0])
    gadget.close()
    host = amd.WitnessCalculator(example["prog"], device=-1)
    with pytest.raises(amd.G16Error, match="stage inputs: the calculator runs on the host route"):
        prover.stage_inputs(2, host, inputs)
    host.close()
    broken = bytearray(tbs)
    broken[27] = 0x80                                   # not a claims map at the expected offset
    status = prover.stage_inputs(1, calc, amd.nzcp_inputs(bytes(broken), max_bytes))
    assert calc.check_text(status) == "ReadMapLength: not a map"
    with pytest.raises(amd.G16Error, match="witness slot not staged"):
        prover.prove_staged(1, r, s)
    assert prover.prove_staged(0, r, s) == want           # the other slot is untouched
    prover.close()
    calc.close()
