"""wtns calculate on the host route (device = -1): witness programs (csrc/witness_program.h) loaded, validated and
evaluated without a GPU.  Crafted programs are compared word for word with the big-integer evaluator of
wtns_prog_ref.py; the programs the native builders record are compared with the builders themselves (nzcp_gadget over
the vectors test_cpu_nzcp_circuit.py takes from the reference's test/cbor.js, quinSelector.js and nzcp.js).  Every
comparison is exact."""
import hashlib

import pytest

import formats as f
import wtns_prog_ref as ref
from test_cpu_nzcp_circuit import enc_arr, enc_int, enc_str, pad
from test_cpu_sha256_circuit import _bits_msb_first, example_to_be_signed

CASES = ref.crafted_cases()


# ------------------------------------------------------------------ crafted programs against the Python evaluator
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_crafted_program_matches_reference(amd, case):
    img = ref.write(case["n_wires"], case["ops"], case["checks"])
    calc = amd.WitnessCalculator(img, device=-1)
    assert (calc.n_wires, calc.n_inputs) == (case["n_wires"], len(case["inputs"][0]))
    for inp in case["inputs"]:
        w, status = ref.evaluate(case["n_wires"], case["ops"], inp)
        assert calc.calculate(inp) == (ref.words(w), status), inp
    # ... and as one batch, with the words left out
    got = calc.calculate_batch(case["inputs"], want_words=False)
    assert got == [(None, ref.evaluate(case["n_wires"], case["ops"], inp)[1]) for inp in case["inputs"]]
    calc.close()


def test_bits_edges_and_check_texts(amd):
    """What the crafted cases must show, spelled out: 2^n - 1 fits, 2^n raises the check and leaves zero bits; of two
    violated checks the lower index is reported."""
    for n in (1, 32, 64, 253):
        case = next(c for c in CASES if c["name"] == f"bits_{n}")
        calc = amd.WitnessCalculator(ref.write(case["n_wires"], case["ops"], case["checks"]), device=-1)
        w, st = calc.calculate([2 ** n - 1])
        assert st == amd.NO_CHECK and w[64:] == ref.words([1] * n)
        w, st = calc.calculate([2 ** n])
        assert st == 0 and w[64:] == bytes(32 * n) and calc.check_text(0) == "does not fit"
    case = next(c for c in CASES if c["name"] == "two_checks")
    calc = amd.WitnessCalculator(ref.write(case["n_wires"], case["ops"], case["checks"]), device=-1)
    assert [calc.calculate([v])[1] for v in (0, 1, 2, 3)] == [1, 0, 0, 0]      # v = 3 violates all three
    assert calc.check_text(2) == "w1 is 2" and calc.check_text(3) is None
    assert calc.calculate([2])[1] == 0 and calc.calculate([0])[1] == 1             # v = 0: checks 1 and 2, lower wins


def test_inputs_must_be_canonical_and_counted(amd):
    case = next(c for c in CASES if c["name"] == "quad")
    img = ref.write(case["n_wires"], case["ops"], inputs=[("x", 0, 1), ("y", 1, 1)])
    calc = amd.WitnessCalculator(img, device=-1)
    assert calc.inputs == {"x": (0, 1), "y": (1, 1)}
    with pytest.raises(amd.G16Error, match=r"witness 1: input y\[0\] is not reduced modulo the scalar field"):
        calc.calculate_batch([[1, 2], (3).to_bytes(32, "little") + ref.R.to_bytes(32, "little")])
    with pytest.raises(amd.G16Error, match="takes 2 input words, 3 given"):
        calc.calculate([1, 2, 3])
    assert calc.calculate({"y": 4, "x": 9}) == calc.calculate([9, 4])
    with pytest.raises(amd.G16Error, match="no input z"):
        calc.calculate({"z": 1})


def test_wtns_image(amd):
    case = next(c for c in CASES if c["name"] == "check")
    calc = amd.WitnessCalculator(ref.write(case["n_wires"], case["ops"], case["checks"]), device=-1)
    assert f.read_wtns(calc.wtns([5, 5]))["w"] == [1, 5, 5]
    with pytest.raises(amd.G16Error, match="constraint not satisfied: a === b"):
        calc.wtns([5, 6])


# ------------------------------------------------------------------ loader rejects (each before any evaluation)
def _reject(amd, img, text):
    with pytest.raises(amd.G16Error, match=text) as e:
        amd.WitnessCalculator(img, device=-1)
    assert e.value.code == -2                                           # G16_E_FORMAT


def test_loader_rejects_malformed_programs(amd):
    ok = [("input", 1, 0), ("quad", 2, [(1, 1)], [(1, 1)], []), ("quad", 3, [], [], [(2, 1)])]
    amd.WitnessCalculator(ref.write(4, ok), device=-1).close()
    # a wire defined twice; a wire never defined
    _reject(amd, ref.write(4, ok + [("isz", 2, [(1, 1)])]), "wire 2 is defined twice")
    _reject(amd, ref.write(5, ok), "wire 4 is never defined")
    # a term reading a wire of the same, or of a higher, level
    _reject(amd, ref.write(4, ok, levels=[1, 2, 2]), "op 2 at level 2 reads wire 2 of level 2")
    _reject(amd, ref.write(4, ok, levels=[1, 3, 2]), "op 1 at level 2 reads wire 2 of level 3")
    # indices out of range: a wire, a term's wire, an input word, a check, the terms of an op, BITS beyond 253
    _reject(amd, ref.write(3, ok), "defines wire 3, which is out of range")
    _reject(amd, ref.write(4, ok[:2] + [("quad", 3, [], [], [(9, 1)])], levels=[1, 2, 3]), "reads wire 9, which is out of range")
    _reject(amd, ref.write(4, ok, n_inputs=0), "reads input word 0, which is out of range")
    _reject(amd, ref.write(4, ok + [("check", [(3, 1)], 1)], checks=["only one"]), "names check 1, which is out of range")

    def far_terms(secs):
        secs[2] = secs[2][:16] + (1000).to_bytes(4, "little") + secs[2][20:]   # op 0: t_off
    _reject(amd, ref.write(4, ok, raw=far_terms), "has terms out of range")
    _reject(amd, ref.write(256, [("input", 1, 0), ("bits", list(range(2, 256)), [(1, 1)], None)]), "takes 254 bits")
    # a level index that does not cover the ops

    def short_index(secs):
        secs[4] = secs[4][:-4] + (2).to_bytes(4, "little")
    _reject(amd, ref.write(4, ok, raw=short_index), "the level index does not cover the ops")

    def unsorted_index(secs):
        secs[4] = secs[4][:4] + (3).to_bytes(4, "little") + secs[4][8:]
    _reject(amd, ref.write(4, ok, raw=unsorted_index), "the level index does not cover the ops")
    # a truncated file, at every section boundary and inside the sections
    img = ref.write(4, ok)
    for cut in (0, 3, 11, 20, len(img) // 2, len(img) - 1):
        _reject(amd, img[:cut], "Invalid File format")
    _reject(amd, b"wtns" + img[4:], "Invalid File format")


# ------------------------------------------------------------------ templates through nzcp_gadget_program
def _sha_inputs(msg, bs):
    bits = _bits_msb_first(bytes(msg) + bytes((64 << bs) - len(msg)))
    return [8 * len(msg)] + bits


def _jack():
    inp = []
    for s in ("Jack", "Sparrow", "1960-04-16"):
        inp += pad([ord(c) for c in s], 64) + [len(s)]
    return inp


def _short_given():   # given name of one letter: k - givenNameLen - 1 goes "negative" from k = 0 on
    inp = []
    for s in ("A", "B", "2000-01-01"):
        inp += pad([ord(c) for c in s], 64) + [len(s)]
    return inp


def template_vectors():
    """(name, params, [(gadget inputs, program inputs)]): the vectors of test_cpu_nzcp_circuit.py, violating ones included."""
    tbs = list(example_to_be_signed())
    same = lambda xs: [(x, x) for x in xs]                                   # noqa: E731
    v = [
        ("quinSelector", [5], same([[1, 2, 3, 4, 5, i] for i in range(5)] + [[1, 2, 3, 4, 5, 8]])),   # 8: out of range
        ("getType", [], same([[0], [167], [255], [256]])),                    # 256: not a byte
        ("decodeUint", [4], same([[0, 0, 0, 0, 0, 167], [31, 0, 0, 0, 0, 120], [42, 69, 0, 0, 0, 25],
                                  [97, 218, 192, 48, 0, 26]])),               # all four branches
        ("skipValue", [5, 4], same([pad(enc_str("abc"), 5) + [0], pad(enc_int(0xFFFF), 5) + [0],
                                    pad(enc_arr([enc_int(23)] * 3), 5) + [0], pad(enc_arr([enc_str("q")] * 2), 5) + [0]])),
        ("stringEquals", [5, 5] + [ord(c) for c in "abcde"], same([[ord(c) for c in "abcde"] + [0, 5],
                                                                    [ord("b")] * 5 + [0, 5], pad([ord("b")] * 2, 5) + [0, 2]])),
        ("copyString", [5, 4], same([pad(enc_str(s), 5) + [0] for s in ("", "ab", "abcd")] + [pad(enc_int(3), 5) + [0]])),
        ("readCredSubj", [314, 32], same([tbs + [247, 3], tbs + [247, 4]])),   # map length 4: refused
        ("concatCredSubj", [64], same([_jack(), _short_given()])),
    ]
    for bs, lens in ((0, (0, 55)), (1, (0, 55, 56, 64, 119))):
        msgs = [bytes((11 * i + n) & 0xFF for i in range(n)) for n in lens]
        v.append(("sha256Var", [bs], [([8 * len(m)] + list(m), _sha_inputs(m, bs)) for m in msgs]))
    return v


TEMPLATES = template_vectors()


def gadget_result(amd, name, params, inputs):
    """nzcp_gadget -> (outputs, None) or (None, the text of the violated constraint)."""
    try:
        return amd.nzcp_gadget(name, params, inputs)[0], None
    except amd.G16Error as e:
        assert str(e).startswith("constraint not satisfied: ")
        return None, str(e)[len("constraint not satisfied: "):]


def check_template(amd, calc, name, params, vectors):
    """Every vector through `calc` against nzcp_gadget; -> the words of every vector (for a second route to compare)."""
    got = calc.calculate_batch([prog_in for _, prog_in in vectors])
    for (gad_in, _), (words, status) in zip(vectors, got):
        outs, text = gadget_result(amd, name, params, gad_in)
        if text is None:
            assert status == amd.NO_CHECK
            assert [int.from_bytes(words[32 * k:32 * k + 32], "little") for k in calc.outputs] == outs
        else:
            assert calc.check_text(status) == text
    return got


@pytest.mark.parametrize("name,params,vectors", TEMPLATES, ids=[f"{t[0]}{i}" for i, t in enumerate(TEMPLATES)])
def test_template_program_matches_builder(amd, name, params, vectors):
    calc = amd.WitnessCalculator(amd.nzcp_gadget_program(name, params), device=-1)
    check_template(amd, calc, name, params, vectors)
    calc.close()


def test_sha256_var_program_matches_hashlib_and_negative_index_uses_field_inverses(amd):
    calc = amd.WitnessCalculator(amd.nzcp_gadget_program("sha256Var", [1]), device=-1)
    msg = bytes(range(119))
    words, st = calc.calculate(_sha_inputs(msg, 1))
    assert st == amd.NO_CHECK
    assert [words[32 * k] for k in calc.outputs] == _bits_msb_first(hashlib.sha256(msg).digest())
    # concatCredSubj with a one-letter given name: the selector of the family name sees k - 2 for k = 0, 1, a field
    # element near r, whose inverse INV0 must produce
    calc = amd.WitnessCalculator(amd.nzcp_gadget_program("concatCredSubj", [64]), device=-1)
    words, st = calc.calculate(_short_given())
    vals = [int.from_bytes(words[32 * k:32 * k + 32], "little") for k in range(calc.n_wires)]
    assert st == amd.NO_CHECK and pow(ref.R - 2, ref.R - 2, ref.R) in vals
    res = "A,B,2000-01-01"
    assert [vals[k] for k in calc.outputs] == pad([ord(c) for c in res], 64) + [len(res)]


def test_program_parameter_checks(amd):
    for bad in ((0, 0, 0, 4, 2, 4, 5), (0, 504, 0, 4, 2, 4, 5), (0, 314, 0, 4, 2, 4, 1), (0, 314, 0, 4, 2, 4, 7)):
        with pytest.raises(amd.G16Error, match="nzcp circuit: bad arguments"):
            amd.nzcp_witness_program(bad)
    with pytest.raises(amd.G16Error, match="unknown gadget"):
        amd.nzcp_gadget_program("noSuchTemplate", [])
    words = amd.nzcp_inputs(b"\x80\x01", 3)
    assert [int.from_bytes(words[32 * i:32 * i + 32], "little") for i in range(25)] == [1] + [0] * 14 + [1] + [0] * 8 + [2]


# ------------------------------------------------------------------ the recorder is inert
def test_recorder_is_inert(amd):
    """Recording a program changes nothing the builders emit: nzcp_gadget's outputs and row counts, and the .r1cs and
    .wtns of nzcp_fixed_layout_setup, are the same before and after programs were recorded in this process."""
    tbs = example_to_be_signed()
    jack = bytes(tbs).index(b"Jack")

    def snapshot():
        g1 = amd.nzcp_gadget("concatCredSubj", [64], _jack())
        g2 = amd.nzcp_gadget("sha256Var", [1], [8 * 55] + list(range(55)))
        fl = amd.nzcp_fixed_layout_setup(tbs, [(jack, 4), (jack + 4, 1), (jack + 5, 2)], 69, 1, want_zkey=False, want_r1cs=True)
        return g1, g2, fl["r1cs"], fl["wtns"]
    before = snapshot()
    amd.nzcp_gadget_program("concatCredSubj", [64])
    amd.nzcp_gadget_program("sha256Var", [1])
    assert snapshot() == before
    # and the recorded program numbers its wires as the builder does: same count of wires as the builder's rows imply
    d = ref.read(amd.nzcp_gadget_program("quinSelector", [3]))
    assert d["n_inputs"] == 4 and [op[0] for op in d["ops"][:4]] == ["input"] * 4 and d["levels"][:4] == [1] * 4
