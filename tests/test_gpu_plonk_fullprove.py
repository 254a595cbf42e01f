"""g16_plonk_fullprove_batch and PlonkProver.fullprove: inputs in, PLONK proofs and public signals out, the raw witness
of each proof read from the calculator's chunk buffer (csrc/plonk.hip).  The reference route is
PlonkProver.prove(calc.wtns(inputs), blinding) with the same nine scalars, which the new call must equal byte for byte.
Circuits: fullprove_circuits.py."""
import pytest

import fullprove_circuits as fc
import plonk as pk
import wtns_prog_ref as ref

pytestmark = pytest.mark.gpu

NMAX = 5


def blinding_of(i):
    """Nine fixed scalars b1..b9 of pass i, distinct across passes."""
    return [pow(3, 100 * i + k + 11, ref.R) for k in range(9)]


@pytest.fixture(scope="module", params=["tiny", "ladder"])
def world(request, amd):
    c = fc.tiny() if request.param == "tiny" else fc.ladder(fc.LADDER_K)
    zkey = amd.plonk_setup(c["r1cs"], 9, device=0)
    host = amd.WitnessCalculator(c["prog"], device=-1)
    prover = amd.PlonkProver(zkey, device=0)
    assert prover.n_vars - prover.n_additions == c["n_wires"]
    exp = []
    for i in range(NMAX):
        proof, pub = prover.prove(host.wtns(fc.inputs(i)), blinding_of(i))
        assert [int(x) for x in pub] == fc.witness(c, i)[0][1:1 + c["n_public"]]
        exp.append((proof, fc.public_bytes(c, i), amd.NO_CHECK))
    prover.close(), host.close()
    return {"c": c, "zkey": zkey, "exp": exp}


def handles(amd, monkeypatch, world, chunk=None):
    if chunk:
        monkeypatch.setenv("G16_WTNS_CALC_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("G16_WTNS_CALC_CHUNK", raising=False)
    return amd.PlonkProver(world["zkey"], device=0), amd.WitnessCalculator(world["c"]["prog"], device=0)


@pytest.mark.parametrize("chunk", [None, 2])
def test_bit_identity(amd, monkeypatch, world, chunk):
    prover, calc = handles(amd, monkeypatch, world, chunk)
    for count in (1, 3, 5):
        got = prover.fullprove_batch(calc, [fc.inputs(i) for i in range(count)], [blinding_of(i) for i in range(count)])
        assert got == world["exp"][:count], (count, chunk)
    prover.close(), calc.close()


@pytest.mark.parametrize("bad", [[0], [2], [4], [1, 2], [0, 1, 2, 3, 4]], ids=["first", "middle", "last", "straddle", "all"])
def test_verdicts(amd, monkeypatch, world, bad):
    prover, calc = handles(amd, monkeypatch, world, 2)
    n = 5
    inputs = [fc.inputs(i, violate=i in bad) for i in range(n)]
    got = prover.fullprove_batch(calc, inputs, [blinding_of(i) for i in range(n)])
    for i in range(n):
        if i in bad:
            assert got[i] == (None, None, 0) and calc.check_text(got[i][2]) == fc.TEXT
        else:
            assert got[i] == world["exp"][i], i
    # ... the bytes behind the binding's None: all zero
    import ctypes as C
    p = 32 * world["c"]["n_public"]
    prs, pub, st = (amd.PlonkProof * n)(), C.create_string_buffer(b"\xaa" * (n * p), n * p), (C.c_uint32 * n)()
    C.memset(prs, 0xaa, C.sizeof(prs))
    blind = b"".join(int(x).to_bytes(32, "little") for i in range(n) for x in blinding_of(i))
    words = b"".join(calc.words(x) for x in inputs)
    assert amd.load().g16_plonk_fullprove_batch(prover._h, calc._h, words, 2, n, blind, prs, pub, st) == 0
    for i in range(n):
        zero = i in bad
        assert (bytes(prs[i]) == bytes(C.sizeof(amd.PlonkProof))) == zero and (pub.raw[i * p:(i + 1) * p] == bytes(p)) == zero
        assert st[i] == (0 if zero else amd.NO_CHECK)
        if not zero:
            assert amd.plonk_proof_to_obj(prs[i]) == world["exp"][i][0] and pub.raw[i * p:(i + 1) * p] == world["exp"][i][1]
    prover.close(), calc.close()


def test_random_blinding_and_one_pass_form(amd, monkeypatch, world):
    from test_gpu_plonk import _vk_json
    prover, calc = handles(amd, monkeypatch, world, 2)
    k = world["c"]["n_public"]
    ver = amd.PlonkVerifier(_vk_json(pk.vkey_from_zkey(world["zkey"])))
    runs = [prover.fullprove_batch(calc, [fc.inputs(i) for i in range(3)]) for _ in range(2)]
    for got in runs:
        assert [(pub, st) for _, pub, st in got] == [(pub, st) for _, pub, st in world["exp"][:3]]
        pubs = [[str(int.from_bytes(pub[32 * j:32 * j + 32], "little")) for j in range(k)] for _, pub, _ in got]
        assert ver.verify_batch([(pubs[i], got[i][0]) for i in range(3)]) == [True] * 3
    assert all(runs[0][i][0] != runs[1][i][0] for i in range(3))
    # fullprove: one pass, snarkjs's shape; a violated check raises with its text, and the next proof is correct
    proof, pub = prover.fullprove(calc, fc.inputs(1), blinding_of(1))
    assert proof == world["exp"][1][0] and pub == [str(x) for x in fc.witness(world["c"], 1)[0][1:1 + k]]
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove(calc, {"x": 5, "y": 5}, blinding_of(0))
    assert str(e.value) == "constraint not satisfied: " + fc.TEXT
    assert prover.fullprove(calc, {"x": 4, "y": 3}, blinding_of(2))[0] == world["exp"][2][0]
    assert ver.verify(*reversed(prover.fullprove(calc, fc.inputs(4))))
    assert prover.timings()["total"] > 0
    prover.close(), calc.close(), ver.close()


def test_refusals_and_errors(amd, monkeypatch, world):
    prover, calc = handles(amd, monkeypatch, world)
    c = world["c"]
    host = amd.WitnessCalculator(c["prog"], device=-1)
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(host, [fc.inputs(0)])
    assert str(e.value).endswith("plonk fullprove: the calculator runs on the host route (create it on the prover's device)")
    other = fc.ladder(fc.LADDER_K) if c["n_public"] == 1 else fc.tiny()
    wrong = amd.WitnessCalculator(other["prog"], device=0)
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(wrong, [fc.inputs(0)])
    # (the key's R1CS wire count: nVars less the addition signals)
    assert str(e.value).endswith(f"plonk fullprove: the program has {other['n_wires']} wires and {other['n_public']} public "
                                 f"signals, the key {c['n_wires']} and {c['n_public']}")
    assert prover.fullprove_batch(calc, []) == []
    assert amd.load().g16_plonk_fullprove_batch(prover._h, calc._h, None, 2, 0, None, None, None, None) == 0
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(calc, [fc.inputs(0), [ref.R + 1, 2]], [blinding_of(0), blinding_of(1)])
    assert e.value.code == -2 and "witness 1: input x[0] is not reduced modulo the scalar field" in str(e.value)
    # a blinding scalar that is not below r fails the call; the handles stay usable
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(calc, [fc.inputs(0), fc.inputs(1)], [blinding_of(0), [ref.R] * 9])
    assert "blinding scalar not below r" in str(e.value)
    got = prover.fullprove_batch(calc, [fc.inputs(i) for i in range(2)], [blinding_of(i) for i in range(2)])
    assert got == world["exp"][:2]
    prover.close(), calc.close(), host.close(), wrong.close()
