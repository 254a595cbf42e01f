"""g16_fullprove_batch: a batch of inputs in, Groth16 proofs and public signals out, the witnesses computed in device
chunks and proved from the chunk buffer (csrc/wtns_calc.hip, csrc/prover.cpp).  The reference route is the one that
exists beside it: calc.wtns -> Prover.stage -> prove_staged with the same (r, s), which the new call must equal byte for
byte; the public signals are checked against the host-route calculator and against wtns_prog_ref's big-integer
evaluation.  The circuits are crafted (fullprove_circuits.py: tiny, and ladder(300) whose 9.6 KB of public signals per
witness make the collection cross rows and chunks)."""
import pytest

import formats as f
import fullprove_circuits as fc
import wtns_prog_ref as ref

pytestmark = pytest.mark.gpu

NMAX = 7


def rs_of(i):
    """Fixed, distinct blinding scalars of pass i."""
    return f.le(1000003 * (i + 1) + 17), f.le(pow(7, 40 + i, ref.R))


@pytest.fixture(scope="module", params=["tiny", "ladder"])
def world(request, amd):
    """A circuit, its key, and the reference route's proofs of passes 0..NMAX-1 (computed once, never changed)."""
    c = fc.tiny() if request.param == "tiny" else fc.ladder(fc.LADDER_K)
    zkey, vkey = amd.r1cs_setup(c["r1cs"], 5)
    host = amd.WitnessCalculator(c["prog"], device=-1)
    prover = amd.Prover(zkey, device=0)
    exp = []
    for i in range(NMAX):
        prover.stage(0, host.wtns(fc.inputs(i)))
        proof, pub = prover.prove_staged(0, *rs_of(i))
        words, status = host.calculate(fc.inputs(i))
        pub_bytes = words[32:32 * (1 + c["n_public"])]
        assert status == amd.NO_CHECK and pub_bytes == fc.public_bytes(c, i)
        assert [int(x) for x in pub] == [int.from_bytes(pub_bytes[32 * j:32 * j + 32], "little") for j in range(c["n_public"])]
        exp.append((proof, pub_bytes, amd.NO_CHECK))
    prover.close(), host.close()
    return {"c": c, "zkey": zkey, "vkey": vkey, "exp": exp}


def handles(amd, monkeypatch, world, chunk=None, ctx=None):
    """-> (prover, device calculator), created under the chunk and context settings (both are read at create)."""
    for name, v in (("G16_WTNS_CALC_CHUNK", chunk), ("G16_BATCH_CTX", ctx)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    return amd.Prover(world["zkey"], device=0), amd.WitnessCalculator(world["c"]["prog"], device=0)


@pytest.mark.parametrize("ctx", [1, 3])
@pytest.mark.parametrize("chunk", [None, 1, 2])
def test_bit_identity(amd, monkeypatch, world, chunk, ctx):
    """Proof i and row i of pub equal the reference route's, whatever the chunking and the number of contexts; count 7
    with chunk 1 and chunk 2 goes through each of the two chunk buffers at least twice."""
    prover, calc = handles(amd, monkeypatch, world, chunk, ctx)
    for count in (1, 2, 3, 4, 7):
        got = prover.fullprove_batch(calc, [fc.inputs(i) for i in range(count)], [rs_of(i) for i in range(count)])
        assert got == world["exp"][:count], (count, chunk, ctx)
    prover.close(), calc.close()


@pytest.mark.parametrize("ctx", [1, 3])
@pytest.mark.parametrize("bad", [[0], [2], [4], [1, 2], [0, 1, 2, 3, 4]], ids=["first", "middle", "last", "straddle", "all"])
def test_verdicts(amd, monkeypatch, world, bad, ctx):
    """A violated check is a verdict: status and text, a zeroed proof and pub row (the binding's None, None), and
    neighbours that are bit identical to the reference route.  Chunk 2: positions 1 and 2 straddle a chunk boundary."""
    prover, calc = handles(amd, monkeypatch, world, 2, ctx)
    n = 5
    got = prover.fullprove_batch(calc, [fc.inputs(i, violate=i in bad) for i in range(n)], [rs_of(i) for i in range(n)])
    for i in range(n):
        if i in bad:
            assert got[i] == (None, None, 0) and calc.check_text(got[i][2]) == fc.TEXT
        else:
            assert got[i] == world["exp"][i], i
    # ... the bytes behind the binding's None: all zero
    import ctypes as C
    words = b"".join(calc.words(fc.inputs(i, violate=i in bad)) for i in range(n))
    p = 32 * world["c"]["n_public"]
    prs, pub, st = (amd.Proof * n)(), C.create_string_buffer(b"\xaa" * (n * p), n * p), (C.c_uint32 * n)()
    C.memset(prs, 0xaa, C.sizeof(prs))
    blind = b"".join(r + s for r, s in map(rs_of, range(n)))
    assert amd.load().g16_fullprove_batch(prover._h, calc._h, words, 2, n, blind, prs, pub, st) == 0
    for i in range(n):
        zero = i in bad
        assert (bytes(prs[i]) == bytes(256)) == zero and (pub.raw[i * p:(i + 1) * p] == bytes(p)) == zero
        assert st[i] == (0 if zero else amd.NO_CHECK)
        if not zero:
            assert amd.proof_to_obj(prs[i]) == world["exp"][i][0] and pub.raw[i * p:(i + 1) * p] == world["exp"][i][1]
    prover.close(), calc.close()


def test_random_blinding(amd, monkeypatch, world):
    """rs=None: the OS CSPRNG blinds; every proof verifies with its public signals, and two calls differ."""
    prover, calc = handles(amd, monkeypatch, world, 2)
    ver = amd.Verifier(world["vkey"], world["c"]["n_public"])
    n = 5
    runs = [prover.fullprove_batch(calc, [fc.inputs(i) for i in range(n)]) for _ in range(2)]
    for got in runs:
        assert [(pub, st) for _, pub, st in got] == [(pub, st) for _, pub, st in world["exp"][:n]]
        pubs = [[int.from_bytes(pub[32 * j:32 * j + 32], "little") for j in range(world["c"]["n_public"])] for _, pub, _ in got]
        assert ver.verify_batch([(pubs[i], got[i][0]) for i in range(n)]) == [True] * n
        assert all(got[i][0] != world["exp"][i][0] for i in range(n))
    assert all(runs[0][i][0] != runs[1][i][0] for i in range(n))
    prover.close(), calc.close(), ver.close()


def test_handle_state(amd, monkeypatch, world):
    """The prover's witness slots are as they were; both handles stay usable after a success, a verdict and an error."""
    prover, calc = handles(amd, monkeypatch, world, 2)
    host = amd.WitnessCalculator(world["c"]["prog"], device=-1)
    prover.stage(0, host.wtns(fc.inputs(6)))
    prover.stage(3, host.wtns(fc.inputs(5)))
    assert prover.prove_staged(0, *rs_of(6))[0] == world["exp"][6][0]
    n = 5
    got = prover.fullprove_batch(calc, [fc.inputs(i, violate=i == 1) for i in range(n)], [rs_of(i) for i in range(n)])
    assert got == [world["exp"][i] if i != 1 else (None, None, 0) for i in range(n)]
    assert prover.prove_staged(0, *rs_of(6))[0] == world["exp"][6][0]
    assert prover.prove_staged(3, *rs_of(5))[0] == world["exp"][5][0]
    # a second, shorter batch on the same two handles
    assert prover.fullprove_batch(calc, [fc.inputs(i) for i in range(2)], [rs_of(i) for i in range(2)]) == world["exp"][:2]
    # an input word equal to r: the whole call fails before the device is touched, and the next call is correct
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(calc, [fc.inputs(0), fc.inputs(1), [3, ref.R]], [rs_of(i) for i in range(3)])
    assert e.value.code == -2   # G16_E_FORMAT
    assert "witness 2: input y[0] is not reduced modulo the scalar field" in str(e.value)
    assert prover.fullprove_batch(calc, [fc.inputs(i) for i in range(3)], [rs_of(i) for i in range(3)]) == world["exp"][:3]
    assert prover.prove_staged(0, *rs_of(6))[0] == world["exp"][6][0]
    # the calculator alone, and the one-pass device route, still work
    assert calc.calculate(fc.inputs(4)) == host.calculate(fc.inputs(4))
    assert prover.stage_inputs(1, calc, fc.inputs(2)) == amd.NO_CHECK
    assert prover.prove_staged(1, *rs_of(2))[0] == world["exp"][2][0]
    t = prover.timings()
    assert t["total_ms"] > 0
    prover.close(), calc.close(), host.close()


def test_refusals(amd, monkeypatch, world):
    prover, calc = handles(amd, monkeypatch, world)
    c = world["c"]
    host = amd.WitnessCalculator(c["prog"], device=-1)
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(host, [fc.inputs(0)])
    assert str(e.value).endswith("fullprove: the calculator runs on the host route (create it on the prover's device)")
    # the other circuit's program against this key
    other = fc.ladder(fc.LADDER_K) if c["n_public"] == 1 else fc.tiny()
    wrong = amd.WitnessCalculator(other["prog"], device=0)
    with pytest.raises(amd.G16Error) as e:
        prover.fullprove_batch(wrong, [fc.inputs(0)])
    assert str(e.value).endswith(f"fullprove: the program has {other['n_wires']} wires and {other['n_public']} public signals, "
                                 f"the key {c['n_wires']} and {c['n_public']}")
    # count == 0 succeeds and touches nothing
    assert prover.fullprove_batch(calc, []) == []
    assert amd.load().g16_fullprove_batch(prover._h, calc._h, None, 2, 0, None, None, None, None) == 0
    # one (r, s) too few is the binding's refusal
    with pytest.raises(amd.G16Error):
        prover.fullprove_batch(calc, [fc.inputs(0), fc.inputs(1)], [rs_of(0)])
    assert prover.fullprove_batch(calc, [fc.inputs(0)], [rs_of(0)]) == world["exp"][:1]
    prover.close(), calc.close(), host.close(), wrong.close()
