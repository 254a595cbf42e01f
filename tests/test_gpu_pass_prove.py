"""g16_pass_fullprove_batch, its PLONK twin and the device route of g16_pass_inputs: pass URIs in, proofs out, the
circuit's input words formed on the device by pass_inputs_kernel (csrc/pass_prove.hip) where the witness calculator reads
them.  The reference route is the one that exists beside it: host g16_pass_inputs -> WitnessCalculator(-1).wtns ->
Prover.stage -> prove_staged with the same (r, s), which the new call must equal byte for byte; the records are
PassVerifier.verify_batch's.  Circuits and passes: pass_prove_circuits.py."""
import ctypes as C

import pytest

import formats as f
import pass_cases as pc
import pass_prove_circuits as ppc
import wtns_prog_ref as ref
from test_cpu_pass_inputs import edge_passes

pytestmark = pytest.mark.gpu

M = ppc.M_MAIN
NOW = pc.NOW
NMAX = 7
DONE, PASS, TOO_LONG, CHECK, MISMATCH = range(5)


def rs_of(i):
    return f.le(1000003 * (i + 1) + 17), f.le(pow(7, 40 + i, ref.R))


def blinding_of(i):
    return [pow(3, 100 * i + k + 11, ref.R) for k in range(9)]


# ------------------------------------------------------------------ the layer: device rows == host rows
def test_layer_device_equals_host(amd):
    uris = [u for _, u in edge_passes()] + list(pc.corpus()[0]) + [c[1] for c in pc.cbor_cases()] + [c[1] for c in pc.cap_cases()]
    for m in (M, 400):
        assert amd.pass_inputs(uris, m, device=0) == amd.pass_inputs(uris, m, device=-1), m
    assert amd.pass_inputs([], M, device=0) == []


def test_layer_counts_and_rewritten_rows(amd):
    """counts 1, 2, 3 and 65 with mixed lengths in one batch; then the 65 again with a short pass in every slot that held
    a long one: rows that are written again hold nothing of the longer pass.  M_ODD: 8 M + 1 words are no multiple of the
    workgroup's 256 lanes."""
    good = list(ppc.good_passes(7, ppc.M_ODD)) + list(ppc.good_passes(7, M))
    lens = [len(ppc.tbs_of(u)) for u in good]
    short = good[lens.index(min(lens))]
    batch = [good[(5 * i) % len(good)] for i in range(65)]
    for m in (M, ppc.M_ODD):
        for count in (1, 2, 3, 65):
            assert amd.pass_inputs(batch[:count], m, device=0) == amd.pass_inputs(batch[:count], m, device=-1), (m, count)
        again = [short if len(ppc.tbs_of(u)) > min(lens) + 8 else u for u in batch]
        assert again != batch
        assert amd.pass_inputs(again, m, device=0) == amd.pass_inputs(again, m, device=-1), m


# ------------------------------------------------------------------ Groth16
def reference(amd, prover, host, m, uri, i):
    """the existing route for pass `uri` as proof i: (proof object, public bytes)"""
    (words, ok), = amd.pass_inputs([uri], m, device=-1)
    assert ok
    prover.stage(0, host.wtns(words))
    proof, pub = prover.prove_staged(0, *rs_of(i))
    pub_bytes = ppc.public_bytes(ppc.tbs_of(uri), m)
    assert [int(x) for x in pub] == ppc.public_values(ppc.tbs_of(uri), m)
    return proof, pub_bytes


@pytest.fixture(scope="module")
def world(amd):
    """pack(320), its key, and the reference route's proofs of the good passes 0..NMAX-1 (computed once, never changed)"""
    c = ppc.pack(M)
    zkey, vkey = amd.r1cs_setup(c["r1cs"], 5)
    host = amd.WitnessCalculator(c["prog"], device=-1)
    prover = amd.Prover(zkey, device=0)
    uris = ppc.good_passes(NMAX, M)
    exp = [reference(amd, prover, host, M, u, i) for i, u in enumerate(uris)]
    prover.close(), host.close()
    return {"c": c, "zkey": zkey, "vkey": vkey, "uris": list(uris), "exp": exp}


def handles(amd, monkeypatch, world, chunk=None, ctx=None):
    """-> (prover, device calculator, pass verifier), created under the chunk and context settings (read at create)"""
    for name, v in (("G16_WTNS_CALC_CHUNK", chunk), ("G16_BATCH_CTX", ctx)):
        if v:
            monkeypatch.setenv(name, str(v))
        else:
            monkeypatch.delenv(name, raising=False)
    return (amd.Prover(world["zkey"], device=0), amd.WitnessCalculator(world["c"]["prog"], device=0),
            amd.PassVerifier(pc.key_set()[0], device=0))


def close(*hs):
    for h in hs:
        h.close()


def done(world, i, rec):
    """what the binding returns for good pass i"""
    return {"outcome": DONE, "check": 0xFFFFFFFF, "text": None, "pass": rec, "proof": world["exp"][i][0], "public": world["exp"][i][1]}


@pytest.mark.parametrize("ctx", [1, 3])
@pytest.mark.parametrize("chunk", [None, 1, 2])
def test_bit_identity(amd, monkeypatch, world, chunk, ctx):
    prover, calc, ver = handles(amd, monkeypatch, world, chunk, ctx)
    records = ver.verify_batch(world["uris"], NOW)
    assert all(r["verdict"] == 0 for r in records)
    for count in (1, 2, 3, 4, 7):
        got = prover.pass_fullprove_batch(calc, ver, world["uris"][:count], NOW, rs=[rs_of(i) for i in range(count)])
        assert got == [done(world, i, records[i]) for i in range(count)], (count, chunk, ctx)
    close(prover, calc, ver)


def test_bit_identity_odd_size(amd, monkeypatch):
    """pack(299): 2393 input words, no multiple of the workgroup; passes above 299 bytes are TOO_LONG, not proofs"""
    m = ppc.M_ODD
    c = ppc.pack(m)
    zkey, _ = amd.r1cs_setup(c["r1cs"], 6)
    monkeypatch.setenv("G16_WTNS_CALC_CHUNK", "2")
    prover, calc, host = amd.Prover(zkey, device=0), amd.WitnessCalculator(c["prog"], device=0), amd.WitnessCalculator(c["prog"], device=-1)
    ver = amd.PassVerifier(pc.key_set()[0], device=0)
    uris = list(ppc.good_passes(3, m))
    uris.insert(1, ppc.base_pass())
    exp = [reference(amd, prover, host, m, u, i) if len(ppc.tbs_of(u)) <= m else None for i, u in enumerate(uris)]
    got = prover.pass_fullprove_batch(calc, ver, uris, NOW, rs=[rs_of(i) for i in range(len(uris))])
    assert [g["outcome"] for g in got] == [DONE, TOO_LONG, DONE, DONE]
    for g, e in zip(got, exp):
        assert (g["proof"], g["public"]) == (e if e else (None, None))
    close(prover, calc, host, ver)


# ------------------------------------------------------------------ outcomes
def kinds():
    good = ppc.base_pass()
    return {
        "malformed": pc.make(unprotected=pc.cmap([(b"\x00", pc.nested(16))]), cti=bytes(16)),
        "alg": pc.make(protected=pc.protected_header(pc.KID_A, alg=b"\x27"), cti=bytes(16)),
        "key": pc.make(kid="nobody", d=pc.D_A, cti=bytes(16)),
        "sig": pc.spoil_sig(good),
        "nbf": pc.make(nbf=NOW + 1000, cti=bytes(16)),
        "exp": pc.make(exp=NOW - 5, cti=bytes(16)),
        "long": ppc.pass_with_tbs_len(M + 1),
        "violate": ppc.base_pass(odd=True),
    }


VERDICT = {"malformed": 1, "alg": 2, "key": 3, "sig": 4, "nbf": 5, "exp": 6, "long": 0, "violate": 0, "good": 0}
LAYOUTS = {
    "first-middle-last": ["malformed", "good", "alg", "good", "violate", "good", "long"],
    "straddle": ["good", "key", "sig", "nbf", "exp", "good", "good"],   # chunk 2: 1|2 and 3|4 are chunk boundaries
    "all": ["alg", "key", "sig", "nbf", "exp", "long", "violate"],
    "all-malformed-first": ["malformed", "violate", "long", "exp", "nbf", "sig", "key"],
}


def raw_call(amd, prover, calc, ver, uris, flags, n_public):
    """the C call on buffers pre-filled with 0xaa -> (proofs, pub bytes, results)"""
    n, p = len(uris), 32 * n_public
    text, offsets = amd._pass_items(uris)
    prs, pub, res = (amd.Proof * n)(), C.create_string_buffer(b"\xaa" * (n * p), n * p), (amd.PassProveResult * n)()
    C.memset(prs, 0xaa, C.sizeof(prs))
    C.memset(res, 0xaa, C.sizeof(res))
    blind = b"".join(r + s for r, s in map(rs_of, range(n)))
    assert amd.load().g16_pass_fullprove_batch(prover._h, calc._h, ver._h, text, offsets, n, NOW, flags, blind, prs, pub, res) == 0
    return prs, pub.raw, res


@pytest.mark.parametrize("unsigned_too", [False, True], ids=["signed", "unsigned"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_outcomes(amd, monkeypatch, world, layout, unsigned_too):
    prover, calc, ver = handles(amd, monkeypatch, world, 2, 3)
    host = amd.WitnessCalculator(world["c"]["prog"], device=-1)
    check = amd.Verifier(world["vkey"], world["c"]["n_public"])
    k = kinds()
    names = LAYOUTS[layout]
    uris = [world["uris"][i] if nm == "good" else k[nm] for i, nm in enumerate(names)]
    records = ver.verify_batch(uris, NOW)
    assert [r["verdict"] for r in records] == [VERDICT[nm] for nm in names]
    p = 32 * world["c"]["n_public"]
    prs, pub, res = raw_call(amd, prover, calc, ver, uris, amd.PASS_PROVE_UNSIGNED if unsigned_too else 0, world["c"]["n_public"])
    for i, nm in enumerate(names):
        v = VERDICT[nm]
        want = (PASS if v and not (unsigned_too and 3 <= v <= 6) else TOO_LONG if nm == "long" else CHECK if nm == "violate" else DONE)
        assert res[i].outcome == want, (i, nm)
        assert res[i].check == (0 if want == CHECK else 0xFFFFFFFF)
        if want == CHECK:
            assert calc.check_text(res[i].check) == ppc.TEXT
        assert amd._pass_record(res[i].record) == records[i], (i, nm)
        row = pub[i * p:(i + 1) * p]
        if want != DONE:
            assert bytes(prs[i]) == bytes(256) and row == bytes(p), (i, nm)
        elif nm == "good":   # the neighbours: bit identical to the reference route
            assert (amd.proof_to_obj(prs[i]), row) == world["exp"][i], i
        else:   # proved although the relying party would refuse it: the proof is a proof, the verdict is recorded
            assert 3 <= res[i].record.verdict <= 6
            assert row == ppc.public_bytes(ppc.tbs_of(uris[i]), M)
            signals = [int.from_bytes(row[32 * j:32 * j + 32], "little") for j in range(world["c"]["n_public"])]
            assert check.verify_batch([(signals, amd.proof_to_obj(prs[i]))]) == [True]
            assert (amd.proof_to_obj(prs[i]), row) == reference(amd, prover, host, M, uris[i], i)
    close(prover, calc, ver, host, check)


# ------------------------------------------------------------------ the PLONK twin
def test_plonk_twin(amd, monkeypatch, world):
    c = world["c"]
    zkey = amd.plonk_setup(c["r1cs"], 9, device=0)
    monkeypatch.setenv("G16_WTNS_CALC_CHUNK", "2")
    prover, calc, host = amd.PlonkProver(zkey, device=0), amd.WitnessCalculator(c["prog"], device=0), amd.WitnessCalculator(c["prog"], device=-1)
    ver = amd.PassVerifier(pc.key_set()[0], device=0)
    uris = world["uris"][:3]
    exp = []
    for i, u in enumerate(uris):
        (words, ok), = amd.pass_inputs([u], M, device=-1)
        proof, pub = prover.prove(host.wtns(words), blinding_of(i))
        assert [int(x) for x in pub] == ppc.public_values(ppc.tbs_of(u), M)
        exp.append((proof, world["exp"][i][1]))
    for count in (1, 3):
        got = prover.pass_fullprove_batch(calc, ver, uris[:count], NOW, blindings=[blinding_of(i) for i in range(count)])
        assert [(g["outcome"], g["proof"], g["public"]) for g in got] == [(DONE,) + e for e in exp[:count]]
    # a blocked pass and a violating one between two proofs
    mixed = [uris[0], kinds()["exp"], ppc.base_pass(odd=True), uris[1]]
    got = prover.pass_fullprove_batch(calc, ver, mixed, NOW, blindings=[blinding_of(i) for i in (0, 5, 6, 1)])
    assert [g["outcome"] for g in got] == [DONE, PASS, CHECK, DONE] and got[2]["text"] == ppc.TEXT
    assert [(g["proof"], g["public"]) for g in got] == [exp[0], (None, None), (None, None), exp[1]]
    host2 = amd.WitnessCalculator(c["prog"], device=-1)
    with pytest.raises(amd.G16Error) as e:
        prover.pass_fullprove_batch(host2, ver, uris[:1], NOW)
    assert str(e.value).endswith("plonk pass prove: the calculator runs on the host route (create it on the prover's device)")
    close(prover, calc, host, host2, ver)


# ------------------------------------------------------------------ state and refusals
def test_state_and_refusals(amd, monkeypatch, world):
    import fullprove_circuits as fc
    prover, calc, ver = handles(amd, monkeypatch, world, 2)
    c = world["c"]
    host = amd.WitnessCalculator(c["prog"], device=-1)
    uris, exp = world["uris"], world["exp"]
    words = [amd.pass_inputs([u], M, device=-1)[0][0] for u in uris]
    # witness slots staged before the call prove the same afterwards
    prover.stage(0, host.wtns(words[6]))
    prover.stage(3, host.wtns(words[5]))
    records = ver.verify_batch(uris, NOW)
    old_fullprove = prover.fullprove_batch(calc, words[:3], [rs_of(i) for i in range(3)])
    assert [(pr, pb) for pr, pb, _ in old_fullprove] == exp[:3]
    mixed = uris[:2] + [ppc.base_pass(odd=True), kinds()["sig"], uris[4]]
    got = prover.pass_fullprove_batch(calc, ver, mixed, NOW, rs=[rs_of(i) for i in range(5)])
    assert [g["outcome"] for g in got] == [DONE, DONE, CHECK, PASS, DONE]
    assert [(g["proof"], g["public"]) for g in got if g["outcome"] == DONE] == [exp[0], exp[1], exp[4]]
    assert prover.prove_staged(0, *rs_of(6))[0] == exp[6][0]
    assert prover.prove_staged(3, *rs_of(5))[0] == exp[5][0]
    # a second, shorter batch on the same handles; then the old calls give their old answers
    got = prover.pass_fullprove_batch(calc, ver, uris[:2], NOW, rs=[rs_of(i) for i in range(2)])
    assert [(g["proof"], g["public"]) for g in got] == exp[:2]
    assert ver.verify_batch(uris, NOW) == records
    assert prover.fullprove_batch(calc, words[:3], [rs_of(i) for i in range(3)]) == old_fullprove

    def refused(code, tail, *args, **kw):
        with pytest.raises(amd.G16Error) as e:
            prover.pass_fullprove_batch(*args, **kw)
        assert e.value.code == code and str(e.value).endswith(tail), str(e.value)
        # ... and every handle is as usable as before
        assert ver.verify_batch(uris[:2], NOW) == records[:2]
        assert prover.fullprove_batch(calc, words[:3], [rs_of(i) for i in range(3)]) == old_fullprove
        got = prover.pass_fullprove_batch(calc, ver, uris[:1], NOW, rs=[rs_of(0)])
        assert (got[0]["proof"], got[0]["public"]) == exp[0]

    refused(-5, "pass prove: the calculator runs on the host route (create it on the prover's device)", host, ver, uris[:1], NOW)
    host_ver = amd.PassVerifier(pc.key_set()[0], device=-1)
    refused(-5, "pass prove: the pass verifier runs on the host route (create it on the prover's device)", calc, host_ver, uris[:1], NOW)
    # a program with other inputs: the tiny circuit of the fullprove tests, under its own key
    t = fc.tiny()
    tz, _ = amd.r1cs_setup(t["r1cs"], 5)
    tp, tc = amd.Prover(tz, device=0), amd.WitnessCalculator(t["prog"], device=0)
    with pytest.raises(amd.G16Error) as e:
        tp.pass_fullprove_batch(tc, ver, uris[:1], NOW)
    assert e.value.code == -1 and str(e.value).endswith("pass prove: the program's inputs are not toBeSigned[8 M] and toBeSignedLen")
    with pytest.raises(amd.G16Error) as e:
        prover.pass_fullprove_batch(tc, ver, uris[:1], NOW)
    assert str(e.value).endswith(f"pass prove: the program has {t['n_wires']} wires and 1 public signals, the key {c['n_wires']} and {c['n_public']}")
    refused(-1, f"pass prove: MATCH_PUBLIC takes the 513 public signals of NZCPPubIdentity, the program has {c['n_public']}",
            calc, ver, uris[:1], NOW, flags=amd.PASS_PROVE_MATCH_PUBLIC)
    # count = 0 with NULL buffers succeeds
    assert prover.pass_fullprove_batch(calc, ver, [], NOW) == []
    assert amd.load().g16_pass_fullprove_batch(prover._h, calc._h, ver._h, None, None, 0, NOW, 0, None, None, None, None) == 0
    close(prover, calc, ver, host, host_ver, tp, tc)


# ------------------------------------------------------------------ MATCH_PUBLIC
def test_mismatch_on_a_program_that_ignores_the_pass(amd, monkeypatch):
    """513 public outputs that are constants: the front end's digests cannot be theirs, so MATCH_PUBLIC leaves the pass
    out with G16_PROVE_MISMATCH and zero bytes; without the flag the same pass is proved."""
    c = ppc.constant(513)
    zkey, vkey = amd.r1cs_setup(c["r1cs"], 7)
    monkeypatch.delenv("G16_WTNS_CALC_CHUNK", raising=False)
    prover, calc = amd.Prover(zkey, device=0), amd.WitnessCalculator(c["prog"], device=0)
    ver = amd.PassVerifier(pc.key_set()[0], device=0)
    uris = list(ppc.good_passes(2, M)) + [ppc.base_pass(odd=True)]
    prs, pub, res = raw_call(amd, prover, calc, ver, uris, amd.PASS_PROVE_MATCH_PUBLIC, 513)
    assert [r.outcome for r in res] == [MISMATCH, MISMATCH, CHECK]
    assert all(bytes(pr) == bytes(256) for pr in prs) and pub == bytes(len(pub))
    prs, pub, res = raw_call(amd, prover, calc, ver, uris, 0, 513)
    assert [r.outcome for r in res] == [DONE, DONE, CHECK]
    assert pub[:2 * 513 * 32] == ref.words([7] * 1026) and bytes(prs[0]) != bytes(256)
    close(prover, calc, ver)


# ------------------------------------------------------------------ the real circuit
def test_real_circuit_fed_on_the_device(amd):
    """nzcp_exampleTest's program on the device, its input words formed by pass_inputs_kernel from the example URI (no
    key, no proof): the 513 public signals are the golden ones, and they are the bits of the front end's two digests
    and its exp -- the MATCH_PUBLIC relation on real data."""
    from test_cpu_sha256_circuit import example_public_signals
    uri = pc.example_uri()
    calc = amd.WitnessCalculator(amd.nzcp_witness_program(amd.NZCP_EXAMPLE_PARAMS), device=0)
    assert calc.n_public == 513 and calc.inputs == {"toBeSigned": (0, 8 * 314), "toBeSignedLen": (8 * 314, 1)}
    got = amd.pass_wtns_public(calc, [uri, "NZCP:/1/====", ppc.base_pass()])
    calc.close()
    assert got[1] == (None, amd.PASS_WTNS_NO_ROW) and got[2] == (None, amd.PASS_WTNS_NO_ROW)   # malformed; 318 > 314 bytes
    pub, status = got[0]
    assert status == amd.NO_CHECK
    signals = [int.from_bytes(pub[32 * j:32 * j + 32], "little") for j in range(513)]
    assert signals == list(example_public_signals())
    (rec,) = pc.run_batch(amd, 0, [uri], NOW)
    bits = lambda d: [(d[k >> 3] >> (7 - (k & 7))) & 1 for k in range(256)]
    assert rec["flags"] & amd.PASS_HAS_SUBJECT
    assert signals == bits(rec["cred_subj_sha256"]) + bits(rec["tbs_sha256"]) + [rec["exp"]]
