"""g16_pass_inputs on the host route (device -1): a pass URI -> the input words of its proof, toBeSigned[8 M] (a bit a
word, MSB first per byte, zero beyond the length) and toBeSignedLen -- the csrc/nzcp_pass.cuh code that pass_inputs_kernel
runs on the device (test_gpu_pass_prove.py compares the two routes byte for byte on the same passes).  The expectation is
Python's: pass_ref.front says whether a pass is well-formed and how long its ToBeSigned is, pass_prove_circuits.tbs_of
gives the bytes, and the words are Python integers."""
import functools
import hashlib

import pytest

import pass_cases as pc
import pass_prove_circuits as ppc
import pass_ref
import wtns_prog_ref as ref

M = ppc.M_MAIN


def expected_row(uri, m):
    """(words, ok) by the contract: a zero row for a pass that is not well-formed or whose ToBeSigned exceeds m"""
    rec = pass_ref.front(uri, [])[0]
    if rec["verdict"] in (pass_ref.MALFORMED, pass_ref.TOO_LONG) or rec["tbs_len"] > m:
        return bytes((8 * m + 1) * 32), False
    return ppc.input_words(ppc.tbs_of(uri), m), True


@functools.lru_cache(None)
def edge_passes():
    """(name, uri): the passes the issue names, shared with the GPU tests"""
    out = [("example", pc.example_uri())]
    out += [(name, uri) for name, uri, _ in pc.padding_cases()]
    # the protected header's byte-string head grows at 24 bytes: a kid of 18 / 19 bytes makes a header of 23 / 24
    for k in (18, 19):
        uri = pc.make(kid="k" * k, d=pc.D_A)
        assert len(pc.protected_header("k" * k)) == 5 + k
        out.append((f"protected {5 + k} bytes", uri))
    out += [(name, uri) for name, uri, _ in pc.cbor_cases()[:2]]   # payload of 255 / 256 bytes: its head grows
    for n in (M - 1, M, M + 1):
        out.append((f"tbs_len {n}", ppc.pass_with_tbs_len(n)))
    return out


def test_edges_word_for_word(amd):
    names, uris = zip(*edge_passes())
    for m in (M, 400):   # (400: the padding cases reach 375 bytes)
        got = amd.pass_inputs(uris, m, device=-1)
        for name, uri, g in zip(names, uris, got):
            assert g == expected_row(uri, m), (name, m)
    oks = dict(zip(names, [ok for _, ok in amd.pass_inputs(uris, M, device=-1)]))
    assert oks[f"tbs_len {M - 1}"] and oks[f"tbs_len {M}"] and not oks[f"tbs_len {M + 1}"]
    assert oks["example"] and oks["payload 255 bytes"] and oks["payload 256 bytes"]
    oks = dict(zip(names, [ok for _, ok in amd.pass_inputs(uris, 400, device=-1)]))
    assert all(oks.values())   # (the headers of 23 / 24 bytes and the padding cases among them)


def test_corpus_and_malformed(amd):
    """every pass of the corpus, the malformed and the too long ones among them: a zero row and ok = 0"""
    uris, records = pc.corpus()
    uris = list(uris) + [c[1] for c in pc.cbor_cases()] + [c[1] for c in pc.cap_cases()]
    got = amd.pass_inputs(uris, M, device=-1)
    n_bad = 0
    for i, (uri, g) in enumerate(zip(uris, got)):
        assert g == expected_row(uri, M), (i, uri[:40])
        if pass_ref.front(uri, [])[0]["verdict"] in (1, 7):
            assert g == (bytes((8 * M + 1) * 32), False)
            n_bad += 1
    assert n_bad >= 10
    assert amd.pass_inputs([], M, device=-1) == []


def test_equals_nzcp_inputs(amd):
    """the image g16_nzcp_inputs writes from the Python-derived ToBeSigned"""
    for name, uri in edge_passes():
        tbs = ppc.tbs_of(uri)
        for m in (M, 503):
            if len(tbs) <= m:
                assert amd.pass_inputs([uri], m, device=-1)[0] == (amd.nzcp_inputs(tbs, m), True), (name, m)


@pytest.mark.parametrize("m", [ppc.M_MAIN, ppc.M_ODD])
def test_pack_circuit_on_the_words(amd, m):
    """pack(m) evaluated by the host-route calculator on those words gives the Python public signals; the pass with the
    last bit set violates check 0 with its text"""
    c = ppc.pack(m)
    calc = amd.WitnessCalculator(c["prog"], device=-1)
    uris = list(ppc.good_passes(5, m)) + [ppc.base_pass(odd=True)]
    rows = amd.pass_inputs(uris, m, device=-1)
    for uri, (words, ok) in zip(uris, rows):
        tbs = ppc.tbs_of(uri)
        if len(tbs) > m:
            assert not ok
            continue
        assert ok
        body, status = calc.calculate(words)
        w, want_status = ref.evaluate(c["n_wires"], c["ops"], ppc.bits_of(tbs, m) + [len(tbs)])
        assert status == want_status == (0 if ppc.violates(tbs, m) else amd.NO_CHECK)
        if status == amd.NO_CHECK:
            assert body[32:32 * (1 + c["n_public"])] == ppc.public_bytes(tbs, m)
        else:
            assert calc.check_text(status) == ppc.TEXT
    calc.close()


def test_argument_errors(amd):
    for m in (0, 504):
        with pytest.raises(amd.G16Error) as e:
            amd.pass_inputs([pc.example_uri()], m, device=-1)
        assert e.value.code == -1 and "max_bytes must be 1 to 503" in str(e.value)
    with pytest.raises(amd.G16Error):
        amd.pass_inputs([pc.example_uri()], M, device=-2)


def test_real_circuit_public_signals_match_the_front_end(amd):
    """The MATCH_PUBLIC relation on real data, host routes only: the 513 public signals of nzcp_exampleTest, computed by
    the host calculator from g16_pass_inputs' words of the example URI, are the bits of the host front end's
    cred_subj_sha256 and tbs_sha256 (MSB first) and its exp -- two routes that share no code."""
    from test_cpu_sha256_circuit import example_public_signals
    uri = pc.example_uri()
    m = amd.NZCP_EXAMPLE_PARAMS[1]
    (words, ok), = amd.pass_inputs([uri], m, device=-1)
    assert ok
    calc = amd.WitnessCalculator(amd.nzcp_witness_program(amd.NZCP_EXAMPLE_PARAMS), device=-1)
    assert calc.n_public == 513
    body, status = calc.calculate(words)
    calc.close()
    assert status == amd.NO_CHECK
    pub = [int.from_bytes(body[32 * j:32 * j + 32], "little") for j in range(1, 514)]
    assert pub == list(example_public_signals())
    (rec,) = pc.run_batch(amd, -1, [uri], pc.NOW)
    assert rec["flags"] & amd.PASS_HAS_SUBJECT
    bits = lambda d: [(d[k >> 3] >> (7 - (k & 7))) & 1 for k in range(256)]
    assert pub == bits(rec["cred_subj_sha256"]) + bits(rec["tbs_sha256"]) + [rec["exp"]]
    assert rec["cred_subj_sha256"] == hashlib.sha256(b"Jack,Sparrow,1960-04-16").digest()
