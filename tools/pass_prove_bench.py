#!/usr/bin/env python3
"""Timing of "pass URI in, proof out" on one MI355X (the record is profiles/pass_prove_bench.json): --batch copies of the
specification's example pass on the nzcp_exampleTest key, by two routes in one process --

  one    g16_pass_fullprove_batch: the front end, ES256, the input words formed on the device, witnesses, proofs;
  three  what there was: g16_pass_verify_batch, then g16_nzcp_inputs per pass on the host (from ToBeSigned bytes the caller
         already holds: the host's own parse of the pass is NOT charged to this route), then g16_fullprove_batch.

Before anything is timed the tool asserts that both routes give the same proofs byte for byte under the same (r, s) and
that every pass was proved.  Wall ms per call: the median of --reps calls after one warm-up call, min, max and the spread
(max - min) beside it; bytes uploaded per call by each route are counted from the buffers handed to the library.

    python tools/pass_prove_bench.py [--batch 256] [--reps 5] [--out profiles/pass_prove_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as entry  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NOW = 1700000000


def stats(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2),
            "spread": round(max(xs) - min(xs), 2), "n": len(xs)}


def timed(fn, reps):
    fn()                                            # warm-up: buffers grow here
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    amd = entry.load_package()
    lib = amd.load()
    uri = open(os.path.join(GOLDEN, "example_pass_uri.txt")).read().strip()
    keys = json.load(open(os.path.join(GOLDEN, "nzcp_example_issuer.json")))["keys"]
    params = amd.NZCP_EXAMPLE_PARAMS
    m = params[1]
    (words, ok), = amd.pass_inputs([uri], m, device=-1)
    assert ok
    tbs_len = int.from_bytes(words[-32:], "little")
    tbs = bytes(sum(words[32 * (8 * i + k)] << (7 - k) for k in range(8)) for i in range(tbs_len))
    assert amd.nzcp_inputs(tbs, m) == words

    built = amd.nzcp_circuit_setup(params, tbs, 77, want_zkey=True)
    prover = amd.Prover(built["zkey"])
    calc = amd.WitnessCalculator(amd.nzcp_witness_program(params), device=0)
    ver = amd.PassVerifier(keys, device=0)
    n, p = a.batch, prover.info.n_public * 32
    uris = [uri] * n
    text, offsets = amd._pass_items(uris)
    blind = b"".join((1000 + 2 * i).to_bytes(32, "little") + (1001 + 2 * i).to_bytes(32, "little") for i in range(n))
    out1, out3 = (amd.Proof * n)(), (amd.Proof * n)()
    pub1, pub3 = C.create_string_buffer(n * p), C.create_string_buffer(n * p)
    res = (amd.PassProveResult * n)()
    records = (amd.PassResult * n)()
    st = (C.c_uint32 * n)()
    row = (8 * m + 1) * 32
    blob = C.create_string_buffer(n * row)

    def one():
        rc = lib.g16_pass_fullprove_batch(prover._h, calc._h, ver._h, text, offsets, n, NOW, amd.PASS_PROVE_MATCH_PUBLIC, blind, out1, pub1, res)
        assert rc == 0, lib.g16_last_error()

    def three():
        rc = lib.g16_pass_verify_batch(ver._h, text, offsets, n, NOW, records)
        assert rc == 0, lib.g16_last_error()
        for i in range(n):
            assert records[i].verdict == 0
            rc = lib.g16_nzcp_inputs(tbs, len(tbs), m, C.cast(C.addressof(blob) + i * row, C.c_char_p))
            assert rc == 0, lib.g16_last_error()
        rc = lib.g16_fullprove_batch(prover._h, calc._h, blob, 8 * m + 1, n, blind, out3, pub3, st)
        assert rc == 0, lib.g16_last_error()

    one()
    three()
    assert all(r.outcome == 0 for r in res), [r.outcome for r in res]
    assert bytes(out1) == bytes(out3) and pub1.raw == pub3.raw, "the two routes differ"
    t_one = timed(one, a.reps)
    ms_front = ver.timings()
    ms_prover = prover.timings()
    t_three = timed(three, a.reps)
    s1, s3 = stats(t_one), stats(t_three)
    text_bytes = len(text) + (n + 1) * 8
    out = {"what": "tools/pass_prove_bench.py on one MI355X; wall ms per call (median, min, max, spread = max - min of n calls after a warm-up call)",
           "workload": f"{n} copies of the example pass, nzcp_exampleTest key ({calc.n_wires} wires), MATCH_PUBLIC set on the one call",
           "checked": "both routes give the same proofs and public signals byte for byte; every pass proved",
           "one_call_ms": s1, "three_call_ms": s3,
           "one_call_minus_three_call_ms": round(s1["median"] - s3["median"], 2),
           "within_spread": s1["median"] - s3["median"] <= max(s1["spread"], s3["spread"]),
           "bytes_uploaded": {"one_call": text_bytes + 4 * n + 64 * n, "three_call": text_bytes + n * row + 64 * n,
                              "note": "text + offsets (+ the selection list; + the input words), and r | s per proof"},
           "timings_of_the_last_one_call": {"pass_verifier_ms": [round(x, 3) for x in ms_front], "prover": ms_prover}}
    line = json.dumps(out, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    prover.close(), calc.close(), ver.close()


if __name__ == "__main__":
    main()
