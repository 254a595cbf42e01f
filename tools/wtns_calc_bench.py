#!/usr/bin/env python3
"""Timing of g16_wtns_calc at the nzcp_live size on one MI355X (the record is profiles/wtns_calc_bench.json):

  - the builder's route, the only one there was: nzcp_circuit_setup(want_zkey=False), seconds per witness;
  - the host route (device = -1), ms per witness, one thread;
  - the device, one witness (wall, and the device time of upload / kernel / download);
  - witnesses per second over a batch of distinct passes (tools/nzcp_pass.py), statuses only;
  - g16_stage_inputs + g16_prove_staged against g16_stage_witness + g16_prove_staged on the same witness (--key:
    the trapdoor setup of the live circuit takes a while, so it is optional).

    python tools/wtns_calc_bench.py [--batch 256] [--reps 5] [--key] [--params live|example] [--out file.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as entry  # noqa: E402
import nzcp_pass  # noqa: E402


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn, reps):
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
    ap.add_argument("--key", action="store_true")
    ap.add_argument("--params", default="live")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    amd = entry.load_package()
    live = a.params == "live"
    params = amd.NZCP_LIVE_PARAMS if live else amd.NZCP_EXAMPLE_PARAMS
    max_bytes = params[1]

    def tbs_of(i):
        return nzcp_pass.to_be_signed(f"Given{i}", f"Family{i % 97}", f"19{60 + i % 40}-0{1 + i % 9}-1{i % 10}", live=live,
                                      exp=1700000000 + i)
    res = {"circuit": "nzcp_" + a.params, "what": "tools/wtns_calc_bench.py on one MI355X; times in ms unless named otherwise "
           "(median, min, max of n calls after a warm-up call)"}
    tbs = tbs_of(0)
    t = time.perf_counter()
    built = amd.nzcp_circuit_setup(params, tbs, 77, want_zkey=a.key, want_r1cs=False)
    res["builder_s_per_witness" if not a.key else "builder_and_setup_s"] = round(time.perf_counter() - t, 3)
    if a.key:
        t = time.perf_counter()
        amd.nzcp_circuit_setup(params, tbs, 77, want_zkey=False)
        res["builder_s_per_witness"] = round(time.perf_counter() - t, 3)
    t = time.perf_counter()
    prog = amd.nzcp_witness_program(params)
    res["program_record_s"] = round(time.perf_counter() - t, 3)
    res["program_bytes"] = len(prog)
    t = time.perf_counter()
    host = amd.WitnessCalculator(prog, device=-1)
    res["program_load_s"] = round(time.perf_counter() - t, 3)
    res.update({"n_wires": host.n_wires, "n_inputs": host.n_inputs, "n_levels": host.n_levels})
    inputs = amd.nzcp_inputs(tbs, max_bytes)
    words, status = host.calculate(inputs)
    assert status == amd.NO_CHECK and words == built["wtns"][-len(words):], "host route differs from the builder"
    res["host_route_ms_per_witness"] = stats(timed(lambda: host.calculate(inputs, want_words=False), a.reps))
    t = time.perf_counter()
    dev = amd.WitnessCalculator(prog, device=0)
    res["device_create_s"] = round(time.perf_counter() - t, 3)
    dwords, dstatus = dev.calculate(inputs)
    assert (dwords, dstatus) == (words, status), "device differs from the host route"
    wall, parts = [], {"upload_ms": [], "kernel_ms": [], "download_ms": []}
    for _ in range(a.reps):
        t = time.perf_counter()
        dev.calculate(inputs, want_words=False)
        wall.append((time.perf_counter() - t) * 1e3)
        for k, v in dev.timings().items():
            parts[k].append(v)
    res["device_one_witness_wall_ms"] = stats(wall)
    res["device_one_witness"] = {k: stats(v) for k, v in parts.items()}
    batch = [amd.nzcp_inputs(tbs_of(i), max_bytes) for i in range(a.batch)]
    out = dev.calculate_batch(batch, want_words=False)          # warm-up: the chunk buffers grow here
    assert all(s == amd.NO_CHECK for _, s in out)
    secs = []
    for _ in range(2):
        t = time.perf_counter()
        dev.calculate_batch(batch, want_words=False)
        secs.append(round(time.perf_counter() - t, 4))
    res["batch"] = {"count": a.batch, "seconds": secs, "witnesses_per_s": round(a.batch / min(secs), 1),
                    "kernel_ms_total": round(dev.timings()["kernel_ms"], 2)}
    if a.key:
        import ctypes
        prover = amd.Prover(built["zkey"])
        r = s = (12345).to_bytes(32, "little")
        pr, pub = amd.Proof(), ctypes.create_string_buffer(prover.info.n_public * 32)

        def via_wtns():
            prover.stage(0, built["wtns"])
            assert prover.prove_staged_raw(0, r, s, pr, pub) == 0
            return bytes(pr.a) + bytes(pr.b) + bytes(pr.c) + pub.raw

        def via_inputs():
            assert prover.stage_inputs(1, dev, inputs) == amd.NO_CHECK
            assert prover.prove_staged_raw(1, r, s, pr, pub) == 0
            return bytes(pr.a) + bytes(pr.b) + bytes(pr.c) + pub.raw
        assert via_wtns() == via_inputs(), "the two staging routes give different proofs"
        res["stage_witness_plus_prove_ms"] = stats(timed(via_wtns, a.reps))
        res["stage_inputs_plus_prove_ms"] = stats(timed(via_inputs, a.reps))
        prover.close()
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
