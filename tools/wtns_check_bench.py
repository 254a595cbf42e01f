#!/usr/bin/env python3
"""Measures g16_wtns_check at the nzcp_live size (DESIGN.md "Witness check"; results: profiles/wtns_check_bench.json).

  1. one check on the device: host wall time of the call (parse, upload, kernels, verdict) and the device times of the
     upload and of the kernels alone, beside qap_ms of a prover on the same circuit in the same process (g16_get_timings);
  2. the same check on the host route (device = -1, at most 16 threads);
  3. checks per second over a batch of 1024 witnesses (g16_wtns_check_batch; the batch repeats one witness image, as the
     chunks are uploaded and checked one witness at a time this changes nothing but the host memory the script needs).

  python tools/wtns_check_bench.py [--out profiles/wtns_check_bench.json] [--circuit nzcp_live|nzcp_example|sha256]
                                   [--batch 1024] [--device 0 | -1 = host route only, no GPU needed]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wtns_check_bench.json"))
    ap.add_argument("--circuit", default="nzcp_live", choices=["nzcp_live", "nzcp_example", "sha256"])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()
    import formats as f
    dev = a.device
    threads = min(16, len(os.sched_getaffinity(0)))
    if dev >= 0:
        amd.setup_device(dev)
    t0 = time.time()
    if a.circuit == "sha256":
        out = amd.sha256_message_setup(bytes(range(64)), 5, threads, want_zkey=dev >= 0, want_r1cs=True)
    else:
        import nzcp_pass
        live = a.circuit == "nzcp_live"
        tbs = nzcp_pass.to_be_signed("Jack", "Sparrow", "1960-04-16", live=live, exp=1951416330)
        out = amd.nzcp_circuit_setup(amd.NZCP_LIVE_PARAMS if live else amd.NZCP_EXAMPLE_PARAMS, tbs, 77, threads,
                                     want_zkey=dev >= 0, want_r1cs=True)
    r1cs, wtns = out["r1cs"], out["wtns"]
    n_wires = (len(wtns) - 76) // 32
    hdr = f.read_binfile(r1cs, "r1cs", 1)
    n_cons = int.from_bytes(f.section(r1cs, hdr, 1)[60:64], "little")
    res = {"circuit": a.circuit, "n_constraints": n_cons, "n_wires": n_wires, "wtns_bytes": len(wtns),
           "host_threads": threads, "setup_s": round(time.time() - t0, 1)}
    print(res, flush=True)
    # a witness that breaks somewhere in the middle: the verdicts of both routes must agree (not a timing)
    w = f.read_wtns(wtns)["w"]
    bad = list(w)
    bad[n_wires // 2] = (bad[n_wires // 2] + 1) % f.R
    bad_wtns = f.write_wtns(bad)
    del w, bad

    host = amd.R1csChecker(r1cs, device=-1)
    assert host.check(wtns).ok
    vb = host.check(bad_wtns)
    assert not vb.ok
    res["host_check_ms"] = stats(timed(lambda: host.check(wtns), 5))
    res["bad_witness"] = {"constraint": vb.constraint, "n_failed": vb.n_failed}
    print("host", res["host_check_ms"], flush=True)
    if dev >= 0:
        prover = amd.Prover(out["zkey"], device=dev)
        qap = []
        for _ in range(6):
            prover.prove(wtns)
            qap.append(prover.timings()["qap_ms"])
        res["prover_qap_ms"] = stats(qap[1:])
        t0 = time.time()
        k = amd.R1csChecker(r1cs, device=dev)
        res["checker_create_s"] = round(time.time() - t0, 2)
        for _ in range(3):
            assert k.check(wtns).ok
        vd = k.check(bad_wtns)
        assert (vd.constraint, vd.n_failed, vd.a, vd.b, vd.c) == (vb.constraint, vb.n_failed, vb.a, vb.b, vb.c)
        wall, up, kern = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            k.check(wtns)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = k.timings()
            up.append(t["upload_ms"])
            kern.append(t["kernel_ms"])
        res["device_check_wall_ms"] = stats(wall)       # parse + upload + kernels + verdict, host clock around the call
        res["device_upload_ms"] = stats(up)             # device events around the copy of the 32-byte words
        res["device_kernels_ms"] = stats(kern)          # witness already uploaded: Montgomery images + the check kernel
        res["kernels_over_qap"] = round(res["device_kernels_ms"]["median"] / res["prover_qap_ms"]["median"], 3)
        print({x: res[x] for x in ("prover_qap_ms", "device_check_wall_ms", "device_upload_ms", "device_kernels_ms")}, flush=True)
        batch = [wtns] * a.batch
        k.check_batch(batch[:8])
        runs = []
        for _ in range(2):
            t0 = time.perf_counter()
            vs = k.check_batch(batch)
            runs.append(time.perf_counter() - t0)
            assert all(v.ok for v in vs)
        t = k.timings()
        res["batch"] = {"count": a.batch, "seconds": [round(x, 3) for x in runs], "checks_per_s": round(a.batch / min(runs), 1),
                        "upload_ms_total": round(t["upload_ms"], 1), "kernels_ms_total": round(t["kernel_ms"], 1)}
        print(res["batch"], flush=True)
        k.close()
        prover.close()
    host.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
