#!/usr/bin/env python3
"""Measures pass verification from URIs (results: profiles/pass_verify_bench.json).

  1. wall time of g16_pass_verify_batch at batches of 1, 64, 1 024 and 65 536 on device 0 and on the host route (device
     -1), with the three phase times of g16_pass_verifier_timings (the batch repeats 64 valid passes of the test builders
     over three keys);
  2. the front end's cost: the same batch through g16_es256_verify_batch alone, digests precomputed, in the same process;
  3. with --parent-lib NAME (a build of the parent commit beside this one, nzcp-circom_amd/lib/NAME: the G16_LIB_NAME
     switch): g16_es256_verify_batch's 1 024-signature time under both builds, --repeats child processes each, alternating.
Medians of 7 calls after a warm-up.  Every step that uses the GPU is a child process under its own `timeout -k 10`; the
first that fails ends the run.

  python tools/pass_verify_bench.py [--out profiles/pass_verify_bench.json] [--device 0 | -1 = host route only] [--parent-lib NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
from es256_bench import _Tolerant, stats, wall_ms  # noqa: E402

BATCHES = (1, 64, 1024, 65536)


def pass_pool():
    """64 valid passes over three keys, and what the ES256 handle needs for the same work: keys, digests, r | s, indices"""
    import base64

    import pass_cases as cases
    import pass_ref
    keys, names, _, _ = cases.key_set()
    uris = [cases.example_uri()]
    for i in range(63):
        uris.append(cases.make(kid=(cases.KID_A, cases.KID_B)[i % 2], subj=cases.subject(f"Given{i}", "Family" + "x" * (i % 9), "1980-01-02")))
    fronts = [pass_ref.front(u, names) for u in uris]
    assert all(r["verdict"] == 0 for r, _ in fronts)
    b64 = lambda v: base64.urlsafe_b64decode(v + "=" * (-len(v) % 4))
    packed = [b64(keys[n]["x"]) + b64(keys[n]["y"]) for n in names]
    return keys, uris, packed, [r["tbs_sha256"] for r, _ in fronts], [s for _, s in fronts], [r["key_idx"] for r, _ in fronts]


def step_route(device, reps):
    amd = entry.load_package()
    amd.load()
    keys, uris, packed, digests, sigs, idx = pass_pool()
    v = amd.PassVerifier(keys, device=device)
    es = amd.Es256Verifier(packed, device=device)
    out = {}
    for n in BATCHES:
        reps_n = 2 if device < 0 and n > 1024 else reps
        k = (n + 63) // 64
        batch = (uris * k)[:n]
        d, s, ix = b"".join(digests * k)[:32 * n], b"".join(sigs * k)[:64 * n], (idx * k)[:n]
        text, offsets = amd._pass_items(batch)
        records = (amd.PassResult * n)()
        lib = amd.load()

        def call():
            amd._check(lib.g16_pass_verify_batch(v._h, text, offsets, n, 1700000000, records))
        # (both calls straight through ctypes on prepared buffers: the wrappers' per-item conversions are not the library's)
        key_idx, ok = (amd.C.c_uint32 * n)(*ix), amd.C.create_string_buffer(n)

        def call_es():
            amd._check(lib.g16_es256_verify_batch(es._h, d, s, key_idx, n, ok))
        call()   # warm-up, and every verdict
        assert all(r.verdict == 0 for r in records)
        call_es()
        assert ok.raw == b"\x01" * n
        walls, phases, alone = [], [], []
        for _ in range(reps_n):
            walls.append(wall_ms(call))
            phases.append(v.timings())
            alone.append(wall_ms(call_es))
        med, med_alone = statistics.median(walls), statistics.median(alone)
        out[str(n)] = {"wall_ms": stats(walls), "passes_per_s": round(n / med * 1e3, 1), "text_bytes": len(text),
                       "front_ms": stats([p[0] for p in phases]), "scalars_ms": stats([p[1] for p in phases]),
                       "sum_compare_ms": stats([p[2] for p in phases]), "es256_alone_wall_ms": stats(alone),
                       "front_end_cost_ms": round(med - med_alone, 4)}
    v.close()
    es.close()
    print(json.dumps(out))


def step_child():
    """One process, one build (G16_LIB_NAME): median wall time of five 1 024-signature g16_es256_verify_batch calls after two."""
    amd = entry.load_package()
    amd.C.CDLL = _Tolerant
    amd.load()
    _, _, packed, digests, sigs, idx = pass_pool()
    es = amd.Es256Verifier(packed, device=0)
    d, s, ix = b"".join(digests * 16), b"".join(sigs * 16), idx * 16
    assert all(es.verify_batch(d, s, ix))
    xs = [wall_ms(lambda: es.verify_batch(d, s, ix)) for _ in range(7)][2:]
    es.close()
    print(json.dumps({"es256_verify_batch_ms": statistics.median(xs)}))


def run_step(args, limit, env=None):
    """a child of this tool under its own time limit; its last line is its JSON"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    out = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if out.returncode:
        raise SystemExit(f"step {' '.join(args)} failed with {out.returncode}: nothing more is started\n{out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def bench_parent(parent_lib, repeats):
    res = {"parent": [], "this": []}
    for _ in range(repeats):
        for which, name in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("G16_LIB_NAME", None)
            if name:
                env["G16_LIB_NAME"] = name
            res[which].append(run_step(["--step", "child"], 120, env)["es256_verify_batch_ms"])
    p, t = res["parent"], res["this"]
    return {"signatures": 1024, "parent_ms": stats(p), "this_ms": stats(t),
            "this_median_inside_parent_spread": min(p) <= statistics.median(t) <= max(p)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pass_verify_bench.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--step", default=None)
    a = ap.parse_args()
    if a.step == "child":
        return step_child()
    if a.step == "route":
        return step_route(a.device, a.reps)
    res = {"tool": "tools/pass_verify_bench.py", "passes_per_workgroup": 32,
           "host_route": run_step(["--step", "route", "--device", "-1", "--reps", str(a.reps)], 300)}
    if a.device >= 0:
        res["device"] = run_step(["--step", "route", "--device", str(a.device), "--reps", str(a.reps)], 300)
        if a.parent_lib:
            res["es256_verify_batch_parent_vs_this"] = bench_parent(a.parent_lib, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
