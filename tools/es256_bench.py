#!/usr/bin/env python3
"""Measures ES256 pass-signature verification (DESIGN.md "ES256"; results: profiles/es256_bench.json).

  1. signatures per second at batches of 1, 64, 1 024 and 65 536 on device 0 and on the host route (device -1), with the
     two phase times of g16_es256_verifier_timings at each size (the batch repeats 64 signatures of the reference over
     three keys: the work does not depend on the values);
  2. g16_verify_batch alone against g16_nzcp_pass_proof_verify_batch for 1 024 proofs of the 513-signal test circuit,
     alternating: how much of the signature work the Miller loops hide;
  3. with --parent-lib NAME (a build of the parent commit beside this one, nzcp-circom_amd/lib/NAME: the G16_LIB_NAME
     switch): g16_verify_batch's 1 024-proof time under both builds, --repeats child processes each, alternating.

  python tools/es256_bench.py [--out profiles/es256_bench.json] [--device 0 | -1 = host route only] [--parent-lib NAME]
"""
import argparse
import ctypes
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

BATCHES = (1, 64, 1024, 65536)
PROOFS = 1024


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs),
            "all": [round(x, 4) for x in xs]}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def signature_pool():
    import random

    import p256_ref as ref
    rng = random.Random(9)
    ds = [rng.randrange(1, ref.N) for _ in range(3)]
    keys = [ref.point_bytes(ref.mul(d, ref.G)) for d in ds]
    digests, sigs, idx = [], [], []
    for i in range(64):
        e = rng.randrange(2**256)
        r, s = ref.sign(ds[i % 3], rng.randrange(1, 2**40), e)
        digests.append(ref.be(e))
        sigs.append(ref.be(r) + ref.be(s))
        idx.append(i % 3)
    return keys, digests, sigs, idx


def bench_signatures(amd, device, reps):
    keys, digests, sigs, idx = signature_pool()
    v = amd.Es256Verifier(keys, device=device)
    out = {}
    for n in BATCHES:
        if device < 0 and n > 1024:
            reps_n = 2
        else:
            reps_n = reps
        k = (n + 63) // 64
        d, s, ix = b"".join(digests * k)[:32 * n], b"".join(sigs * k)[:64 * n], (idx * k)[:n]
        assert all(v.verify_batch(d, s, ix))   # warm-up, and every verdict
        walls, phases = [], []
        for _ in range(reps_n):
            walls.append(wall_ms(lambda: v.verify_batch(d, s, ix)))
            phases.append(v.timings())
        med = statistics.median(walls)
        out[str(n)] = {"wall_ms": stats(walls), "signatures_per_s": round(n / med * 1e3, 1),
                       "scalars_ms": stats([p[0] for p in phases]), "sum_compare_ms": stats([p[1] for p in phases])}
    v.close()
    return out


def proofs_1024(amd):
    import es256_cases as cases
    vkey, pubs, proofs = cases.pass_circuit(amd)
    pr = amd.proof_from_obj(proofs["a"]) * PROOFS
    pb = b"".join(int(x).to_bytes(32, "little") for x in pubs["a"]) * PROOFS
    return vkey, pr, pb


def bench_combined(amd, reps):
    import es256_cases as cases
    vkey, pr, pb = proofs_1024(amd)
    _, sig, _ = cases.golden_pass()
    ver = amd.Verifier(vkey, cases.N_PUB, montgomery=True, device=0)
    es = amd.Es256Verifier([cases.golden_key()], device=0)
    sg = sig * PROOFS
    alone, both = [], []
    for i in range(reps + 2):   # (two warm-up rounds)
        a = wall_ms(lambda: ver.verify_raw(pr, pb, PROOFS))
        b = wall_ms(lambda: amd.nzcp_pass_proof_verify(ver, es, pr, pb, sg))
        if i >= 2:
            alone.append(a)
            both.append(b)
    assert all(ver.verify_raw(pr, pb, PROOFS)) and set(amd.nzcp_pass_proof_verify(ver, es, pr, pb, sg)) == {0}
    sig_alone = [wall_ms(lambda: es.verify_batch(cases.golden_pass()[0] * PROOFS, sg)) for _ in range(reps)]
    ver.close()
    es.close()
    return {"proofs": PROOFS, "verify_batch_ms": stats(alone), "pass_proof_verify_batch_ms": stats(both),
            "es256_alone_ms": stats(sig_alone)}


class _Tolerant(ctypes.CDLL):
    """A build of the parent commit lacks the entry points this one adds: the binding's load() may name them."""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if not name.startswith("g16_"):
                raise
            return type("Missing", (), {})()


def child_verify_ms():
    """One process, one build (G16_LIB_NAME): median wall time of five 1 024-proof g16_verify_batch calls after two."""
    amd = entry.load_package()
    amd.C.CDLL = _Tolerant
    amd.load()
    import es256_cases as cases
    vkey, pr, pb = proofs_1024(amd)
    ver = amd.Verifier(vkey, cases.N_PUB, montgomery=True, device=0)
    xs = [wall_ms(lambda: ver.verify_raw(pr, pb, PROOFS)) for _ in range(7)][2:]
    ver.close()
    print(json.dumps({"verify_batch_ms": statistics.median(xs)}))


def bench_parent(parent_lib, repeats):
    res = {"parent": [], "this": []}
    for _ in range(repeats):
        for which, name in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("G16_LIB_NAME", None)
            if name:
                env["G16_LIB_NAME"] = name
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                                 timeout=300)
            if out.returncode:
                raise SystemExit(f"child ({which}) failed:\n{out.stdout}{out.stderr}")
            res[which].append(json.loads(out.stdout.strip().splitlines()[-1])["verify_batch_ms"])
    p, t = res["parent"], res["this"]
    return {"proofs": PROOFS, "parent_ms": stats(p), "this_ms": stats(t),
            "this_median_inside_parent_spread": min(p) <= statistics.median(t) <= max(p)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "es256_bench.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child_verify_ms()
        return
    amd = entry.load_package()
    amd.load()
    res = {"tool": "tools/es256_bench.py", "lanes_per_signature": 16, "host_route": bench_signatures(amd, -1, a.reps)}
    if a.device >= 0:
        res["device"] = bench_signatures(amd, a.device, a.reps)
        res["combined_1024"] = bench_combined(amd, a.reps)
        if a.parent_lib:
            res["verify_batch_parent_vs_this"] = bench_parent(a.parent_lib, a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
