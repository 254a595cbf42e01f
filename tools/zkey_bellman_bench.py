#!/usr/bin/env python3
"""MPCParams exchange bench (csrc/zkey_bellman.hip, csrc/zkey_bellman_host.cpp) on a 2^20-domain key of the nzcp_live
shape (g16_synth_setup, as tools/zkey_contribute_bench.py: 850 000 wires and rows, 513 public signals), ONE run of each
call in one process:
  - `zkey export bellman`, `zkey bellman contribute`, `zkey import bellman`: wall time and the library's G16_TRACE_HOST
    line of each (the basis change's kernel time and product count are in the export's and the import's);
  - the transform's ns per scalar product, forward and inverse;
  - the yardstick, same process and device: ptau_scale's ns per G1 product from one `powersoftau contribute` of power
    `--ptau-power` (its trace line), as tools/ptau_challenge_bench.py takes it;
  - that `zkey verify frominit` accepts the imported key.
No threshold: the figures are recorded.

    python tools/zkey_bellman_bench.py [--n 850000] [--ptau-power 18]
Prints one JSON line.  A tool, not a test; not part of bench.py."""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry  # noqa: E402
from ptau_contribute_bench import traced  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=850_000)
    ap.add_argument("--ptau-power", type=int, default=18)
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()
    entry.oracle_path()
    import synth

    def log(m):
        print(f"[zkey bellman bench] {m}", file=sys.stderr, flush=True)
    t0 = time.time()
    amd.setup_device(0)
    try:
        zkey, _, _ = amd.synth_setup(a.n, 513, a.n, synth.SEED_NZCP, 0)
    finally:
        amd.setup_device(-1)
    log(f"synthetic key nVars = nConstraints = {a.n}: {len(zkey) / 1e6:.0f} MB in {time.time() - t0:.1f}s")
    d, s = 0x1f2e3d4c5b6a7988 ** 3, 0x0123456789abcdef ** 3

    def line(text, what):
        return [x for x in text.splitlines() if f"[g16] {what}:" in x][-1]

    def basis(trace):
        m = re.search(r"basis ([\d.]+) ms \((\d+) products\)", trace)
        ms, n = float(m.group(1)), int(m.group(2))
        return {"kernel_ms": ms, "products": n, "ns_per_product": round(ms * 1e6 / n, 2)}

    calls = {}
    exp, text, wall = traced(lambda: amd.zkey_export_bellman(zkey, device=0))
    calls["export"] = {"wall_s": round(wall, 3), "bytes": len(exp), "trace": line(text, "zkey export bellman")}
    log(f"export: {calls['export']}")
    (resp, h), text, wall = traced(lambda: amd.zkey_bellman_contribute(exp, d, s, device=0))
    calls["contribute"] = {"wall_s": round(wall, 3), "trace": line(text, "zkey bellman contribute")}
    log(f"contribute: {calls['contribute']}")
    new, text, wall = traced(lambda: amd.zkey_import_bellman(zkey, resp, "bench", device=0))
    calls["import"] = {"wall_s": round(wall, 3), "trace": line(text, "zkey import bellman")}
    log(f"import: {calls['import']}")
    transform = {"forward": basis(calls["export"]["trace"]), "inverse": basis(calls["import"]["trace"])}
    t0 = time.time()
    ok, why = amd.zkey_verify_from_init(zkey, new, device=0)
    verify = {"ok": ok, "reason": why, "wall_s": round(time.time() - t0, 3)}
    direct, h2 = amd.zkey_contribute(zkey, "bench", d, s, device=0)
    same = h == h2
    del exp, resp, new, direct

    secret = tuple(pow(7 + i, 12345 + i, (1 << 253) - 1) | 1 for i in range(6))
    old = amd.ptau_contribute(amd.ptau_new(a.ptau_power), "before", secret, device=0)[0]
    _, text, wall = traced(lambda: amd.ptau_contribute(old, "bench", secret, device=0))
    m = re.search(r"points G1 (\d+) G2 (\d+); kernels G1 ([\d.]+) ms G2 ([\d.]+) ms", text)
    yard = {"power": a.ptau_power, "g1_points": int(m.group(1)), "g1_kernel_ms": float(m.group(3)),
            "g1_ns_per_product": round(float(m.group(3)) * 1e6 / int(m.group(1)), 2)}
    print(json.dumps({"tool": "zkey_bellman_bench", "n": a.n, "runs": 1, "calls": calls, "transform": transform,
                      "ptau_scale_yardstick": yard, "verify_imported_key": verify, "same_hash_as_zkey_contribute": same,
                      "transform_over_yardstick": {k: round(v["ns_per_product"] / yard["g1_ns_per_product"], 2) for k, v in transform.items()}}))


if __name__ == "__main__":
    main()
