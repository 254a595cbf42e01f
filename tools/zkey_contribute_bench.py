#!/usr/bin/env python3
"""`zkey contribute` / `zkey verify frominit` bench (csrc/zkey_scale.hip, csrc/zkey_mpc.cpp) on a 2^20-domain key of the
nzcp_live shape (g16_synth_setup: 850 000 wires and rows, 513 public signals -- 849 486 points in section 8, 2^20 in
section 9).  Runs contribute and verify `--repeats` times each and prints the device time of the scaling kernels, points
per second and the wall times (the library's G16_TRACE_HOST lines).  Yardstick, same process and device: the per-product
time of the existing variable-base product, kernel time / point multiplications of the G1 sections of one
`powersoftau prepare phase2` of power 16 (pp_mul_kernel, a per-lane scalar and signed 3-bit windows).

    python tools/zkey_contribute_bench.py [--n 850000] [--repeats 3] [--ptau-power 16] [--windows 3,4,5] [--ptau-leg]
--windows: also time the kernel at these window widths (G16_CONTRIBUTE_WINDOW), `--repeats` contributions each.
--ptau-leg: after the verifications without a ptau, as many with the ptau leg (csrc/zkey_verify_h.hip), in the same
process: an unprepared g16_ptau_synth ceremony of the key's own tau at the key's power, so the leg accepts; the
library's whole G16_TRACE_HOST line of every verification is kept ("trace").
Prints one JSON line.  A tool, not a test; not part of bench.py."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def traced(fn):
    """fn() with G16_TRACE_HOST=1 and the library's stderr lines captured -> (result, text, wall seconds)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["G16_TRACE_HOST"] = "1"
        t0 = time.time()
        try:
            out = fn()
        finally:
            wall = time.time() - t0
            del os.environ["G16_TRACE_HOST"]
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode("utf-8", "replace"), wall


def zkey_header(zkey):
    """section 2 of a .zkey image"""
    entry.oracle_path()
    import formats
    return formats.section(zkey, formats.read_binfile(zkey, "zkey", 2), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=850_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ptau-power", type=int, default=16)
    ap.add_argument("--windows", default="")
    ap.add_argument("--ptau-leg", action="store_true")
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()
    entry.oracle_path()
    import synth

    def log(m):
        print(f"[zkey contribute bench] {m}", file=sys.stderr, flush=True)
    t0 = time.time()
    amd.setup_device(0)
    try:
        zkey, _, _ = amd.synth_setup(a.n, 513, a.n, synth.SEED_NZCP, 0)
    finally:
        amd.setup_device(-1)
    log(f"synthetic key nVars = nConstraints = {a.n}: {len(zkey) / 1e6:.0f} MB in {time.time() - t0:.1f}s")
    d, s = 0x1f2e3d4c5b6a7988 ** 3, 0x0123456789abcdef ** 3
    runs = []
    new = None
    for i in range(a.repeats):
        (new, _), text, wall = traced(lambda: amd.zkey_contribute(zkey, "bench", d + i, s, device=0))
        m = re.search(r"zkey contribute: points (\d+); kernels ([\d.]+) ms, transfers ([\d.]+) ms", text)
        pts, kern, xfer = int(m.group(1)), float(m.group(2)), float(m.group(3))
        runs.append({"points": pts, "kernel_ms": kern, "transfer_ms": xfer, "wall_s": round(wall, 3),
                     "ns_per_product": round(kern * 1e6 / pts, 2), "points_per_s": round(pts / (kern * 1e-3))})
        log(f"contribute {i}: {runs[-1]}")
    sweep = {}
    for w in [int(x) for x in a.windows.split(",") if x]:
        os.environ["G16_CONTRIBUTE_WINDOW"] = str(w)
        try:
            ns = []
            for i in range(a.repeats):
                (other, _), text, _ = traced(lambda: amd.zkey_contribute(zkey, "bench", d + a.repeats - 1, s, device=0))
                assert other == new, f"window {w} gives other bytes"
                m = re.search(r"points (\d+); kernels ([\d.]+) ms", text)
                ns.append(round(float(m.group(2)) * 1e6 / int(m.group(1)), 2))
        finally:
            del os.environ["G16_CONTRIBUTE_WINDOW"]
        sweep[str(w)] = ns
        log(f"window {w}: ns per product {ns}")
    verifies = []
    for i in range(a.repeats):
        (ok, why), text, wall = traced(lambda: amd.zkey_verify_from_init(zkey, new, device=0))
        m = re.search(r"MSM ([\d.]+) ms, pairings ([\d.]+) ms", text)
        verifies.append({"ok": ok, "msm_ms": float(m.group(1)), "pairing_ms": float(m.group(2)), "wall_s": round(wall, 3),
                         "trace": text.strip()})
        log(f"verify {i}: {verifies[-1]} {why}")
    leg = []
    if a.ptau_leg:
        import groth16
        td = groth16.trapdoor(synth.SEED_NZCP + 1)   # g16_synth_setup's trapdoor for this seed
        power = int.from_bytes(zkey_header(zkey)[80:84], "little").bit_length() - 1   # log2 of the domain
        t0 = time.time()
        pot = amd.ptau_synth(power, td["tau"], td["alpha"], td["beta"], prepared=False, device=0)
        log(f"ptau of power {power}: {len(pot) / 1e6:.0f} MB in {time.time() - t0:.1f}s")
        for i in range(a.repeats):
            (ok, why), text, wall = traced(lambda: amd.zkey_verify_from_init(zkey, new, device=0, ptau=pot))
            m = re.search(r"MSM ([\d.]+) ms, pairings ([\d.]+) ms \((\d+)\); ptau leg: points (\d+), NTT ([\d.]+) ms, MSM ([\d.]+) ms", text)
            leg.append({"ok": ok, "msm_ms": float(m.group(1)), "pairing_ms": float(m.group(2)), "leg_points": int(m.group(4)),
                        "leg_ntt_ms": float(m.group(5)), "leg_msm_ms": float(m.group(6)), "wall_s": round(wall, 3),
                        "trace": text.strip()})
            log(f"verify with the ptau leg {i}: {leg[-1]} {why}")
        del pot
    # the yardstick: pp_mul_kernel's products in one prepare of power P (G1 sections 12, 14, 15)
    ptau = amd.ptau_synth(a.ptau_power, 12345, 678, 91011, prepared=False, device=0)
    _, text, wall = traced(lambda: amd.ptau_prepare(ptau, device=0))
    m = re.search(r"kernels section 12 ([\d.]+) ms, 13 ([\d.]+) ms, 14 ([\d.]+) ms, 15 ([\d.]+) ms; point multiplications G1 (\d+)", text)
    g1_ms = float(m.group(1)) + float(m.group(3)) + float(m.group(4))
    g1_muls = int(m.group(5))
    old = {"power": a.ptau_power, "g1_kernel_ms": round(g1_ms, 3), "g1_muls": g1_muls,
           "ns_per_product": round(g1_ms * 1e6 / g1_muls, 2), "wall_s": round(wall, 3)}
    log(f"ptau prepare: {old}")
    per = [r["ns_per_product"] for r in runs]
    print(json.dumps({"tool": "zkey_contribute_bench", "n": a.n, "window": int(os.environ.get("G16_CONTRIBUTE_WINDOW", 5)), "contribute": runs, "window_sweep_ns_per_product": sweep, "verify": verifies, "verify_ptau_leg": leg,
                      "ptau_prepare_yardstick": old, "new_ns_per_product_min_max": [min(per), max(per)],
                      "spread_ns": round(max(per) - min(per), 2),
                      "within_yardstick": min(per) <= old["ns_per_product"] + (max(per) - min(per))}))


if __name__ == "__main__":
    main()
