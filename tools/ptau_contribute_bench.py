#!/usr/bin/env python3
"""`powersoftau contribute` / `powersoftau verify` bench (csrc/ptau_scale.hip, csrc/ptau_mpc.cpp): one contribution to
the generator file of power `--power` (2^(power+1) - 1 + 2 * 2^power products on G1, 2^power + 1 on G2), at every window
width of `--windows`, `--repeats` runs each, the whole sweep twice so that the widths alternate (drift shows as a
difference between the two rounds), all in one process.  Prints ns per product for G1 and for G2 from the kernel events
(scaling + conversion to affine + big-endian images) and the wall time of the call (the library's G16_TRACE_HOST line),
then one verification of the result.  Yardstick, same process and device: kernel time / point multiplications of one
`powersoftau prepare phase2` of power `--ptau-power` (pp_mul_kernel: the same per-lane product at window 3 inside the
transform, butterflies included), for the G1 sections and for the G2 section.

    python tools/ptau_contribute_bench.py [--power 20] [--repeats 3] [--windows 3,4,5] [--ptau-power 16]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--windows", default="3,4,5")
    ap.add_argument("--ptau-power", type=int, default=16)
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()

    def log(m):
        print(f"[ptau contribute bench] {m}", file=sys.stderr, flush=True)
    src = amd.ptau_new(a.power)
    log(f"generator file of power {a.power}: {len(src) / 1e6:.0f} MB")
    secret = tuple(pow(7 + i, 12345 + i, (1 << 253) - 1) | 1 for i in range(6))
    windows = [int(x) for x in a.windows.split(",") if x]
    sweep = {str(w): [] for w in windows}
    first = None
    for rnd in range(2):
        for w in windows:
            os.environ["G16_PTAU_WINDOW"] = str(w)
            try:
                for i in range(a.repeats):
                    (new, _), text, wall = traced(lambda: amd.ptau_contribute(src, "bench", secret, device=0))
                    if first is None:
                        first = new
                    assert new == first, f"window {w} gives other bytes"
                    m = re.search(r"points G1 (\d+) G2 (\d+); kernels G1 ([\d.]+) ms G2 ([\d.]+) ms, transfers ([\d.]+) ms; host hashing ([\d.]+) ms",
                                  text)
                    g1, g2, k1, k2, xf, hs = int(m.group(1)), int(m.group(2)), *(float(m.group(j)) for j in (3, 4, 5, 6))
                    run = {"round": rnd, "g1_ns_per_product": round(k1 * 1e6 / g1, 2), "g2_ns_per_product": round(k2 * 1e6 / g2, 2),
                           "kernel_ms": round(k1 + k2, 3), "transfer_ms": xf, "host_hashing_ms": hs, "wall_s": round(wall, 3)}
                    sweep[str(w)].append(run)
                    log(f"window {w} round {rnd} run {i}: {run}")
            finally:
                del os.environ["G16_PTAU_WINDOW"]
    (ok, why), text, wall = traced(lambda: amd.ptau_verify(first, device=0))
    m = re.search(r"MSM ([\d.]+) ms \((\d+) points\), pairings ([\d.]+) ms", text)
    verify = {"ok": ok, "msm_ms": float(m.group(1)), "msm_points": int(m.group(2)), "pairing_ms": float(m.group(3)), "wall_s": round(wall, 3)}
    log(f"verify: {verify} {why}")
    del first, src
    # the yardstick: pp_mul_kernel's products in one prepare of power P (G1 sections 12, 14, 15; G2 section 13)
    ptau = amd.ptau_synth(a.ptau_power, 12345, 678, 91011, prepared=False, device=0)
    old = []
    for i in range(a.repeats):
        _, text, wall = traced(lambda: amd.ptau_prepare(ptau, device=0))
        m = re.search(r"kernels section 12 ([\d.]+) ms, 13 ([\d.]+) ms, 14 ([\d.]+) ms, 15 ([\d.]+) ms; point multiplications G1 (\d+) G2 (\d+)", text)
        g1_ms = float(m.group(1)) + float(m.group(3)) + float(m.group(4))
        old.append({"power": a.ptau_power, "g1_ns_per_product": round(g1_ms * 1e6 / int(m.group(5)), 2),
                    "g2_ns_per_product": round(float(m.group(2)) * 1e6 / int(m.group(6)), 2), "wall_s": round(wall, 3)})
        log(f"ptau prepare {i}: {old[-1]}")
    best = {w: {k: min(r[k] for r in runs) for k in ("g1_ns_per_product", "g2_ns_per_product")} for w, runs in sweep.items()}
    print(json.dumps({"tool": "ptau_contribute_bench", "power": a.power, "runs": sweep, "min_ns_per_product": best, "verify": verify,
                      "ptau_prepare_yardstick": old}))


if __name__ == "__main__":
    main()
