#!/usr/bin/env python3
"""Challenge / response exchange bench (csrc/ptau_points.hip, csrc/ptau_mpc.cpp) at power `--power`, all in one process:
  - the three point kernels through their layer entries on section 2 (G1, 2^(power+1) - 1 points) and section 3 (G2,
    2^power points) of a contributed file: `--repeats` runs each of compress, decompress (with the big-endian images)
    and from-be, ns per point from the kernel events;
  - the yardstick, same process and device: ptau_scale's ns per product for G1 and G2 from `--repeats` runs of
    `powersoftau contribute` on the same file (the library's G16_TRACE_HOST line);
  - the wall time of export challenge, challenge contribute and import response, and that the imported file is the
    contributed one byte for byte.
Condition, by operation count: a G1 root is one exponentiation in Fq (~380 products) against ~3 500 for a scalar
multiplication, a G2 root two of them against three times as many: decompression must come out below the scaling's ns per
product of the same group.  "condition" in the result says whether it does; the ratios are recorded, not fixed.

    python tools/ptau_challenge_bench.py [--power 20] [--repeats 3]
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


def section(ptau, sid):
    """Payload of section `sid` of a binfile image (u32 id, u64 size records after the 12-byte header)."""
    pos = 12
    while pos < len(ptau):
        i, size = int.from_bytes(ptau[pos:pos + 4], "little"), int.from_bytes(ptau[pos + 4:pos + 12], "little")
        if i == sid:
            return ptau[pos + 12:pos + 12 + size]
        pos += 12 + size
    raise KeyError(sid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()

    def log(m):
        print(f"[ptau challenge bench] {m}", file=sys.stderr, flush=True)
    secret = tuple(pow(7 + i, 12345 + i, (1 << 253) - 1) | 1 for i in range(6))
    old = amd.ptau_contribute(amd.ptau_new(a.power), "before", secret, device=0)[0]
    log(f"contributed file of power {a.power}: {len(old) / 1e6:.0f} MB")

    # the yardstick: ptau_scale per product
    scale, want = [], None
    for i in range(a.repeats):
        want, text, wall = traced(lambda: amd.ptau_contribute(old, "bench", secret, device=0))
        m = re.search(r"points G1 (\d+) G2 (\d+); kernels G1 ([\d.]+) ms G2 ([\d.]+) ms", text)
        scale.append({"g1_ns_per_product": round(float(m.group(3)) * 1e6 / int(m.group(1)), 2),
                      "g2_ns_per_product": round(float(m.group(4)) * 1e6 / int(m.group(2)), 2), "wall_s": round(wall, 3)})
        log(f"contribute {i}: {scale[-1]}")

    # the kernels, per group
    kernels = {}
    for group, sid in ((1, 2), (2, 3)):
        lem = section(old, sid)
        n = len(lem) // (64 * group)
        runs = []
        for i in range(a.repeats):
            comp, bad, c_ms = amd.ptau_points_compress(group, lem)
            back, bad2, d_ms, be = amd.ptau_points_decompress(group, comp)
            again, bad3, f_ms = amd.ptau_points_from_be(group, be)
            assert (bad, bad2, bad3) == (-1, -1, -1) and back == lem and again == lem
            runs.append({"compress_ns_per_point": round(c_ms * 1e6 / n, 3), "decompress_ns_per_point": round(d_ms * 1e6 / n, 3),
                         "from_be_ns_per_point": round(f_ms * 1e6 / n, 3)})
            log(f"G{group} ({n} points) run {i}: {runs[-1]}")
        kernels[f"g{group}"] = {"points": n, "runs": runs}
        del lem, comp, back, be, again

    # the three calls
    t0 = time.time()
    challenge = amd.ptau_export_challenge(old)
    calls = {"export_challenge_wall_s": round(time.time() - t0, 3)}
    (response, h), text, wall = traced(lambda: amd.ptau_challenge_contribute(challenge, secret, device=0))
    calls["challenge_contribute_wall_s"] = round(wall, 3)
    calls["challenge_contribute_trace"] = [x for x in text.splitlines() if "[g16] ptau challenge contribute" in x][-1:]
    (new, h2), text, wall = traced(lambda: amd.ptau_import_response(old, response, "bench", device=0))
    calls["import_response_wall_s"] = round(wall, 3)
    calls["import_response_trace"] = [x for x in text.splitlines() if "[g16] ptau import response" in x][-1:]
    calls["same_bytes_as_contribute"] = (new, h2) == want and h == h2
    log(f"calls: {calls}")

    best_scale = {g: min(r[f"{g}_ns_per_product"] for r in scale) for g in ("g1", "g2")}
    worst = {g: max(r["decompress_ns_per_point"] for r in kernels[g]["runs"]) for g in ("g1", "g2")}
    ratio = {g: round(best_scale[g] / worst[g], 2) for g in ("g1", "g2")}
    print(json.dumps({"tool": "ptau_challenge_bench", "power": a.power, "kernels": kernels, "ptau_scale_yardstick": scale, "calls": calls,
                      "scale_ns_per_product_over_decompress_ns_per_point": ratio,
                      "condition": all(worst[g] < best_scale[g] for g in ("g1", "g2")) and calls["same_bytes_as_contribute"]}))


if __name__ == "__main__":
    main()
