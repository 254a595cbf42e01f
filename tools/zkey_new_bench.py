#!/usr/bin/env python3
"""`zkey new` with the circuit hash (csrc/zkey_cshash.hip, csrc/zkey_cshash_host.cpp) beside the setup without it, on the
nzcp_live circuit (830 227 rows, domain 2^20) and a g16_ptau_synth ceremony of power 20, all in one process on one
device:
  * wall time of g16_zkey_new and of g16_groth16_setup_ptau, alternating, `--repeats` runs each after one warm-up setup;
  * the library's G16_TRACE_HOST line of the hash stage of every zkey_new run: kernel time of the difference kernel and
    of the to-be conversions, transfers, time inside the hash, the stage's own wall time;
  * the streaming hash alone (g16_blake2b512) over a buffer of the image's length, `--repeats` times.
What is wanted: zkey_new exceeds the setup by the hash's own time plus the spread of the setup runs; more means the
overlap of device work and hash is not working.  The two keys are checked to differ in section 10 alone.

    python tools/zkey_new_bench.py [--repeats 3] [--power 20]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--power", type=int, default=20)
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()
    import nzcp_pass

    def log(m):
        print(f"[zkey new bench] {m}", file=sys.stderr, flush=True)
    t0 = time.time()
    tbs = nzcp_pass.to_be_signed("Anne-Marie", "Te Whare", "1987-11-30", live=True, exp=1700000000)
    r1cs = amd.nzcp_circuit_setup(amd.NZCP_LIVE_PARAMS, tbs, 77, want_zkey=False, want_r1cs=True)["r1cs"]
    log(f"nzcp_live r1cs: {len(r1cs) / 1e6:.0f} MB in {time.time() - t0:.1f}s")
    t0 = time.time()
    ptau = amd.ptau_synth(a.power, 12345, 678, 91011, prepared=True, device=0)
    log(f"prepared ptau of power {a.power}: {len(ptau) / 1e6:.0f} MB in {time.time() - t0:.1f}s")

    amd.groth16_setup_ptau(r1cs, ptau, device=0)   # warm-up: the device context, the first allocations
    runs = {"setup": [], "zkey_new": []}
    keys = {}
    for i in range(a.repeats):
        for what, fn in (("setup", lambda: amd.groth16_setup_ptau(r1cs, ptau, device=0)),
                         ("zkey_new", lambda: amd.zkey_new(r1cs, ptau, device=0)[0])):
            key, text, wall = traced(fn)
            keys[what] = key
            line = [x for x in text.splitlines() if x.startswith("[g16] zkey cs hash")]
            run = {"wall_s": round(wall, 4)}
            if line:
                run["trace"] = line[0]
                m = re.search(r"image (\d+) bytes; kernels H ([\d.]+) ms, to-be ([\d.]+) ms, transfers ([\d.]+) ms; hash ([\d.]+) ms; call ([\d.]+) ms", line[0])
                run.update(image_bytes=int(m.group(1)), h_kernel_ms=float(m.group(2)), to_be_kernel_ms=float(m.group(3)),
                           transfers_ms=float(m.group(4)), hash_ms=float(m.group(5)), stage_ms=float(m.group(6)))
            runs[what].append(run)
            log(f"{what} {i}: {run}")
    assert len(keys["setup"]) == len(keys["zkey_new"])
    # section 10 (csHash | u32 0) is the last section of both keys
    assert keys["setup"][-68:-4] == bytes(64) and keys["setup"][:-68] == keys["zkey_new"][:-68], "the keys differ outside csHash"
    image = runs["zkey_new"][0]["image_bytes"]
    del keys
    buf = bytes(image)
    alone = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        amd.blake2b512(buf)
        alone.append(round((time.perf_counter() - t0) * 1e3, 3))
    log(f"blake2b512 alone over {image} bytes: {alone} ms")
    s = [r["wall_s"] for r in runs["setup"]]
    z = [r["wall_s"] for r in runs["zkey_new"]]
    print(json.dumps({"tool": "zkey_new_bench", "circuit": "nzcp_live", "power": a.power, "runs": runs,
                      "setup_wall_s_min_max": [min(s), max(s)], "zkey_new_wall_s_min_max": [min(z), max(z)],
                      "added_wall_s_min": round(min(z) - min(s), 4), "hash_alone_ms": alone,
                      "hash_alone_gb_per_s": round(image / (min(alone) * 1e-3) / 1e9, 3)}))


if __name__ == "__main__":
    main()
