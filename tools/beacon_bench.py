#!/usr/bin/env python3
"""`powersoftau beacon` / `zkey beacon` bench (csrc/beacon.h, csrc/ptau_mpc.cpp, csrc/zkey_mpc.cpp).  Three figures, all in
one process on one device:
  * the host rate of the delay function: g16_beacon_scalars at e = `--chain-exp` (2^e dependent SHA-256 applications on
    one thread), in hashes per second, and the time of the chain at the e the two beacon calls below use;
  * `powersoftau beacon` at power `--power`, e = `--exp`, beside `powersoftau contribute` with the same six scalars on
    the same generator file, alternating, `--repeats` runs each after one warm-up contribution;
  * `zkey beacon` beside `zkey contribute` likewise, on a 2^20-domain key of the nzcp_live shape (g16_synth_setup:
    850 000 wires and rows, 513 public signals).
The kernels of a beacon call are its contribute's: a beacon may exceed its contribute by the chain's own time and the
run-to-run spread, no more.  Each pair is checked to give the same contribution hash (that the files differ in the new
record's type and params alone is tests/test_gpu_beacon.py's subject).

    python tools/beacon_bench.py [--power 20] [--n 850000] [--exp 10] [--chain-exp 20] [--repeats 3]
Prints one JSON line.  A tool, not a test; not part of bench.py."""
import argparse
import json
import os
import re
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

BEACON = bytes((37 * i + 11) & 0xff for i in range(32))


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


def box():
    """the machine and its first GPU agent, as rocminfo names it"""
    gpu = "unknown"
    try:
        text = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = [x.split(":", 1)[1].strip() for x in text.splitlines() if "Marketing Name" in x]
        archs = re.findall(r"Name:\s+(gfx\w+)", text)
        gpu = " / ".join([n for n in names if "Instinct" in n or "MI3" in n][:1] + archs[:1]) or gpu
    except (OSError, subprocess.SubprocessError):
        pass
    return {"host": socket.gethostname(), "gpu": gpu}


def pair(log, what, contribute, beacon, repeats):
    """contribute() and beacon() alternating -> per call the wall seconds and the library's trace line"""
    contribute()   # warm-up: the device context, the first allocation
    runs = {"contribute": [], "beacon": []}
    hashes = {}
    for i in range(repeats):
        for key, fn in (("contribute", contribute), ("beacon", beacon)):
            (new, h), text, wall = traced(fn)
            hashes[key] = h
            del new
            line = [x for x in text.splitlines() if x.startswith("[g16] " + what)]
            runs[key].append({"wall_s": round(wall, 4), "trace": line[0] if line else text.strip()})
            log(f"{what} {key} {i}: {runs[key][-1]}")
    assert hashes["contribute"] == hashes["beacon"], "the contribution hashes differ"
    for key in ("contribute", "beacon"):
        runs[key + "_wall_s_min"] = min(r["wall_s"] for r in runs[key])
    runs["beacon_minus_contribute_s"] = round(runs["beacon_wall_s_min"] - runs["contribute_wall_s_min"], 4)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--power", type=int, default=20)
    ap.add_argument("--n", type=int, default=850_000)
    ap.add_argument("--exp", type=int, default=10)
    ap.add_argument("--chain-exp", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    amd = entry.load_package()
    amd.load()
    entry.oracle_path()
    import synth

    def log(m):
        print(f"[beacon bench] {m}", file=sys.stderr, flush=True)
    out = {"tool": "beacon_bench", "box": box(), "beacon_bytes": len(BEACON), "exp": a.exp}

    # 1. the chain on the host
    chain = []
    for e in (a.exp, a.chain_exp):
        best = None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            six = amd.beacon_scalars(BEACON, e, 6)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        chain.append({"exp": e, "hashes": 1 << e, "seconds_min": round(best, 6), "hashes_per_s": round((1 << e) / best)})
        log(f"chain: {chain[-1]}")
        if e == a.exp:
            secret = six
    out["chain"] = chain

    # 2. powersoftau beacon beside powersoftau contribute
    src = amd.ptau_new(a.power)
    log(f"generator file of power {a.power}: {len(src) / 1e6:.0f} MB")
    out["ptau"] = {"power": a.power, **pair(log, "ptau", lambda: amd.ptau_contribute(src, "bench", secret, device=0),
                                            lambda: amd.ptau_beacon(src, BEACON, a.exp, "bench", device=0), a.repeats)}
    del src

    # 3. zkey beacon beside zkey contribute
    t0 = time.time()
    amd.setup_device(0)
    try:
        zkey, _, _ = amd.synth_setup(a.n, 513, a.n, synth.SEED_NZCP, 0)
    finally:
        amd.setup_device(-1)
    log(f"synthetic key nVars = nConstraints = {a.n}: {len(zkey) / 1e6:.0f} MB in {time.time() - t0:.1f}s")
    out["zkey"] = {"n": a.n, **pair(log, "zkey", lambda: amd.zkey_contribute(zkey, "bench", secret[0], secret[1], device=0),
                                    lambda: amd.zkey_beacon(zkey, BEACON, a.exp, "bench", device=0), a.repeats)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
