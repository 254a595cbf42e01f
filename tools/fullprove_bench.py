#!/usr/bin/env python3
"""Timing of the batched fullprove on one MI355X (the record is profiles/fullprove_bench.json): many passes in, proofs
out, by three routes in one process --

  a) g16_fullprove_batch: witnesses computed in device chunks and proved from the chunk buffers;
  b) the only device route there was: g16_wtns_calc with the bodies copied to the host, then g16_prove_batch from them,
     cut by hand into pieces of --piece passes so that the host can hold the witnesses;
  c) g16_prove_batch from witnesses that already lie on the host (--distinct of them, cycled): the ceiling.

Groth16 at the live parameters over --batch distinct passes (tools/nzcp_pass.py), ONE of which violates a check (its
toBeSignedLen exceeds the maximum), so that a mishandled verdict cannot hide; PLONK at the example parameters over
--plonk-batch passes.  Before anything is timed the tool asserts that proof 0 of route a) equals stage + prove_staged with
the same (r, s) and that every other proof passes the device verifier; a mismatch ends it non-zero.  Times are medians of
--reps calls after a warm-up call, min and max beside them.

    python tools/fullprove_bench.py [--batch 256] [--plonk-batch 8] [--reps 5] [--piece 32] [--distinct 32] [--out file.json]
"""
import argparse
import ctypes as C
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
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2), "n": len(xs)}


def timed(fn, reps):
    fn()                                            # warm-up: buffers grow here
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def report(ms, count):
    s = stats(ms)
    s["proofs_per_s"] = round(count / (s["median"] / 1e3), 1)
    return s


class Routes:
    """The three routes over one circuit: `prove(inputs, blind)` fills self.out / self.pub / self.st."""

    def __init__(self, amd, plonk, prover, dev, header, inputs, blind, piece, distinct):
        self.amd, self.lib, self.plonk, self.prover, self.dev = amd, amd.load(), plonk, prover, dev
        self.header, self.inputs, self.blind, self.piece = header, inputs, blind, piece
        self.n = len(inputs)
        self.per = 288 if plonk else 64
        self.n_public = prover.n_public if plonk else prover.info.n_public
        self.out = ((amd.PlonkProof if plonk else amd.Proof) * self.n)()
        self.pub = C.create_string_buffer(max(1, self.n * self.n_public * 32))
        self.st = (C.c_uint32 * self.n)()
        self.blob = b"".join(inputs)
        self.good = None            # indices of the passes whose witness violates nothing (known after route a)
        self.host_wtns = None
        self.images = None
        self.distinct = distinct

    def a(self):
        fn = self.lib.g16_plonk_fullprove_batch if self.plonk else self.lib.g16_fullprove_batch
        rc = fn(self.prover._h, self.dev._h, self.blob, len(self.inputs[0]) // 32, self.n, self.blind, self.out, self.pub, self.st)
        assert rc == 0, self.lib.g16_last_error()

    def _prove_host(self, images, blind, out, pub, size):
        if self.plonk:
            for i, w in enumerate(images):
                rc = self.lib.g16_plonk_prove(self.prover._h, w, size, blind[i * 288:(i + 1) * 288], C.byref(out[i]), None)
                assert rc == 0, self.lib.g16_last_error()
            return
        k = len(images)
        arr = (C.c_char_p * k)(*images)
        lens = (C.c_size_t * k)(*[size] * k)
        rc = self.lib.g16_prove_batch(self.prover._h, arr, lens, k, blind, out, pub)
        assert rc == 0, self.lib.g16_last_error()

    def b(self):
        """g16_wtns_calc with the bodies copied to the host, then the prover fed from them, piece by piece, at the C ABI:
        one copy of each body behind its .wtns header, nothing else (the violating pass is left out by hand)"""
        w, hl, n_in = self.dev.n_wires * 32, len(self.header), len(self.inputs[0]) // 32
        if self.images is None:
            self.bodies = C.create_string_buffer(self.piece * w)
            self.images = [C.create_string_buffer(self.header, hl + w) for _ in range(self.piece)]
        st = (C.c_uint32 * self.piece)()
        for at in range(0, self.n, self.piece):
            idx = list(range(at, min(self.n, at + self.piece)))
            rc = self.lib.g16_wtns_calc(self.dev._h, b"".join(self.inputs[i] for i in idx), n_in, len(idx), self.bodies, st)
            assert rc == 0, self.lib.g16_last_error()
            keep = [j for j in range(len(idx)) if st[j] == self.amd.NO_CHECK]
            for k, j in enumerate(keep):
                C.memmove(C.addressof(self.images[k]) + hl, C.addressof(self.bodies) + j * w, w)
            images = [C.cast(self.images[k], C.c_char_p) for k in range(len(keep))]
            blind = b"".join(self.blind[idx[j] * self.per:(idx[j] + 1) * self.per] for j in keep)
            out = (type(self.out[0]) * len(keep))()
            pub = C.create_string_buffer(max(1, len(keep) * self.n_public * 32))
            self._prove_host(images, blind, out, pub, hl + w)
            self.last_b = ([idx[j] for j in keep], out)

    def prepare_c(self):
        good = [i for i in range(self.n) if self.st[i] == self.amd.NO_CHECK][:self.distinct]
        bodies = self.dev.calculate_batch([self.inputs[i] for i in good], want_words=True)
        self.host_wtns = [self.header + body for body, _ in bodies]

    def c(self):
        k = sum(1 for i in range(self.n) if self.st[i] == self.amd.NO_CHECK)
        images = [self.host_wtns[i % len(self.host_wtns)] for i in range(k)]
        out = (type(self.out[0]) * k)()
        pub = C.create_string_buffer(max(1, k * self.n_public * 32))
        self._prove_host(images, self.blind[:k * self.per], out, pub, len(self.host_wtns[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--plonk-batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--piece", type=int, default=32)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--skip-plonk", action="store_true")
    ap.add_argument("--params", default="live", help="the Groth16 circuit: live or example")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    amd = entry.load_package()
    res = {"what": "tools/fullprove_bench.py on one MI355X; wall ms per call (median, min, max of n calls after a warm-up call)",
           "routes": {"a": "fullprove_batch", "b": f"wtns calc with bodies to the host + prove from them, pieces of {a.piece}",
                      "c": f"prove from witnesses on the host ({a.distinct} distinct, cycled): the ceiling"}}

    def tbs_of(i, live):   # (the example circuit takes 314 bytes: shorter names there)
        given, family = (f"Given{i}", f"Family{i % 97}") if live else (f"G{i}", f"F{i % 97}")
        return nzcp_pass.to_be_signed(given, family, f"19{60 + i % 40}-0{1 + i % 9}-1{i % 10}", live=live, exp=1700000000 + i)

    def circuit(params_name, count):
        live = params_name == "live"
        params = amd.NZCP_LIVE_PARAMS if live else amd.NZCP_EXAMPLE_PARAMS
        built = amd.nzcp_circuit_setup(params, tbs_of(0, live), 77, want_zkey=True, want_r1cs=True)
        prog = amd.nzcp_witness_program(params)
        dev = amd.WitnessCalculator(prog, device=0)
        inputs = [amd.nzcp_inputs(tbs_of(i, live), params[1]) for i in range(count)]
        if count > 2:   # one pass violates a check: a toBeSignedLen beyond the maximum
            bad = count // 2
            inputs[bad] = inputs[bad][:-32] + (8 * params[1] + 8).to_bytes(32, "little")
        header = built["wtns"][:len(built["wtns"]) - dev.n_wires * 32]
        return built, dev, inputs, header

    # ------------------------------------------------------------------ Groth16
    built, dev, inputs, header = circuit(a.params, a.batch)
    prover = amd.Prover(built["zkey"])
    n = a.batch
    blind = b"".join((1000 + 2 * i).to_bytes(32, "little") + (1001 + 2 * i).to_bytes(32, "little") for i in range(n))
    g = Routes(amd, False, prover, dev, header, inputs, blind, a.piece, a.distinct)
    g.a()
    bad = [i for i in range(n) if g.st[i] != amd.NO_CHECK]
    assert len(bad) == (1 if n > 2 else 0), f"violating passes: {bad}"
    assert all(bytes(g.out[i]) == bytes(256) for i in bad), "a violated pass has a proof"
    prover.stage(0, built["wtns"])
    ref, _ = prover.prove_staged(0, blind[:32], blind[32:64])
    assert amd.proof_to_obj(g.out[0]) == ref, "fullprove_batch proof 0 differs from stage + prove_staged"
    ver = amd.Verifier(built["vkey"], prover.info.n_public)
    good = [i for i in range(n) if i not in bad]
    p = prover.info.n_public * 32
    ok = ver.verify_raw(b"".join(bytes(g.out[i]) for i in good), b"".join(g.pub.raw[i * p:(i + 1) * p] for i in good), len(good))
    assert all(ok), f"proofs rejected by the device verifier: {[good[i] for i, x in enumerate(ok) if not x]}"
    ver.close()
    res["groth16"] = {"circuit": "nzcp_" + a.params, "passes": n, "violating": bad, "proofs": len(good), "n_wires": dev.n_wires,
                      "checked": "proof 0 == stage + prove_staged; every proof accepted by the device verifier"}
    res["groth16"]["a_fullprove_batch"] = report(timed(g.a, a.reps), len(good))
    res["groth16"]["b_calc_to_host_then_prove"] = report(timed(g.b, a.reps), len(good))
    keep, out = g.last_b
    assert all(bytes(out[k]) == bytes(g.out[i]) for k, i in enumerate(keep)), "route b differs from route a"
    g.prepare_c()
    res["groth16"]["c_prove_from_host"] = report(timed(g.c, a.reps), len(good))
    # the calculator's chunk kernel and the proofs side by side: one chunk of the batch, statuses only
    dev.calculate_batch(inputs, want_words=False)
    res["groth16"]["calc_kernel_ms_all_passes"] = round(dev.timings()["kernel_ms"], 2)
    prover.close(), dev.close()
    del g, built, inputs

    # ------------------------------------------------------------------ PLONK
    if not a.skip_plonk:
        built, dev, inputs, header = circuit("example", a.plonk_batch)
        t = time.perf_counter()
        zkey = amd.plonk_setup(built["r1cs"], 7, device=0, with_lagrange=False)
        setup_s = round(time.perf_counter() - t, 2)
        pp = amd.PlonkProver(zkey)
        del zkey
        n = a.plonk_batch
        blind = b"".join((5000 + 9 * i + k).to_bytes(32, "little") for i in range(n) for k in range(9))
        q = Routes(amd, True, pp, dev, header, inputs, blind, a.piece, a.distinct)
        q.a()
        bad = [i for i in range(n) if q.st[i] != amd.NO_CHECK]
        good = [i for i in range(n) if i not in bad]
        ref, _ = pp.prove_raw(built["wtns"], blind[:288])
        assert bytes(q.out[0]) == bytes(ref), "plonk fullprove_batch proof 0 differs from plonk prove"
        res["plonk"] = {"circuit": "nzcp_example", "passes": n, "violating": bad, "proofs": len(good), "setup_s": setup_s,
                        "checked": "proof 0 == plonk prove with the same blinding"}
        res["plonk"]["a_fullprove_batch"] = report(timed(q.a, a.reps), len(good))
        res["plonk"]["b_calc_to_host_then_prove"] = report(timed(q.b, a.reps), len(good))
        q.prepare_c()
        res["plonk"]["c_prove_from_host"] = report(timed(q.c, a.reps), len(good))
        pp.close(), dev.close()
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
