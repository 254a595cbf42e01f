#!/usr/bin/env python3
"""Regenerates setup_digests.json: SHA-256 and length of every output buffer of the setup-side entry points of the C ABI
(synthetic circuit, SHA-256 / NZCP circuit builders, .r1cs trapdoor setup, the test ceremony writer, PLONK setup, Groth16
setup from a prepared .ptau, prepare phase2 and the three file-path forms).  The oracle pins keys byte for byte, but the
builders' .r1cs bytes and row order were only checked for satisfiability and the ceremony writer and the path forms only
structurally; every output here is made of affine points and field words, so it is deterministic.

    make_setup_digests.py                      the "cpu" table: host path (setup_device(-1)), any machine
    make_setup_digests.py --gpu [--out FILE]   the "gpu" table: one run on an MI355X, added to the existing file

The table in this directory was recorded before the host setup code was split into circuit, setup and ptau units, and must not
be regenerated to make a failing replay pass.  tests/test_cpu_setup_digests.py and tests/test_gpu_setup_digests.py import
this module for the case tables (CPU_CASES, GPU_CASES, GPU_SAME_AS_CPU) and for digests(), so that the recording and the
replay cannot drift apart.

A case is fn(amd, inp, dev) -> {output name: bytes | int | list}; inp = inputs(), dev = -1 (host threads) or a device
ordinal, which run() also hands to g16_setup_device for the duration of the call.  bytes are stored as {"sha256", "len"},
anything else as it is.  A case that raises G16Error is stored as {"error": [code, text]}.
{"cpu": {case: {output: ...}}, "gpu": {case: {output: ...}}}"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "setup_digests.json")
TD = (0x1234567 ** 5, 0xabcdef ** 7, 0x55aa ** 11)     # (tau, alpha, beta) of the test ceremonies, reduced in inputs()
SYNTH = (96, 5, 70, 11)                                  # (n, p, m, seed): domain 2^7; 216 PLONK gates, domain 2^8


def inputs():
    """-> the shared call arguments (all from the Python oracle or the committed example pass, deterministic)."""
    import formats as f
    import groth16 as g
    import synth
    from test_cpu_sha256_circuit import EXAMPLE_EXP_OFF, EXAMPLE_SEGS, example_to_be_signed
    tau, alpha, beta = [x % g.R for x in TD]
    return {
        "r1cs150": f.write_r1cs(150, 6, 0, synth.gen_circuit(150, 6, 120, 2)[1]),          # Groth16 domain 2^7
        # the 150-wire circuit makes 374 PLONK gates: too many for the power-8 ceremony of the .ptau cases (recorded as
        # that error); the 96-wire one fills the 2^8 domain with 216
        "r1cs96": f.write_r1cs(SYNTH[0], SYNTH[1], 0, synth.gen_circuit(*SYNTH)[1]),
        "tbs": example_to_be_signed(), "segs": EXAMPLE_SEGS, "exp_off": EXAMPLE_EXP_OFF,
        "tab": (tau, alpha, beta), "td": {"tau": tau, "alpha": alpha, "beta": beta, "gamma": 0x77 ** 9 % g.R, "delta": 0x3d ** 13 % g.R},
        "msg32": bytes(range(7, 39)),
    }


def _msg(n):
    return bytes((7 * i + n) & 0xFF for i in range(n))


def _sha_chain(blocks, all_four):
    def fn(amd, inp, dev):
        out = amd.sha256_chain_setup(blocks, inp["msg32"], 3, want_zkey=all_four, want_r1cs=True)
        return out if all_four else {"r1cs": out["r1cs"], "wtns": out["wtns"]}
    return fn


def _sha_message(n):
    def fn(amd, inp, dev):
        out = amd.sha256_message_setup(_msg(n), 1, want_zkey=False, want_r1cs=True)
        return {"r1cs": out["r1cs"], "wtns": out["wtns"]}
    return fn


def _fixed_layout(amd, inp, dev):
    out = amd.nzcp_fixed_layout_setup(inp["tbs"], inp["segs"], inp["exp_off"], 1, want_zkey=False, want_r1cs=True)
    return {"r1cs": out["r1cs"], "wtns": out["wtns"]}


def _nzcp_circuit(amd, inp, dev):
    out = amd.nzcp_circuit_setup(amd.NZCP_EXAMPLE_PARAMS, inp["tbs"], 1, want_zkey=False, want_r1cs=True)
    return {"r1cs": out["r1cs"], "wtns": out["wtns"], "n_constraints": out["n_constraints"]}


def gadget_vectors(inp):
    """-> [(name, params, inputs)]: every gadget name run_gadget knows, once, on a vector of test_cpu_nzcp_circuit.py."""
    from test_cpu_nzcp_circuit import enc_arr, enc_int, enc_map, enc_str, pad
    tbs = list(inp["tbs"])
    abcde = [ord(c) for c in "abcde"]
    pairs = [(enc_int(4), enc_int(5)), (enc_int(5), enc_int(4)), (enc_int(7), enc_int(3))]
    subj = []
    for s in ("Jack", "Sparrow", "1960-04-16"):
        subj += pad([ord(c) for c in s], 64) + [len(s)]
    return [
        ("getType", [], [0xA7]), ("getX", [], [0xA7]),
        ("quinSelector", [5], [1, 2, 3, 4, 5, 3]), ("getV", [5], [1, 2, 3, 4, 5, 2]),
        ("decodeUint23", [], [0xB7]), ("decodeUint", [4], [97, 218, 192, 48, 0, 26]),
        ("readType", [3], [0, 0xA7, 0, 1]),
        ("skipValueScalar", [5], pad(enc_str("abc"), 5) + [0]),
        ("skipValue", [5, 4], pad(enc_arr([enc_str("q"), enc_int(0xFF)]), 5) + [0]),
        ("stringEquals", [5, 5] + abcde, abcde + [0, 5]),
        ("readStringLength", [5], pad(enc_str("abc"), 5) + [0]),
        ("readMapLength", [7], pad(enc_map(pairs), 7) + [0]),
        ("copyString", [5, 4], pad(enc_str("ab"), 5) + [0]),
        ("findVCAndExp", [314, 0, 4], tbs + [28, 5]), ("findCredSubj", [314, 2, 4], tbs + [77, 4]),
        ("readCredSubj", [314, 32], tbs + [247, 3]), ("concatCredSubj", [64], subj),
        ("sha256Var", [1], [8 * 56] + list(_msg(56))),
    ]


def _gadgets(amd, inp, dev):
    out = {}
    for name, params, vec in gadget_vectors(inp):
        outputs, ncons = amd.nzcp_gadget(name, params, vec)
        out[name] = {"outputs": hashlib.sha256(json.dumps(outputs).encode()).hexdigest() if len(outputs) > 8 else outputs,
                     "n_constraints": ncons}
    return out


def _ptau_synth(power, prepared):
    return lambda amd, inp, dev: {"ptau": amd.ptau_synth(power, *inp["tab"], prepared=prepared, device=dev)}


CPU_CASES = {
    "synth_setup": lambda amd, inp, dev: dict(zip(("zkey", "wtns", "vkey"), amd.synth_setup(*SYNTH))),
    "synth_witness": lambda amd, inp, dev: {"wtns": amd.synth_witness(*SYNTH, SYNTH[3] + 5)},
    "sha256_chain_1": _sha_chain(1, True),
    "sha256_chain_2": _sha_chain(2, False),
    "sha256_message_0": _sha_message(0),
    "sha256_message_55": _sha_message(55),
    "sha256_message_56": _sha_message(56),
    "nzcp_fixed_layout": _fixed_layout,
    "nzcp_circuit": _nzcp_circuit,
    "nzcp_gadgets": _gadgets,
    "r1cs_setup": lambda amd, inp, dev: dict(zip(("zkey", "vkey"), amd.r1cs_setup(inp["r1cs150"], 21, 3))),
    "r1cs_setup_trapdoor": lambda amd, inp, dev: dict(zip(("zkey", "vkey"), amd.r1cs_setup_trapdoor(inp["r1cs150"], inp["td"], 3))),
    "ptau_synth_3": _ptau_synth(3, False),
    "ptau_synth_3_prepared": _ptau_synth(3, True),
}
# run on the device, these must give the CPU table's digests: they have no record of their own
GPU_SAME_AS_CPU = ("synth_setup", "r1cs_setup", "r1cs_setup_trapdoor", "ptau_synth_3", "ptau_synth_3_prepared")


def _ptau8(amd, inp, dev, prepared):
    return amd.ptau_synth(8, *inp["tab"], prepared=prepared, device=dev)


def _files(amd, entry, ins, tail):
    """The file-path form `entry` on the input images `ins` -> the bytes of the file it wrote."""
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k, data in enumerate(ins):
            paths.append(os.path.join(d, "in%d" % k).encode())
            with open(paths[-1], "wb") as fh:
                fh.write(data)
        out = os.path.join(d, "out").encode()
        lib = amd.load()
        rc = getattr(lib, entry)(*paths, out, *tail)
        if rc:
            raise amd.G16Error(rc, lib.g16_last_error().decode())
        with open(out, "rb") as fh:
            return fh.read()


def _ptau_prepare(power):
    return lambda amd, inp, dev: {"ptau": amd.ptau_prepare(amd.ptau_synth(power, *inp["tab"], prepared=False, device=dev), device=dev)}


GPU_CASES = {
    "plonk_setup": lambda amd, inp, dev: {"zkey": amd.plonk_setup(inp["r1cs150"], 9, device=dev, with_lagrange=True)},
    "plonk_setup_no_lagrange": lambda amd, inp, dev: {"zkey": amd.plonk_setup(inp["r1cs150"], 9, device=dev, with_lagrange=False)},
    "plonk_setup_ptau": lambda amd, inp, dev: {"zkey": amd.plonk_setup_ptau(inp["r1cs96"], _ptau8(amd, inp, dev, False), device=dev)},
    "plonk_setup_ptau_too_big": lambda amd, inp, dev: {"zkey": amd.plonk_setup_ptau(inp["r1cs150"], _ptau8(amd, inp, dev, False), device=dev)},
    "groth16_setup_ptau": lambda amd, inp, dev: {"zkey": amd.groth16_setup_ptau(inp["r1cs150"], _ptau8(amd, inp, dev, True), device=dev)},
    "groth16_setup_ptau_96": lambda amd, inp, dev: {"zkey": amd.groth16_setup_ptau(inp["r1cs96"], _ptau8(amd, inp, dev, True), device=dev)},
    "ptau_prepare_0": _ptau_prepare(0),
    "ptau_prepare_1": _ptau_prepare(1),
    "ptau_prepare_3": _ptau_prepare(3),
}
# the file-path forms: (case whose digests the written file must carry, entry point, inputs, trailing arguments)
GPU_FILES = {
    "plonk_setup_files": ("plonk_setup_ptau", "g16_plonk_setup_files",
                          lambda amd, inp, dev: [inp["r1cs96"], _ptau8(amd, inp, dev, False)], lambda dev: (dev, 1)),
    "groth16_setup_files": ("groth16_setup_ptau", "g16_groth16_setup_files",
                            lambda amd, inp, dev: [inp["r1cs150"], _ptau8(amd, inp, dev, True)], lambda dev: (dev,)),
    "ptau_prepare_files": ("ptau_prepare_3", "g16_ptau_prepare_files",
                           lambda amd, inp, dev: [amd.ptau_synth(3, *inp["tab"], prepared=False, device=dev)], lambda dev: (dev,)),
}


def run_files(amd, inp, name, dev):
    """-> (the buffer-form case it must equal, digests of the written file)."""
    same_as, entry, ins, tail = GPU_FILES[name]
    out_name = next(iter(GPU_CASES[same_as](amd, inp, dev)))
    return same_as, digests({out_name: _files(amd, entry, ins(amd, inp, dev), tail(dev))})


def digests(outputs):
    def one(v):
        if isinstance(v, (bytes, bytearray)):
            return {"sha256": hashlib.sha256(v).hexdigest(), "len": len(v)}
        if isinstance(v, dict):
            return {k: one(x) for k, x in v.items()}
        return v
    return {k: one(v) for k, v in outputs.items() if v is not None}


def run(amd, cases, name, inp, dev):
    """-> the digests of case `name` with the fixed-base multiplications on `dev`."""
    amd.setup_device(dev)
    try:
        return digests(cases[name](amd, inp, dev))
    except amd.G16Error as e:
        return {"error": [e.code, str(e)]}
    finally:
        amd.setup_device(-1)


def main():
    import __graft_entry__ as entry
    amd = entry.load_package()
    amd.load()
    gpu = "--gpu" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    table = json.load(open(OUT)) if os.path.exists(OUT) else {}
    inp = inputs()
    cases, dev, key = (GPU_CASES, 0, "gpu") if gpu else (CPU_CASES, -1, "cpu")
    table[key] = {name: run(amd, cases, name, inp, dev) for name in cases}
    if gpu:
        for name in GPU_SAME_AS_CPU:
            assert run(amd, CPU_CASES, name, inp, 0) == table["cpu"][name], name
        for name in GPU_FILES:
            same_as, got = run_files(amd, inp, name, 0)
            assert got == table["gpu"][same_as], name
    with open(out, "w") as fh:
        fh.write("{\n")
        for i, part in enumerate(sorted(table)):
            rows = ",\n  ".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in table[part].items())
            fh.write(' %s: {\n  %s\n }%s\n' % (json.dumps(part), rows, "," if i + 1 < len(table) else ""))
        fh.write("}\n")
    json.load(open(out))
    print("%s: %d cases -> %s (%d bytes)" % (key, len(table[key]), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
