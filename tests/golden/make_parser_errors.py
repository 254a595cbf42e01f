#!/usr/bin/env python3
"""Regenerates parser_errors.json: what every entry point of the C ABI that parses a snarkjs container before it
touches a device answers -- (return code, g16_last_error text) -- for deterministic mutants of small valid files.

Run it on a machine WITHOUT a GPU, against the library whose answers are to be pinned (the table in this directory was
recorded before the five hand-written section-table walkers became csrc/binfile.h, and must not be regenerated to make
a failing replay pass).  tests/test_cpu_parser_errors.py imports this module for the base files, the entry points and
the mutation replay, and asserts the recorded code and text for every case.

Per entry point: mutants are drawn with a fixed seed from the four mutation kinds of
test_cpu_host.py::test_parsers_survive_mutated_keys (0: one to three bytes of the first 600; 1: a truncation; 2: a
32-bit field overwritten; 3: a 64-bit field among the first section records overwritten).  A mutant whose result is
G16_E_FORMAT or G16_E_ARG is recorded -- both come before the device check, so they are the same with or without a
GPU -- and one that passes the parser (0 or G16_E_NOGPU) is dropped, until FUZZ_CASES are held.  Hand-written cases
follow: cuts inside the file header and inside a section record, absurd and off-by-one section sizes, a duplicated
id, an id of 16 or more, version max + 1, and for the .ptau routes missing sections and a bad power next to them.
A hand-written case that passes an entry point's parser is dropped like a mutant: the Groth16 .ptau route reads no
section 2 or 3, so its table holds no plain "section 2 missing" / "section 3 missing"; sections 4 and 12 stand in.

A mutation is stored as its edits, not as a file image: an int is a cut length, a list is [offset, hex, offset, hex,
...] of same-length overwrites applied in order.
{"texts": [...], "entries": {name: {"seed": s, "fuzz": [[kind, mutation, rc, text index]], "hand": [[label, ...]]}}}"""
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "parser_errors.json")
FUZZ_CASES = 200
MAX_DRAWS = 2000
E_ARG, E_FORMAT = -1, -2
MUST_APPEAR = ("Version not supported", "zkey: Missing section", "r1cs: truncated section table", "r1cs: truncated section",
               "ptau: Invalid File format (bn128 powers of tau expected)", "Powers of tau is not prepared.")
TD = (0x1234567 ** 5, 0xabcdef ** 7, 0x55aa ** 11)     # (tau, alpha, beta) of the prepared file, reduced below


def bases():
    """-> {name: bytes}: the valid files the mutants are made from (all from the Python oracle, deterministic)."""
    import formats as f
    import groth16 as g
    import plonk as pk
    import synth
    from ptau_prepared import write_ptau_prepared
    rows, _w = synth.make(24, 2, 12, 1)
    return {
        "tiny.zkey": open(os.path.join(HERE, "tiny.zkey"), "rb").read(),
        "plonk.zkey": pk.write_zkey(pk.setup(24, 2, rows, tau=5)),
        "r1cs": f.write_r1cs(24, 2, 0, synth.gen_circuit(24, 2, 12, 1)[1]),
        # m + p + 1 = 6: fits the power-3 ceremony, so a mutant that passes both parsers goes on to the device check
        "r1cs_pow3": f.write_r1cs(8, 1, 0, synth.gen_circuit(8, 1, 4, 1)[1]),
        "ptau6": pk.write_ptau(6, 777),
        "ptau3_prepared": write_ptau_prepared(3, *[x % g.R for x in TD]),
    }


# name -> (base file, magic, max version, seed, call(amd, bases, mutant))
ONE = (1).to_bytes(32, "little")
ENTRIES = {
    "Prover": ("tiny.zkey", "zkey", 2, 101, lambda amd, b, m: amd.Prover(m).close()),
    "g16_finish_host": ("tiny.zkey", "zkey", 2, 102, lambda amd, b, m: amd.finish_host(m, [bytes(amd.PARTIAL_BYTES)], ONE, ONE)),
    "PlonkProver": ("plonk.zkey", "zkey", 2, 103, lambda amd, b, m: amd.PlonkProver(m).close()),
    "r1cs_setup": ("r1cs", "r1cs", 1, 104, lambda amd, b, m: amd.r1cs_setup(m, 1, 2)),
    "plonk_setup_ptau": ("ptau6", "ptau", 1, 105, lambda amd, b, m: amd.plonk_setup_ptau(b["r1cs"], m, device=0)),
    "groth16_setup_ptau": ("ptau3_prepared", "ptau", 1, 106, lambda amd, b, m: amd.groth16_setup_ptau(b["r1cs_pow3"], m, device=0)),
    "ptau_prepare": ("ptau3_prepared", "ptau", 1, 107, lambda amd, b, m: amd.ptau_prepare(m, device=0)),
}


def apply(buf, mut):
    """The mutant of `buf` that `mut` describes."""
    if isinstance(mut, int):
        return buf[:mut]
    b = bytearray(buf)
    for off, hx in zip(mut[0::2], mut[1::2]):
        data = bytes.fromhex(hx)
        b[off:off + len(data)] = data
    return bytes(b)


def run(amd, name, files, mutant):
    """-> (return code, error text) of entry point `name` on `mutant`; (0, "") when it succeeds."""
    try:
        ENTRIES[name][4](amd, files, mutant)
    except amd.G16Error as e:
        return e.code, str(e)
    return 0, ""


def draw(rng, buf):
    """One mutation of the four kinds -> (kind, mutation)."""
    k = rng.randrange(4)
    if k == 0:
        mut = []
        for _j in range(rng.randrange(1, 4)):
            mut += [rng.randrange(min(len(buf), 600)), "%02x" % rng.randrange(256)]
        return k, mut
    if k == 1:
        return k, rng.randrange(len(buf))
    if k == 2:
        i = rng.randrange(len(buf) - 4)
        return k, [i, struct.pack("<I", rng.choice([0, 1, 0xffffffff, 0x7fffffff, rng.randrange(1 << 32)])).hex()]
    i = 12 + rng.randrange(200)
    return k, [i, struct.pack("<Q", rng.choice([0, 1, len(buf), 1 << 40, (1 << 64) - 1])).hex()]


def hand_cases(buf, magic, max_version):
    """-> [(label, mutation)] built from the file's own section table (records in file order)."""
    import formats as f
    secs = f.read_binfile(buf, magic, max_version)
    recs = sorted((pos - 12, sid, size) for sid, lst in secs.items() for pos, size in lst)   # (record offset, id, size)
    u32 = lambda v: struct.pack("<I", v).hex()      # noqa: E731
    u64 = lambda v: struct.pack("<Q", v).hex()      # noqa: E731
    at = {sid: off for off, sid, _ in recs}
    (r0, _, _), (r1, _, _), (rl, _, sl) = recs[0], recs[1], recs[-1]
    out = [("cut inside the file header", 7), ("cut at the end of the file header", 12),
           ("cut inside the first section record", r0 + 5), ("cut inside the second section record", r1 + 7),
           ("cut inside the last section record", rl + 11), ("cut one byte short", len(buf) - 1),
           ("first section size 2^64 - 1", [r0 + 4, u64((1 << 64) - 1)]),
           ("last section size 2^64 - 1", [rl + 4, u64((1 << 64) - 1)]),
           ("first section size one byte past the end", [r0 + 4, u64(len(buf) - (r0 + 12) + 1)]),
           ("last section size one byte past the end", [rl + 4, u64(sl + 1)]),
           ("section count one more than the records", [8, u32(len(recs) + 1)]),
           ("section 1 renamed to id 17", [at[1], u32(17)]),
           ("version max + 1", [4, u32(max_version + 1)]),
           ("version max + 1 and a wrong magic", [0, b"xxxx".hex(), 4, u32(max_version + 1)])]
    for sid in (2, 4):   # (the Groth16 route reads no section 2 or 3 of a .ptau: its cases are those of section 4)
        if sid in at:
            out += [("duplicated id: section %d renamed to 1, the first copy must win" % sid, [at[sid], u32(1)]),
                    ("section %d renamed to id %d" % (sid, sid + 16), [at[sid], u32(sid + 16)])]
    if magic == "ptau":
        power_at = at[1] + 12 + 36
        for sid in (1, 2, 3):
            out.append(("section %d missing" % sid, [at[sid], u32(11)]))
        out += [("power 29", [power_at, u32(29)]),
                ("section 2 missing and power 29", [at[2], u32(11), power_at, u32(29)]),
                ("section 3 missing and power 29", [at[3], u32(11), power_at, u32(29)]),
                ("section 2 missing and another prime", [at[2], u32(11), at[1] + 12 + 4, "00"]),
                ("section 3 one byte", [at[3] + 4, u64(1)])]
        if 12 in at:
            out += [("section 12 missing", [at[12], u32(11)]),
                    ("section 12 missing and section 4 missing", [at[12], u32(11), at[4], u32(11)])]
    return out


def main():
    import __graft_entry__ as entry
    amd = entry.load_package()
    amd.load()
    files = bases()
    texts, entries = [], {}

    def idx(t):
        if t not in texts:
            texts.append(t)
        return texts.index(t)
    for name, (base, magic, max_version, seed, _call) in ENTRIES.items():
        buf = files[base]
        assert run(amd, name, files, buf)[0] in (0, -4), (name, run(amd, name, files, buf))
        rng = random.Random(seed)
        fuzz, draws = [], 0
        while len(fuzz) < FUZZ_CASES:
            draws += 1
            assert draws <= MAX_DRAWS, "%s: %d cases after %d draws" % (name, len(fuzz), MAX_DRAWS)
            kind, mut = draw(rng, buf)
            rc, text = run(amd, name, files, apply(buf, mut))
            if rc in (E_ARG, E_FORMAT):
                fuzz.append([kind, mut, rc, idx(text)])
        hand = []
        for label, mut in hand_cases(buf, magic, max_version):
            rc, text = run(amd, name, files, apply(buf, mut))
            if rc in (E_ARG, E_FORMAT):     # (a route that does not read the section a case removes passes it: dropped)
                hand.append([label, mut, rc, idx(text)])
        entries[name] = {"seed": seed, "fuzz": fuzz, "hand": hand}
        print("%-20s %4d draws, %d + %d cases" % (name, draws, len(fuzz), len(hand)))
    for want in MUST_APPEAR:
        assert any(t == want or (want.endswith("Missing section") and t.startswith(want + " ")) for t in texts), want
    with open(OUT, "w") as fh:
        fh.write('{"texts": %s,\n "entries": {\n' % json.dumps(texts))
        for k, (name, e) in enumerate(entries.items()):
            fh.write('  %s: {"seed": %d,\n' % (json.dumps(name), e["seed"]))
            for key in ("fuzz", "hand"):
                rows = ",\n    ".join(json.dumps(c, separators=(",", ":")) for c in e[key])
                fh.write('   "%s": [\n    %s]%s\n' % (key, rows, "," if key == "fuzz" else ""))
            fh.write("  }%s\n" % ("," if k + 1 < len(entries) else ""))
        fh.write(" }}\n")
    json.load(open(OUT))
    print("texts:", len(texts), "bytes:", os.path.getsize(OUT))


if __name__ == "__main__":
    main()
