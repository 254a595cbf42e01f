#!/usr/bin/env python3
"""Regenerates ptau_challenge.json: Blake2b-512 digests of what the Python twin of the challenge / response exchange
(tests/ptau_challenge_ref.py) produces at power 2 for fixed secrets -- the challenge file of the generator file, the
response to it, the file the import writes, and the same three one round later.  The twin is what the device code is
compared with, byte for byte; this table pins the twin itself against drift, so it must not be regenerated to make a
failing replay pass.  tests/test_cpu_ptau_challenge.py imports run() for the replay.  Pure Python: needs no library."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "ptau_challenge.json")
POWER = 2
SECRETS = ((11, 22, 33, 44, 55, 66), (0x1234567 ** 5, 0xabcdef ** 7, 0x55aa ** 11, 0x77 ** 9, 0x3d ** 13, 0x101 ** 17))
NAMES = ("first", None)


def run():
    """-> {name: {"blake2b": hex, "len": n}} of the six files, and the two contribution hashes."""
    from bn254 import R
    from ptau_challenge_ref import challenge_contribute_ref, export_challenge_ref, import_response_ref
    from ptau_prepared import write_ptau_prepared
    ptau, out = write_ptau_prepared(POWER, 1, 1, 1, prepared=False), {}
    for k, (secret, name) in enumerate(zip(SECRETS, NAMES)):
        secret = tuple(x % R for x in secret)
        challenge = export_challenge_ref(ptau)
        response, h = challenge_contribute_ref(challenge, secret)
        ptau, h2 = import_response_ref(ptau, response, name)
        assert h == h2
        for what, data in (("challenge", challenge), ("response", response), ("ptau", ptau)):
            out["%s_%d" % (what, k)] = {"blake2b": hashlib.blake2b(data, digest_size=64).hexdigest(), "len": len(data)}
        out["contribution_hash_%d" % k] = h.hex()
    return out


if __name__ == "__main__":
    with open(OUT, "w") as fh:
        json.dump(run(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")
