"""Pass verification from Node.js (nzcp.verifyPass, nzcp.verifyPassProof) and the CLI's `nzcp verify` commands.  The
pass signatures take the host route (device -1), so all but the proof command run without a GPU."""
import json
import os
import shutil
import subprocess

import pytest

import es256_cases as cases
from conftest import ROOT, golden_path

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
KEYS = golden_path("nzcp_example_issuer.json")
URI = open(golden_path("example_pass_uri.txt")).read().strip()
pytestmark = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


def test_verify_pass_verdicts():
    """the example pass: valid with its claims; past its exp; under an unknown kid; one base32 character changed, in the
    header region (no longer a pass) and in the signature (a pass whose signature fails) -- never an exception"""
    damaged_head = URI[:40] + ("B" if URI[40] == "A" else "A") + URI[41:]
    damaged_sig = URI[:-20] + ("B" if URI[-20] == "A" else "A") + URI[-19:]
    script = f"""
    const {{ nzcp }} = require({json.dumps(JS)});
    const keys = require({json.dumps(KEYS)}).keys;
    const uri = {json.dumps(URI)};
    (async () => {{
      const out = {{}};
      out.ok = await nzcp.verifyPass(uri, {{ keys, now: 1700000000 }});
      out.expired = await nzcp.verifyPass(uri, {{ keys, now: 1951416330 }});
      out.early = await nzcp.verifyPass(uri, {{ keys, now: 1635883529 }});
      out.kid = await nzcp.verifyPass(uri, {{ keys: {{ "did:web:nzcp.covid19.health.nz#key-2": Object.values(keys)[0] }}, now: 1700000000 }});
      out.many = await nzcp.verifyPass([{json.dumps(damaged_head)}, uri, {json.dumps(damaged_sig)}, "NZCP:/2/AAAA"], {{ keys, now: 1700000000 }});
      out.reasons = nzcp.PASS_REASONS;
      console.log(JSON.stringify(out));
    }})();
    """
    r = subprocess.run(["node", "-e", script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    why = out["reasons"]
    assert out["ok"] == {"ok": True, "reason": None,
                         "claims": {"exp": 1951416330, "nbf": 1635883530, "iss": "did:web:nzcp.covid19.health.nz",
                                    "givenName": "Jack", "familyName": "Sparrow", "dob": "1960-04-16"}}
    assert out["expired"] == {"ok": False, "reason": why["expired"]}
    assert out["early"] == {"ok": False, "reason": why["notYet"]}
    assert out["kid"] == {"ok": False, "reason": why["key"]}
    assert [x["ok"] for x in out["many"]] == [False, True, False, False]
    assert out["many"][0]["reason"] == why["malformed"] and out["many"][3]["reason"] == why["malformed"]
    assert out["many"][2]["reason"] == why["signature"]


def _cli(*args):
    return subprocess.run(["node", CLI, *args], capture_output=True, text=True, timeout=120)


def test_cli_nzcp_verify(tmp_path):
    r = _cli("nzcp", "verify", URI, "--keys", KEYS, "--now", "1700000000")
    assert r.returncode == 0 and r.stdout.strip() == "pass 0: OK Jack Sparrow 1960-04-16", r.stdout + r.stderr
    listing = tmp_path / "passes.txt"
    listing.write_text(URI + "\n\nNZCP:/1/AAAA\n")
    r = _cli("nzcp", "verify", str(listing), "--keys", KEYS, "--now", "1700000000")
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["pass 0: OK Jack Sparrow 1960-04-16", "pass 1: INVALID the pass URI is malformed"]
    r = _cli("nzcp", "verify", URI, "--keys", KEYS, "--now", "2000000000")
    assert r.returncode == 1 and "INVALID the pass has expired (exp)" in r.stdout
    assert _cli("nzcp", "verify", URI).returncode == 2


@pytest.mark.gpu
def test_cli_nzcp_verify_proof(amd, tmp_path):
    vkey, pubs, proofs = cases.pass_circuit(amd)
    (tmp_path / "vk.json").write_text(json.dumps(amd.vkey_json(vkey, cases.N_PUB)))
    for name in ("a", "c"):
        (tmp_path / f"public_{name}.json").write_text(json.dumps([str(x) for x in pubs[name]]))
        (tmp_path / f"proof_{name}.json").write_text(json.dumps(proofs[name]))

    def run(name, now):
        return _cli("nzcp", "verify", "proof", str(tmp_path / "vk.json"), str(tmp_path / f"public_{name}.json"),
                    str(tmp_path / f"proof_{name}.json"), URI, "--keys", KEYS, "--now", str(now), "--device", "0")
    r = run("a", cases.NOW)
    assert r.returncode == 0 and "[INFO]  snarkJS: OK!" in r.stdout, r.stdout + r.stderr
    r = run("a", cases.EXP + 1)
    assert r.returncode == 1 and "[ERROR] snarkJS: the pass has expired (exp)" in r.stderr
    r = run("c", cases.NOW)
    assert r.returncode == 1 and "[ERROR] snarkJS: public signals 0..511 are not all bits" in r.stderr
