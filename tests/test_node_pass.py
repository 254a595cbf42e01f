"""nzcp.verifyPassBatch, nzcp.passPublicSignals and `nzcp verify --batch` from Node.js, on the host route (device -1), against
the one-pass-at-a-time nzcp.verifyPass and against pass_ref.  No GPU needed."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import pass_cases as cases
from conftest import ROOT, golden_path

JS = os.path.join(ROOT, "nzcp-circom_amd", "js")
CLI = os.path.join(JS, "cli.js")
pytestmark = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
REASONS = ["malformed", "alg", "key", "signature", "notYet", "expired", "tooLong"]


def _node(script, tmp_path, data):
    (tmp_path / "data.json").write_text(json.dumps(data))
    r = subprocess.run(["node", "-e", script, str(tmp_path / "data.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_batch_agrees_with_verify_pass(tmp_path):
    """the corpus (without its too long items, which the one-pass reader has no verdict for): the same {ok, reason} pass by
    pass; the digests, nbf and exp of the records are the reference's; the too long items and the depth-17 item apart"""
    uris, records = cases.corpus()
    common = [i for i, r in enumerate(records) if r["verdict"] != 7]
    deep = next(c[1] for c in cases.cbor_cases() if c[0] == "nesting 17")
    script = f"""
    const {{ nzcp }} = require({json.dumps(JS)});
    const d = JSON.parse(require("fs").readFileSync(process.argv[1], "utf-8"));
    (async () => {{
      const opts = {{ keys: d.keys, now: d.now, device: -1 }};
      const one = await nzcp.verifyPass(d.common, opts);
      const batch = await nzcp.verifyPassBatch(d.common, opts);
      const apart = await nzcp.verifyPassBatch(d.apart, opts);
      const deepOne = await nzcp.verifyPass(d.apart[d.apart.length - 1], opts);
      console.log(JSON.stringify({{ one: one.map((r) => ({{ ok: r.ok, reason: r.reason }})), batch, apart, deepOne, reasons: nzcp.PASS_REASONS }}));
    }})();
    """
    apart = [uris[i] for i, r in enumerate(records) if r["verdict"] == 7] + [deep]
    out = _node(script, tmp_path, {"keys": cases.key_set()[0], "now": cases.NOW, "common": [uris[i] for i in common], "apart": apart})
    why = out["reasons"]
    assert [{"ok": r["ok"], "reason": r["reason"]} for r in out["batch"]] == out["one"]
    for i, got in zip(common, out["batch"]):
        want = records[i]
        assert got["ok"] == (want["verdict"] == 0) and got["reason"] == (why[REASONS[want["verdict"] - 1]] if want["verdict"] else None)
        if want["verdict"] == 1:
            assert got["toBeSignedSha256"] is None and got["exp"] is None
        else:
            assert got["toBeSignedSha256"] == want["tbs_sha256"].hex() and (got["nbf"], got["exp"]) == (want["nbf"], want["exp"])
            assert got["credSubjSha256"] == want["cred_subj_sha256"].hex()
    assert len(apart) >= 3
    assert [r["reason"] for r in out["apart"][:-1]] == [why["tooLong"]] * (len(apart) - 1)
    assert why["tooLong"] == "the pass URI is longer than 2048 bytes"
    # 17 arrays deep inside the unprotected header: the nesting cap makes it malformed here; the one-pass reader recurses
    assert out["apart"][-1]["reason"] == why["malformed"] and out["deepOne"]["ok"] is True


def test_pass_public_signals(tmp_path):
    uri = cases.example_uri()
    script = f"""
    const {{ nzcp }} = require({json.dumps(JS)});
    const input = require({json.dumps(os.path.join(JS, "nzcpInput.js"))});
    const d = JSON.parse(require("fs").readFileSync(process.argv[1], "utf-8"));
    (async () => {{
      const [res] = await nzcp.verifyPassBatch([d.uri], {{ keys: d.keys, now: d.now, device: -1 }});
      let refused = false;
      try {{ nzcp.passPublicSignals({{ ok: false, toBeSignedSha256: null, credSubjSha256: null }}); }} catch (e) {{ refused = true; }}
      console.log(JSON.stringify({{ res, got: nzcp.passPublicSignals(res), want: input.expectedPublicSignals(d.uri), refused }}));
    }})();
    """
    out = _node(script, tmp_path, {"keys": cases.key_set()[0], "now": cases.NOW, "uri": uri})
    assert out["res"]["ok"] is True and out["refused"] is True
    assert len(out["got"]) == 513 and out["got"] == out["want"]
    assert out["res"]["credSubjSha256"] == hashlib.sha256(b"Jack,Sparrow,1960-04-16").hexdigest()


def test_cli_batch(tmp_path):
    keys = golden_path("nzcp_example_issuer.json")
    uri = cases.example_uri()
    cred = hashlib.sha256(b"Jack,Sparrow,1960-04-16").hexdigest()

    def cli(*args):
        return subprocess.run(["node", CLI, *args], capture_output=True, text=True, timeout=120)
    r = cli("nzcp", "verify", uri, "--batch", "--keys", keys, "--now", "1700000000", "--device", "-1")
    assert r.returncode == 0 and r.stdout.strip() == f"pass 0: OK exp 1951416330 {cred}", r.stdout + r.stderr
    listing = tmp_path / "passes.txt"
    listing.write_text(uri + "\n\nNZCP:/1/AAAA\n" + uri + "=" * 1500 + "\n")
    r = cli("nzcp", "verify", str(listing), "--batch", "--keys", keys, "--now", "1700000000", "--device", "-1")
    assert r.returncode == 1, r.stdout + r.stderr
    assert r.stdout.splitlines() == [f"pass 0: OK exp 1951416330 {cred}", "pass 1: INVALID the pass URI is malformed",
                                     "pass 2: INVALID the pass URI is longer than 2048 bytes"]
    r = cli("nzcp", "verify", uri, "--batch", "--keys", keys, "--now", "2000000000", "--device", "-1")
    assert r.returncode == 1 and r.stdout.strip() == "pass 0: INVALID the pass has expired (exp)"
    # the one-pass output is what it was
    r = cli("nzcp", "verify", uri, "--keys", keys, "--now", "1700000000")
    assert r.returncode == 0 and r.stdout.strip() == "pass 0: OK Jack Sparrow 1960-04-16"
