#!/usr/bin/env node
// CLI twin of `snarkjs groth16 prove <circuit.zkey> <witness.wtns> <proof.json> <public.json>`
// (snarkjs cli.js groth16Prove [EXT]; the reference's Makefile scripts the sibling PLONK lines,
// /root/reference/Makefile:30-33).  Writes JSON.stringify(x, null, 1) like snarkjs.
// And of `snarkjs groth16 setup <circuit.r1cs> <pot.ptau> <circuit_0000.zkey>` (alias `zkey new`; prepared ptau only).
// [--cshash]: the key carries the circuit hash of snarkjs's zkey_new.js at the head of section 10 (printed as snarkjs
// prints it) instead of the legacy 64 zero bytes, which stay the default; every later contribution, beacon, export and
// `zkey verify` chains from and compares what the key holds.  That the value equals snarkjs's own is not claimed.
// And of `snarkjs powersoftau prepare phase2 <powersoftau.ptau> <new_powersoftau.ptau>` (alias `pt2`).
// And of `snarkjs powersoftau new bn128 <power> <pot_0000.ptau>` (alias `ptn`), `snarkjs powersoftau contribute <old.ptau>
// <new.ptau> [--name=..] [-e=..]` (alias `ptc`: prints the contribution hash as snarkjs does; -e: THIS CLI's derivation of
// the six secret scalars, index.js ptauSecretFromEntropy, not snarkjs's) and `snarkjs powersoftau verify <pot.ptau>`
// (alias `ptv`): prints "[INFO]  snarkJS: Powers of tau Ok!" and exits 0, or "[ERROR] snarkJS: <reason>" and exits 1.
// And of the challenge / response exchange: `snarkjs powersoftau export challenge <pot.ptau> <challenge>` (alias `ptec`:
// prints the challenge hash), `snarkjs powersoftau challenge contribute bn128 <challenge> <response> [-e=..]` (alias
// `ptcc`) and `snarkjs powersoftau import response <old.ptau> <response> <new.ptau> [--name=..]` (alias `ptir`); the last
// two print the contribution hash, which is this library's responseHash and not snarkjs's hash of the response file.
// The transcript hashes are this library's (INTEGRATION.md 5b): snarkjs's `powersoftau verify` is not claimed to accept
// these files, nor this one snarkjs's.
// And of `snarkjs zkey contribute <old.zkey> <new.zkey> [--name=..] [-e=..]` (alias `zkc`): prints the contribution hash
// as snarkjs does.  -e: THIS CLI's derivation of the secret from the text (index.js secretFromEntropy), not snarkjs's.
// And of the two commands that close a ceremony: `snarkjs powersoftau beacon <old.ptau> <new.ptau> <beaconHash(hex)>
// <numIterationsExp> [--name=..]` (alias `ptb`) and `snarkjs zkey beacon <old.zkey> <new.zkey> <beaconHash(hex)>
// <numIterationsExp> [--name=..]` (alias `zkb`): a last contribution whose secret anyone recomputes from the beacon hash
// (1 to 255 bytes) by 2^numIterationsExp SHA-256 applications (10 to 63); both print the contribution hash.  A hex string
// of odd length or with other characters, or a missing argument, prints the usage and exits 2; a value out of range
// prints "[ERROR] snarkJS: <text>" and exits 1, nothing is written.  The derivation of the secret from the beacon is THIS
// LIBRARY'S, as the -e rule is: a beacon made by snarkjs fails `verify` here, and one made here fails snarkjs's.
// And of the phase-2 file exchange: `snarkjs zkey export bellman <circuit.zkey> <circuit.mpcparams>` (alias `zkeb`),
// `snarkjs zkey bellman contribute bn128 <challenge> <response> [-e=..]` (alias `zkbc`: prints the contribution hash; -e
// by the rule of `zkey contribute`, so the same text gives the same contribution through either route) and `snarkjs zkey
// import bellman <old.zkey> <response> <new.zkey> [--name=..]` (alias `zkib`: a refused response prints "[ERROR] snarkJS:
// <the verdict>" and exits 1, nothing is written).  An exchange with a snarkjs or bellman contributor is not claimed
// (INTEGRATION.md 5b).
// And of `snarkjs zkey verify frominit <init.zkey> <pot.ptau> <circuit.zkey>` (alias `zkvi`) and `snarkjs zkey verify
// <circuit.r1cs> <pot.ptau> <circuit.zkey>` (alias `zkv`: the setup runs in memory, no file is written): prints
// "[INFO]  snarkJS: ZKey Ok!" and exits 0, or "[ERROR] snarkJS: <reason>" and exits 1.  Both open the ptau and run the
// ptau leg: section 9 of the key against the ceremony file's section 2.  [--skip-ptau]: without the leg (`zkv` then runs
// the setup into a temporary file beside the zkey: a legacy zero-hash initial key, so a key made with --cshash is
// rejected on that path).  `zkv` with the leg gives the in-memory initial key the circuit hash when the key under test
// carries one.  csHash is built as snarkjs's zkey_new.js describes it; equality with snarkjs's value is not claimed
// (see INTEGRATION.md 5b).
// And of `snarkjs groth16 verify <verification_key.json> <public.json> <proof.json>` (groth16Verify [EXT]): prints
// "[INFO]  snarkJS: OK!" and exits 0, or "[ERROR] snarkJS: Invalid proof" and exits 1.
// And of `snarkjs wtns check <circuit.r1cs> <witness.wtns>` (alias `wchk`) of LATER snarkjs releases -- the pinned 0.4.12
// has none: prints "WITNESS IS CORRECT" and exits 0, or "[ERROR] snarkJS: WITNESS CHECKING FAILED", the lowest failing
// constraint, how many fail and its three values A.w, B.w, C.w, and exits 1.  [--device n]: a GPU ordinal, -1 = host
// threads.  `[groth16] prove ... --check <circuit.r1cs>` runs the same check first and stops with the same report and
// exit status 1 before anything is written.  These texts are modelled on later snarkjs and not compared with it.
// And of `snarkjs wtns calculate <circuit.wasm> <input.json> <witness.wtns>` (alias `wc`) and `snarkjs groth16 fullprove
// <input.json> <circuit.wasm> <circuit.zkey> <proof.json> <public.json>` (alias `g16f`), with a WITNESS PROGRAM where
// snarkjs takes the .wasm: `cli.js nzcp program <example|live> <file>` records one (no circom .wasm is run).  An input
// that violates a constraint prints "[ERROR] snarkJS: <the constraint's text>" and exits 1 before anything is written.
// `wtns calculate` runs on host threads unless --device names a GPU; `fullprove` computes the witness likewise and proves
// on the GPU.
// And of `snarkjs plonk fullprove <input.json> <circuit.wasm> <circuit.zkey> [proof.json] [public.json]` (alias `pkf`), with
// a witness program likewise: the witness is computed on the GPU and proved from where it lies (g16_plonk_fullprove_batch).
// A violated constraint prints "[ERROR] snarkJS: <its text>" and exits 1 before anything is written; a usage error exits 2.
// [--blinding b1,..,b9]: TEST-ONLY, the nine blinding scalars (reproducible bytes).
// `nzcp prove <file of URIs | URI> <program> <circuit.zkey> --keys keys.json [--out dir]` has no snarkjs counterpart: every
// pass is checked as `nzcp verify --batch` checks it, its input words are formed on the GPU and its proof made there, in one
// native call (g16_pass_fullprove_batch; --protocol plonk: its twin).  One line per pass; exit 0 iff all were proved.
"use strict";
const fs = require("fs");
const { groth16 } = require("./index.js");

async function main(argv) {
  let a = argv.slice(2);
  if (a[0] === "zkey" && a[1] === "export" && a[2] === "verificationkey") {   // snarkjs zkey export verificationkey <zkey> [vk.json]
    const { exportVerificationKey } = require("./index.js");
    const [zk, out = "verification_key.json"] = a.slice(3);
    fs.writeFileSync(out, JSON.stringify(exportVerificationKey(zk), null, 1), "utf-8");
    return;
  }
  if ((a[0] === "wtns" && a[1] === "check") || a[0] === "wchk") {
    const rest = a.slice(a[0] === "wchk" ? 1 : 2);
    const pos = [];
    let device = 0;
    for (let i = 0; i < rest.length; i++) {
      if (rest[i] === "--device") device = parseInt(rest[++i], 10);
      else if (!rest[i].startsWith("--")) pos.push(rest[i]);
    }
    if (pos.length < 2) { console.error("usage: cli.js wtns check <circuit.r1cs> <witness.wtns> [--device n]"); process.exit(2); }
    const { wtns, wtnsCheckReport } = require("./index.js");
    const v = await wtns.check(pos[0], pos[1], { device });
    if (!v.ok) throw new Error(wtnsCheckReport(v));
    console.log("WITNESS IS CORRECT");
    return;
  }
  if ((a[0] === "wtns" && a[1] === "calculate") || a[0] === "wc") {
    const rest = a.slice(a[0] === "wc" ? 1 : 2);
    const pos = [];
    let device = -1;
    for (let i = 0; i < rest.length; i++) {
      if (rest[i] === "--device") device = parseInt(rest[++i], 10);
      else if (!rest[i].startsWith("--")) pos.push(rest[i]);
    }
    if (pos.length < 3) { console.error("usage: cli.js wtns calculate <program> <input.json> <witness.wtns> [--device n]"); process.exit(2); }
    const { wtns } = require("./index.js");
    await wtns.calculate(pos[1], pos[0], pos[2], { device });
    return;
  }
  if ((a[0] === "groth16" && a[1] === "fullprove") || a[0] === "g16f") {
    const rest = a.slice(a[0] === "g16f" ? 1 : 2);
    const opts = {};
    const pos = [];
    for (let i = 0; i < rest.length; i++) {
      if (rest[i] === "--r") opts.r = rest[++i];
      else if (rest[i] === "--s") opts.s = rest[++i];
      else if (rest[i] === "--device") opts.device = parseInt(rest[++i], 10);
      else pos.push(rest[i]);
    }
    if (pos.length < 3) { console.error("usage: cli.js groth16 fullprove <input.json> <program> <circuit.zkey> [proof.json] [public.json] [--r dec --s dec --device n]"); process.exit(2); }
    const [input, program, zkey, proofFile = "proof.json", publicFile = "public.json"] = pos;
    const { proof, publicSignals } = await groth16.fullProve(input, program, zkey, opts);
    fs.writeFileSync(proofFile, JSON.stringify(proof, null, 1), "utf-8");
    fs.writeFileSync(publicFile, JSON.stringify(publicSignals, null, 1), "utf-8");
    return;
  }
  if (a[0] === "nzcp" && a[1] === "verify") {
    // nzcp verify <file of URIs | URI> --keys keys.json [--now t] [--device n]: one line per pass, exit 0 iff all are valid
    // nzcp verify <file of URIs | URI> --batch --keys keys.json [--now t] [--device n]: the same verdicts from ONE native call
    //   that parses and hashes the passes too (device 0 unless --device; -1 = host threads); prints exp and credSubjSha256
    // nzcp verify proof <verification_key.json> <public.json> <proof.json> <pass URI> --keys keys.json [--now t] [--device n]
    const rest = a.slice(2);
    const opts = {};
    const pos = [];
    let keysFile, batch = false;
    for (let i = 0; i < rest.length; i++) {
      if (rest[i] === "--keys") keysFile = rest[++i];
      else if (rest[i] === "--batch") batch = true;
      else if (rest[i] === "--now") opts.now = parseInt(rest[++i], 10);
      else if (rest[i] === "--device") opts.device = parseInt(rest[++i], 10);
      else pos.push(rest[i]);
    }
    const proofMode = pos[0] === "proof";
    if (!keysFile || pos.length < (proofMode ? 5 : 1)) {
      console.error("usage: cli.js nzcp verify <file of URIs | URI> [--batch] --keys keys.json [--now t] [--device n]\n" +
                    "       cli.js nzcp verify proof <verification_key.json> <public.json> <proof.json> <pass URI> --keys keys.json [--now t] [--device n]");
      process.exit(2);
    }
    const { nzcp } = require("./index.js");
    const doc = JSON.parse(fs.readFileSync(keysFile, "utf-8"));
    opts.keys = doc.keys || doc;
    const readJson = (f) => JSON.parse(fs.readFileSync(f, "utf-8"));
    if (proofMode) {
      const p = require("./nzcpInput.js").passSignatureInput(pos[4]);
      const [res] = await nzcp.verifyPassProof(readJson(pos[1]), [{ proof: readJson(pos[3]), publicSignals: readJson(pos[2]), signature: p.signature, iss: p.iss, kid: p.kid }], opts);
      if (!res.ok) throw new Error(res.reason);
      console.log("[INFO]  snarkJS: OK!");
      return;
    }
    const uris = /^NZCP:/.test(pos[0]) ? [pos[0]] : fs.readFileSync(pos[0], "utf-8").split("\n").map((x) => x.trim()).filter((x) => x);
    if (batch) {   // every pass parsed, hashed and checked in one native call
      const res = await nzcp.verifyPassBatch(uris, opts);
      res.forEach((r, i) => console.log(r.ok ? `pass ${i}: OK exp ${r.exp} ${r.credSubjSha256 || "-"}` : `pass ${i}: INVALID ${r.reason}`));
      if (!res.every((r) => r.ok)) process.exit(1);
      return;
    }
    const res = await nzcp.verifyPass(uris, opts);
    res.forEach((r, i) => console.log(r.ok ? `pass ${i}: OK ${r.claims.givenName} ${r.claims.familyName} ${r.claims.dob}` : `pass ${i}: INVALID ${r.reason}`));
    if (!res.every((r) => r.ok)) process.exit(1);
    return;
  }
  if (a[0] === "nzcp" && a[1] === "prove") {
    // nzcp prove <file of URIs | URI> <program> <circuit.zkey> --keys keys.json [--out dir] [--now t] [--unsigned]
    //   [--match-public] [--protocol groth16|plonk] [--device n]: every pass checked, its witness computed and proved in ONE
    //   native call; one line per pass, proof_<i>.json / public_<i>.json into --out for the proved ones; exit 0 iff all are
    const rest = a.slice(2);
    const opts = {};
    const pos = [];
    let keysFile, outDir;
    for (let i = 0; i < rest.length; i++) {
      if (rest[i] === "--keys") keysFile = rest[++i];
      else if (rest[i] === "--out") outDir = rest[++i];
      else if (rest[i] === "--now") opts.now = parseInt(rest[++i], 10);
      else if (rest[i] === "--device") opts.device = parseInt(rest[++i], 10);
      else if (rest[i] === "--protocol") opts.protocol = rest[++i];
      else if (rest[i] === "--unsigned") opts.unsigned = true;
      else if (rest[i] === "--match-public") opts.matchPublic = true;
      else pos.push(rest[i]);
    }
    if (!keysFile || pos.length < 3) {
      console.error("usage: cli.js nzcp prove <file of URIs | URI> <program> <circuit.zkey> --keys keys.json [--out dir] [--now t] [--unsigned] [--match-public] [--protocol groth16|plonk] [--device n]");
      process.exit(2);
    }
    const { nzcp } = require("./index.js");
    const doc = JSON.parse(fs.readFileSync(keysFile, "utf-8"));
    opts.keys = doc.keys || doc;
    opts.program = pos[1];
    opts.zkey = fs.readFileSync(pos[2]);
    const uris = /^NZCP:/.test(pos[0]) ? [pos[0]] : fs.readFileSync(pos[0], "utf-8").split("\n").map((x) => x.trim()).filter((x) => x);
    const res = await nzcp.provePasses(uris, opts);
    res.forEach((r, i) => {
      console.log(r.outcome === "done" ? `pass ${i}: PROVED` : `pass ${i}: NOT PROVED (${r.outcome}) ${r.text}`);
      if (r.outcome === "done" && outDir) {
        fs.writeFileSync(require("path").join(outDir, `proof_${i}.json`), JSON.stringify(r.proof, null, 1), "utf-8");
        fs.writeFileSync(require("path").join(outDir, `public_${i}.json`), JSON.stringify(r.publicSignals, null, 1), "utf-8");
      }
    });
    if (!res.every((r) => r.outcome === "done")) process.exit(1);
    return;
  }
  if (a[0] === "nzcp" && a[1] === "program") {
    const pos = a.slice(2).filter((x) => !x.startsWith("--"));
    if (pos.length < 2) { console.error("usage: cli.js nzcp program <example|live> <file>"); process.exit(2); }
    const { nzcp } = require("./index.js");
    await nzcp.witnessProgram(pos[0], pos[1]);
    return;
  }
  const ptb = (a[0] === "powersoftau" && a[1] === "beacon") || a[0] === "ptb";
  if (ptb || (a[0] === "zkey" && a[1] === "beacon") || a[0] === "zkb") {
    const rest = a.slice(a[0] === "ptb" || a[0] === "zkb" ? 1 : 2);
    const name = rest.map((x) => (x.startsWith("--name=") ? x.slice(7) : x.startsWith("-n=") ? x.slice(3) : undefined)).find((x) => x !== undefined);
    const pos = rest.filter((x) => !x.startsWith("-"));
    const hex = pos.length >= 3 && /^0x/i.test(pos[2]) ? pos[2].slice(2) : pos[2];
    if (pos.length < 4 || hex.length % 2 !== 0 || !/^[0-9a-fA-F]*$/.test(hex) || !/^\d{1,9}$/.test(pos[3])) {
      console.error(ptb ? "usage: cli.js powersoftau beacon <old_powersoftau.ptau> <new_powersoftau.ptau> <beaconHash(hex)> <numIterationsExp> [--name=..]"
        : "usage: cli.js zkey beacon <circuit_old.zkey> <circuit_new.zkey> <beaconHash(hex)> <numIterationsExp> [--name=..]");
      process.exit(2);
    }
    const { powersOfTau, zKey, formatHash } = require("./index.js");
    const hash = await (ptb ? powersOfTau : zKey).beacon(pos[0], pos[1], name, hex, parseInt(pos[3], 10));
    console.log(`[INFO]  snarkJS: Contribution Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "zkey" && a[1] === "export" && a[2] === "bellman") || a[0] === "zkeb") {
    const pos = a.slice(a[0] === "zkeb" ? 1 : 3).filter((x) => !x.startsWith("-"));
    if (pos.length < 2) { console.error("usage: cli.js zkey export bellman <circuit.zkey> <circuit.mpcparams>"); process.exit(2); }
    const { zKey } = require("./index.js");
    await zKey.exportBellman(pos[0], pos[1]);
    return;
  }
  if ((a[0] === "zkey" && a[1] === "bellman" && a[2] === "contribute") || a[0] === "zkbc") {
    const rest = a.slice(a[0] === "zkbc" ? 1 : 3);
    const entropy = rest.map((x) => (x.startsWith("--entropy=") ? x.slice(10) : x.startsWith("-e=") ? x.slice(3) : undefined)).find((x) => x !== undefined);
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 3) { console.error("usage: cli.js zkey bellman contribute bn128 <circuit.mpcparams> <circuit_response.mpcparams> [-e=..]"); process.exit(2); }
    if (!["bn128", "bn254", "altbn128"].includes(pos[0].toLowerCase())) throw new Error(`Curve not supported: ${pos[0]}`);
    const { zKey, formatHash } = require("./index.js");
    const hash = await zKey.bellmanContribute(pos[1], pos[2], entropy);
    console.log(`[INFO]  snarkJS: Contribution Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "zkey" && a[1] === "import" && a[2] === "bellman") || a[0] === "zkib") {
    const rest = a.slice(a[0] === "zkib" ? 1 : 3);
    const name = rest.map((x) => (x.startsWith("--name=") ? x.slice(7) : x.startsWith("-n=") ? x.slice(3) : undefined)).find((x) => x !== undefined);
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 3) { console.error("usage: cli.js zkey import bellman <circuit_old.zkey> <circuit.mpcparams> <circuit_new.zkey> [--name=..]"); process.exit(2); }
    const { zKey } = require("./index.js");
    await zKey.importBellman(pos[0], pos[1], pos[2], name);
    return;
  }
  if ((a[0] === "zkey" && a[1] === "contribute") || a[0] === "zkc") {
    const rest = a.slice(a[0] === "zkc" ? 1 : 2);
    const opt = (long, short) => {
      for (const x of rest) {
        if (x.startsWith(`--${long}=`)) return x.slice(long.length + 3);
        if (x.startsWith(`-${short}=`)) return x.slice(short.length + 2);
      }
      return undefined;
    };
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 2) { console.error("usage: cli.js zkey contribute <circuit_old.zkey> <circuit_new.zkey> [--name=..] [-e=..]"); process.exit(2); }
    const { zKey, formatHash } = require("./index.js");
    const hash = await zKey.contribute(pos[0], pos[1], opt("name", "n"), opt("entropy", "e"));
    console.log(`[INFO]  snarkJS: Contribution Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "zkey" && a[1] === "verify") || a[0] === "zkv" || a[0] === "zkvi") {
    let rest = a.slice(a[0] === "zkey" ? 2 : 1);
    const frominit = a[0] === "zkvi" || rest[0] === "frominit";
    if (rest[0] === "frominit") rest = rest.slice(1);
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 3) { console.error("usage: cli.js zkey verify [frominit] <circuit.r1cs | init.zkey> <pot.ptau> <circuit.zkey> [--skip-ptau]"); process.exit(2); }
    const { zKey, newZKey } = require("./index.js");
    const skipPtau = rest.includes("--skip-ptau");
    let res;
    if (frominit) {
      res = await zKey.verifyFromInit(pos[0], pos[1], pos[2], { reason: true, ptau: !skipPtau });
    } else if (!skipPtau) {
      res = await zKey.verifyFromR1cs(pos[0], pos[1], pos[2], { reason: true });
    } else {
      const tmp = `${pos[2]}.init.${process.pid}.tmp`;
      try {
        await newZKey(pos[0], pos[1], tmp);
        res = await zKey.verifyFromInit(tmp, pos[1], pos[2], { reason: true, ptau: false });
      } finally {
        if (fs.existsSync(tmp)) fs.unlinkSync(tmp);
      }
    }
    if (!res.ok) throw new Error(res.reason);
    console.log("[INFO]  snarkJS: ZKey Ok!");
    return;
  }
  if ((a[0] === "groth16" && a[1] === "setup") || (a[0] === "zkey" && a[1] === "new")) {
    // snarkjs groth16 setup <circuit.r1cs> <powersoftau.ptau> <circuit_0000.zkey>   (alias: zkey new)
    const pos = a.slice(2).filter((x) => !x.startsWith("--"));
    if (pos.length < 3) { console.error("usage: cli.js groth16 setup <circuit.r1cs> <pot.ptau> <circuit_0000.zkey> [--cshash]"); process.exit(2); }
    const { newZKey, formatHash } = require("./index.js");
    const hash = await newZKey(pos[0], pos[1], pos[2], { csHash: a.includes("--cshash") });
    if (hash) console.log(`[INFO]  snarkJS: Circuit Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "new") || a[0] === "ptn") {
    // snarkjs powersoftau new <curve> <power> [powersoftau_0000.ptau]   (alias: ptn)
    const pos = a.slice(a[0] === "ptn" ? 1 : 2).filter((x) => !x.startsWith("-"));
    if (pos.length < 3) { console.error("usage: cli.js powersoftau new bn128 <power> <powersoftau_0000.ptau>"); process.exit(2); }
    if (!/^\d+$/.test(pos[1])) throw new Error(`powersoftau new: bad power ${pos[1]}`);
    const { powersOfTau } = require("./index.js");
    await powersOfTau.newAccumulator(pos[0], parseInt(pos[1], 10), pos[2]);
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "contribute") || a[0] === "ptc") {
    const rest = a.slice(a[0] === "ptc" ? 1 : 2);
    const opt = (long, short) => {
      for (const x of rest) {
        if (x.startsWith(`--${long}=`)) return x.slice(long.length + 3);
        if (x.startsWith(`-${short}=`)) return x.slice(short.length + 2);
      }
      return undefined;
    };
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 2) { console.error("usage: cli.js powersoftau contribute <powersoftau.ptau> <new_powersoftau.ptau> [--name=..] [-e=..]"); process.exit(2); }
    const { powersOfTau, formatHash } = require("./index.js");
    const hash = await powersOfTau.contribute(pos[0], pos[1], opt("name", "n"), opt("entropy", "e"));
    console.log(`[INFO]  snarkJS: Contribution Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "export" && a[2] === "challenge") || a[0] === "ptec") {
    const pos = a.slice(a[0] === "ptec" ? 1 : 3).filter((x) => !x.startsWith("-"));
    if (pos.length < 2) { console.error("usage: cli.js powersoftau export challenge <powersoftau.ptau> <challenge>"); process.exit(2); }
    const { powersOfTau, formatHash } = require("./index.js");
    const hash = await powersOfTau.exportChallenge(pos[0], pos[1]);
    console.log(`[INFO]  snarkJS: Challenge Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "challenge" && a[2] === "contribute") || a[0] === "ptcc") {
    const rest = a.slice(a[0] === "ptcc" ? 1 : 3);
    const entropy = rest.map((x) => (x.startsWith("--entropy=") ? x.slice(10) : x.startsWith("-e=") ? x.slice(3) : undefined)).find((x) => x !== undefined);
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 3) { console.error("usage: cli.js powersoftau challenge contribute bn128 <challenge> <response> [-e=..]"); process.exit(2); }
    if (!["bn128", "bn254", "altbn128"].includes(pos[0].toLowerCase())) throw new Error(`Curve not supported: ${pos[0]}`);
    const { powersOfTau, formatHash } = require("./index.js");
    const hash = await powersOfTau.challengeContribute(pos[1], pos[2], entropy);
    console.log(`[INFO]  snarkJS: Contribution Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "import" && a[2] === "response") || a[0] === "ptir") {
    const rest = a.slice(a[0] === "ptir" ? 1 : 3);
    const name = rest.map((x) => (x.startsWith("--name=") ? x.slice(7) : x.startsWith("-n=") ? x.slice(3) : undefined)).find((x) => x !== undefined);
    const pos = rest.filter((x) => !x.startsWith("-"));
    if (pos.length < 3) { console.error("usage: cli.js powersoftau import response <powersoftau_old.ptau> <response> <powersoftau_new.ptau> [--name=..]"); process.exit(2); }
    const { powersOfTau, formatHash } = require("./index.js");
    const hash = await powersOfTau.importResponse(pos[0], pos[1], pos[2], name);
    console.log(`[INFO]  snarkJS: Contribution Hash: \n${formatHash(hash)}`);
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "verify") || a[0] === "ptv") {
    const pos = a.slice(a[0] === "ptv" ? 1 : 2).filter((x) => !x.startsWith("-"));
    if (pos.length < 1) { console.error("usage: cli.js powersoftau verify <powersoftau.ptau>"); process.exit(2); }
    const { powersOfTau } = require("./index.js");
    const res = await powersOfTau.verify(pos[0], { reason: true });
    if (!res.ok) throw new Error(res.reason);
    console.log("[INFO]  snarkJS: Powers of tau Ok!");
    return;
  }
  if ((a[0] === "powersoftau" && a[1] === "prepare" && a[2] === "phase2") || a[0] === "pt2") {
    // snarkjs powersoftau prepare phase2 <powersoftau.ptau> <new_powersoftau.ptau>   (alias: pt2)
    const pos = a.slice(a[0] === "pt2" ? 1 : 3).filter((x) => !x.startsWith("--"));
    if (pos.length < 2) { console.error("usage: cli.js powersoftau prepare phase2 <powersoftau.ptau> <new_powersoftau.ptau>"); process.exit(2); }
    const { powersOfTau } = require("./index.js");
    await powersOfTau.preparePhase2(pos[0], pos[1]);
    return;
  }
  if (a[0] === "plonk" && a[1] === "setup") {   // snarkjs plonk setup <circuit.r1cs> <powersoftau.ptau> <circuit.zkey>
    const pos = a.slice(2).filter((x) => !x.startsWith("--"));
    if (pos.length < 3) { console.error("usage: cli.js plonk setup <circuit.r1cs> <pot.ptau> <circuit.zkey> [--lagrange]"); process.exit(2); }
    const { plonk } = require("./index.js");
    await plonk.setup(pos[0], pos[1], pos[2], { lagrange: a.includes("--lagrange") });
    return;
  }
  if ((a[0] === "plonk" && a[1] === "fullprove") || a[0] === "pkf") {
    // snarkjs plonk fullprove <input.json> <circuit.wasm> <circuit.zkey> [proof.json] [public.json]   (alias: pkf)
    const rest = a.slice(a[0] === "pkf" ? 1 : 2);
    const opts = {};
    const pos = [];
    for (let i = 0; i < rest.length; i++) {
      if (rest[i] === "--device") opts.device = parseInt(rest[++i], 10);
      else if (rest[i] === "--blinding") opts.blinding = rest[++i].split(",");
      else pos.push(rest[i]);
    }
    if (pos.length < 3) { console.error("usage: cli.js plonk fullprove <input.json> <program> <circuit.zkey> [proof.json] [public.json] [--device n --blinding b1,..,b9]"); process.exit(2); }
    const [input, program, zkey, proofFile = "proof.json", publicFile = "public.json"] = pos;
    const { plonk } = require("./index.js");
    const { proof, publicSignals } = await plonk.fullProve(input, program, zkey, opts);
    fs.writeFileSync(proofFile, JSON.stringify(proof, null, 1), "utf-8");
    fs.writeFileSync(publicFile, JSON.stringify(publicSignals, null, 1), "utf-8");
    return;
  }
  if (a[0] === "plonk" && a[1] === "prove") {   // snarkjs plonk prove <circuit.zkey> <witness.wtns> [proof.json] [public.json]
    const [zk, wt, proofFile = "proof.json", publicFile = "public.json"] = a.slice(2).filter((x) => !x.startsWith("--"));
    const { plonk } = require("./index.js");
    const { proof, publicSignals } = await plonk.prove(zk, wt);
    fs.writeFileSync(proofFile, JSON.stringify(proof, null, 1), "utf-8");
    fs.writeFileSync(publicFile, JSON.stringify(publicSignals, null, 1), "utf-8");
    return;
  }
  if (a[0] === "groth16") a = a.slice(1);
  if (a[0] === "plonk" && a[1] === "verify") {   // snarkjs plonk verify <verification_key.json> <public.json> <proof.json>
    const { plonk } = require("./index.js");
    const [vk = "verification_key.json", pub = "public.json", proof = "proof.json"] = a.slice(2).filter((x) => !x.startsWith("--"));
    const ok = await plonk.verify(JSON.parse(fs.readFileSync(vk, "utf-8")), JSON.parse(fs.readFileSync(pub, "utf-8")),
      JSON.parse(fs.readFileSync(proof, "utf-8")));
    if (!ok) throw new Error("Invalid proof");
    console.log("[INFO]  snarkJS: OK!");
    return;
  }
  if (a[0] === "verify") {
    const pos = a.slice(1).filter((x) => !x.startsWith("--"));
    const di = a.indexOf("--device");
    const [vk = "verification_key.json", pub = "public.json", proof = "proof.json"] = pos.filter((x, i) => di < 0 || a.indexOf(x) !== di + 1);
    const ok = await groth16.verify(JSON.parse(fs.readFileSync(vk, "utf-8")), JSON.parse(fs.readFileSync(pub, "utf-8")),
      JSON.parse(fs.readFileSync(proof, "utf-8")), { device: di >= 0 ? parseInt(a[di + 1], 10) : 0 });
    if (!ok) throw new Error("Invalid proof");
    console.log("[INFO]  snarkJS: OK!");
    return;
  }
  if (a[0] === "prove") a = a.slice(1);
  const opts = {};
  const pos = [];
  for (let i = 0; i < a.length; i++) {
    if (a[i] === "--r") opts.r = a[++i];
    else if (a[i] === "--s") opts.s = a[++i];
    else if (a[i] === "--device") opts.device = parseInt(a[++i], 10);
    else if (a[i] === "--check") opts.check = a[++i];
    else pos.push(a[i]);
  }
  if (pos.length < 2) {
    console.error("usage: cli.js [groth16] prove <circuit.zkey> <witness.wtns> [proof.json] [public.json] [--r dec --s dec --device n --check circuit.r1cs]");
    process.exit(2);
  }
  const [zkey, wtns, proofFile = "proof.json", publicFile = "public.json"] = pos;
  if (opts.check) {   // the witness against its circuit first: a bad one stops here, nothing is written
    const { wtns: wt, wtnsCheckReport } = require("./index.js");
    const v = await wt.check(opts.check, wtns, { device: opts.device });
    if (!v.ok) throw new Error(wtnsCheckReport(v));
  }
  const { proof, publicSignals } = await groth16.prove(zkey, wtns, opts);
  fs.writeFileSync(proofFile, JSON.stringify(proof, null, 1), "utf-8");
  fs.writeFileSync(publicFile, JSON.stringify(publicSignals, null, 1), "utf-8");
}

main(process.argv).then(() => process.exit(0), (e) => { console.error(`[ERROR] snarkJS: ${e.message}`); process.exit(1); });
