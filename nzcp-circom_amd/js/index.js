// snarkjs-shaped host API over the MI355X prover (Node.js >= 12, N-API addon, no npm deps).
//
// Drop-in for the prove path of snarkjs 0.4.12 (pin /root/reference/yarn.lock:987-1001;
// /root/reference/package.json:12):
//     const { groth16 } = require("nzcp-circom_amd/js");
//     const { proof, publicSignals } = await groth16.prove(zkey, wtns);
// zkey / wtns: a path, a Buffer/Uint8Array, or snarkjs's {type: "mem", data: Uint8Array}.
// proof / publicSignals have exactly snarkjs's shape (decimal strings; key order pi_a, pi_b, pi_c,
// protocol, curve), so JSON.stringify(x, null, 1) reproduces proof.json / public.json byte for byte
// given the same blinding (r, s).  Errors are thrown Errors with snarkjs's messages.
// groth16.verify(vk, publicSignals, proof) is snarkjs's too (GPU pairing check, csrc/verify.hip); createVerifier(vk)
// keeps the key resident and verifies batches, one verdict per proof.
// wtns.check(r1cs, wtns) is later snarkjs's witness check (csrc/wtns_check.hip): {ok, constraint, nFailed, a, b, c}.
// wtns.calculate(input, program, wtnsFile) and groth16.fullProve(input, program, zkey) are snarkjs's, with a witness
// program recorded by the native builders (nzcp.witnessProgram) where snarkjs takes a circom .wasm.
// Extensions (not in snarkjs): opts = {r, s, device, devices, windowBits}; groth16.createProver() keeps the
// proving key resident in HBM across proofs; prover.proveBatch(wtnsList); createProver(zkey, {devices: [0, 1, ...]})
// shards ONE proof over several GPUs of the node (BASELINE config 4: MSM point ranges + the A/B/C evaluation split
// across the devices, partial sums added on the host).
"use strict";
const fs = require("fs");
const path = require("path");

let addon = null;
function native() {
  if (!addon) {
    const p = path.join(__dirname, "addon", "g16_napi.node");
    if (!fs.existsSync(p)) throw new Error(`${p} not built (run make -C ${path.dirname(p)}); there is no JS fallback`);
    addon = require(p);
  }
  return addon;
}

function toBuffer(x, what) {
  if (typeof x === "string") return fs.readFileSync(x);
  if (Buffer.isBuffer(x)) return x;
  if (x instanceof Uint8Array) return Buffer.from(x.buffer, x.byteOffset, x.byteLength);
  if (x && x.type === "mem" && x.data) return toBuffer(x.data, what);
  throw new Error(`${what}: expected a path, a Buffer/Uint8Array or {type:"mem", data}`);
}

function scalarToBuffer(v) {
  if (v === undefined || v === null) return null;
  if (Buffer.isBuffer(v)) return v;
  let n = BigInt(v);
  const out = Buffer.alloc(32);
  for (let i = 0; i < 32; i++) { out[i] = Number(n & 0xffn); n >>= 8n; }
  return out;
}

function dec(buf, off) {
  let n = 0n;
  for (let i = 31; i >= 0; i--) n = (n << 8n) | BigInt(buf[off + i]);
  return n.toString();
}
function isZero(buf, off, len) {
  for (let i = 0; i < len; i++) if (buf[off + i]) return false;
  return true;
}

// g16_proof bytes -> what snarkjs's G1/G2.toObject + stringifyBigInts produce
function proofObject(raw) {
  const g1 = (o) => (isZero(raw, o, 64) ? ["0", "1", "0"] : [dec(raw, o), dec(raw, o + 32), "1"]);
  const pi_b = isZero(raw, 64, 128)
    ? [["0", "0"], ["1", "0"], ["0", "0"]]
    : [[dec(raw, 64), dec(raw, 96)], [dec(raw, 128), dec(raw, 160)], ["1", "0"]];
  return { pi_a: g1(0), pi_b, pi_c: g1(192), protocol: "groth16", curve: "bn128" };
}
function publicSignals(pub) {
  const out = [];
  for (let o = 0; o < pub.length; o += 32) out.push(dec(pub, o));
  return out;
}

class Prover {
  constructor(handle) { this._h = handle; this._busy = Promise.resolve(); }
  get info() { return native().info(this._h); }
  get timings() { return native().timings(this._h); }
  // one in-flight prove per handle: serialise callers
  prove(wtns, opts = {}) {
    if (!this._h) return Promise.reject(new Error("prover is closed"));
    const w = toBuffer(wtns, "wtns"), h = this._h;
    const run = () => native().prove(h, w, scalarToBuffer(opts.r), scalarToBuffer(opts.s))
      .then(({ proof, pub }) => ({ proof: proofObject(proof), publicSignals: publicSignals(pub) }));
    const p = this._busy.then(run, run);
    this._busy = p.catch(() => {});
    return p;
  }
  // Batch of independent witnesses against the resident key (g16_prove_batch: the library overlaps
  // proof i+1's device work with proof i's tail).  opts.r / opts.s are TEST-ONLY: they pin ONE blinding pair
  // for every proof of the batch (reproducible bytes), which breaks zero-knowledge across the batch -- leave
  // them unset in production and every proof draws its own (r, s) from the OS CSPRNG.
  proveBatch(wtnsList, opts = {}) {
    if (!this._h) return Promise.reject(new Error("prover is closed"));
    const ws = wtnsList.map((w) => toBuffer(w, "wtns"));
    let rs = null;
    const r = scalarToBuffer(opts.r), s = scalarToBuffer(opts.s);
    if (r && s) {
      rs = Buffer.alloc(ws.length * 64);
      for (let i = 0; i < ws.length; i++) { r.copy(rs, i * 64); s.copy(rs, i * 64 + 32); }
    }
    const h = this._h;
    const run = () => native().proveBatch(h, ws, rs)
      .then((list) => list.map(({ proof, pub }) => ({ proof: proofObject(proof), publicSignals: publicSignals(pub) })));
    const p = this._busy.then(run, run);
    this._busy = p.catch(() => {});
    return p;
  }
  // Releases the resident key.  Proofs already requested (awaited or not) finish first: the native handle is
  // destroyed after the last of them settles, never under a running proof.  Returns a Promise.
  close() {
    if (!this._h) return this._busy;
    const h = this._h;
    this._h = null;
    this._busy = this._busy.then(() => native().destroy(h));
    return this._busy;
  }
}

async function createProver(zkey, opts = {}) {
  const z = toBuffer(zkey, "zkey");
  if (opts.shardCount > 1 || opts.shardRank)
    throw new Error("createProver: shardRank/shardCount belong to the C ABI of multi-process hosts; in Node pass " +
                    "devices: [ordinal, ...] and the proof is sharded over those GPUs inside this process");
  const nopts = { device: opts.device | 0, windowBits: opts.windowBits | 0, taskLen: opts.taskLen | 0 };
  if (Array.isArray(opts.devices) && opts.devices.length) nopts.devices = opts.devices.map((d) => d | 0);
  const h = await native().create(z, nopts);
  return new Prover(h);
}

// ------------------------------------------------------------------ verifier (snarkjs groth16.verify, batched on the GPU)
function le32(v) {
  let n = BigInt(v);
  if (n < 0n) throw new Error("negative field element");
  const out = Buffer.alloc(32);
  for (let i = 0; i < 32; i++) { out[i] = Number(n & 0xffn); n >>= 8n; }
  return out;   // (values >= 2^256 are cut: no field element is that large)
}
function g1Bytes(t) { return String(t[2]) === "0" ? Buffer.alloc(64) : Buffer.concat([le32(t[0]), le32(t[1])]); }
function g2Bytes(t) {
  if (String(t[2][0]) === "0" && String(t[2][1]) === "0") return Buffer.alloc(128);
  return Buffer.concat([le32(t[0][0]), le32(t[0][1]), le32(t[1][0]), le32(t[1][1])]);
}
// proof.json object -> g16_proof bytes; verification_key.json object -> the C ABI's point image (standard form)
function proofBytes(p) { return Buffer.concat([g1Bytes(p.pi_a), g2Bytes(p.pi_b), g1Bytes(p.pi_c)]); }
function vkeyBytes(vk) {
  if (!vk || vk.protocol !== "groth16" || !Array.isArray(vk.IC) || vk.IC.length !== Number(vk.nPublic) + 1)
    throw new Error("verification key: not a groth16 key (protocol / IC / nPublic)");
  return Buffer.concat([g1Bytes(vk.vk_alpha_1), g2Bytes(vk.vk_beta_2), g2Bytes(vk.vk_gamma_2), g2Bytes(vk.vk_delta_2),
    ...vk.IC.map(g1Bytes)]);
}

class Verifier {
  constructor(handle, nPublic) { this._h = handle; this.nPublic = nPublic; }
  // items: [{publicSignals, proof}] -> Promise<boolean[]>, one verdict per proof (g16_verify_batch)
  async verifyBatch(items) {
    if (!this._h) throw new Error("verifier is closed");
    const short = items.map((it) => it.publicSignals.length !== this.nPublic);
    const proofs = Buffer.concat(items.map((it) => proofBytes(it.proof)));
    const pubs = Buffer.concat(items.map((it, i) => (short[i] ? Buffer.alloc(this.nPublic * 32)
      : Buffer.concat(it.publicSignals.map(le32)))));
    const ok = await native().verifyBatch(this._h, proofs, pubs);
    return items.map((_, i) => !short[i] && ok[i] !== 0);
  }
  async verify(publicSignals, proof) { return (await this.verifyBatch([{ publicSignals, proof }]))[0]; }
  close() { if (this._h) { native().destroyVerifier(this._h); this._h = null; } }
}

async function createVerifier(vk, opts = {}) {
  const h = await native().createVerifier(vkeyBytes(vk), Number(vk.nPublic), 0, opts.device | 0);
  return new Verifier(h, Number(vk.nPublic));
}

// ------------------------------------------------------------------ PLONK (snarkjs plonk.prove on the GPU, csrc/plonk.hip)
const PLONK_G1 = ["A", "B", "C", "Z", "T1", "T2", "T3"];
const PLONK_EV = ["eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw", "eval_r"];
// g16_plonk_proof bytes -> the object snarkjs's plonk_prove.js stringifies (its key order)
function plonkProofObject(raw) {
  const g1 = (o) => (isZero(raw, o, 64) ? ["0", "1", "0"] : [dec(raw, o), dec(raw, o + 32), "1"]);
  const out = {};
  let o = 0;
  for (const k of PLONK_G1) { out[k] = g1(o); o += 64; }
  for (const k of PLONK_EV) { out[k] = dec(raw, o); o += 32; }
  out.Wxi = g1(o); out.Wxiw = g1(o + 64);
  out.protocol = "plonk"; out.curve = "bn128";
  return out;
}
class PlonkProver {
  constructor(handle) { this._h = handle; this._busy = Promise.resolve(); }
  // opts.blinding: nine scalars b1..b9 (decimal strings / BigInts) for a reproducible proof; default: fresh randomness
  prove(wtns, opts = {}) {
    if (!this._h) return Promise.reject(new Error("prover is closed"));
    const w = toBuffer(wtns, "wtns"), h = this._h;
    let bl = null;
    if (opts.blinding) {
      if (opts.blinding.length !== 9) return Promise.reject(new Error("blinding: nine scalars b1..b9 expected"));
      bl = Buffer.concat(opts.blinding.map(scalarToBuffer));
    }
    const run = () => native().plonkProve(h, w, bl)
      .then(({ proof, pub }) => ({ proof: plonkProofObject(proof), publicSignals: publicSignals(pub) }));
    const p = this._busy.then(run, run);
    this._busy = p.catch(() => {});
    return p;
  }
  close() {
    if (!this._h) return this._busy;
    const h = this._h;
    this._h = null;
    this._busy = this._busy.then(() => native().plonkDestroy(h));
    return this._busy;
  }
}
// verification_key.json / proof.json of PLONK -> the C ABI images (g16_plonk_verifier_create, g16_plonk_proof)
function plonkVkeyBytes(vk) {
  if (!vk || vk.protocol !== "plonk") throw new Error("verification key: not a plonk key");
  const head = Buffer.alloc(8);
  head.writeUInt32LE(Number(vk.power), 0);
  head.writeUInt32LE(Number(vk.nPublic), 4);
  return Buffer.concat([head, le32(vk.k1), le32(vk.k2), ...["Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"].map((k) => g1Bytes(vk[k])),
    g2Bytes(vk.X_2)]);
}
function plonkProofBytes(p) {
  return Buffer.concat([...PLONK_G1.map((k) => g1Bytes(p[k])), ...PLONK_EV.map((k) => le32(p[k])), g1Bytes(p.Wxi), g1Bytes(p.Wxiw)]);
}
class PlonkVerifier {
  constructor(handle, nPublic) { this._h = handle; this.nPublic = nPublic; }
  async verifyBatch(items) {
    if (!this._h) throw new Error("verifier is closed");
    const short = items.map((it) => it.publicSignals.length !== this.nPublic);
    const proofs = Buffer.concat(items.map((it) => plonkProofBytes(it.proof)));
    const pubs = Buffer.concat(items.map((it, i) => (short[i] ? Buffer.alloc(this.nPublic * 32)
      : Buffer.concat(it.publicSignals.map(le32)))));
    const ok = await native().verifyBatch(this._h, proofs, pubs);
    return items.map((_, i) => !short[i] && ok[i] !== 0);
  }
  async verify(publicSignals, proof) { return (await this.verifyBatch([{ publicSignals, proof }]))[0]; }
  close() { if (this._h) { native().destroyVerifier(this._h); this._h = null; } }
}

const plonk = {
  // snarkjs: plonk.verify(vk_verifier, publicSignals, proof[, logger]) -> boolean
  async verify(vk, publicSignals, proof, opts = {}) {
    const v = await plonk.createVerifier(vk, opts && typeof opts.debug === "function" ? {} : opts);
    try {
      return await v.verify(publicSignals, proof);
    } finally {
      v.close();
    }
  },
  async createVerifier(vk, opts = {}) {
    const h = await native().createVerifier(plonkVkeyBytes(vk), Number(vk.nPublic), 0, opts.device | 0, 1);
    return new PlonkVerifier(h, Number(vk.nPublic));
  },
  // snarkjs: plonk.prove(zkeyFileName, witnessFileName[, logger]) -> {proof, publicSignals}
  async prove(zkey, wtns, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = {};
    const prover = await plonk.createProver(zkey, opts);
    try {
      return await prover.prove(wtns, opts);
    } finally {
      await prover.close();
    }
  },
  async createProver(zkey, opts = {}) {
    return new PlonkProver(await native().plonkCreate(toBuffer(zkey, "zkey"), opts.device | 0));
  },
  // snarkjs: plonk.setup(r1csName, ptauName, zkeyName[, logger]) -- file names (a ceremony file exceeds a Buffer).
  // opts.lagrange: also write the Lagrange section 13 (snarkjs's own prover reads it; this one does not -- it is
  // nPublic x 5N field elements, 344 GB for 513 public signals at N = 2^22).
  async setup(r1csName, ptauName, zkeyName, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = {};
    await native().plonkSetupFiles(String(r1csName), String(ptauName), String(zkeyName), opts.device | 0, opts.lagrange ? 1 : 0);
  },
};

// ------------------------------------------------------------------ groth16 setup (zkey new)
// snarkjs: zKey.newZKey(r1csName, ptauName, zkeyName[, logger]) / CLI `groth16 setup` = `zkey new` -- file names (a
// ceremony file exceeds a Buffer).  The ptau must be prepared (`powersoftau prepare phase2`).  The key is a fresh
// _0000 key (gamma = delta = 1, no contribution): not safe to deploy before a phase-2 contribution.
// opts.csHash: the key carries the circuit hash of snarkjs's zkey_new.js (g16_zkey_new; resolves with its 64 bytes)
// instead of the legacy 64 zero bytes, which stay the default.  Equality with snarkjs's own value is not claimed.
async function newZKey(r1csName, ptauName, zkeyName, opts = {}) {
  if (!opts || typeof opts.debug === "function") opts = {};
  if (opts.csHash) return native().zkeyNewFiles(String(r1csName), String(ptauName), String(zkeyName), opts.device | 0);
  await native().groth16SetupFiles(String(r1csName), String(ptauName), String(zkeyName), opts.device | 0);
  return undefined;
}
// The circuit hash `newZKey(.., { csHash: true })` stores for this INITIAL key over this ceremony file (g16_zkey_cs_hash):
// what section 10 already holds is not read, so the owner of a legacy zero-hash key can check or upgrade it.
async function csHash(zkeyName, ptauName, opts = {}) {
  return native().zkeyCsHashFiles(String(zkeyName), String(ptauName), (opts && opts.device) | 0);
}

// ------------------------------------------------------------------ powersoftau prepare phase2
// snarkjs: powersOfTau.preparePhase2(oldPtauFilename, newPTauFilename[, logger]) / CLI `powersoftau prepare phase2`
// (alias `pt2`) -- file names.  Sections 1-7 are copied; the Lagrange sections 12-15 are computed on the device.
const powersOfTau = {
  async preparePhase2(oldPtauName, newPtauName, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = {};
    await native().ptauPrepareFiles(String(oldPtauName), String(newPtauName), opts.device | 0);
  },
  // snarkjs: powersOfTau.newAccumulator(curve, power, fileName[, logger]) / CLI `powersoftau new bn128 <power> <file>`
  // (alias `ptn`).  The curve is bn128: (power, fileName) here, or snarkjs's three arguments with "bn128" first.
  async newAccumulator(...args) {
    if (typeof args[0] === "string" && args.length >= 3) {
      if (!["bn128", "bn254", "altbn128"].includes(args[0].toLowerCase())) throw new Error(`Curve not supported: ${args[0]}`);
      args = args.slice(1);
    }
    const power = Number(args[0]);
    if (!Number.isInteger(power) || power < 0) throw new Error("powersoftau new: the power is a non-negative integer");
    await native().ptauNewFile(power, String(args[1]));
  },
  // snarkjs: powersOfTau.contribute(oldPtauFilename, newPTauFilename, name, entropy[, logger]) -> the 64-byte
  // contribution hash / CLI `powersoftau contribute` (alias `ptc`).  entropy: a string (or Buffer) turned into the six
  // secret scalars by ptauSecretFromEntropy -- THIS LIBRARY'S rule, not snarkjs's.  Absent: the OS CSPRNG.  The
  // transcript (challenge and response hashes) is this library's too: see INTEGRATION.md 5b.
  async contribute(oldPtauName, newPtauName, name, entropy, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = {};
    const secret = entropy === undefined || entropy === null || entropy === "" ? null : ptauSecretFromEntropy(entropy);
    return native().ptauContributeFiles(String(oldPtauName), String(newPtauName), name ? String(name) : null, secret, opts.device | 0);
  },
  // snarkjs: powersOfTau.beacon(oldPtauFilename, newPTauFilename, name, beaconHashStr, numIterationsExp[, logger]) ->
  // the 64-byte contribution hash / CLI `powersoftau beacon` (alias `ptb`).  beaconHashStr: hex (or a Buffer), 1 to 255
  // bytes; numIterationsExp: 10 to 63.  The secret scalars come from the beacon by THIS LIBRARY'S rule (g16_beacon_scalars),
  // not snarkjs's: `verify` here recomputes them, snarkjs's would not find them.
  async beacon(oldPtauName, newPtauName, name, beaconHash, numIterationsExp, opts = {}) {
    if (typeof opts !== "object" || opts === null || typeof opts.debug === "function") opts = {};
    return native().ptauBeaconFiles(String(oldPtauName), String(newPtauName), name ? String(name) : null, beaconBytes(beaconHash),
      beaconExp(numIterationsExp), opts.device | 0);
  },
  // snarkjs: powersOfTau.verify(tauFilename[, logger]) -> boolean / CLI `powersoftau verify` (alias `ptv`).
  // opts.reason = true returns {ok, reason} instead.
  async verify(ptauName, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = {};
    const res = await native().ptauVerifyFile(String(ptauName), opts.device | 0);
    return opts.reason ? res : res.ok;
  },
  // The challenge / response file exchange: how somebody who does not hold the .ptau contributes (INTEGRATION.md 5b).
  // snarkjs: powersOfTau.exportChallenge(pTauFilename, challengeFilename[, logger]) / CLI `powersoftau export
  // challenge` (alias `ptec`) -> the 64-byte challenge hash.  Host only.
  async exportChallenge(ptauName, challengeName) {
    return native().ptauExportChallengeFiles(String(ptauName), String(challengeName));
  },
  // snarkjs: powersOfTau.challengeContribute(curve, challengeFilename, responseFileName, entropy[, logger]) / CLI
  // `powersoftau challenge contribute bn128 <challenge> <response> [-e=..]` (alias `ptcc`) -> the 64-byte contribution
  // hash (this library's responseHash, not snarkjs's hash of the response file).  The curve is bn128 and may be left out.
  async challengeContribute(...args) {
    if (args.length >= 3 && typeof args[0] === "string" && typeof args[2] === "string" && ["bn128", "bn254", "altbn128"].includes(args[0].toLowerCase())) args = args.slice(1);
    const [challengeName, responseName, entropy] = args;
    let opts = args[3] || {};
    if (opts && typeof opts.debug === "function") opts = {};
    const secret = entropy === undefined || entropy === null || entropy === "" ? null : ptauSecretFromEntropy(entropy);
    return native().ptauChallengeContributeFiles(String(challengeName), String(responseName), secret, opts.device | 0);
  },
  // snarkjs: powersOfTau.importResponse(oldPtauFilename, contributionFilename, newPTauFilename, name, importPoints[,
  // logger]) / CLI `powersoftau import response` (alias `ptir`) -> the 64-byte contribution hash.  A response that
  // fails a check of its record rejects with that check's text and writes nothing.
  async importResponse(oldPtauName, responseName, newPtauName, name, opts = {}) {
    if (typeof opts !== "object" || opts === null || typeof opts.debug === "function") opts = {};
    return native().ptauImportResponseFiles(String(oldPtauName), String(responseName), String(newPtauName), name ? String(name) : null, opts.device | 0);
  },
};
// a beacon hash as snarkjs takes it (misc.js hex2ByteArray: hex digits, "0x" allowed), checked; a Buffer passes as it is
function beaconBytes(h) {
  if (Buffer.isBuffer(h) || h instanceof Uint8Array) return Buffer.from(h);
  let s = String(h);
  if (/^0x/i.test(s)) s = s.slice(2);
  if (s.length % 2 !== 0 || !/^[0-9a-fA-F]*$/.test(s)) throw new Error("beacon: the beacon hash must be a hex string of whole bytes");
  return Buffer.from(s, "hex");
}
function beaconExp(e) {
  const n = Number(e);
  if (!Number.isInteger(n) || n < 0 || n > 0xffffffff) throw new Error("beacon: numIterationsExp must be between 10 and 63");
  return n;
}
// tau | alpha | beta | s_tau | s_alpha | s_beta from a text: h_j = Blake2b-512(text | byte j), j = 0, 1, 2; the first
// 32 bytes of h_j (little-endian, reduced mod r, 0 becomes 1) are key j, the last 32 bytes s_j (g16_ptau_secret_from_text).
// This library's rule, not snarkjs's -- as is the rule that turns a beacon hash into scalars (g16_beacon_scalars).
function ptauSecretFromEntropy(entropy) {
  const out = Buffer.alloc(192);
  for (let j = 0; j < 3; j++) {
    const h = require("crypto").createHash("blake2b512").update(entropy).update(Buffer.from([j])).digest();
    for (let half = 0; half < 2; half++) {
      let v = leBig(h, 32 * half) % FR;
      if (v === 0n) v = 1n;
      for (let i = 0; i < 32; i++) { out[96 * half + 32 * j + i] = Number(v & 0xffn); v >>= 8n; }
    }
  }
  return out;
}

// ------------------------------------------------------------------ zkey contribute / zkey verify
// snarkjs: zKey.contribute(oldZkeyName, newZKeyName, name, entropy[, logger]) -> the 64-byte contribution hash.
// entropy: a string (or Buffer), hashed with Blake2b-512 into the two secret scalars d | s -- each 32-byte half, read
// little-endian, reduced mod r (0 becomes 1): THIS LIBRARY'S derivation, not snarkjs's (which seeds a ChaCha stream),
// so the same text gives the same key here and another one there.  Absent: the OS CSPRNG.  (A beacon's d | s come from
// g16_beacon_scalars, this library's rule likewise: see beacon() below.)
function secretFromEntropy(entropy) {
  const h = require("crypto").createHash("blake2b512").update(entropy).digest();
  const out = Buffer.alloc(64);
  for (let k = 0; k < 2; k++) {
    let v = leBig(h, 32 * k) % FR;
    if (v === 0n) v = 1n;
    for (let i = 0; i < 32; i++) { out[32 * k + i] = Number(v & 0xffn); v >>= 8n; }
  }
  return out;
}
async function contribute(oldZkeyName, newZkeyName, name, entropy, opts = {}) {
  if (opts && typeof opts.debug === "function") opts = {};
  const secret = entropy === undefined || entropy === null || entropy === "" ? null : secretFromEntropy(entropy);
  return native().zkeyContributeFiles(String(oldZkeyName), String(newZkeyName), name ? String(name) : null, secret, opts.device | 0);
}
// snarkjs: zKey.beacon(zkeyNameOld, zkeyNameNew, name, beaconHashStr, numIterationsExp[, logger]) -> the 64-byte
// contribution hash / CLI `zkey beacon` (alias `zkb`).  Arguments and the rule as in powersOfTau.beacon.
async function beacon(oldZkeyName, newZkeyName, name, beaconHash, numIterationsExp, opts = {}) {
  if (typeof opts !== "object" || opts === null || typeof opts.debug === "function") opts = {};
  return native().zkeyBeaconFiles(String(oldZkeyName), String(newZkeyName), name ? String(name) : null, beaconBytes(beaconHash),
    beaconExp(numIterationsExp), opts.device | 0);
}
// The MPCParams file exchange (g16_prover.h: g16_zkey_export_bellman and the two entries after it).
// snarkjs: zKey.exportBellman(zkeyName, mpcparamsName[, logger]).
async function exportBellman(zkeyName, mpcparamsName, opts = {}) {
  if (typeof opts !== "object" || opts === null || typeof opts.debug === "function") opts = {};
  return native().zkeyExportBellmanFiles(String(zkeyName), String(mpcparamsName), opts.device | 0);
}
// snarkjs: zKey.bellmanContribute(curve, challengeName, responseName, entropy[, logger]) -> the 64-byte contribution
// hash.  The curve is bn128 and may be left out.  entropy: the rule of contribute() above, so the same text gives the
// same contribution through either route.
async function bellmanContribute(...args) {
  if (args.length >= 3 && typeof args[0] === "string" && typeof args[2] === "string" && ["bn128", "bn254", "altbn128"].includes(args[0].toLowerCase())) args = args.slice(1);
  const [challengeName, responseName, entropy] = args;
  let opts = args[3] || {};
  if (typeof opts !== "object" || typeof opts.debug === "function") opts = {};
  const secret = entropy === undefined || entropy === null || entropy === "" ? null : secretFromEntropy(entropy);
  return native().zkeyBellmanContributeFiles(String(challengeName), String(responseName), secret, opts.device | 0);
}
// snarkjs: zKey.importBellman(zkeyNameOld, mpcparamsName, zkeyNameNew, name[, logger]).  A response the import refuses
// rejects with the verdict's text and writes nothing.
async function importBellman(oldZkeyName, responseName, newZkeyName, name, opts = {}) {
  if (typeof opts !== "object" || opts === null || typeof opts.debug === "function") opts = {};
  return native().zkeyImportBellmanFiles(String(oldZkeyName), String(responseName), String(newZkeyName), name ? String(name) : null, opts.device | 0);
}
// snarkjs: zKey.verifyFromInit(initFileName, pTauFileName, zkeyFileName[, logger]) -> boolean.  The ptau (prepared or
// not) is opened and the ptau leg runs: section 9 of the key is the H basis of that file's section 2 scaled by 1 / delta.
// opts.ptau === false: without the leg, the ptau argument is then not opened.  opts.reason = true returns {ok, reason}
// instead.
async function verifyFromInit(initName, ptauName, zkeyName, opts = {}) {
  if (opts && typeof opts.debug === "function") opts = {};
  const res = opts.ptau === false
    ? await native().zkeyVerifyFromInitFiles(String(initName), String(zkeyName), opts.device | 0)
    : await native().zkeyVerifyFromInitPtauFiles(String(initName), String(ptauName), String(zkeyName), opts.device | 0);
  return opts.reason ? res : res.ok;
}
// snarkjs: zKey.verifyFromR1cs(r1csFileName, pTauFileName, zkeyFileName[, logger]) -> boolean.  The initial key is set
// up again from the .r1cs and the prepared ptau in memory (no file is written), then verifyFromInit with the ptau leg.
async function verifyFromR1cs(r1csName, ptauName, zkeyName, opts = {}) {
  if (opts && typeof opts.debug === "function") opts = {};
  const res = await native().zkeyVerifyR1csFiles(String(r1csName), String(ptauName), String(zkeyName), opts.device | 0);
  return opts.reason ? res : res.ok;
}
// snarkjs formatHash: four lines of four big-endian u32 in 8 hex digits, each line led by two tabs
function formatHash(b) {
  let s = "";
  for (let i = 0; i < 4; i++) {
    if (i > 0) s += "\n";
    s += "\t\t";
    for (let j = 0; j < 4; j++) {
      if (j > 0) s += " ";
      s += b.readUInt32BE(i * 16 + j * 4).toString(16).padStart(8, "0");
    }
  }
  return s;
}

// ------------------------------------------------------------------ zkey export verificationkey (host-only: header reads)
// snarkjs `zKey.exportVerificationKey(zkey)` / CLI `zkey export verificationkey <zkey> <vk.json>` -- the second line of
// the reference's PLONK flow (/root/reference/Makefile:32).  Groth16 and PLONK keys; points leave Montgomery form here
// (BigInt arithmetic, a few hundred values).  Groth16: `vk_alphabeta_12` -- redundant, snarkjs's verifier does not
// read it -- is not written.
const FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583n;
const FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
function modpow(b, e, m) { let r = 1n; b %= m; while (e > 0n) { if (e & 1n) r = (r * b) % m; b = (b * b) % m; e >>= 1n; } return r; }
const RQ_INV = modpow((1n << 256n) % FQ, FQ - 2n, FQ), RR_INV = modpow((1n << 256n) % FR, FR - 2n, FR);
function leBig(buf, off) { let n = 0n; for (let i = 31; i >= 0; i--) n = (n << 8n) | BigInt(buf[off + i]); return n; }
function sections(buf, what) {
  if (buf.length < 12 || buf.toString("latin1", 0, 4) !== what) throw new Error(`${what}: Invalid File format`);
  const n = buf.readUInt32LE(8), out = {};
  let pos = 12;
  for (let i = 0; i < n; i++) {
    if (pos + 12 > buf.length) throw new Error(`${what}: Invalid File format`);
    const id = buf.readUInt32LE(pos), size = Number(buf.readBigUInt64LE(pos + 4));
    pos += 12;
    if (size > buf.length - pos) throw new Error(`${what}: Invalid File format`);
    if (!(id in out)) out[id] = { pos, size };
    pos += size;
  }
  return out;
}
function exportVerificationKey(zkey) {
  const b = toBuffer(zkey, "zkey"), s = sections(b, "zkey");
  if (!s[1] || !s[2]) throw new Error("zkey: Invalid File format");
  const proto = b.readUInt32LE(s[1].pos);
  const fq = (o) => ((leBig(b, o) * RQ_INV) % FQ).toString();
  const g1 = (o) => (isZero(b, o, 64) ? ["0", "1", "0"] : [fq(o), fq(o + 32), "1"]);
  const g2 = (o) => (isZero(b, o, 128) ? [["0", "0"], ["1", "0"], ["0", "0"]]
    : [[fq(o), fq(o + 32)], [fq(o + 64), fq(o + 96)], ["1", "0"]]);
  let h = s[2].pos + 72;   // past n8q, q, n8r, r
  if (proto === 1) {
    const nPublic = b.readUInt32LE(h + 4);
    h += 12;
    const vk = { protocol: "groth16", curve: "bn128", nPublic, vk_alpha_1: g1(h), vk_beta_2: g2(h + 128), vk_gamma_2: g2(h + 256),
      vk_delta_2: g2(h + 448), IC: [] };
    if (!s[3] || s[3].size !== (nPublic + 1) * 64) throw new Error("zkey: Invalid File format");
    for (let i = 0; i <= nPublic; i++) vk.IC.push(g1(s[3].pos + 64 * i));
    return vk;
  }
  if (proto === 2) {
    const nPublic = b.readUInt32LE(h + 4), domainSize = b.readUInt32LE(h + 8);
    const power = 31 - Math.clz32(domainSize);
    h += 20;
    const fr = (o) => ((leBig(b, o) * RR_INV) % FR).toString();
    const vk = { protocol: "plonk", curve: "bn128", nPublic, power, k1: fr(h), k2: fr(h + 32) };
    h += 64;
    for (const k of ["Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"]) { vk[k] = g1(h); h += 64; }
    vk.X_2 = g2(h);
    vk.w = modpow(5n, (FR - 1n) >> BigInt(power), FR).toString();   // Fr.w[power]: 5^((r-1)/2^power)
    return vk;
  }
  throw new Error("zkey: unknown protocol");
}

// ------------------------------------------------------------------ wtns check
// Later snarkjs releases: wtns.check(r1csFilename, wtnsFilename[, logger]) -> boolean / CLI `wtns check` (alias `wchk`);
// the pinned 0.4.12 has none, and nothing here is compared with snarkjs.  Resolves to {ok, constraint, nFailed, a, b, c}:
// constraint = the lowest failing row (-1: none), nFailed = how many rows fail, a, b, c = the values A.w, B.w, C.w of
// that row as decimal strings ("0" when ok).  A malformed file rejects with the library's text.  opts.device: a GPU
// ordinal (default 0) or -1 = host threads.
const wtns = {
  async check(r1csName, wtnsName, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = {};
    const device = opts.device === undefined || opts.device === null ? 0 : opts.device | 0;
    const v = await native().wtnsCheckFiles(String(r1csName), String(wtnsName), device);
    return { ok: v.constraint < 0, constraint: v.constraint, nFailed: v.nFailed, a: dec(v.a, 0), b: dec(v.b, 0), c: dec(v.c, 0) };
  },
  // snarkjs: wtns.calculate(input, wasmFileName, wtnsFileName) -- here the second argument is a WITNESS PROGRAM recorded
  // by the native builders (nzcp.witnessProgram), not a circom .wasm, which this library does not run.  input: an object
  // (or the name of its .json) whose keys are the program's named inputs.  A violated check rejects with its text before
  // anything is written.  opts.device: a GPU ordinal, or -1 = host threads (the default).
  async calculate(input, programName, wtnsName, opts = {}) {
    const image = calculateWitness(input, programName, opts);
    fs.writeFileSync(String(wtnsName), image);
  },
};
function calculateWitness(input, programName, opts) {
  const device = !opts || opts.device === undefined || opts.device === null ? -1 : opts.device | 0;
  const { names, values } = inputArrays(input);
  const res = native().wtnsCalculate(String(programName), names, values, device);
  if (res.status >= 0) throw new Error(res.text);
  return res.wtns;
}
// One pass's input object (or the name of its .json) -> what the addon matches against the program's input table
function inputArrays(input) {
  if (typeof input === "string") input = JSON.parse(fs.readFileSync(input, "utf-8"));
  const names = Object.keys(input);
  const values = names.map((k) => Buffer.concat((Array.isArray(input[k]) ? input[k].flat(Infinity) : [input[k]]).map((x) => scalarToBuffer(x))));
  return { names, values };
}
// Batched fullprove (g16_fullprove_batch, g16_plonk_fullprove_batch): the witnesses are computed on the GPU in chunks and
// proved from the chunk buffers; only inputs, public signals and proofs cross the bus.  `blind`: per pass its fixed
// blinding bytes, or null.  -> per pass {proof, publicSignals}, or {error: the violated check's text}.
function fullProveBatchNative(isPlonk, inputs, programName, zkey, opts, blind) {
  const device = !opts || opts.device === undefined || opts.device === null ? 0 : opts.device | 0;
  const passes = inputs.map(inputArrays);
  const res = native().fullProveBatch(isPlonk, String(programName), toBuffer(zkey, "zkey"), passes.map((p) => p.names),
    passes.map((p) => p.values), device, blind);
  return res.map((r) => (r.status >= 0 ? { error: r.text }
    : { proof: isPlonk ? plonkProofObject(r.proof) : proofObject(r.proof), publicSignals: publicSignals(r.pub) }));
}
// opts.blinding of a PLONK proof: the nine scalars b1..b9 (TEST-ONLY: reproducible bytes) -> 288 bytes, or null
function plonkBlinding(b) {
  if (b === undefined || b === null) return null;
  if (Buffer.isBuffer(b)) return b;
  if (!Array.isArray(b) || b.length !== 9) throw new Error("plonk: blinding takes the nine scalars b1..b9");
  return Buffer.concat(b.map((x) => scalarToBuffer(x)));
}
// ---- pass verification (the twin of @vaxxnz/nzcp's offline verification; fetching the issuer's DID document stays with
// the caller): keys = { "<iss>#<kid>": {x, y} } with base64url P-256 coordinates as in a DID document's publicKeyJwk
const nzcpInput = require("./nzcpInput.js");
const PASS_REASONS = {
  malformed: "the pass URI is malformed",
  alg: "the pass is not signed with ES256 (alg -7)",
  key: "no issuer key for this iss and kid",
  signature: "the signature does not verify",
  notYet: "the pass is not yet valid (nbf)",
  expired: "the pass has expired (exp)",
  proof: "the proof does not verify",
  bits: "public signals 0..511 are not all bits",
  tooLong: "the pass URI is longer than 2048 bytes",
};
const PASS_PROOF_VERDICTS = [null, PASS_REASONS.proof, PASS_REASONS.bits, PASS_REASONS.signature, PASS_REASONS.expired];
function issuerKeys(keys) {
  const names = Object.keys(keys || {});
  if (!names.length) throw new Error("verifyPass: no issuer keys given");
  const coord = (v, name) => {
    const b = Buffer.from(String(v).replace(/-/g, "+").replace(/_/g, "/"), "base64");
    if (b.length !== 32) throw new Error(`verifyPass: key ${name}: a coordinate is not 32 bytes`);
    return b;
  };
  return { names, bytes: Buffer.concat(names.map((n) => Buffer.concat([coord(keys[n].x, n), coord(keys[n].y, n)]))) };
}
function keyIndexBuffer(idx) {
  const b = Buffer.alloc(idx.length * 4);
  idx.forEach((k, i) => b.writeUInt32LE(k, i * 4));
  return b;
}
function passNow(opts) { return opts.now === undefined ? Math.floor(Date.now() / 1000) : Number(opts.now); }

// nzcp.verifyPass(uri | uris, {keys, now, device = -1}) -> {ok, reason, claims} (an array for an array): the URI is parsed,
// the key looked up and nbf / exp checked here; the signatures of all passes go through ONE g16_es256_verify_batch
async function verifyPass(uriOrUris, opts = {}) {
  const many = Array.isArray(uriOrUris);
  const uris = many ? uriOrUris : [uriOrUris];
  const { names, bytes } = issuerKeys(opts.keys);
  const now = passNow(opts);
  const res = uris.map(() => null);
  const batch = [];
  uris.forEach((uri, i) => {
    let p;
    try { p = nzcpInput.passSignatureInput(String(uri)); } catch (e) { res[i] = { ok: false, reason: PASS_REASONS.malformed }; return; }
    const key = names.indexOf(`${p.iss}#${p.kid}`);
    if (p.alg !== -7) res[i] = { ok: false, reason: PASS_REASONS.alg };
    else if (key < 0) res[i] = { ok: false, reason: PASS_REASONS.key };
    else batch.push({ i, p, key });
  });
  if (batch.length) {
    const ok = await native().es256VerifyBatch(bytes, Buffer.concat(batch.map((b) => b.p.digest)), Buffer.concat(batch.map((b) => b.p.signature)),
      keyIndexBuffer(batch.map((b) => b.key)), opts.device === undefined ? -1 : opts.device | 0);
    batch.forEach(({ i, p }, k) => {
      const reason = !ok[k] ? PASS_REASONS.signature : now < p.nbf ? PASS_REASONS.notYet : now >= p.exp ? PASS_REASONS.expired : null;
      res[i] = reason ? { ok: false, reason } : { ok: true, reason: null, claims: p.claims };
    });
  }
  return many ? res : res[0];
}

// nzcp.verifyPassBatch(uris, {keys, now, device = 0}) -> [{ok, reason, nbf, exp, toBeSignedSha256, credSubjSha256}]: the whole
// check of every pass -- text, base32, the COSE_Sign1 / CWT walk, the digests, the key lookup, the signature, nbf / exp -- in
// ONE g16_pass_verify_batch (include/g16_prover.h has the contract; device -1 = host threads).  The digests are hex
// strings, null where the pass is malformed or too long; credSubjSha256 is null too when the pass has no name or dob.
const PASS_BATCH_REASONS = [null, PASS_REASONS.malformed, PASS_REASONS.alg, PASS_REASONS.key, PASS_REASONS.signature,
  PASS_REASONS.notYet, PASS_REASONS.expired, PASS_REASONS.tooLong];
// the key table and the passes as the addon takes them: keys, "iss\0kid\0" per key, the text, the count + 1 offsets
function passBatchBuffers(uris, keys) {
  const { names, bytes } = issuerKeys(keys);
  const split = names.map((n) => { const at = n.lastIndexOf("#"); return [n.slice(0, Math.max(at, 0)), n.slice(at + 1)]; });
  const nameBytes = Buffer.concat(split.map(([iss, kid]) => Buffer.concat([Buffer.from(iss, "utf-8"), Buffer.from([0]), Buffer.from(kid, "utf-8"), Buffer.from([0])])));
  const texts = uris.map((u) => Buffer.from(String(u), "utf-8"));
  const offsets = Buffer.alloc((texts.length + 1) * 8);
  let at = 0;
  texts.forEach((t, i) => { at += t.length; offsets.writeBigUInt64LE(BigInt(at), (i + 1) * 8); });
  return { bytes, nameBytes, text: Buffer.concat(texts), offsets };
}
// one g16_pass_result record (96 bytes) as verifyPassBatch reports it
function passRecord(r) {
  const verdict = r.readUInt32LE(0), parsed = verdict !== 1 && verdict !== 7;
  return { ok: verdict === 0, reason: PASS_BATCH_REASONS[verdict], nbf: parsed ? Number(r.readBigInt64LE(16)) : null,
           exp: parsed ? Number(r.readBigInt64LE(24)) : null, toBeSignedSha256: parsed ? r.subarray(32, 64).toString("hex") : null,
           credSubjSha256: parsed && (r.readUInt32LE(12) & 1) ? r.subarray(64, 96).toString("hex") : null };
}
async function verifyPassBatch(uris, opts = {}) {
  const b = passBatchBuffers(uris, opts.keys);
  const out = await native().passVerifyBatch(b.bytes, b.nameBytes, b.text, b.offsets, passNow(opts), opts.device === undefined ? 0 : opts.device | 0);
  return uris.map((_, i) => passRecord(out.subarray(i * 96, (i + 1) * 96)));
}

// nzcp.provePasses(uris, {program, zkey, keys, now, unsigned, matchPublic, protocol = "groth16", device = 0}) ->
// [{outcome, text, pass, proof, publicSignals}]: the holder's side in ONE g16_pass_fullprove_batch (protocol "plonk": its
// twin) -- the check of verifyPassBatch, the circuit's input words formed on the GPU, the witnesses, the proofs.  outcome is
// one of PROVE_OUTCOMES; text words it (the violated check's text for "check"); pass is verifyPassBatch's entry; proof and
// publicSignals are null unless the outcome is "done".  unsigned: prove passes the relying party would refuse for their
// key, signature, nbf or exp (the circuit does not check the signature).  opts.rs / opts.blinding: TEST-ONLY fixed blinding.
const PROVE_OUTCOMES = ["done", "pass", "tooLong", "check", "mismatch"];
async function provePasses(uris, opts = {}) {
  const isPlonk = (opts.protocol || "groth16") === "plonk";
  if (!isPlonk && (opts.protocol || "groth16") !== "groth16") throw new Error(`nzcp prove: unknown protocol ${opts.protocol}`);
  if (!opts.program || !opts.zkey) throw new Error("nzcp prove: the program and the zkey are needed");
  const b = passBatchBuffers(uris, opts.keys);
  const flags = (opts.unsigned ? 1 : 0) | (opts.matchPublic ? 2 : 0);
  const one = isPlonk ? plonkBlinding(opts.blinding) : (opts.rs ? Buffer.concat([scalarToBuffer(opts.rs[0]), scalarToBuffer(opts.rs[1])]) : null);
  const res = native().passProveBatch(isPlonk, String(opts.program), toBuffer(opts.zkey, "zkey"), b.bytes, b.nameBytes, b.text, b.offsets,
    passNow(opts), flags, opts.device === undefined || opts.device === null ? 0 : opts.device | 0, one ? Buffer.concat(uris.map(() => one)) : null);
  return res.map((r) => {
    const pass = passRecord(r.record);
    const outcome = PROVE_OUTCOMES[r.outcome];
    const text = outcome === "done" ? null : outcome === "pass" ? pass.reason : outcome === "check" ? r.text
      : outcome === "tooLong" ? "ToBeSigned is longer than the circuit takes" : "the public signals are not the pass's digests and exp";
    return { outcome, text, pass, proof: r.proof ? (isPlonk ? plonkProofObject(r.proof) : proofObject(r.proof)) : null,
             publicSignals: r.pub ? publicSignals(r.pub) : null };
  });
}
// nzcp.passPublicSignals(result): the 513 public signals of NZCPPubIdentity for a pass, from one entry of verifyPassBatch:
// what nzcpInput.expectedPublicSignals(uri) returns
function passPublicSignals(result) {
  if (!result || !result.toBeSignedSha256 || !result.credSubjSha256) throw new Error("passPublicSignals: the pass has no digests (malformed, or without givenName / familyName / dob)");
  const bits = (hex) => Array.from(Buffer.from(hex, "hex")).flatMap((b) => [7, 6, 5, 4, 3, 2, 1, 0].map((k) => String((b >> k) & 1)));
  return bits(result.credSubjSha256).concat(bits(result.toBeSignedSha256), [String(result.exp)]);
}

// nzcp.verifyPassProof(vKey, [{proof, publicSignals, signature, iss, kid}], {keys, now, device = 0}) -> [{ok, reason}]: the
// Groth16 proofs and the pass signatures (64 bytes r | s each, forwarded by the prover) in one
// g16_nzcp_pass_proof_verify_batch; the digest a signature is checked against comes from the proof's public signals
async function verifyPassProof(vk, items, opts = {}) {
  const { names, bytes } = issuerKeys(opts.keys);
  const nPublic = Number(vk.nPublic);
  const res = items.map(() => null);
  const batch = [];
  items.forEach((it, i) => {
    const key = names.indexOf(`${it.iss}#${it.kid}`);
    const sig = Buffer.isBuffer(it.signature) ? it.signature : Buffer.from(it.signature || []);
    if (key < 0) res[i] = { ok: false, reason: PASS_REASONS.key };
    else if (sig.length !== 64) res[i] = { ok: false, reason: PASS_REASONS.signature };
    else if (!Array.isArray(it.publicSignals) || it.publicSignals.length !== nPublic) res[i] = { ok: false, reason: PASS_REASONS.proof };
    else batch.push({ i, it, key, sig });
  });
  if (batch.length) {
    const verdicts = await native().nzcpPassProofVerify(vkeyBytes(vk), nPublic, bytes, Buffer.concat(batch.map((b) => proofBytes(b.it.proof))),
      Buffer.concat(batch.map((b) => Buffer.concat(b.it.publicSignals.map(le32)))), Buffer.concat(batch.map((b) => b.sig)),
      keyIndexBuffer(batch.map((b) => b.key)), passNow(opts), opts.device | 0);
    batch.forEach(({ i }, k) => { res[i] = verdicts[k] === 0 ? { ok: true, reason: null } : { ok: false, reason: PASS_PROOF_VERDICTS[verdicts[k]] }; });
  }
  return res;
}

// nzcp.witnessProgram(params | "example" | "live", file): the witness program of NZCPPubIdentity(params) written to `file`
// (seconds at the full size: keep the file); nzcp.gadgetProgram(name, params, file): one template of the library
const NZCP_PARAMS = { example: [0, 314, 0, 4, 2, 4, 5], live: [1, 355, 0, 4, 2, 4, 6] };
const nzcp = {
  async witnessProgram(params, file) {
    const p = typeof params === "string" ? NZCP_PARAMS[params] : params;
    if (!Array.isArray(p) || p.length !== 7) throw new Error(`nzcp program: expected "example", "live" or seven template parameters`);
    native().nzcpProgramFile(p.map(Number), null, [], String(file));
  },
  async gadgetProgram(name, params, file) {
    native().nzcpProgramFile(null, String(name), (params || []).map(Number), String(file));
  },
  verifyPass,
  verifyPassBatch,
  passPublicSignals,
  verifyPassProof,
  provePasses,
  PASS_REASONS,
  PROVE_OUTCOMES,
};
// what the CLI prints for a failed check (modelled on later snarkjs, not compared with it)
function wtnsCheckReport(v) {
  return `WITNESS CHECKING FAILED\nconstraint ${v.constraint} is not satisfied (${v.nFailed} in all)\na = ${v.a}\nb = ${v.b}\nc = ${v.c}`;
}

const groth16 = {
  // snarkjs: groth16.verify(vk_verifier, publicSignals, proof[, logger]) -> boolean
  async verify(vk, publicSignals, proof, opts = {}) {
    const v = await createVerifier(vk, opts && typeof opts.debug === "function" ? {} : opts);
    try {
      return await v.verify(publicSignals, proof);
    } finally {
      v.close();
    }
  },
  createVerifier,
  // snarkjs: groth16.prove(zkeyFileName, witnessFileName[, logger]) -> {proof, publicSignals}
  async prove(zkey, wtns, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = { logger: opts };   // snarkjs passes a logger third
    const prover = await createProver(zkey, opts);
    try {
      return await prover.prove(wtns, opts);
    } finally {
      await prover.close();
    }
  },
  createProver,
  // snarkjs: groth16.fullProve(input, wasmFile, zkeyFileName) -> {proof, publicSignals}; the second argument is a witness
  // program (see wtns.calculate).  The witness never touches a file.  A violated check rejects with its text.
  async fullProve(input, programName, zkey, opts = {}) {
    if (opts && typeof opts.debug === "function") opts = { logger: opts };
    return groth16.prove(zkey, calculateWitness(input, programName, opts), opts);
  },
  // Many passes at once, the witnesses computed on the GPU and proved where they are (no snarkjs counterpart):
  // resolves to an array of {proof, publicSignals}, or {error: the violated check's text} for a pass whose input violates
  // a constraint.  opts.r / opts.s are TEST-ONLY, as in proveBatch: one blinding pair for every proof of the batch.
  async fullProveBatch(inputs, programName, zkey, opts = {}) {
    const r = scalarToBuffer(opts.r), s = scalarToBuffer(opts.s);
    const rs = r && s ? Buffer.concat(inputs.map(() => Buffer.concat([r, s]))) : null;
    return fullProveBatchNative(false, inputs, programName, zkey, opts, rs);
  },
};
// snarkjs: plonk.fullProve(input, wasmFile, zkeyFileName) -> {proof, publicSignals}; the second argument is a witness
// program (see wtns.calculate), the witness is computed on the GPU and never leaves it.  A violated check rejects with
// its text.  opts.blinding: the nine scalars b1..b9 (TEST-ONLY).  fullProveBatch: many passes, as groth16.fullProveBatch.
plonk.fullProve = async function fullProve(input, programName, zkey, opts = {}) {
  if (opts && typeof opts.debug === "function") opts = { logger: opts };
  const [res] = fullProveBatchNative(true, [input], programName, zkey, opts, plonkBlinding(opts.blinding));
  if (res.error !== undefined) throw new Error(res.error);
  return res;
};
plonk.fullProveBatch = async function fullProveBatch(inputs, programName, zkey, opts = {}) {
  const b = plonkBlinding(opts.blinding);
  return fullProveBatchNative(true, inputs, programName, zkey, opts, b ? Buffer.concat(inputs.map(() => b)) : null);
};

module.exports = { groth16, plonk, powersOfTau, wtns, nzcp, wtnsCheckReport, zKey: { exportVerificationKey, newZKey, csHash, contribute, beacon, exportBellman, bellmanContribute, importBellman, verifyFromInit, verifyFromR1cs }, formatHash, exportVerificationKey, newZKey, PlonkProver, plonkProofObject, createProver, Prover, createVerifier, Verifier, proofObject, publicSignals, proofBytes, vkeyBytes };
