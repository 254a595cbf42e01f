"""One resident g16_prover serves seven entry points that share its device state (proof context 0, the batch contexts,
the lazily read phase timings, the witness slots).  The Node host keeps one handle for its whole life, so what matters
is a proof made AFTER other entry points have used the same handle, or after an error raised once work was already on
the device.  Every proof here is compared with the oracles (the big-int prover, or the trapdoor known answer on the
2^12 key), never with the device alone:

  A. seeded random call sequences on one unsharded handle, checked against a model of what each slot holds;
  B. every entry point called between g16_shard_begin and g16_shard_end: refused with G16_E_STATE, or exact;
  C. the timing contract of g16_get_timings, after every step of A and B;
  D. recovery after errors raised once work is launched (g16_prove_batch, g16_multi_prove).

A failing sequence names its seed, step and history, so it can be replayed once by hand."""
import ctypes as C
import json
import math
import random

import pytest

import bn254 as b
import formats as f
import groth16 as g
import synth
from conftest import golden_path
from test_gpu_edges import _repeated_value_witness
from test_gpu_prove import domain_of, kat_secrets

try:   # a hang must name its test (the thread method also ends a hang inside a native call)
    import pytest_timeout  # noqa: F401
    _hang_marks = [pytest.mark.timeout(180, method="thread")]
except ImportError:
    _hang_marks = []

pytestmark = [pytest.mark.gpu] + _hang_marks

if not _hang_marks:
    import faulthandler

    @pytest.fixture(autouse=True)
    def _dump_on_hang():
        faulthandler.dump_traceback_later(180, exit=True)
        yield
        faulthandler.cancel_dump_traceback_later()

E_STATE = -5
IN_PROGRESS = "g16_shard_begin in progress"
RS = [(7, 9), (0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCD, b.R - 2)]


# ------------------------------------------------------------------------------------------------ keys and oracles
class Key:
    """A proving key, its witnesses and their expected proofs (each computed once per module)."""

    def __init__(self, name, zkey, witnesses, kat=None):
        self.name, self.zkey = name, zkey
        self.zk = f.read_zkey(zkey)
        self.n, self.p, self.N = self.zk["nVars"], self.zk["nPublic"], self.zk["domainSize"]
        self.w = witnesses                          # lists of ints
        self.wtns = [f.write_wtns(w) for w in witnesses]
        self.kat = kat or {}                        # witness index -> trapdoor secrets (satisfying synth witnesses)
        self._proof, self._abc = {}, {}

    def want(self, wi, ri):
        if (wi, ri) not in self._proof:
            r, s = RS[ri]
            w = self.w[wi]
            if wi in self.kat:
                pts = g.expected_proof(self.kat[wi], self.p, w, r, s)
            else:
                pts, _ = g.prove(self.zk, w, r, s)
            self._proof[(wi, ri)] = f.proof_obj(*pts)
        return self._proof[(wi, ri)], [str(x) for x in self.w[wi][1:self.p + 1]]

    def abc(self, wi):
        if wi not in self._abc:
            self._abc[wi] = g.build_abc(self.zk, self.w[wi])
        return self._abc[wi]


def _golden(name):
    zk = open(golden_path(name + ".zkey"), "rb").read()
    wt = open(golden_path(name + ".wtns"), "rb").read()
    return zk, wt, json.load(open(golden_path(name + ".json")))


@pytest.fixture(scope="module")
def keys(amd):
    out = {}
    # golden `small` (n = 150): its own witness, two more satisfying ones, one random non-satisfying assignment
    zk, wt, meta = _golden("small")
    n, p, m, seed = meta["n"], meta["p"], meta["m"], meta["seed"]
    rnd = random.Random(0x5a11)
    ws = [f.read_wtns(wt)["w"]] + [f.read_wtns(amd.synth_witness(n, p, m, seed, 700 + i))["w"] for i in range(2)]
    ws.append([1] + [rnd.randrange(b.R) for _ in range(n - 1)])
    out["small"] = Key("small", zk, ws)
    # a synth key on the 2^12 domain: two satisfying witnesses (trapdoor known answer) and one in the shape of the
    # repeated-value rows (big-int oracle); the H-MSM takes the single-pass binning at this size
    n, p, m, seed = 4000, 4, 3000, 91
    zkey, wtns0, _ = amd.synth_setup(n, p, m, seed)
    cls, rows, slack = synth.gen_circuit(n, p, m, seed)
    sec = kat_secrets(rows, n, p, m, seed, domain_of(m, p))
    sat = [synth.gen_witness(n, p, cls, rows, slack, ws_) for ws_ in (seed, 93)]
    assert f.write_wtns(sat[0]) == wtns0
    key = Key("syn12", zkey, sat + [_repeated_value_witness(n, 92)], kat={0: sec, 1: sec})
    assert key.N == 1 << 12
    out["syn12"] = key
    # nzcp513 (the sharded-pipeline key): its golden witness and two more
    zk, wt, meta = _golden("nzcp513")
    n, p, m, seed = meta["n"], meta["p"], meta["m"], meta["seed"]
    ws = [f.read_wtns(wt)["w"]] + [f.read_wtns(amd.synth_witness(n, p, m, seed, 800 + i))["w"] for i in range(2)]
    k = Key("nzcp513", zk, ws)
    k._proof[(0, "golden")] = meta["proof"]
    out["nzcp513"] = k
    return out


# ------------------------------------------------------------------------------------------------ C: timing contract
TFIELDS = ("upload_ms", "qap_ms", "ntt_ms", "msm_ms", "tail_ms", "total_ms", "msm_accum_kernel_ms")


def check_timings(pv, ctx, completed=False):
    """Read the timings twice and check what holds for any proof.  The events sit on the proof context's streams:
    ev[2] (start) -> ev[3] (QAP done) -> ev[4] (NTTs + join done) -> H-MSM [mev[1][0], mev[1][1]] -> ev[5] (end), all on
    the main stream, so qap + ntt + msm_ms[4] <= total; the accumulate kernels run inside their MSM's span on the same
    stream (H: [4] <= msm_ms[4]; the witness G1 lane: [0] <= msm_ms[0]); [1] and [3] are unused (one front end for A,
    B1, C).  `completed`: a proof has just completed on the handle."""
    t1, t2 = pv.timings(), pv.timings()
    assert t1 == t2, f"two reads differ: {t1} / {t2}\n{ctx}"
    flat = [x for k in TFIELDS for x in (t1[k] if isinstance(t1[k], list) else [t1[k]])]
    assert all(math.isfinite(x) and x >= 0 for x in flat), f"negative or non-finite timing: {t1}\n{ctx}"
    eps = 1e-3
    assert t1["qap_ms"] + t1["ntt_ms"] <= t1["total_ms"] + eps, f"{t1}\n{ctx}"
    assert t1["qap_ms"] + t1["ntt_ms"] + t1["msm_ms"][4] <= t1["total_ms"] + 2 * eps, f"{t1}\n{ctx}"
    assert t1["msm_accum_kernel_ms"][4] <= t1["msm_ms"][4] + eps, f"{t1}\n{ctx}"
    assert t1["msm_accum_kernel_ms"][0] <= t1["msm_ms"][0] + eps, f"{t1}\n{ctx}"
    assert t1["msm_ms"][1] == t1["msm_ms"][3] == 0 and t1["msm_accum_kernel_ms"][1] == t1["msm_accum_kernel_ms"][3] == 0
    if completed:
        assert t1["total_ms"] > 0, f"{t1}\n{ctx}"
    return t1


# ------------------------------------------------------------------------------------------------ raw batch call
def batch_raw(amd, pv, wtns_list, rs_idx, bufs=None):
    """g16_prove_batch over `wtns_list` (bytes, or ctypes buffers in `bufs`); returns (rc, proofs, publics)."""
    k = len(wtns_list)
    arr = (C.c_char_p * k)()
    for i, x in enumerate(bufs or wtns_list):
        arr[i] = C.cast(x, C.c_char_p) if bufs else x
    lens = (C.c_size_t * k)(*[len(x) for x in wtns_list])
    rs = b"".join(f.le(RS[ri][0]) + f.le(RS[ri][1]) for ri in rs_idx)
    out = (amd.Proof * k)()
    p = pv.info.n_public
    pub = C.create_string_buffer(max(1, k * p * 32))
    rc = amd.load().g16_prove_batch(pv._h, arr, lens, k, rs, out, pub)
    pubs = [[str(int.from_bytes(pub.raw[(i * p + j) * 32:(i * p + j + 1) * 32], "little")) for j in range(p)] for i in range(k)]
    return rc, [amd.proof_to_obj(o) for o in out], pubs


def _vec_bufs(amd, N):
    return [C.create_string_buffer(N * amd.LAZY_FR_BYTES) for _ in range(3)]


# ------------------------------------------------------------------------------------------------ A: model-based sequences
def _run_sequence(amd, key, seed, nops=30):
    rnd = random.Random(seed)
    pv = amd.Prover(key.zkey)
    N, nw = key.N, len(key.w)
    vecs = _vec_bufs(amd, N)
    slots = {}                                   # the model: slot -> witness index
    hist = []

    def ctx():
        return f"key {key.name} seed {seed} step {len(hist) - 1}\nhistory: {hist}"

    def check_proof(got, wi, ri, what):
        want, pub = key.want(wi, ri)
        assert got[0] == want, f"{what}: proof differs from the oracle's\n{ctx()}"
        assert got[1] == pub, f"{what}: public signals differ\n{ctx()}"

    ops = ["stage"] * 4 + ["staged"] * 3 + ["prove"] * 3 + ["batch"] * 3 + ["partial"] * 3 + ["shard"] * 3 + ["qap", "timings"]
    for _ in range(nops):
        op = rnd.choice(ops)
        if op in ("staged", "partial", "shard", "qap") and not slots:
            op = "stage"
        ri = rnd.randrange(len(RS))
        r, s = f.le(RS[ri][0]), f.le(RS[ri][1])
        done = False
        if op == "stage":
            slot, wi = rnd.randrange(3), rnd.randrange(nw)
            hist.append(("stage", slot, wi))
            pv.stage(slot, key.wtns[wi])
            slots[slot] = wi
        elif op == "staged":
            slot = rnd.choice(sorted(slots))
            hist.append(("prove_staged", slot, ri))
            check_proof(pv.prove_staged(slot, r, s), slots[slot], ri, "prove_staged")
            done = True
        elif op == "prove":
            wi = rnd.randrange(nw)
            hist.append(("prove", wi, ri))
            check_proof(pv.prove(key.wtns[wi], r, s), wi, ri, "prove")
            slots[0] = wi                        # g16_prove stages its witness in slot 0
            done = True
        elif op == "batch":
            wis = [rnd.randrange(nw) for _ in range(rnd.randint(1, 7))]
            ris = [rnd.randrange(len(RS)) for _ in wis]
            hist.append(("batch", wis, ris))
            rc, proofs, pubs = batch_raw(amd, pv, [key.wtns[i] for i in wis], ris)
            assert rc == 0, f"batch: {amd.load().g16_last_error()}\n{ctx()}"
            for j, (wi, rj) in enumerate(zip(wis, ris)):
                check_proof((proofs[j], pubs[j]), wi, rj, f"batch[{j}]")
            done = True
        elif op == "partial":
            slot = rnd.choice(sorted(slots))
            hist.append(("partial+finish", slot, ri))
            part = pv.prove_partial(slot)
            check_proof(pv.prove_finish(slot, [part], r, s), slots[slot], ri, "prove_partial")
            done = True
        elif op == "shard":
            slot = rnd.choice(sorted(slots))
            hist.append(("shard_begin+end+finish", slot, ri))
            pv.shard_begin(slot, 7, [C.addressof(v) for v in vecs])
            part = pv.shard_end(slot, [C.addressof(v) for v in vecs])
            check_proof(pv.prove_finish(slot, [part], r, s), slots[slot], ri, "shard_begin/shard_end")
            done = True
        elif op == "qap":
            slot = rnd.choice(sorted(slots))
            hist.append(("qap_eval", slot))
            got = pv.qap_eval(slot)
            rinv = pow(b.MONT, -1, b.R)
            for name, gv, ev in zip("ABC", got, key.abc(slots[slot])):
                assert [x * rinv % b.R for x in gv] == ev, f"qap_eval: {name}_T differs from buildABC1\n{ctx()}"
        else:
            hist.append(("timings",))
        check_timings(pv, ctx(), completed=done)
    pv.close()


@pytest.mark.parametrize("nctx", [None, "1", "2"])
@pytest.mark.parametrize("seed", [101, 202, 303])
@pytest.mark.parametrize("name", ["small", "syn12"])
def test_call_sequences_match_the_model(amd, keys, monkeypatch, name, seed, nctx):
    """~30 seeded operations on ONE resident unsharded handle (G16_BATCH_CTX read at create): staged / single / batch /
    partial / begin-end proofs, QAP evaluations and timing reads in any order; every result is the oracle's."""
    if nctx:
        monkeypatch.setenv("G16_BATCH_CTX", nctx)
    _run_sequence(amd, keys[name], seed * 10 + (int(nctx) if nctx else 0))


# ------------------------------------------------------------------------------------------------ B: calls between begin and end
CALLS = ["prove_partial_other", "prove_staged_other", "prove", "batch", "qap_eval_other", "shard_begin_again",
         "stage_begun", "stage_other", "get_info", "timings", "prove_finish"]


class ShardSet:
    """The handles of one test of B: one unsharded handle, or the three shards of nzcp513 (the calls go to shard 1).
    Slot 0 holds w1 (witness 0), slot 1 holds w2 (witness 1)."""

    def __init__(self, amd, key, count):
        self.amd, self.key, self.count = amd, key, count
        self.pvs = [amd.Prover(key.zkey, shard_rank=k, shard_count=count) for k in range(count)]
        self.me = 1 if count > 1 else 0
        self.vecs = _vec_bufs(amd, key.N)
        for pv in self.pvs:
            pv.stage(0, key.wtns[0])
            pv.stage(1, key.wtns[1])
        # the partial sums of w2 from every shard, to finish a partial of the tested shard with
        self.parts_w2 = [pv.prove_partial(1) for pv in self.pvs]

    @property
    def pv(self):
        return self.pvs[self.me]

    def mask(self, k):
        return sum(1 << v for v in range(3) if v % self.count == k)

    def begin(self, k, slot):
        m = self.mask(k)
        self.pvs[k].shard_begin(slot, m, [C.addressof(self.vecs[v]) if (m >> v) & 1 else 0 for v in range(3)])

    def end(self, k, slot):
        lo, hi = self.amd.shard_range(self.key.N, k, self.count)
        eb = self.amd.LAZY_FR_BYTES
        sl = [C.create_string_buffer(self.vecs[v].raw[lo * eb:hi * eb], max(1, (hi - lo) * eb)) for v in range(3)]
        return self.pvs[k].shard_end(slot, [C.addressof(x) for x in sl])

    def whole(self, slot, ri):
        """begin on every shard, end on every shard, finish: the proof of the witness in `slot`."""
        for k in range(self.count):
            self.begin(k, slot)
        parts = [self.end(k, slot) for k in range(self.count)]
        r, s = RS[ri]
        return self.pvs[-1].prove_finish(slot, parts, f.le(r), f.le(s))

    def close(self):
        for pv in self.pvs:
            pv.close()


def _call(S, call, ctx):
    """Run `call` on the tested handle and check its own result (exact, or refused: the caller checks the refusal)."""
    amd, key, pv = S.amd, S.key, S.pv
    r, s = f.le(RS[0][0]), f.le(RS[0][1])
    want_w2 = key.want(1, 0)
    if call == "prove_partial_other":
        part = pv.prove_partial(1)
        parts = list(S.parts_w2)
        parts[S.me] = part
        assert pv.prove_finish(1, parts, r, s) == want_w2, f"partial of w2 is wrong\n{ctx}"
    elif call == "prove_staged_other":
        assert pv.prove_staged(1, r, s) == want_w2, ctx
    elif call == "prove":
        assert pv.prove(key.wtns[1], r, s) == want_w2, ctx
        pv.stage(0, key.wtns[0])        # g16_prove staged w2 in slot 0: put w1 back
    elif call == "batch":
        rc, proofs, pubs = batch_raw(amd, pv, [key.wtns[1], key.wtns[2], key.wtns[1], key.wtns[2]], [0, 1, 0, 1])
        if rc:
            raise amd.G16Error(rc, amd.load().g16_last_error().decode())
        for j, (wi, ri) in enumerate([(1, 0), (2, 1), (1, 0), (2, 1)]):
            assert (proofs[j], pubs[j]) == key.want(wi, ri), f"batch[{j}]\n{ctx}"
    elif call == "qap_eval_other":
        got = pv.qap_eval(1)
        rinv = pow(b.MONT, -1, b.R)
        assert [[x * rinv % b.R for x in gv] for gv in got] == [list(v) for v in key.abc(1)], ctx
    elif call == "shard_begin_again":
        S.begin(S.me, 1)
        return "begun"
    elif call == "stage_begun":
        pv.stage(0, key.wtns[1])
        return "staged"
    elif call == "stage_other":
        pv.stage(1, key.wtns[2])
        pv.stage(1, key.wtns[1])
    elif call == "get_info":
        inf = amd.Info()
        assert amd.load().g16_get_info(pv._h, C.byref(inf)) == 0
        assert (inf.n_vars, inf.n_public, inf.domain_size) == (key.n, key.p, key.N), ctx
    elif call == "timings":
        pv.timings()
    elif call == "prove_finish":
        assert pv.prove_finish(1, S.parts_w2, r, s) == want_w2, ctx
    return None


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("shards", [1, 3])
def test_every_call_between_shard_begin_and_end(amd, keys, shards, call):
    """stage slot 0 = w1, slot 1 = w2; shard_begin(0); C; shard_end(0); prove_finish == w1's oracle proof.  C is refused
    with G16_E_STATE naming the shard in progress, or returns its own exact result; a refused C succeeds after the end.
    Timing reads in between return the last completed proof's struct (the first one made only after the begin).  Once on an unsharded handle, once on shard 1 of
    a 3-shard nzcp513 set (only shard 1 sees C)."""
    key = keys["nzcp513"]
    S = ShardSet(amd, key, shards)
    ctx = f"shards={shards} call={call}"
    want_w1 = (key._proof[(0, "golden")], [str(x) for x in key.w[0][1:key.p + 1]])
    assert S.pvs[-1].prove_finish(1, S.parts_w2, f.le(RS[0][0]), f.le(RS[0][1])) == key.want(1, 0)
    meta = json.load(open(golden_path("nzcp513.json")))
    rg = int(meta["r"]), int(meta["s"])
    # (no read between the last proof and the begin: the first read after it must still be that proof's)
    for k in range(shards):
        S.begin(k, 0)
    t0 = check_timings(S.pv, ctx + " (after begin)", completed=True)
    refused = False
    state = None
    try:
        state = _call(S, call, ctx)
    except amd.G16Error as e:
        refused = True
        sharded_refusal = shards > 1 and call in ("prove_staged_other", "prove", "batch") and "sharded handle" in str(e)
        assert e.code == E_STATE and (IN_PROGRESS in str(e) or sharded_refusal), f"{ctx}: refused with {e.code} {e}"
        assert check_timings(S.pv, ctx + " (after the refusal)") == t0
    assert not (call == "shard_begin_again" and not refused and state), \
        "a second g16_shard_begin while one is in progress was accepted"
    assert not (call == "stage_begun" and not refused and state), \
        "g16_stage_witness on the slot of the shard in progress was accepted"
    if call in ("get_info", "timings", "prove_finish"):
        assert not refused, f"{call} is host-only and stays allowed between begin and end"
        assert check_timings(S.pv, ctx) == t0
    parts = [S.end(k, 0) for k in range(shards)]
    got = S.pvs[-1].prove_finish(0, parts, f.le(rg[0]), f.le(rg[1]))
    assert got == want_w1, f"{ctx}: the begun proof is not w1's"
    check_timings(S.pv, ctx + " (after end)", completed=True)
    if refused:     # allowed again after the end, and exact
        try:
            state = _call(S, call, ctx + " (after end)")
        except amd.G16Error as e:
            assert shards > 1 and "sharded handle" in str(e), f"{ctx}: still refused after the end: {e}"
        if state == "begun":
            for k in range(shards):
                if k != S.me:
                    S.begin(k, 1)
            parts = [S.end(k, 1) for k in range(shards)]
            assert S.pvs[-1].prove_finish(1, parts, f.le(RS[0][0]), f.le(RS[0][1])) == key.want(1, 0), ctx
        elif state == "staged":
            for pv in S.pvs:
                pv.stage(0, key.wtns[1])
            assert S.whole(0, 0) == key.want(1, 0), ctx
            for pv in S.pvs:
                pv.stage(0, key.wtns[0])
    # and the handle still proves w1 exactly
    assert S.whole(0, 1) == key.want(0, 1), ctx
    check_timings(S.pv, ctx + " (final)", completed=True)
    S.close()


# ------------------------------------------------------------------------------------------------ D: recovery after launched errors
def _bad_word(wt):
    bad = bytearray(wt)
    pos, _ = f.read_binfile(wt, "wtns", 2)[2][0]
    bad[pos + 32 * 5:pos + 32 * 6] = f.le(b.R + 3)
    return bytes(bad)


@pytest.mark.parametrize("nctx", [None, "1", "2"])
@pytest.mark.parametrize("kind", ["format", "not_reduced"])
def test_batch_error_at_position_3_of_6_leaves_the_handle_exact(amd, keys, monkeypatch, kind, nctx):
    """g16_prove_batch fails at position 3 of 6: a malformed file (refused on the host, with proofs 0..2 in flight) or a
    word >= r (the device's verdict, after later proofs were launched).  The caller overwrites its witness buffers as
    soon as the call returns; then a full batch and single proofs on the same handle are exact, a failed single proof
    leaves the timings of the last completed one, and the timing contract holds throughout."""
    if nctx:
        monkeypatch.setenv("G16_BATCH_CTX", nctx)
    key = keys["syn12"]
    pv = amd.Prover(key.zkey)
    ctx = f"kind={kind} nctx={nctx}"
    seq = [0, 1, 2, 0, 1, 2]
    wts = [key.wtns[i] for i in seq]
    wts[3] = b"zkey" + wts[3][4:] if kind == "format" else _bad_word(wts[3])
    bufs = [C.create_string_buffer(w, len(w)) for w in wts]
    rc, _, _ = batch_raw(amd, pv, wts, [0] * 6, bufs=bufs)
    err = amd.load().g16_last_error().decode()
    for x in bufs:                      # the caller reuses its buffers at once
        C.memset(x, 0xA5, len(x))
    if kind == "format":
        assert rc == -2 and "Invalid File format" in err, (rc, err)
    else:
        assert rc == -2 and "signal 5 is not reduced" in err, (rc, err)
    check_timings(pv, ctx)
    rc, proofs, pubs = batch_raw(amd, pv, [key.wtns[i] for i in seq], [0, 1, 0, 1, 0, 1])
    assert rc == 0, amd.load().g16_last_error()
    for j, wi in enumerate(seq):
        assert (proofs[j], pubs[j]) == key.want(wi, j % 2), f"{ctx}: batch[{j}]"
    t0 = check_timings(pv, ctx, completed=True)
    with pytest.raises(amd.G16Error, match="signal 5 is not reduced"):
        pv.prove(_bad_word(key.wtns[1]), f.le(RS[0][0]), f.le(RS[0][1]))
    assert check_timings(pv, ctx + " (after a failed proof)") == t0
    for wi in (2, 0):
        assert pv.prove(key.wtns[wi], f.le(RS[1][0]), f.le(RS[1][1])) == key.want(wi, 1), ctx
        check_timings(pv, ctx, completed=True)
    pv.close()


def test_multi_prove_after_a_non_reduced_word(amd, keys):
    """g16_multi_prove with a word >= r: the verdict comes after the shards ran; the next proofs are the golden one."""
    key = keys["nzcp513"]
    zk, wt, meta = _golden("nzcp513")
    r, s = f.le(int(meta["r"])), f.le(int(meta["s"]))
    mp = amd.MultiProver(zk, [0, 0])
    with pytest.raises(amd.G16Error, match="signal 5 is not reduced"):
        mp.prove(_bad_word(wt), r, s)
    for _ in range(2):
        assert mp.prove(wt, r, s) == (meta["proof"], meta["public"])
    assert mp.prove(key.wtns[1], f.le(RS[0][0]), f.le(RS[0][1])) == key.want(1, 0)
    mp.close()


def test_multi_prove_task_buffer_overflow_is_an_error(amd, monkeypatch):
    """A g16_multi whose bucket-task buffers are forced too small (test hook G16_TEST_MAX_TASKS, read at create): every
    call returns G16_E_STATE "bucket tasks" and returns (the H lanes drained as well); a fresh handle on the same key
    then gives the golden proof.  The single-handle twin is test_task_buffer_overflow_is_an_error_not_a_fault."""
    zk, wt, meta = _golden("nzcp513")
    r, s = f.le(int(meta["r"])), f.le(int(meta["s"]))
    monkeypatch.setenv("G16_TEST_MAX_TASKS", "16")
    small = amd.MultiProver(zk, [0, 0])
    monkeypatch.delenv("G16_TEST_MAX_TASKS")
    for _ in range(2):
        with pytest.raises(amd.G16Error) as e:
            small.prove(wt, r, s)
        assert e.value.code == E_STATE and "bucket tasks" in str(e.value), e.value
    small.close()
    mp = amd.MultiProver(zk, [0, 0])
    assert mp.prove(wt, r, s) == (meta["proof"], meta["public"])
    mp.close()


# ------------------------------------------------------------------------------------------------ E: create ... destroy, over and over
# Every device resource of the prover handles is an owner (csrc/device_job.h) that releases itself when the handle goes.
# What a handle must not do is keep a share of itself, or hand the next handle a device in another state: four handles
# in a row on one key give the same bytes, and the device's free memory comes back.
def _free_bytes(amd):
    """Free memory of the current device once it is idle: hipMemGetInfo, which torch.cuda.mem_get_info() wraps, read
    through the HIP runtime the library itself is linked with (torch's bundled runtime, loaded after the library's in
    this process, sees no device: see __graft_entry__.smoke)."""
    lib = amd.load()
    free, total = C.c_size_t(), C.c_size_t()
    assert lib.hipDeviceSynchronize() == 0
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def _four_cycles(amd, cycle, what):
    """cycle() = create -> stage -> prove -> destroy with fixed blinding; `cycle(probe)` calls probe() while its handle
    is live.  Returns cycle 1's result after checking that cycles 2 to 4 equal it, and that the device's free memory
    after cycle 4 is below that after cycle 1 (the warm-up) by at most F / 2, F = what one live handle takes (measured in
    cycle 2: free before its create minus free with the handle live).  A handle that leaks itself costs 3 F."""
    free_after, live = [], []
    results = []
    for k in range(4):
        before = _free_bytes(amd)
        results.append(cycle(lambda: live.append(before - _free_bytes(amd))))
        free_after.append(_free_bytes(amd))
    for k in range(1, 4):
        assert results[k] == results[0], f"{what}: cycle {k + 1} differs from cycle 1"
    F, drift = live[1], free_after[0] - free_after[3]
    print(f"{what}: a live handle takes F = {F} bytes (cycles: {live}); free memory after each cycle {free_after}, "
          f"drift from cycle 1 to cycle 4 = {drift} bytes")
    assert F > 0, f"{what}: a live handle takes no device memory ({live})"
    assert drift <= F / 2, f"{what}: free memory fell by {drift} bytes over cycles 2 to 4, a live handle takes {F}"
    return results[0]


def _g16_cycle(amd, key):
    def cycle(probe):
        pv = amd.Prover(key.zkey)
        pv.stage(0, key.wtns[0])
        got = pv.prove_staged(0, f.le(RS[1][0]), f.le(RS[1][1]))
        probe()
        pv.close()
        return got
    return cycle


def _g16_verifies(key, got):
    pr, pub = got
    return g.verify(key.zk, [int(x) for x in pub], (f.g1_from_obj(pr["pi_a"]), f.g2_from_obj(pr["pi_b"]), f.g1_from_obj(pr["pi_c"])))


@pytest.mark.parametrize("env", [("G16_BATCH_CTX", "1"), ("G16_BATCH_CTX", "3"), ("G16_SERIAL_MSM", "1"), ("G16_ROWS_COPY", "1")],
                         ids=lambda e: "=".join(e))
def test_groth16_create_prove_destroy_four_times(amd, keys, monkeypatch, env):
    """With one and three proof contexts, with the MSM streams aliased to the main stream (G16_SERIAL_MSM) and with the
    lanes' row sums in a device buffer of their own (G16_ROWS_COPY): all read at create."""
    monkeypatch.setenv(*env)
    key = keys["small"]
    got = _four_cycles(amd, _g16_cycle(amd, key), "groth16 " + "=".join(env))
    assert got == key.want(0, 1) and _g16_verifies(key, got)


def test_plonk_create_prove_destroy_four_times(amd):
    import plonk as pk
    zkey, wtns, meta = _golden("plonk_small")

    def cycle(probe):
        pv = amd.PlonkProver(zkey)
        got = pv.prove(wtns, [int(x) for x in meta["blinding"]])
        probe()
        pv.close()
        return got
    proof, pub = _four_cycles(amd, cycle, "plonk")
    assert (proof, pub) == (meta["proof"], meta["public"])
    assert pk.verify(pk.vkey_from_zkey(zkey), [int(x) for x in pub], pk.proof_from_obj(proof))


def test_multi_create_prove_destroy_four_times(amd, keys):
    """g16_multi with two shards on device 0 (its events and both shard handles go with it)."""
    key = keys["small"]

    def cycle(probe):
        mp = amd.MultiProver(key.zkey, [0, 0])
        got = mp.prove(key.wtns[0], f.le(RS[1][0]), f.le(RS[1][1]))
        probe()
        mp.close()
        return got
    got = _four_cycles(amd, cycle, "multi")
    assert got == key.want(0, 1) and _g16_verifies(key, got)


def test_destroy_with_a_proof_in_flight(amd, keys):
    """g16_shard_begin on a one-shard handle enqueues a proof and returns with the witness MSMs still running; the handle
    is destroyed without g16_shard_end.  A legal sequence: the handle's streams are waited for before what their work
    touches is freed, the call returns, and a fresh handle proves exactly."""
    key = keys["small"]
    vecs = _vec_bufs(amd, key.N)
    pv = amd.Prover(key.zkey)
    pv.stage(0, key.wtns[0])
    pv.shard_begin(0, 7, [C.addressof(v) for v in vecs])
    pv.close()
    got = _g16_cycle(amd, key)(lambda: None)
    assert got == key.want(0, 1) and _g16_verifies(key, got)
