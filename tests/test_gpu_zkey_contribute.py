"""`zkey contribute` and `zkey verify frominit` on the device (csrc/zkey_mpc.cpp, csrc/zkey_scale.hip).  A contribution
with a KNOWN d to the ptau route's fresh key must give, byte for byte, the trapdoor key of the Python oracle with
delta = d (sections 1-9) and the twin's section 10 and hash (tests/zkey_mpc_ref.py); the verifier accepts honest chains
and names what is wrong with tampered ones."""
import pytest

import bn254 as b
import formats as f
import groth16 as g
import synth
import zkey_mpc_ref as ref
from bn254 import R

pytestmark = pytest.mark.gpu

CASES = {"small": (24, 2, 12, 1), "mid": (150, 6, 120, 2), "large": (1000, 513, 400, 5)}
S = 0x0123456789abcdef ** 3 % R
D1, D2 = 0x1f2e3d4c5b6a7988 ** 3 % R, 0x2b3f5d7c9e1a3b5c ** 3 % R
_cache = {}


def _case(amd, name):
    """rows, witness, trapdoor (gamma = delta = 1), the ptau route's fresh key and the oracle's key for it, once."""
    if name not in _cache:
        n, p, m, seed = CASES[name]
        rows, w = synth.make(n, p, m, seed)
        t = g.trapdoor(seed + 1000)
        td = {"tau": t["tau"], "alpha": t["alpha"], "beta": t["beta"], "gamma": 1, "delta": 1}
        L = 0
        while (1 << L) < m + p + 1:
            L += 1
        ptau = amd.ptau_synth(L, td["tau"], td["alpha"], td["beta"], device=0)
        init = amd.groth16_setup_ptau(f.write_r1cs(n, p, 0, rows), ptau, device=0)
        zk, sec = g.setup(n, p, rows, td)
        _cache[name] = {"n": n, "p": p, "rows": rows, "w": w, "td": td, "init": init, "zk": zk, "sec": sec}
    return _cache[name]


def _oracle_key(c, delta):
    """f.write_zkey(g.setup(n, p, rows, td with delta)): only delta1, delta2, C and H depend on delta, so the cached
    delta = 1 setup is reused and those four are recomputed with g.setup's own formulas."""
    zk, sec, p, n = dict(c["zk"]), c["sec"], c["p"], c["n"]
    N = zk["domainSize"]
    dinv = pow(delta, -1, R)
    kk = [(sec["beta"] * sec["u"][i] + sec["alpha"] * sec["v"][i] + sec["t"][i]) % R for i in range(n)]
    L2 = g.lagrange_at(2 * N, sec["tau"])
    zk["delta1"] = b.G1.mul(b.G1_GEN, delta)
    zk["delta2"] = b.G2.mul(b.G2_GEN, delta)
    zk["C"] = b.G1.gen_mul_many([kk[i] * dinv % R for i in range(p + 1, n)])
    zk["H"] = b.G1.gen_mul_many([L2[2 * i + 1] * dinv % R for i in range(N)])
    return f.write_zkey(zk)


def _sections(buf):
    secs = f.read_binfile(buf, "zkey", 2)
    return {sid: f.section(buf, secs, sid) for sid in secs}


def _rewrite(buf, repl):
    secs = f.read_binfile(buf, "zkey", 2)
    order = sorted(secs, key=lambda sid: secs[sid][0][0])
    return f.write_binfile("zkey", 1, [(sid, repl.get(sid, f.section(buf, secs, sid))) for sid in order])


def _assert_is_trapdoor_key(new, want):
    got, exp = _sections(new), _sections(want)
    assert sorted(got) == sorted(exp) == list(range(1, 11))
    for sid in range(1, 10):
        assert got[sid] == exp[sid], f"section {sid}"


def _proves(amd, c, key):
    prover = amd.Prover(key, device=0)
    proof, pub = prover.prove(f.write_wtns(c["w"]))
    prover.close()
    pts = (f.g1_from_obj(proof["pi_a"]), f.g2_from_obj(proof["pi_b"]), f.g1_from_obj(proof["pi_c"]))
    return g.verify(f.read_zkey(key), [int(x) for x in pub], pts)


@pytest.fixture(scope="module")
def chain(amd):
    """The small case's fresh key, one contribution (D1) and two (D1, D2), and a one-contribution key with another d."""
    c = _case(amd, "small")
    one, h1 = amd.zkey_contribute(c["init"], "first", D1, S, device=0)
    two, h2 = amd.zkey_contribute(one, "second", D2, S + 1, device=0)
    other, _ = amd.zkey_contribute(c["init"], "first", D1 + 5, S, device=0)
    return {"c": c, "init": c["init"], "one": one, "two": two, "other": other, "h1": h1, "h2": h2}


# ------------------------------------------------------------------ 1. equals the trapdoor key
@pytest.mark.parametrize("name", list(CASES))
def test_contributed_key_equals_trapdoor_key_and_proves(amd, name):
    c = _case(amd, name)
    new, chash = amd.zkey_contribute(c["init"], "first", D1, S, device=0)
    _assert_is_trapdoor_key(new, _oracle_key(c, D1))
    want_h, want_s10, want_hash = ref.contribute_ref(c["init"], "first", D1, S)
    got = _sections(new)
    assert got[2] == want_h and got[10] == want_s10 and chash == want_hash
    assert _proves(amd, c, new)


# ------------------------------------------------------------------ 2. multiplier edges
EDGES = [1, 2, 3, R - 1, R - 2, R - 3, 1 << 128, (1 << 128) - 1, 1 << 253,
         int("5" * 64, 16) % R, int("a" * 64, 16) % R, R // 2, R // 2 + 1]


@pytest.mark.parametrize("k", EDGES, ids=lambda k: "k%x" % k)
def test_multiplier_edges(amd, k):
    """d = 1 / k: the kernel multiplies by k itself -- every digit pattern, long carry runs, the top window with and
    without a carry."""
    c = _case(amd, "mid")
    d = pow(k, -1, R)
    new, chash = amd.zkey_contribute(c["init"], None, d, S, device=0)
    _assert_is_trapdoor_key(new, _oracle_key(c, d))
    want_h, want_s10, want_hash = ref.contribute_ref(c["init"], None, d, S)
    got = _sections(new)
    assert got[2] == want_h and got[10] == want_s10 and chash == want_hash


# ------------------------------------------------------------------ 3. infinity and the grid's tail
def test_unused_private_wire_stays_infinity(amd):
    n, p = 6, 1
    rows = [([(2, 1)], [(3, 1)], [(4, 1)]), ([(1, 1)], [(2, 5)], [(3, R - 2)])]   # wire 5 appears in no row
    td = g.trapdoor(77)
    ptau = amd.ptau_synth(2, td["tau"], td["alpha"], td["beta"], device=0)
    init = amd.groth16_setup_ptau(f.write_r1cs(n, p, 0, rows), ptau, device=0)
    at = (5 - p - 1) * 64
    assert _sections(init)[8][at:at + 64] == bytes(64)
    new, _ = amd.zkey_contribute(init, None, D1, S, device=0)
    s8 = _sections(new)[8]
    assert s8[at:at + 64] == bytes(64)
    assert all(s8[i:i + 64] != bytes(64) for i in range(0, len(s8), 64) if i != at)
    zk, _ = g.setup(n, p, rows, dict(td, gamma=1, delta=D1))
    _assert_is_trapdoor_key(new, f.write_zkey(zk))
    ok, why = amd.zkey_verify_from_init(init, new, device=0)
    assert ok, why


@pytest.mark.parametrize("env", [{"G16_CONTRIBUTE_LANES": "192"},
                                 {"G16_CONTRIBUTE_LANES": "64", "G16_CONTRIBUTE_CHUNK": "200"},
                                 {"G16_CONTRIBUTE_LANES": "64", "G16_CONTRIBUTE_CHUNK": "243"}],
                         ids=["lanes192", "lanes64_chunk200", "lanes64_chunk243"])
def test_grid_stride_passes_and_chunks_give_the_same_bytes(amd, monkeypatch, env):
    """486 + 512 points on 192 lanes: six grid-stride passes with a ragged tail; on 64 lanes in chunks of 200 points:
    three chunks per section over the two buffer sets, the last one short; in chunks of 243: section 8 is exactly two full
    chunks, section 9 two and a tail of 26."""
    c = _case(amd, "large")
    whole, _ = amd.zkey_contribute(c["init"], "first", D1, S, device=0)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    again, _ = amd.zkey_contribute(c["init"], "first", D1, S, device=0)
    assert again == whole


@pytest.mark.parametrize("win", ["3", "4", "5"])
def test_every_window_width_gives_the_same_bytes(amd, monkeypatch, win):
    """G16_CONTRIBUTE_WINDOW: the table of odd multiples has 2, 4 or 8 entries; multiplier r - 2 (d = 1 / (r - 2))."""
    c = _case(amd, "mid")
    d = pow(R - 2, -1, R)
    monkeypatch.setenv("G16_CONTRIBUTE_WINDOW", win)
    new, _ = amd.zkey_contribute(c["init"], None, d, S, device=0)
    _assert_is_trapdoor_key(new, _oracle_key(c, d))


# ------------------------------------------------------------------ 4. chain
def test_two_contributions(amd, chain):
    c = chain["c"]
    _assert_is_trapdoor_key(chain["two"], _oracle_key(c, D1 * D2 % R))
    cs, recs = ref.parse_section10(_sections(chain["two"])[10])
    assert len(recs) == 2 and recs[0]["raw"] == ref.parse_section10(_sections(chain["one"])[10])[1][0]["raw"]
    assert recs[1]["transcript"] == ref.transcript_hash(cs, recs[:1], recs[1]["g1_s"], recs[1]["g1_sx"])
    assert recs[1]["transcript"] != ref.transcript_hash(cs, [], recs[1]["g1_s"], recs[1]["g1_sx"])
    want_h, want_s10, want_hash = ref.contribute_ref(chain["one"], "second", D2, S + 1)
    got = _sections(chain["two"])
    assert got[2] == want_h and got[10] == want_s10 and chain["h2"] == want_hash
    assert _proves(amd, c, chain["two"])


# ------------------------------------------------------------------ 5. verify accepts
@pytest.mark.parametrize("which", ["init", "one", "two"])
def test_verify_accepts(amd, chain, which):
    ok, why = amd.zkey_verify_from_init(chain["init"], chain[which], device=0)
    assert ok and why == "", why


def test_verify_accepts_from_a_contributed_start(amd, chain):
    ok, why = amd.zkey_verify_from_init(chain["one"], chain["two"], device=0)
    assert ok, why


# ------------------------------------------------------------------ 6. verify rejects
def _swap(buf, i, j, size):
    x = bytearray(buf)
    x[i * size:(i + 1) * size], x[j * size:(j + 1) * size] = buf[j * size:(j + 1) * size], buf[i * size:(i + 1) * size]
    return bytes(x)


def _tampered(chain):
    one, two, other = _sections(chain["one"]), _sections(chain["two"]), _sections(chain["other"])
    s9 = one[9]
    i, j = [k for k in range(len(s9) // 64) if s9[k * 64:(k + 1) * 64] != bytes(64)][:2]
    assert s9[i * 64:(i + 1) * 64] != s9[j * 64:(j + 1) * 64]
    out = {"s9_swapped": ("one", {9: _swap(s9, i, j, 64)})}
    s8 = one[8]
    out["s8_overwritten"] = ("one", {8: s8[:64] + s8[:64] + s8[128:]})
    assert s8[:64] != s8[64:128] and s8[:64] != bytes(64)
    out["delta2_of_another_d"] = ("one", {2: one[2][:ref.HDR_DELTA2] + other[2][ref.HDR_DELTA2:]})
    r0 = 68
    out["g2_spx_of_another_d"] = ("one", {10: one[10][:r0 + 192] + other[10][r0 + 192:r0 + 320] + one[10][r0 + 320:]})
    flipped = bytearray(one[10])
    flipped[r0 + 320 + 7] ^= 0x10
    out["transcript_byte"] = ("one", {10: bytes(flipped)})
    _, recs = ref.parse_section10(two[10])
    out["records_swapped"] = ("two", {10: two[10][:68] + recs[1]["raw"] + recs[0]["raw"]})
    a = one[5]
    i, j = [k for k in range(len(a) // 64) if a[k * 64:(k + 1) * 64] != bytes(64)][:2]
    out["s5_swapped"] = ("one", {5: _swap(a, i, j, 64)})
    coef = bytearray(one[4])
    coef[4 + 12] ^= 1
    out["s4_byte"] = ("one", {4: bytes(coef)})
    out["s8_short"] = ("one", {8: s8[:-64]})
    return out


@pytest.mark.parametrize("what", ["s9_swapped", "s8_overwritten", "delta2_of_another_d", "g2_spx_of_another_d",
                                  "transcript_byte", "records_swapped", "s5_swapped", "s4_byte", "s8_short"])
def test_verify_rejects(amd, chain, what):
    base, repl = _tampered(chain)[what]
    assert _rewrite(chain[base], {}) == chain[base]
    ok, why = amd.zkey_verify_from_init(chain["init"], _rewrite(chain[base], repl), device=0)
    assert not ok and why.startswith("zkey verify: "), why


def test_verify_truncated_section_10_is_a_format_error(amd, chain):
    s10 = _sections(chain["one"])[10]
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_verify_from_init(chain["init"], _rewrite(chain["one"], {10: s10[:-1]}), device=0)
    assert e.value.code == -2 and "zkey: Invalid File format" in str(e.value)


# ------------------------------------------------------------------ 7. the CSPRNG path
def test_random_contributions_differ_and_verify(amd, chain):
    a, ha = amd.zkey_contribute(chain["init"], "anon", device=0)
    bb, hb = amd.zkey_contribute(chain["init"], "anon", device=0)
    assert a != bb and ha != hb
    for key in (a, bb):
        ok, why = amd.zkey_verify_from_init(chain["init"], key, device=0)
        assert ok, why
