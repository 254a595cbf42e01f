"""Exact checks at the mid-size domains 2^12 .. 2^19, between the big-int oracle (domain <= 2^11) and the C oracle
(2^20 .. 2^22).  Most size-dependent code paths switch on in this range:

  * the H-MSM window geometry (choose_c / msm_group_create): plain windows at 2^12 .. 2^13, the salted top window at
    2^14, full window precomputation from 2^15 with the even window layouts (wb, wx) at 2^16 and 2^19;
  * the witness group's repeated-value rows (c = 13 by default from ~2^16 variables);
  * the third NTT pass of 1 .. 3 stages at 2^17 .. 2^19 (ntt_tables_create: tile 9, min_tb 2), also in the fused
    coset round trip (ntt_mid_pass_kernel) and the fused join (ntt_last_pass_join_kernel);
  * the PLONK grand product over several kZBlock = 2048-row chunks (k_z_scan, k_prefix_prod, k_z_apply).

Groth16 proofs are pinned by the trapdoor known answer (Fr arithmetic only, test_gpu_prove.trapdoor_kat), the coset
evaluations by the Python NTT, the PLONK proof by oracle/plonk.py on the key the device setup wrote.  Every case asserts
the geometry the handle reports, so that a change to the choice has to update the tables here on purpose."""
import ctypes

import pytest

import bn254 as b
import formats as f
import groth16 as g
import plonk as pk
import synth
from test_gpu_fullsize import cpu_threads
from test_gpu_prove import domain_of, trapdoor_kat

pytestmark = pytest.mark.gpu

# window bits the product picks for itself: (witness group = info.window_bits[0], H group = info.window_bits[4]).
# H (dense, n = N points): 2^12, 2^13 -> 8 (32 windows of 8 bits, top 6 bits); 2^14 -> 13 (salted top window, 5 salt
# bits); 2^15 -> 15 (full precomputation from 2^15 on: 17 x 15); 2^16 -> 16 (even: wb = 15, wx = 15); 2^17, 2^18 -> 17
# (15 x 17); 2^19 -> 19 (even: wb = 18, wx = 3).  Witness: c for n_eff = (largest section) / 3 + 1, capped at 13;
# 13 switches on the repeated-value rows (B = 4096 >= 1024).
# (L, n_vars, n_public, n_constraints, seed, witness c, H c)
KAT_CASES = [
    (12, 3000, 513, 3000, 1201, 7, 8),
    (13, 6000, 513, 6000, 1301, 8, 8),
    (14, 12000, 513, 12000, 1401, 9, 13),
    (15, 30000, 513, 30000, 1501, 8, 15),
    (16, 65000, 513, 65000, 1601, 13, 16),
    (17, 130000, 513, 130000, 1701, 13, 17),
    (18, 250000, 513, 250000, 1801, 13, 17),
    (19, 500000, 513, 500000, 1901, 13, 19),
    # m + p + 1 == N: no padding rows
    (14, 28000, 513, (1 << 14) - 514, 1410, 8, 13),
    # m + p + 1 == N / 2 + 1: the most padding rows a domain can have
    (14, 7679, 513, (1 << 13) + 1 - 514, 1420, 8, 13),
]


@pytest.mark.parametrize("L,n,p,m,seed,cw,ch", KAT_CASES, ids=[f"2^{c[0]}-m{c[3]}" for c in KAT_CASES])
def test_trapdoor_kat_default_geometry(amd, L, n, p, m, seed, cw, ch):
    """Default tuning (no window_bits / task_len / precomp): two witnesses of one key, each proof == the known answer."""
    assert domain_of(m, p) == 1 << L
    info = trapdoor_kat(amd, n, p, m, seed, wseeds=(None, seed + 1000))
    assert info.domain_size == 1 << L
    assert (info.window_bits[0], info.window_bits[4]) == (cw, ch)


_KEY_12 = {}


def _key_2_12(amd):
    """One 2^12 key (and its witness) for the forced H windows."""
    if not _KEY_12:
        _KEY_12["key"] = amd.synth_setup(3000, 513, 3000, 1201, threads=cpu_threads())[:2]
    return _KEY_12["key"]


# c -> (wb, wx) of the fully precomputed H group (Ws = ceil(255 / c) windows; even widths when Ws c > 255)
H_LAYOUTS = {15: (15, 0), 16: (15, 15), 17: (17, 0), 18: (17, 0), 19: (18, 3), 20: (19, 8), 21: (19, 8), 22: (21, 3)}


@pytest.mark.parametrize("c", sorted(H_LAYOUTS), ids=[f"c{c}-wb{wb}-wx{wx}" for c, (wb, wx) in sorted(H_LAYOUTS.items())])
def test_forced_h_window_layouts_at_2_12(amd, monkeypatch, c):
    """Every window layout of a fully precomputed H group (precomp=255), forced on a 2^12 key: c = 15 .. 22 covers every
    (wb, wx) production can reach and c = 21, 22, which no size picks today.  Nearly every one of the 2^(c-1) buckets is
    empty.  No c in this range is refused at create: with 12 low bits the binning keeps rows x bins <= 12288."""
    monkeypatch.setenv("G16_WINDOW_BITS", f"0,{c}")    # H only; read at create
    info = trapdoor_kat(amd, 3000, 513, 3000, 1201, key=_key_2_12(amd), precomp=255)
    assert info.domain_size == 1 << 12 and info.window_bits[4] == c


def _abc_on_domain(rows, w, p, m, N):
    """buildABC1 from the circuit's rows: A_T, B_T (with the public-input binding rows), C_T = A_T o B_T."""
    a, bb = [0] * N, [0] * N
    for c, (A, B, _) in enumerate(rows):
        a[c] = sum(cf * w[s] for s, cf in A) % b.R
        bb[c] = sum(cf * w[s] for s, cf in B) % b.R
    for i in range(p + 1):
        a[m + i] = (a[m + i] + w[i]) % b.R
    return a, bb, [x * y % b.R for x, y in zip(a, bb)]


def _on_coset(vals):
    """ntt(shift(intt(vals))): the evaluations at w_2N^(2i+1) (oracle/groth16.py h_scalars)."""
    N = len(vals)
    inc = b.fr_root(N.bit_length())
    coef = g.ntt(vals, inverse=True)
    t = 1
    for i in range(N):
        coef[i] = coef[i] * t % b.R
        t = t * inc % b.R
    return g.ntt(coef)


# NTT pass plans (lo_bits, S) of ntt_tables_create: 2^17 -> (0, 9) (9, 7) (16, 1); 2^18 -> (0, 9) (9, 7) (16, 2)
@pytest.mark.parametrize("L", [17, 18])
def test_coset_evaluation_with_a_short_third_pass(amd, L):
    """g16_shard_begin with all three vectors: qap_eval, then the fused coset round trip (inverse passes, the coset
    table inside ntt_mid_pass_kernel, forward passes) with a third pass of S = 1 or 2 stages.  Each vector, decoded from
    the lazy 9 x 29-bit words (Montgomery 2^261), == the Python NTT's, every word below 16 r."""
    N = 1 << L
    n, p, m, seed = 3 * N // 5, 5, 3 * N // 5, 2000 + L
    zkey, wtns, _ = amd.synth_setup(n, p, m, seed, threads=cpu_threads())
    rows, w = synth.make(n, p, m, seed)
    assert f.write_wtns(w) == wtns
    pv = amd.Prover(zkey, shard_rank=0, shard_count=2)
    assert pv.info.domain_size == N
    eb = amd.LAZY_FR_BYTES
    vecs = [ctypes.create_string_buffer(N * eb) for _ in range(3)]
    pv.stage(0, wtns)
    pv.shard_begin(0, 0b111, [ctypes.addressof(x) for x in vecs])
    pv.close()
    rinv = pow(1 << 261, -1, b.R)
    for k, ev in enumerate(_abc_on_domain(rows, w, p, m, N)):
        want = _on_coset(ev)
        raw = vecs[k].raw
        got = [amd.f29_unpack(raw[i * eb:(i + 1) * eb]) for i in range(N)]
        assert max(got) < 16 * b.R, k
        bad = [i for i in range(N) if got[i] * rinv % b.R != want[i]]
        assert not bad, (k, len(bad), bad[:8])


def test_plonk_four_grand_product_chunks(amd):
    """PLONK at domain 2^13: the grand product runs as four kZBlock = 2048-row chunks joined by k_prefix_prod's
    carries.  Key from the device setup (byte-equal to the oracle's setup: test_gpu_plonk.test_setup_tool_equals_oracle),
    read back by the oracle; the proof with fixed blinding b1..b9 == oracle/plonk.py's, bit for bit.  Then one copy
    constraint broken in chunk 3 (an A-wire of a row >= 6144 moved to another signal in the key's map): the flag computed
    over all four chunks refuses the witness."""
    n, p, m, seed = 2500, 3, 2500, 61
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    zkey = amd.plonk_setup(f.write_r1cs(n, p, 0, rows), seed, device=0)
    zk = pk.read_zkey(zkey)
    assert zk["domainSize"] == 1 << 13 and zk["nConstraints"] > 3 * 2048
    _, w = synth.make(n, p, m, seed)
    wtns = f.write_wtns(w)
    rng = synth.Xoshiro(seed + 40)
    bl = {i: rng.rand_fr() for i in range(1, 10)}
    prover = amd.PlonkProver(zkey)
    assert prover.domain_size == 1 << 13
    proof, pub = prover.prove(wtns, [bl[i] for i in range(1, 10)])
    prover.close()
    exp, exp_pub = pk.prove(zk, w, bl)
    assert proof == pk.proof_obj(exp)
    assert pub == [str(x) for x in exp_pub]
    assert pk.verify(pk.vkey_from_zkey(zkey), [int(x) for x in pub], pk.proof_from_obj(proof))
    # break a copy constraint in chunk 3: the A-wire of row r takes signal s2 instead of s (s appears elsewhere, so the
    # position is on a cycle of the permutation; w[s2] != w[s])
    we = [0] + list(w[1:])
    we = pk.extend_witness(we, zk["additions"])
    uses = {}
    for col in zk["maps"]:
        for s in col[:zk["nConstraints"]]:
            uses[s] = uses.get(s, 0) + 1
    r = next(r for r in range(3 * 2048 + 100, zk["nConstraints"]) if zk["maps"][0][r] != 0 and uses[zk["maps"][0][r]] > 1)
    s = zk["maps"][0][r]
    s2 = next(x for x in range(1, len(we)) if we[x] != we[s])
    secs = f.read_binfile(zkey, "zkey", 2)
    pos, _ = secs[4][0]
    bad = bytearray(zkey)
    bad[pos + 4 * r:pos + 4 * r + 4] = s2.to_bytes(4, "little")
    prover = amd.PlonkProver(bytes(bad))
    with pytest.raises(amd.G16Error) as e:
        prover.prove(wtns, [bl[i] for i in range(1, 10)])
    assert "Copy constraints does not match" in str(e.value)
    prover.close()
