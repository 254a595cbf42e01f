"""CPU side of the ptau leg of `zkey verify` (g16_zkey_verify_from_init_ptau): the big-integer twin of the leg's scalar
vectors (tests/zkey_verify_ptau_ref.py) against the closed form, for both forms of the H block, and through the library
every error that must come out before the device is touched, by its text and return code."""
import pytest

import formats as f
import synth
from bn254 import Q, R
from ptau_prepared import rewrite
from zkey_verify_ptau_ref import h_block, h_scalars_ref

TD = {"tau": 0x1234567 ** 5 % R, "alpha": 0xabcdef ** 7 % R, "beta": 0x55aa ** 11 % R, "gamma": 1, "delta": 1}


# ------------------------------------------------------------------ the twin against the closed form
@pytest.mark.parametrize("truncated", [False, True], ids=["full_block", "truncated_block"])
@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_twin_equals_closed_form(L, truncated):
    """2N sum rho_i H_i = sum t_j tau^j, H_i = point 2i+1 of the size-2N block (the twin's rho keeps 1 / 2N)."""
    N = 1 << L
    rng = synth.Xoshiro(100 + L)
    tau = rng.rand_fr()
    u = [rng.rand_fr() for _ in range(N - 1)] + [0]
    u[0] = R - 1
    if N > 2:
        u[1] = 0
    rho, t = h_scalars_ref(u, L)
    assert len(rho) == N and len(t) == 2 * N - 1 and t[N - 1] == 0
    H = h_block(L, tau, truncated)
    lhs = 2 * N * sum(r * h for r, h in zip(rho, H)) % R
    assert lhs == sum(x * pow(tau, j, R) for j, x in enumerate(t)) % R
    assert lhs == sum(u[k] * (pow(tau, k, R) - pow(tau, k + N, R)) for k in range(N - 1)) % R


def test_an_unconstrained_rho_tells_the_two_blocks_apart():
    """why the combination is drawn from the hyperplane: off it, the same scalars give two different sums"""
    L, tau = 3, synth.Xoshiro(7).rand_fr()
    rho = [1] + [0] * 7
    full, cut = h_block(L, tau, False), h_block(L, tau, True)
    assert sum(r * h for r, h in zip(rho, full)) % R != sum(r * h for r, h in zip(rho, cut)) % R


# ------------------------------------------------------------------ errors ahead of the device
@pytest.fixture(scope="module")
def key(amd):
    n, p, m, seed = 24, 2, 12, 1          # m + p + 1 = 15: domain 2^4
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    zkey, _ = amd.r1cs_setup_trapdoor(f.write_r1cs(n, p, 0, rows), TD, 2)
    assert f.read_zkey(zkey)["domainSize"] == 16
    return zkey


@pytest.fixture(scope="module")
def ptau4(amd):
    return amd.ptau_synth(4, TD["tau"], TD["alpha"], TD["beta"], prepared=False, device=-1)


def _err(amd, key, ptau):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_verify_from_init(key, key, device=0, ptau=ptau)
    return e.value


def test_truncated_ptau(amd, key, ptau4):
    for cut in (0, 5, 12, 100, len(ptau4) // 2, len(ptau4) - 1):
        e = _err(amd, key, ptau4[:cut])
        assert e.code == -2 and "ptau: Invalid File format" in str(e), (cut, str(e))


def test_wrong_curve_ptau(amd, key, ptau4):
    other = rewrite(ptau4, lambda sid, d: d[:4] + (Q - 2).to_bytes(32, "little") + d[36:] if sid == 1 else d)
    e = _err(amd, key, other)
    assert e.code == -2 and "ptau: Invalid File format (bn128 powers of tau expected)" in str(e)


def test_section_2_shorter_than_the_leg_reads(amd, key, ptau4):
    # 2N - 1 = 31 points are read: 30 are too few, and so is a file without section 2
    e = _err(amd, key, rewrite(ptau4, lambda sid, d: d[:30 * 64] if sid == 2 else d))
    assert e.code == -2 and str(e).endswith("ptau: Invalid File format")
    e = _err(amd, key, rewrite(ptau4, lambda sid, d: None if sid == 2 else d))
    assert e.code == -2 and str(e).endswith("ptau: Invalid File format")


@pytest.mark.parametrize("at", [0, 17, 30])
def test_section_2_point_off_the_curve(amd, key, ptau4, at):
    def edit(sid, d):
        if sid != 2:
            return d
        b = bytearray(d)
        b[at * 64 + 32] ^= 1      # y of point `at`
        return bytes(b)
    e = _err(amd, key, rewrite(ptau4, edit))
    assert e.code == -2 and str(e).endswith("ptau: Invalid File format")


def test_section_2_coordinate_not_below_q(amd, key, ptau4):
    def edit(sid, d):
        return d[:64] + Q.to_bytes(32, "little") + d[96:] if sid == 2 else d
    e = _err(amd, key, rewrite(ptau4, edit))
    assert e.code == -2 and str(e).endswith("ptau: Invalid File format")


def test_a_point_past_the_ones_the_leg_reads_is_not_looked_at(amd, key):
    """a power-5 file: points 31.. of section 2 are not the leg's; the call gets as far as the device check (or, with a
    device, to a verdict)"""
    ptau5 = amd.ptau_synth(5, TD["tau"], TD["alpha"], TD["beta"], prepared=False, device=-1)

    def edit(sid, d):
        if sid != 2:
            return d
        b = bytearray(d)
        b[31 * 64 + 32] ^= 1
        return bytes(b)
    try:
        amd.zkey_verify_from_init(key, key, device=0, ptau=rewrite(ptau5, edit))
    except amd.G16Error as e:
        assert e.code == -4, str(e)


def test_power_too_small_is_a_verdict(amd, key):
    ptau3 = amd.ptau_synth(3, TD["tau"], TD["alpha"], TD["beta"], prepared=False, device=-1)
    ok, why = amd.zkey_verify_from_init(key, key, device=0, ptau=ptau3)     # return code 0, before the device
    assert not ok and why == "zkey verify: the ptau is too small for this key"


def test_the_keys_are_read_before_the_ptau(amd, key, ptau4):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_verify_from_init(key, key[:len(key) - 1], device=0, ptau=ptau4[:40])
    assert e.value.code == -2 and "zkey: Invalid File format" in str(e.value)


def test_files_form_and_r1cs_route_errors(amd, key, ptau4, tmp_path):
    import ctypes as C
    lib = amd.load()
    paths = {}
    for name, data in (("init.zkey", key), ("cut.ptau", ptau4[:100]), ("small.ptau", amd.ptau_synth(
            3, TD["tau"], TD["alpha"], TD["beta"], prepared=False, device=-1))):
        paths[name] = str(tmp_path / name).encode()
        (tmp_path / name).write_bytes(data)
    ok = C.c_int(7)
    rc = lib.g16_zkey_verify_from_init_ptau_files(paths["init.zkey"], paths["cut.ptau"], paths["init.zkey"], 0, C.byref(ok))
    assert rc == -2 and b"ptau: Invalid File format" in lib.g16_last_error()
    rc = lib.g16_zkey_verify_from_init_ptau_files(paths["init.zkey"], paths["small.ptau"], paths["init.zkey"], 0, C.byref(ok))
    assert rc == 0 and ok.value == 0 and lib.g16_last_error() == b"zkey verify: the ptau is too small for this key"
    # the r1cs route is g16_groth16_setup_ptau first: its texts
    n, p, m, seed = 24, 2, 12, 1
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_verify_r1cs(f.write_r1cs(n, p, 0, rows), ptau4, key, device=0)
    assert e.value.code == -2 and "Powers of tau is not prepared." in str(e.value)


def test_h_scalars_refuses_bad_arguments(amd):
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_h_scalars([0], 0, device=0)
    assert e.value.code == -1 and "log_n out of range" in str(e.value)
    with pytest.raises(amd.G16Error) as e:
        amd.zkey_h_scalars([1, 2, 3, 4], 2, device=0)
    assert e.value.code == -1 and "u[N-1] must be zero" in str(e.value)
