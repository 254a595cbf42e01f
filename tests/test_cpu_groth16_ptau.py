"""CPU side of the Groth16 setup from a prepared .ptau (g16_groth16_setup_ptau): every input error comes out before
the device is touched, with snarkjs's texts, and no mutated file crashes the readers.  Also the two test-only
generators on host threads: g16_r1cs_setup_trapdoor equals the oracle's setup for the same trapdoor, and
g16_ptau_synth equals the Python writer (tests/ptau_prepared.py)."""
import random
import struct

import pytest

import formats as f
import groth16 as g
import plonk as pk
import synth
from ptau_prepared import rewrite, write_ptau_prepared

TD = {"tau": 0x1234567 ** 5 % g.R, "alpha": 0xabcdef ** 7 % g.R, "beta": 0x55aa ** 11 % g.R}


def _gpu_present():
    import torch
    return torch.cuda.is_available()


@pytest.fixture(scope="module")
def circuit():
    n, p, m, seed = 60, 5, 40, 3          # m + p + 1 = 46: domain 2^6
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    return f.write_r1cs(n, p, 0, rows)


@pytest.fixture(scope="module")
def ptau6():
    return write_ptau_prepared(6, TD["tau"], TD["alpha"], TD["beta"])


def _err(amd, r1cs, ptau):
    with pytest.raises(amd.G16Error) as e:
        amd.groth16_setup_ptau(r1cs, ptau, device=0)
    return e.value


def test_unprepared_ptau_is_refused(amd, circuit):
    e = _err(amd, circuit, pk.write_ptau(6, 777))
    assert e.code == -2 and "Powers of tau is not prepared." in str(e)


def test_power_too_small(amd, circuit):
    e = _err(amd, circuit, write_ptau_prepared(5, TD["tau"], TD["alpha"], TD["beta"]))
    assert e.code == -2
    assert "circuit too big for this power of tau ceremony." in str(e) and "2**5" in str(e)


def test_missing_block_l_plus_1_of_section_12(amd, circuit, ptau6):
    # section 12 through block 6 only (blocks 0..6 = 127 points): the H points of block 7 are not there
    cut = rewrite(ptau6, lambda sid, d: d[:127 * 64] if sid == 12 else d)
    e = _err(amd, circuit, cut)
    assert e.code == -2 and "circuit too big for this power of tau ceremony." in str(e) and "2**6" in str(e)


def test_truncated_files(amd, circuit, ptau6):
    for cut in (0, 5, 12, 100, len(ptau6) // 2, len(ptau6) - 1):
        e = _err(amd, circuit, ptau6[:cut])
        assert e.code == -2 and "Invalid File format" in str(e), (cut, str(e))
    e = _err(amd, circuit[:len(circuit) - 7], ptau6)
    assert e.code == -2


@pytest.mark.parametrize("sid", [12, 13, 14, 15])
def test_lagrange_section_cut_by_one_point(amd, circuit, ptau6, sid):
    psz = 128 if sid == 13 else 64
    e = _err(amd, circuit, rewrite(ptau6, lambda s, d: d[:-psz] if s == sid else d))
    assert e.code == -2 and "Invalid File format" in str(e)


def test_section_longer_than_the_power_allows(amd, circuit, ptau6):
    # one more whole block in section 13 than a power-6 ceremony can have
    e = _err(amd, circuit, rewrite(ptau6, lambda s, d: d + d[:128] + d if s == 13 else d))
    assert e.code == -2 and "Invalid File format" in str(e)


def test_no_cpu_path(amd, circuit, ptau6):
    if _gpu_present():
        pytest.skip("GPU present")
    e = _err(amd, circuit, ptau6)
    assert e.code == -4


def test_mutated_r1cs_and_ptau_images(amd, circuit, ptau6):
    """An error, never a crash or an allocation sized by an untrusted field."""
    if _gpu_present():
        pytest.skip("GPU present")
    rng = random.Random(5)

    def mutate(buf, head):
        b = bytearray(buf)
        k = rng.randrange(4)
        if k == 0:
            for _j in range(rng.randrange(1, 4)):
                b[rng.randrange(min(len(b), head))] = rng.randrange(256)
        elif k == 1:
            b = b[:rng.randrange(len(b))]
        elif k == 2:
            i = rng.randrange(min(len(b) - 4, head))
            b[i:i + 4] = struct.pack("<I", rng.choice([0, 1, 0xffffffff, 0x7fffffff, rng.randrange(1 << 32)]))
        else:
            i = 12 + rng.randrange(100)
            b[i:i + 8] = struct.pack("<Q", rng.choice([0, 1, len(b), 1 << 40, (1 << 64) - 1]))
        return bytes(b)
    codes = set()
    for _ in range(300):
        for r, pt in ((mutate(circuit, len(circuit)), ptau6), (circuit, mutate(ptau6, 600))):
            try:
                amd.groth16_setup_ptau(r, pt, device=0)
            except amd.G16Error as e:
                codes.add(e.code)
    assert codes <= {-1, -2, -4, -5} and -2 in codes


@pytest.mark.parametrize("n,p,m,seed", [(24, 2, 12, 1), (150, 6, 120, 2)])
def test_trapdoor_setup_equals_oracle(amd, n, p, m, seed):
    _, rows, _ = synth.gen_circuit(n, p, m, seed)
    td = dict(TD, gamma=1, delta=1) if seed == 1 else g.trapdoor(seed + 40)
    zkey, vkey = amd.r1cs_setup_trapdoor(f.write_r1cs(n, p, 0, rows), td, 4)
    zk, _ = g.setup(n, p, rows, td)
    assert zkey == f.write_zkey(zk)
    assert vkey == f.g1_to_lem(zk["alpha1"]) + f.g2_to_lem(zk["beta2"]) + f.g2_to_lem(zk["gamma2"]) + \
        f.g2_to_lem(zk["delta2"]) + b"".join(f.g1_to_lem(P) for P in zk["IC"])


def test_trapdoor_refuses_bad_scalars(amd, circuit):
    with pytest.raises(amd.G16Error):
        amd.r1cs_setup_trapdoor(circuit, dict(TD, gamma=0, delta=1))
    with pytest.raises(amd.G16Error):
        amd.r1cs_setup_trapdoor(circuit, dict(TD, gamma=1, delta=g.R))


@pytest.mark.parametrize("prepared", [True, False])
def test_ptau_synth_on_host_equals_python_writer(amd, prepared):
    got = amd.ptau_synth(4, TD["tau"], TD["alpha"], TD["beta"], prepared=prepared, device=-1)
    assert got == write_ptau_prepared(4, TD["tau"], TD["alpha"], TD["beta"], prepared=prepared)
