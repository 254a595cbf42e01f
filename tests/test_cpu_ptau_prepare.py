"""CPU side of `powersoftau prepare phase2` (g16_ptau_prepare): every input error comes out before the device is
touched, with the texts g16_groth16_setup_ptau gives where they apply, no mutated file crashes the reader, and the
Python restatement the GPU tests compare against (tests/ptau_prepare_ref.py) is itself checked against the Lagrange
basis and against the closed form of section 12's padded top block."""
import random
import struct

import pytest

import groth16 as g
import plonk as pk
from bn254 import R, fr_root
from ptau_prepare_ref import block_scalars, idft, lagrange_scalar, top_block_scalar
from ptau_prepared import rewrite, write_ptau_prepared

TD = {"tau": 0x1234567 ** 5 % g.R, "alpha": 0xabcdef ** 7 % g.R, "beta": 0x55aa ** 11 % g.R}


_GPU = []


def _gpu_present(amd):
    """Whether the library itself finds a device (torch's answer does not bind the library's own HIP runtime when both
    are loaded into one process): a well-formed power-0 file ends at G16_E_NOGPU, or is prepared."""
    if not _GPU:
        try:
            amd.ptau_prepare(write_ptau_prepared(0, 5, 6, 7, prepared=False), device=0)
            _GPU.append(True)
        except amd.G16Error as e:
            assert e.code == -4, str(e)
            _GPU.append(False)
    return _GPU[0]


@pytest.fixture(scope="module")
def ptau6():
    return write_ptau_prepared(6, TD["tau"], TD["alpha"], TD["beta"], prepared=False)


def _err(amd, ptau):
    with pytest.raises(amd.G16Error) as e:
        amd.ptau_prepare(ptau, device=0)
    return e.value


def _accepted(amd, ptau):
    """A well-formed file passes every check: the call then succeeds, or -- no device, the last check of all -- ends at
    G16_E_NOGPU."""
    try:
        out = amd.ptau_prepare(ptau, device=0)
    except amd.G16Error as e:
        assert e.code == -4 and "no HIP device" in str(e), str(e)
    else:
        assert out[:4] == b"ptau" and len(out) >= len(ptau)


def test_well_formed_power_6_file_passes_the_checks(amd, ptau6):
    _accepted(amd, ptau6)


def test_oracle_write_ptau_is_accepted(amd):
    _accepted(amd, pk.write_ptau(6, 777))


def test_prepared_input_is_accepted(amd):
    _accepted(amd, write_ptau_prepared(3, TD["tau"], TD["alpha"], TD["beta"], prepared=True))


def test_missing_section_7_is_accepted(amd, ptau6):
    _accepted(amd, rewrite(ptau6, lambda sid, d: None if sid == 7 else d))


def test_not_a_ptau_and_truncated_files(amd, ptau6):
    for cut in (0, 5, 12, 100, len(ptau6) // 2, len(ptau6) - 1):
        e = _err(amd, ptau6[:cut])
        assert e.code == -2 and "ptau: Invalid File format" in str(e), (cut, str(e))
    e = _err(amd, b"zkey" + ptau6[4:])
    assert e.code == -2 and "ptau: Invalid File format" in str(e)
    e = _err(amd, ptau6[:4] + struct.pack("<I", 2) + ptau6[8:])
    assert e.code == -2 and "Version not supported" in str(e)


def test_bad_section_table(amd, ptau6):
    # the first section's length runs past the end of the file
    e = _err(amd, ptau6[:16] + struct.pack("<Q", 1 << 40) + ptau6[24:])
    assert e.code == -2 and "ptau: Invalid File format" in str(e)


def test_not_bn128(amd, ptau6):
    def other_prime(sid, d):
        return d[:4] + bytes([d[4] ^ 1]) + d[5:] if sid == 1 else d
    e = _err(amd, rewrite(ptau6, other_prime))
    assert e.code == -2 and "ptau: Invalid File format (bn128 powers of tau expected)" in str(e)
    e = _err(amd, rewrite(ptau6, lambda sid, d: None if sid == 1 else d))
    assert e.code == -2 and "bn128 powers of tau expected" in str(e)


@pytest.mark.parametrize("sid", [2, 3, 4, 5, 6])
def test_section_missing_or_of_the_wrong_size(amd, ptau6, sid):
    psz = 128 if sid in (3, 6) else 64
    for edit in (lambda d: None, lambda d: d[:-psz], lambda d: d + d[:psz], lambda d: d[:-1]):
        e = _err(amd, rewrite(ptau6, lambda s, d: edit(d) if s == sid else d))
        assert e.code == -2 and str(e).endswith("ptau: Invalid File format"), str(e)


def test_sizes_follow_the_header_power(amd, ptau6):
    # a power-6 body under a power-5 / power-7 header
    for power in (5, 7):
        hdr = lambda sid, d: d[:36] + struct.pack("<I", power) + d[40:] if sid == 1 else d   # noqa: E731
        e = _err(amd, rewrite(ptau6, hdr))
        assert e.code == -2 and "ptau: Invalid File format" in str(e)


def test_power_above_the_limit_names_the_limit(amd, ptau6):
    for power in (25, 28):
        hdr = lambda sid, d: d[:36] + struct.pack("<I", power) + d[40:] if sid == 1 else d   # noqa: E731
        e = _err(amd, rewrite(ptau6, hdr))
        assert e.code == -1 and "limit of 24" in str(e) and f"power {power}" in str(e), str(e)
    hdr = lambda sid, d: d[:36] + struct.pack("<I", 29) + d[40:] if sid == 1 else d   # noqa: E731
    e = _err(amd, rewrite(ptau6, hdr))          # not a power a ceremony can have
    assert e.code == -2 and "ptau: Invalid File format" in str(e)


def test_no_cpu_path(amd, ptau6):
    if _gpu_present(amd):
        pytest.skip("GPU present")
    assert _err(amd, ptau6).code == -4


def test_files_entry_point_reports_a_missing_input(amd, tmp_path):
    rc = amd.load().g16_ptau_prepare_files(str(tmp_path / "missing.ptau").encode(), str(tmp_path / "out.ptau").encode(), 0)
    assert rc == -1 and b"cannot open" in amd.load().g16_last_error()
    assert not (tmp_path / "out.ptau").exists()


def test_files_entry_point_checks_like_the_buffer_one(amd, ptau6, tmp_path):
    (tmp_path / "cut.ptau").write_bytes(ptau6[:len(ptau6) // 2])
    rc = amd.load().g16_ptau_prepare_files(str(tmp_path / "cut.ptau").encode(), str(tmp_path / "out.ptau").encode(), 0)
    assert rc == -2 and b"ptau: Invalid File format" in amd.load().g16_last_error()
    assert not (tmp_path / "out.ptau").exists()


def test_mutated_ptau_images(amd, ptau6):
    """An error, never a crash or an allocation sized by an untrusted field."""
    if _gpu_present(amd):
        pytest.skip("GPU present")
    rng = random.Random(6)

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
    for _ in range(600):
        try:
            amd.ptau_prepare(mutate(ptau6, 600), device=0)
        except amd.G16Error as e:
            codes.add(e.code)
    assert codes <= {-1, -2, -4} and -2 in codes


# ------------------------------------------------------------------ the restatement itself
def test_idft_is_the_definition():
    rng = random.Random(1)
    for k in range(5):
        n = 1 << k
        xs = [rng.randrange(R) for _ in range(n)]
        winv = pow(fr_root(k), -1, R)
        want = [sum(pow(winv, i * j, R) * xs[i] for i in range(n)) * pow(n, -1, R) % R for j in range(n)]
        assert idft(xs) == want


@pytest.mark.parametrize("power", [0, 1, 3, 6])
def test_restatement_gives_the_lagrange_basis_up_to_the_power(power):
    tau = TD["tau"]
    pw = [pow(tau, i, R) for i in range((2 << power) - 1)]
    got = block_scalars(pw, power + 1)
    for k in range(power + 1):
        assert got[(1 << k) - 1:(2 << k) - 1] == g.lagrange_at(1 << k, tau), k
    # the padded top block: the closed form, and not the Lagrange basis
    M = 2 << power
    top = got[M - 1:]
    assert len(top) == M
    assert top == [top_block_scalar(power, j, tau) for j in range(M)]
    lag = g.lagrange_at(M, tau)
    assert all(a != b for a, b in zip(top, lag))
    assert lag == [lagrange_scalar(M, j, tau) for j in range(M)]


@pytest.mark.parametrize("M", [2, 8, 32])
def test_top_block_closed_form(M):
    """y_j = L_j(tau) - w^j tau^(M-1) / M for an input whose last power is missing."""
    tau = TD["alpha"]
    power = M.bit_length() - 2
    xs = [pow(tau, i, R) for i in range(M - 1)] + [0]
    w = fr_root(power + 1)
    lag = g.lagrange_at(M, tau)
    want = [(lag[j] - pow(w, j, R) * pow(tau, M - 1, R) * pow(M, -1, R)) % R for j in range(M)]
    assert idft(xs) == want


def test_h_basis_cannot_tell_the_padded_block_from_the_lagrange_basis():
    """sum_j p(w^j) y_j is the same for both when p has degree <= M - 2: the extra term w^j tau^(M-1) / M only meets
    the coefficient of x^(M-1)."""
    rng = random.Random(3)
    power, tau = 3, TD["beta"]
    M = 2 << power
    coef = [rng.randrange(R) for _ in range(M - 1)]                 # degree M - 2
    w = fr_root(power + 1)
    ev = [sum(c * pow(w, j * i, R) for i, c in enumerate(coef)) % R for j in range(M)]
    lag = g.lagrange_at(M, tau)
    top = [top_block_scalar(power, j, tau) for j in range(M)]
    assert sum(e * a for e, a in zip(ev, lag)) % R == sum(e * b for e, b in zip(ev, top)) % R
