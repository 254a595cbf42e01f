"""CPU side of `powersoftau beacon` / `zkey beacon`: the secret scalars of g16_beacon_scalars against the Python twin
(tests/beacon_ref.py: hashlib.sha256 and the twin's ChaCha), every argument error with its text, and the order of the
two beacon calls' checks: the file, the arguments, and only then -- after the chain -- the device."""
import pytest

from beacon_ref import chain, params, scalars, walk
from bn254 import R
from conftest import golden_path

HASH_TEXT = "beacon: the beacon hash must be 1 to 255 bytes"
EXP_TEXT = "beacon: numIterationsExp must be between 10 and 63"
BAD_ARGS = [(b"", 10, HASH_TEXT), (bytes(256), 10, HASH_TEXT), (b"\x01" * 32, 9, EXP_TEXT), (b"\x01" * 32, 64, EXP_TEXT)]


def _beacon(n):
    return bytes((37 * i + 11) & 0xff for i in range(n))


@pytest.mark.parametrize("count", [2, 6])
@pytest.mark.parametrize("n", [1, 32, 255])
@pytest.mark.parametrize("exp", [10, 11])
def test_scalars_equal_the_twin(amd, exp, n, count):
    got = amd.beacon_scalars(_beacon(n), exp, count)
    assert got == scalars(_beacon(n), exp, count)
    assert len(got) == count and all(1 <= x < R for x in got)


def test_two_scalars_are_the_first_two_of_six(amd):
    six = amd.beacon_scalars(_beacon(32), 10, 6)
    assert amd.beacon_scalars(_beacon(32), 10, 2) == six[:2]
    assert len(set(six)) == 6
    assert amd.beacon_scalars(_beacon(32), 11, 6) != six and amd.beacon_scalars(_beacon(31), 10, 6) != six


def test_the_first_application_hashes_the_raw_bytes():
    """(the twin against itself: a 32-byte beacon is not taken for h_1)"""
    import hashlib
    b32 = _beacon(32)
    assert chain(b32, 1) == hashlib.sha256(hashlib.sha256(b32).digest()).digest()
    assert chain(hashlib.sha256(b32).digest(), 10) != chain(b32, 10)


@pytest.mark.parametrize("beacon,exp,text", BAD_ARGS, ids=["len0", "len256", "e9", "e64"])
def test_scalars_argument_errors(amd, beacon, exp, text):
    with pytest.raises(amd.G16Error) as e:
        amd.beacon_scalars(beacon, exp, 2)
    assert e.value.code == -1 and str(e.value).endswith(text)


def test_scalars_count_must_be_2_or_6(amd):
    with pytest.raises(amd.G16Error) as e:
        amd.beacon_scalars(_beacon(32), 10, 3)
    assert e.value.code == -1 and str(e.value).endswith("beacon: count must be 2 or 6")


def test_params_builder_and_walker_of_the_twin():
    b32 = _beacon(32)
    assert params(None, b32, 10) == bytes([2, 10, 3, 32]) + b32
    assert params("ab", b"\x09", 63) == bytes([1, 2]) + b"ab" + bytes([2, 63, 3, 1, 9])
    assert walk(params(None, b32, 10)) == (10, b32) and walk(params("name", b32, 10)) == (10, b32)
    assert walk(b"") is None and walk(bytes([1, 2]) + b"ab") is None
    assert walk(bytes([3, 1, 9, 2, 10])) is None            # unsorted
    assert walk(bytes([2, 10, 3, 2, 9])) is None            # cut short
    assert walk(bytes([2, 9, 3, 1, 9])) is None and walk(bytes([2, 64, 3, 1, 9])) is None
    assert walk(bytes([2, 10, 3, 0])) is None and walk(bytes([2, 10, 3, 1, 9, 4, 0])) is None


# ------------------------------------------------------------------ the two calls, up to the device
def _calls(amd):
    ptau = amd.ptau_new(2)
    zkey = open(golden_path("tiny.zkey"), "rb").read()
    return [("ptau", amd.ptau_beacon, amd.load().g16_ptau_beacon_files, ptau), ("zkey", amd.zkey_beacon, amd.load().g16_zkey_beacon_files, zkey)]


def test_argument_errors_come_before_the_device(amd, tmp_path):
    for kind, call, files, data in _calls(amd):
        src, out = tmp_path / ("in." + kind), tmp_path / ("out." + kind)
        src.write_bytes(data)
        for beacon, exp, text in BAD_ARGS:
            with pytest.raises(amd.G16Error) as e:
                call(data, beacon, exp, "x", device=0)
            assert e.value.code == -1 and str(e.value).endswith(text), (kind, str(e.value))
            assert files(str(src).encode(), str(out).encode(), b"x", beacon, len(beacon), exp, 0, None) == -1
            assert not out.exists()
        # a malformed file is reported as `contribute` reports it
        with pytest.raises(amd.G16Error) as e:
            call(data[:-1], _beacon(32), 10, None, device=0)
        assert e.value.code == -2 and "Invalid File format" in str(e.value)


def test_without_a_device_both_calls_end_at_nogpu_and_write_nothing(amd, tmp_path):
    """Well-formed input and arguments: the chain runs, then the device is asked for.  With a device the call succeeds
    (what it writes is tests/test_gpu_beacon.py's subject)."""
    for kind, call, files, data in _calls(amd):
        src, out = tmp_path / ("in." + kind), tmp_path / ("out." + kind)
        src.write_bytes(data)
        try:
            call(data, _beacon(32), 10, "x", device=0)
        except amd.G16Error as e:
            assert e.code == -4 and str(e).endswith(kind + " beacon: no HIP device (there is no CPU path)"), str(e)
            assert files(str(src).encode(), str(out).encode(), b"x", _beacon(32), 32, 10, 0, None) == -4
            assert not out.exists()
