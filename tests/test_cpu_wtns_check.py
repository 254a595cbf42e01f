"""g16_wtns_check on the host route (device = -1): the error texts, the verdict against the big-integer twin
(tests/wtns_check_ref.py), the synthetic circuit and a SHA-256 message circuit."""
import struct

import pytest

import formats as f
import synth
import wtns_check_ref as ref
from bn254 import R


@pytest.fixture(scope="module")
def small():
    """Six short rows, a 20-term and a 100-term row: (builder, r1cs bytes, wtns bytes)."""
    b = ref.Builder(seed=5)
    for _ in range(6):
        b.short_row()
    b.long_row(0, 20)
    b.long_row(2, 100)
    return b, b.r1cs(), b.wtns()


def _section(buf, sid):
    """(offset, size) of the first section `sid` of a binfile image."""
    nsec = struct.unpack_from("<I", buf, 8)[0]
    pos = 12
    for _ in range(nsec):
        i, size = struct.unpack_from("<IQ", buf, pos)
        pos += 12
        if i == sid:
            return pos, size
        pos += size
    raise KeyError(sid)


def _patched(buf, off, data):
    return buf[:off] + data + buf[off + len(data):]


def test_witness_error_texts(amd, small):
    b, r1cs, wtns = small
    k = amd.R1csChecker(r1cs, device=-1)
    n = len(b.w)
    h, _ = _section(wtns, 1)
    body, _ = _section(wtns, 2)
    cases = [
        (b"wtnx" + wtns[4:], "wtns: Invalid File format"),
        (wtns[:8], "wtns: Invalid File format"),
        (wtns[:-5], "wtns: Invalid File format"),
        (_patched(wtns, 4, struct.pack("<I", 3)), "Version not supported"),
        (_patched(wtns, h + 4, f.le(R + 2)), "Curve of the witness does not match the curve of the proving key"),
        (f.write_wtns(b.w + [0]), f"Invalid witness length. Circuit: {n}, witness: {n + 1}"),
        (f.write_wtns(b.w[:-1]), f"Invalid witness length. Circuit: {n}, witness: {n - 1}"),
        (_patched(wtns, body + 32 * 7, f.le(R)), "wtns: signal 7 is not reduced modulo the scalar field"),
        (_patched(wtns, body + 32 * (n - 1), b"\xff" * 32), f"wtns: signal {n - 1} is not reduced modulo the scalar field"),
        (_patched(wtns, body, f.le(2)), "wtns check: signal 0 is not 1"),
        (_patched(wtns, body, f.le(0)), "wtns check: signal 0 is not 1"),
    ]
    for bad, text in cases:
        with pytest.raises(amd.G16Error) as e:
            k.check(bad)
        assert str(e.value) == text
        assert e.value.code == -2   # G16_E_FORMAT
    # a batch fails as a whole on its lowest malformed witness
    with pytest.raises(amd.G16Error) as e:
        k.check_batch([wtns, wtns, wtns[:-5], wtns, wtns[:8]])
    assert str(e.value) == "witness 2: wtns: Invalid File format"
    with pytest.raises(amd.G16Error) as e:
        k.check_batch([wtns, _patched(wtns, body + 32 * 3, f.le(R + 1))])
    assert str(e.value) == "witness 1: wtns: signal 3 is not reduced modulo the scalar field"
    assert k.check(wtns).ok   # the checker survives all of it
    k.close()


def test_r1cs_error_texts(amd, small):
    _, r1cs, wtns = small
    for bad, text in [(b"r1cx" + r1cs[4:], "r1cs: Invalid File format"),
                      (r1cs[:40], "r1cs: truncated section"),
                      (_patched(r1cs, _section(r1cs, 1)[0] + 4, f.le(R + 2)), "r1cs: field is not the bn128 scalar field")]:
        with pytest.raises(amd.G16Error) as e:
            amd.R1csChecker(bad, device=-1)
        assert str(e.value) == text
        with pytest.raises(amd.G16Error) as e:
            amd.wtns_check(bad, wtns, device=-1)
        assert str(e.value) == text


def test_no_constraints(amd):
    r1cs = f.write_r1cs(3, 0, 0, [])
    v = amd.wtns_check(r1cs, f.write_wtns([1, 5, R - 1]), device=-1)
    assert ref.as_dict(v) == ref.verdict([], [1, 5, R - 1])
    assert v.ok and v.constraint == -1 and v.n_failed == 0
    with pytest.raises(amd.G16Error) as e:
        amd.wtns_check(r1cs, f.write_wtns([1, 5]), device=-1)
    assert str(e.value) == "Invalid witness length. Circuit: 3, witness: 2"


def test_small_circuit_verdicts(amd, small):
    b, r1cs, wtns = small
    k = amd.R1csChecker(r1cs, device=-1)
    assert ref.verdict(b.rows, b.w)["ok"]
    assert ref.as_dict(k.check(wtns)) == ref.verdict(b.rows, b.w)
    for rows in [(0,), (5,), (6,), (7,), (2, 6, 7), (7, 3)]:
        w = b.broken(*rows)
        want = ref.verdict(b.rows, w)
        assert want["constraint"] == min(rows) and want["n_failed"] == len(rows)
        v = k.check(f.write_wtns(w))
        assert ref.as_dict(v) == want
        assert v.reason == ref.text(want)
    # the library's own text, and the batch form
    lib = amd.load()
    vs = k.check_batch([wtns, f.write_wtns(b.broken(6)), wtns, f.write_wtns(b.broken(1, 4))])
    assert [ref.as_dict(v) for v in vs] == [ref.verdict(b.rows, w) for w in (b.w, b.broken(6), b.w, b.broken(1, 4))]
    assert lib.g16_last_error().decode() == "witness 1: wtns check: constraint 6 is not satisfied (1 in all)"
    k.check(f.write_wtns(b.broken(7, 3)))
    assert lib.g16_last_error().decode() == "wtns check: constraint 3 is not satisfied (2 in all)"
    assert k.check_batch([]) == []
    k.close()


def test_synthetic_circuit(amd):
    n, p, m, seed = 700, 9, 5000, 21   # (m above the host route's threshold for more than one thread)
    rows, w = synth.make(n, p, m, seed)
    assert synth.check_r1cs(rows, w)
    r1cs = f.write_r1cs(n, p, 0, rows)
    k = amd.R1csChecker(r1cs, device=-1)
    assert ref.as_dict(k.check(f.write_wtns(w))) == ref.verdict(rows, w)
    assert k.check(f.write_wtns(w)).ok
    # the library's own witness of the same circuit passes too
    assert k.check(amd.synth_witness(n, p, m, seed, seed + 9)).ok
    bad = list(w)
    slack = [C[0][0] for _, _, C in rows if C][40]   # a slack wire: the C side of its own row, free in later ones
    bad[slack] = (bad[slack] + 1) % R
    assert not synth.check_r1cs(rows, bad)
    want = ref.verdict(rows, bad)
    assert not want["ok"]
    assert ref.as_dict(k.check(f.write_wtns(bad))) == want
    assert ref.as_dict(amd.wtns_check(r1cs, f.write_wtns(bad), device=-1)) == want
    k.close()


def test_sha256_message_circuit(amd):
    out = amd.sha256_message_setup(b"witness checking", 3, want_zkey=False, want_r1cs=True)
    rows = f.read_r1cs(out["r1cs"])["rows"]
    w = f.read_wtns(out["wtns"])["w"]
    k = amd.R1csChecker(out["r1cs"], device=-1)
    v = k.check(out["wtns"])
    assert v.ok and ref.verdict(rows, w)["ok"]
    # the wires behind the 256 public digest bits are the message bits: flip one input byte
    bad = list(w)
    for i in range(257, 265):
        assert bad[i] in (0, 1)
        bad[i] ^= 1
    want = ref.verdict(rows, bad)
    assert not want["ok"]
    assert ref.as_dict(k.check(f.write_wtns(bad))) == want
    k.close()
