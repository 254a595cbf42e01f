"""g16_wtns_check on the device (csrc/wtns_check.hip): every case is compared with the big-integer twin
(tests/wtns_check_ref.py) and with the host route (device = -1).  The shapes are the smallest at which the kernel can
go wrong: the edges of a 256-thread block, the two thresholds between its three row-length classes (16 and 64 terms)
and the longest row of the NZCP circuit (356), the matrix that decides the class, the sums at their lazy bound."""
import pytest

import formats as f
import wtns_check_ref as ref
from bn254 import R

pytestmark = pytest.mark.gpu

LENGTHS = [16, 17, 64, 65, 356]


def both(amd, r1cs):
    return amd.R1csChecker(r1cs, device=0), amd.R1csChecker(r1cs, device=-1)


def agree(checkers, rows, w):
    """The device verdict, the host route's and the twin's are one; -> the twin's."""
    want = ref.verdict(rows, w)
    wtns = f.write_wtns(w)
    for k in checkers:
        v = k.check(wtns)
        assert ref.as_dict(v) == want
        if not want["ok"]:
            assert v.reason == ref.text(want)
    return want


def close(checkers):
    for k in checkers:
        k.close()


@pytest.mark.parametrize("m", [1, 255, 256, 257])
def test_block_edges(amd, m):
    b = ref.Builder(seed=m)
    for _ in range(m):
        b.short_row()
    ks = both(amd, b.r1cs())
    assert agree(ks, b.rows, b.w)["ok"]
    for row in sorted({0, m - 1, min(256, m - 1)}):   # first, last, and index 256 where there is one
        want = agree(ks, b.rows, b.broken(row))
        assert want["constraint"] == row and want["n_failed"] == 1
    close(ks)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["A", "B", "C"])
@pytest.mark.parametrize("length", LENGTHS)
def test_length_classes(amd, which, length):
    """One long side (A, B, or C ALONE: the two others hold one term each, so only C can put the row into its class)
    between two short rows.  The deciding term is the last of its row: with its wire changed the row fails, and so it
    does when the term is taken out of the circuit."""
    b = ref.Builder(seed=100 * which + length)
    b.short_row()
    r = b.long_row(which, length)
    b.short_row()
    ks = both(amd, b.r1cs())
    assert agree(ks, b.rows, b.w)["ok"]
    last_wire = b.rows[r][which][-1][0]
    w = list(b.w)
    w[last_wire] = (w[last_wire] + 1) % R
    want = agree(ks, b.rows, w)
    assert want["constraint"] == r and want["n_failed"] == 1
    close(ks)
    cut = list(b.rows)
    cut[r] = tuple(side[:-1] if i == which else side for i, side in enumerate(b.rows[r]))
    ks = both(amd, b.r1cs(cut))
    want = agree(ks, cut, b.w)
    assert want["constraint"] == r and want["n_failed"] == 1
    close(ks)


def test_empty_rows(amd):
    rows = [([], [(0, 1)], [(1, 1)]),          # empty A, non-zero C: fails
            ([], [], []),                      # all empty: holds
            ([(1, 0)], [(1, 1)], []),          # an explicit zero coefficient: 0 * w1 = 0 holds
            ([], [(1, 1)], [(1, 0)]),          # ... in C
            ([(1, 1)], [(0, 1)], [(1, 1)])]
    w = [1, 5]
    ks = both(amd, f.write_r1cs(2, 0, 0, rows))
    want = agree(ks, rows, w)
    assert want == {"ok": False, "constraint": 0, "n_failed": 1, "a": 0, "b": 1, "c": 5}
    close(ks)
    ks = both(amd, f.write_r1cs(2, 0, 0, rows[1:]))
    assert agree(ks, rows[1:], w)["ok"]
    close(ks)
    ks = both(amd, f.write_r1cs(2, 0, 0, []))   # no constraints at all
    assert agree(ks, [], w)["ok"]
    close(ks)


@pytest.mark.parametrize("which", [0, 2], ids=["A", "C"])
@pytest.mark.parametrize("kind", ["minus_one", "general", "mixed"])
def test_lazy_sum_bound(amd, kind, which):
    """One 356-term row with every wire r - 1 and every coefficient r - 1 (the subtracting records: two units each), a
    general r - 2 (a product each), or both kinds mixed: the row holds exactly, and fails with its target raised by one."""
    coef = {"minus_one": lambda j: R - 1, "general": lambda j: R - 2, "mixed": lambda j: R - 1 - (j * 7 % 3 == 0)}[kind]
    b = ref.Builder(seed=7)
    r = b.long_row(which, 356, coef=coef, value=lambda j: R - 1)
    ks = both(amd, b.r1cs())
    assert agree(ks, b.rows, b.w)["ok"]
    want = agree(ks, b.rows, b.broken(r))
    assert want["constraint"] == 0 and want["n_failed"] == 1
    close(ks)


@pytest.fixture(scope="module")
def mixed():
    """Rows of all three classes interleaved, 300 short ones among them (more than one block)."""
    b = ref.Builder(seed=77)
    for i in range(300):
        b.short_row()
        if i % 60 == 7:
            b.long_row(i // 60 % 3, 17 + i // 60)
        if i % 100 == 42:
            b.long_row((i // 100 + 1) % 3, 65 + i)
    return b, b.r1cs()


def test_several_failing_rows(amd, mixed):
    b, r1cs = mixed
    ks = both(amd, r1cs)
    assert agree(ks, b.rows, b.w)["ok"]
    classes = {"short": [], "mid": [], "long": []}
    for i, row in enumerate(b.rows):
        n = max(len(s) for s in row)
        classes["short" if n <= 16 else "mid" if n <= 64 else "long"].append(i)
    assert all(len(v) >= 3 for v in classes.values())
    pick = classes["short"][5:200:13] + classes["mid"][1:] + classes["long"][::2]
    want = agree(ks, b.rows, b.broken(*pick))
    assert want["constraint"] == min(pick) and want["n_failed"] == len(pick)
    # the lowest failing row in each class in turn
    for name in ("long", "mid", "short"):
        rows = [classes[name][-1]] + [r for r in pick if r > classes[name][-1]]
        want = agree(ks, b.rows, b.broken(*rows))
        assert want["constraint"] == classes[name][-1] and want["n_failed"] == len(rows)
    close(ks)


@pytest.mark.parametrize("chunk", [None, "2", "1"])
def test_batch(amd, mixed, monkeypatch, chunk):
    """Five witnesses, the third and the fifth bad in different rows; G16_WTNS_CHECK_CHUNK (include/g16_prover.h) forces
    the batch through three and five chunks."""
    b, r1cs = mixed
    if chunk:
        monkeypatch.setenv("G16_WTNS_CHECK_CHUNK", chunk)
    else:
        monkeypatch.delenv("G16_WTNS_CHECK_CHUNK", raising=False)
    ws = [b.w, b.w, b.broken(200, 9), b.w, b.broken(130)]
    want = [ref.verdict(b.rows, w) for w in ws]
    assert [v["constraint"] for v in want] == [-1, -1, 9, -1, 130]
    wtns = [f.write_wtns(w) for w in ws]
    for k in both(amd, r1cs):
        assert [ref.as_dict(v) for v in k.check_batch(wtns)] == want
        assert amd.load().g16_last_error().decode() == "witness 2: wtns check: constraint 9 is not satisfied (2 in all)"
        with pytest.raises(amd.G16Error) as e:
            k.check_batch(wtns[:2] + [wtns[2][:-1]] + wtns[3:])
        assert str(e.value) == "witness 2: wtns: Invalid File format"
        k.close()


def test_reuse(amd, mixed):
    b, r1cs = mixed
    ks = both(amd, r1cs)
    for w in (b.w, b.broken(17, 250), b.w, b.broken(3), b.w):
        agree(ks, b.rows, w)
    close(ks)


def test_sha256_two_blocks(amd):
    """A real shape, still small: SHA-256 of a 64-byte message (two compressions, rows of up to ~260 terms)."""
    out = amd.sha256_message_setup(bytes(range(64)), 5, want_zkey=False, want_r1cs=True)
    rows = f.read_r1cs(out["r1cs"])["rows"]
    assert max(max(len(s) for s in row) for row in rows) > 64
    w = f.read_wtns(out["wtns"])["w"]
    close(both(amd, out["r1cs"]))   # handles that never ran a check
    ks = both(amd, out["r1cs"])
    assert agree(ks, rows, w)["ok"]
    bad = list(w)
    bad[len(w) // 2] = (bad[len(w) // 2] + 1) % R
    assert not agree(ks, rows, bad)["ok"]
    assert ref.as_dict(amd.wtns_check(out["r1cs"], f.write_wtns(bad), device=0)) == ref.verdict(rows, bad)
    close(ks)
