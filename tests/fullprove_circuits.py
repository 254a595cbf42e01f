"""Two crafted circuits for the batched fullprove tests (g16_fullprove_batch, g16_plonk_fullprove_batch): each is a
witness program (wtns_prog_ref.py writes it) and its twin .r1cs (formats.py), so that keys can be set up from the .r1cs
and witnesses computed from the program.  Nothing here calls the library.

    tiny       wires 1 = out (public), 2 = x, 3 = y;   out = x * y          (the circuit of test_node_wtns_calc.py)
    ladder(k)  wires 1..k = out_0..out_{k-1} (public), k + 1 = x, k + 2 = y;
               out_0 = x * y,  out_j = out_{j-1} * x + y: one level per output
both with check 0: x - y - 1 = 0, "x is not y + 1".  R1CS rows: (x)(y) = (out_0), (out_{j-1})(x) = (out_j - y), and the
check row (x - y - 1)(1) = 0.  ladder(300) has more wires than the calculator's workgroup has threads, 300 levels and
9.6 KB of public signals per witness.

Pass i takes (x, y) = (2 + i, 1 + i); a violating pass takes y = x."""
import formats as f
import wtns_prog_ref as ref

TEXT = "x is not y + 1"
LADDER_K = 300


def ladder(k):
    """-> dict(name, n_wires, n_public, ops, checks, prog, r1cs)"""
    x, y = k + 1, k + 2
    ops = [("input", x, 0), ("input", y, 1), ("quad", 1, [(x, 1)], [(y, 1)], [])]
    rows = [([(x, 1)], [(y, 1)], [(1, 1)])]
    for j in range(1, k):
        ops.append(("quad", 1 + j, [(j, 1)], [(x, 1)], [(y, 1)]))
        rows.append(([(j, 1)], [(x, 1)], [(1 + j, 1), (y, ref.R - 1)]))
    ops.append(("check", [(x, 1), (y, -1), (0, -1)], 0))
    rows.append(([(x, 1), (y, ref.R - 1), (0, ref.R - 1)], [(0, 1)], []))
    n = k + 3
    return {"name": "tiny" if k == 1 else f"ladder{k}", "n_wires": n, "n_public": k, "ops": ops, "checks": [TEXT],
            "prog": ref.write(n, ops, [TEXT], n_public=k, inputs=[("x", 0, 1), ("y", 1, 1)], outputs=list(range(1, k + 1))),
            "r1cs": f.write_r1cs(n, k, 0, rows)}


def tiny():
    return ladder(1)


def inputs(i, violate=False):
    """The input words (x, y) of pass i."""
    return [2 + i, 2 + i if violate else 1 + i]


def witness(c, i, violate=False):
    """wtns_prog_ref's evaluation of pass i -> (wire values, status)."""
    return ref.evaluate(c["n_wires"], c["ops"], inputs(i, violate))


def public_bytes(c, i):
    """Words 1..n_public of the witness of pass i, as the fullprove calls return them."""
    w, status = witness(c, i)
    assert status == ref.NO_CHECK
    return ref.words(w[1:1 + c["n_public"]])
