"""Python twin of the Groth16 verdict "in the exponent", written from the pairing equation and not from the C++: when
every point of the key and of the proof is a KNOWN multiple of its generator,

  key    alpha1 = alpha G1, beta2 = beta G2, gamma2 = gamma G2, delta2 = delta G2, IC_j = ic_j G1
  proof  A = a G1, B = b G2, C = c G1           (the point at infinity is the exponent 0)

then e(-A, B) e(alpha1, beta2) e(vk_x, gamma2) e(C, delta2) = e(G1, G2)^(-ab + alpha beta + x gamma + c delta) with
x = ic_0 + sum_j pub_j ic_j, and e(G1, G2) has order r: the proof is accepted iff

  a b = alpha beta + (ic_0 + sum_j pub_j ic_j) gamma + c delta   (mod r).

One line of integer arithmetic, independent of csrc/pairing.cuh and of oracle/bn254.py's pairing; it can be solved for
a free variable, which gives a VALID proof through any branch of the verifier one wants (C at infinity, vk_x at
infinity, A or B at infinity).  tests/test_cpu_verify_exponent.py checks the rule against oracle/groth16.py::verify.

  key scalars  ks = (ics, alpha, beta, gamma, delta), ics = [ic_0 .. ic_n]; alpha .. delta non-zero modulo r
  a case       (a, b, c, pub): exponents of the proof, pub = the public signals (any integers below 2^256)"""
import bn254 as b
import formats as f
from bn254 import R

_G1 = {0: None}
_G2 = {0: None}


def g1_points(ks):
    """[k G1] for many k; every distinct exponent is multiplied once and kept."""
    ks = [k % R for k in ks]
    new = sorted({k for k in ks if k not in _G1})
    _G1.update(zip(new, b.G1.gen_mul_many(new)))
    return [_G1[k] for k in ks]


def g2_points(ks):
    ks = [k % R for k in ks]
    new = sorted({k for k in ks if k not in _G2})
    _G2.update(zip(new, b.G2.gen_mul_many(new)))
    return [_G2[k] for k in ks]


def make_key(ics, alpha, beta, gamma, delta):
    """-> (key bytes for Verifier(key, n_public, montgomery=True): alpha1 | beta2 | gamma2 | delta2 | IC[], Montgomery
    form, zeros for an IC_j at infinity;  the vk dict oracle/groth16.py::verify takes)."""
    assert all(k % R for k in (alpha, beta, gamma, delta))
    alpha1 = g1_points([alpha])[0]
    beta2, gamma2, delta2 = g2_points([beta, gamma, delta])
    ic = g1_points(ics)
    raw = (f.g1_to_lem(alpha1) + f.g2_to_lem(beta2) + f.g2_to_lem(gamma2) + f.g2_to_lem(delta2) +
           b"".join(f.g1_to_lem(P) for P in ic))
    return raw, {"alpha1": alpha1, "beta2": beta2, "gamma2": gamma2, "delta2": delta2, "IC": ic}


def vk_x(ks, pub):
    """The exponent of vk_x = IC_0 + sum_j pub_j IC_{j+1}."""
    ics = ks[0]
    assert len(pub) + 1 == len(ics) and all(0 <= int(p) < 1 << 256 for p in pub)
    return (ics[0] + sum(int(p) * ic for p, ic in zip(pub, ics[1:]))) % R


def accepts(ks, a, b_, c, pub):
    _, alpha, beta, gamma, delta = ks
    return (a * b_ - alpha * beta - vk_x(ks, pub) * gamma - c * delta) % R == 0


# ------------------------------------------------------------------ solvers: the free variable of a valid proof
def solve_c(ks, a, b_, pub):
    """c of the valid proof with these a, b and signals (a = 0 or b = 0: A or B at infinity)."""
    _, alpha, beta, gamma, delta = ks
    return (a * b_ - alpha * beta - vk_x(ks, pub) * gamma) * pow(delta, -1, R) % R


def solve_a(ks, b_, pub):
    """a of the valid proof with C at infinity (c = 0)."""
    _, alpha, beta, gamma, _ = ks
    assert b_ % R
    return (alpha * beta + vk_x(ks, pub) * gamma) * pow(b_, -1, R) % R


def solve_last_signal(ks, head, x=0):
    """The last public signal such that vk_x has the exponent x (0: vk_x at infinity) after the signals `head`."""
    ics = ks[0]
    assert len(head) + 2 == len(ics) and ics[-1] % R
    part = vk_x((ics[:-1],) + tuple(ks[1:]), head)
    return (x - part) * pow(ics[-1], -1, R) % R


def x_without_a_and_c(ks):
    """The exponent of vk_x at which alpha beta + x gamma = 0: valid with A (or B) and C both at infinity."""
    _, alpha, beta, gamma, _ = ks
    return -alpha * beta * pow(gamma, -1, R) % R


# ------------------------------------------------------------------ the proof as users hand it over
def proof_obj(a, b_, c):
    """proof.json object of (a G1, b G2, c G1); infinity as snarkjs writes it (["0", "1", "0"])."""
    A, C = g1_points([a, c])
    return f.proof_obj(A, g2_points([b_])[0], C)


def proof_points(a, b_, c):
    A, C = g1_points([a, c])
    return A, g2_points([b_])[0], C
