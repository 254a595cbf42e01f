"""Test helper: the big-integer twin of g16_zkey_h_scalars (csrc/zkey_verify_h.hip), the scalars of the ptau leg of
`zkey verify`.

N = 2^L, w = the primitive 2N-th root of the NTT tables (bn254.fr_root(L + 1)), u = N values below r with u[N-1] = 0:

  rho[i] = (1 / N) sum_k u[k] w^((2i+1) k)          i < N       (the scalars of section 9)
  t      = u[0..N-2] | 0 | -u[0..N-2]  mod r         2N - 1     (the scalars of the ptau's section 2)

WHERE THE CONSTANT SITS: the check's own combination is 2 sum_k u[k] w^((2i+1) k) = 2N rho[i].  The coset table of the
device's NTT carries 1 / N, so the device leaves 1 / 2N in rho and the host multiplies the ONE point S = sum rho[i] H[i]
by 2N before the pairing.  With L_j the Lagrange basis of the size-2N domain:

  2N sum_i rho[i] L_(2i+1)(tau) = sum_j t[j] tau^j

and the same holds with L_j(tau) - w^j tau^(2N-1) / 2N in place of L_j(tau) (the block a real `prepare phase2` writes at
L = power), because sum_i rho[i] w^(2i+1) = u[N-1] = 0."""
import groth16 as g
from bn254 import R, fr_root


def h_scalars_ref(u, L):
    """-> (rho, t): lists of ints below r, N and 2N - 1 long."""
    N = 1 << L
    assert len(u) == N and u[N - 1] == 0 and all(0 <= x < R for x in u)
    w = fr_root(L + 1)
    ninv = pow(N, -1, R)
    tw, x = [], ninv
    for k in range(N):      # the coset twist, 1 / N folded in
        tw.append(u[k] * x % R)
        x = x * w % R
    rho = g.ntt(tw)         # sum_k (u[k] w^k / N) (w^2)^(ik)
    t = list(u[:N - 1]) + [0] + [(R - x) % R for x in u[:N - 1]]
    return rho, t


def h_block(L, tau, truncated):
    """The N values H_i = point 2i+1 of block L+1 of a prepared ceremony's section 12, as scalars of the generator: the
    full Lagrange basis of the size-2N domain, or the block computed from 2N - 1 powers of tau (truncated)."""
    N = 1 << L
    lag = g.lagrange_at(2 * N, tau)
    if truncated:
        w = fr_root(L + 1)
        top = pow(tau, 2 * N - 1, R) * pow(2 * N, -1, R) % R
        lag = [(lag[j] - pow(w, j, R) * top) % R for j in range(2 * N)]
    return [lag[2 * i + 1] for i in range(N)]
