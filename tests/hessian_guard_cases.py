"""Shapes, operands and host references of the safeguards of the dense stage Hessians (hqpkkt_hessian_row_stats,
hqpkkt_restart_, hqpkkt_gerschgorin_ and hqpkkt_eigen_control_stage_hessians; test_staged_hessian_guard_cpu.py,
test_gpu_staged_hessian_guard.py).

The shapes of hessian_update_cases (tile edges, a middle stage that stays dense on a packed handle, tiny orders) and, around
the 256-thread stride of the per-stage workgroups and the 64-lane row pass, (255, 257, 512) and (513, 1, 2); around the
default cap of 64 Lanczos steps (63, 64, 65).  K = 2, so every case has three blocks."""
import numpy as np

from hqp_amd import hessian_update as hu
import hessian_update_cases as uc

ORDERS = uc.ORDERS + [(255, 257, 512), (513, 1, 2), (63, 64, 65)]
EPS = 2.0 ** -10  # the control's eps: theta = 2^-20 on every stage without a floor of its own

# The rounding allowance of the eigenvalue estimate, in units of 2^-53 nz |Q|_inf: the largest
# |lambda_est(model) - eigvalsh(Q)[0]| / (2^-53 nz |Q|_inf) over eigen_cases(), MEASURED by
# test_staged_hessian_guard_cpu.py::test_model_converges_and_measures_the_allowance (which prints it and fails when the
# cases outgrow this constant): 2.19, from the rank-2 block of order 3, rounded up.  The GPU test allows 8 times it on top
# of the reported rho: the device's sums run in another order than numpy's.
ALLOWANCE = 2.5


def real_blocks(rng, nz):
    """Symmetric blocks of full-mantissa reals."""
    out = []
    for v in nz:
        U = np.triu(rng.standard_normal((v, v)))
        out.append(U + np.triu(U, 1).T)
    return out


def rank2_block(rng, v, c1):
    """3 I + 2 a a' - c1 b b', the form a BFGS update leaves of a scaled identity: three distinct eigenvalues at most, the
    recurrence ends by an invariant subspace.  c1 = 0: positive definite (smallest eigenvalue 3) and, from a handful of
    variables on, not diagonally dominant."""
    a, b = rng.uniform(-1, 1, v), rng.uniform(-1, 1, v)
    return 3.0 * np.eye(v) + 2.0 * np.outer(a, a) - c1 * np.outer(b, b)


def indefinite_block(rng, v):
    """int_blocks(spd=True) minus 128 u u' with integer u: the rank-1 term moves one eigenvalue far below the others, which
    stay in a band of a few hundred sqrt(v) around 128 v - a separated smallest eigenvalue."""
    B = uc.int_blocks(rng, [v], spd=True)[0].astype(np.float64)
    u = rng.integers(-4, 5, v).astype(np.float64)
    u[0] = 3.0
    return B - 128.0 * np.outer(u, u)


def aligned_block(rng, v):
    """3 I - 50 f f' / f'f + (a b' + b a') / (4 sqrt(v)) with f the recurrence's start vector: the smallest eigenvalue, near
    -47 and 50 below the others, belongs to a vector close to f, so that ONE step brackets it: it lies in [alpha_0 - beta_0,
    alpha_0] (alpha_0 is a Rayleigh quotient, beta_0 the residual's norm, far below the gap) - not converged, yet conservative."""
    f = hu.lanczos_start(v)
    a, b = rng.uniform(-1, 1, v), rng.uniform(-1, 1, v)
    E = np.outer(a, b) / (4.0 * np.sqrt(v))
    return 3.0 * np.eye(v) - (50.0 / (f @ f)) * np.outer(f, f) + (E + E.T)


def dominant_block(rng, v):
    return uc.int_blocks(rng, [v], spd=True)[0].astype(np.float64)


KINDS = ("indefinite", "rank2", "definite", "dominant")


def eigen_blocks(nz, turn, seed=5):
    """Three blocks of the orders nz, their kinds taking turns: (kinds, blocks)."""
    rng = np.random.default_rng(seed + turn)
    kinds, out = [], []
    for k, v in enumerate(nz):
        kind = KINDS[(k + turn) % len(KINDS)]
        kinds.append(kind)
        out.append(indefinite_block(rng, v) if kind == "indefinite" else rank2_block(rng, v, 40.0) if kind == "rank2" else
                   rank2_block(rng, v, 0.0) if kind == "definite" else dominant_block(rng, v))
    return kinds, out


def eigen_cases():
    """(nz, kinds, blocks) of every GPU eigen case: every shape, the kinds shifted by the shape's index."""
    return [(nz,) + eigen_blocks(nz, t) for t, nz in enumerate(ORDERS)]


def model(Q, theta, max_steps=0):
    """lanczos_model and eigen_replay of one block: the replay's dict with g, steps and T added."""
    g, steps, T = hu.lanczos_model(Q, theta, max_steps)
    r = hu.eigen_replay(Q.shape[0], g, theta, steps, T)
    r.update(g=g, steps=steps, T=T)
    return r


def norm_inf(Q):
    return float(np.abs(Q).sum(axis=1).max()) if Q.shape[0] else 0.0


def sturm_count(alpha, beta, x):
    """Eigenvalues below x of the tridiagonal (alpha, beta[:-1]) in exact rational arithmetic."""
    from fractions import Fraction as F
    a, b = [F(float(t)) for t in alpha], [F(float(t)) for t in beta]
    x = F(float(x))
    # signs of the leading principal minors of T - x I by the three-term recurrence: no division, so no pivot can vanish
    # a sign change between consecutive minors is an eigenvalue below x; a zero minor takes the sign opposite to its
    # predecessor's
    p0, p1, sign, count = F(1), a[0] - x, 1, 0
    for i in range(len(a)):
        if i > 0:
            p0, p1 = p1, (a[i] - x) * p1 - b[i - 1] * b[i - 1] * p0
        s = -sign if p1 == 0 else (1 if p1 > 0 else -1)
        count += s != sign
        sign = s
    return count
