"""Programs, blocks and host references of hqpkkt_q_eigen_control / hqpkkt_q_eigen_report (test_q_eigen_cpu.py, q_eigen_worker.py).

A case is a program whose Q is made of blocks, a bsize that cuts Q into exactly those blocks (hqpkkt_q_blocks), and per block
the outcomes it may end with.  Block lengths: 1, 2, 3, 63, 64, 65 (a wavefront), 257 (a workgroup), 4095, 4096, 4097 (one
unit of 4096 entries, and the first entry of a second) and 8193 (three units).
  wave      detected blocks, every one at most 64 long: a wavefront per block (WPU == 1)
  mixed     detected blocks of 1 .. 257: short and long blocks in one plan, a workgroup per unit
  long*     one LONG block cut by a fixed bsize (4095, 4097, 8193, and bsize 0 for 4096) and a short dense block behind it.
            A long block is a row of decoupled dense sub-blocks of order SUB = 96 at most - a fixed bsize does not need a
            connected block -, every one 10 I + E with |E|_2 about 1.2, and ONE of them with - 40 u u' / u'u on top: its
            eigenvalue near -30 lies far below the rest of the block's spectrum, [8.8, 11.2], so that the recurrence
            converges in a dozen steps.  The reference value is the minimum of eigvalsh over the sub-blocks: no dense matrix
            of order 8193 is ever formed.
  band7     n = 257, a band of 10 above an indefinite diagonal, bsize 7: every block is a full 7 x 7 matrix and 30 entries per
            block reach ACROSS blocks (never read or written); a wavefront per block
  band100   the same Q with bsize 100: blocks that are not fully stored (the band inside them), no separated eigenvalue -
            they may end "shifted, not converged" after 64 steps
  docp      with_dense_hessian(lq_docp(4, 3, 2)), its diagonals lowered so that the stage blocks are indefinite; detected;
            the three plugins
`fine` refines a case's partition into its sub-blocks: no stored entry of a block crosses two of them (asserted by
test_q_eigen_cpu.py), so eigvalsh of a block is eigvalsh of its sub-blocks.

ALLOWANCE: the rounding allowance of the eigenvalue estimate in units of 2^-53 L |B|_inf (L the block's length), the largest
|lambda_est(model) - eigvalsh(block)[0]| / (2^-53 L |B|_inf) over every block of cases() whose model converges, MEASURED by
test_q_eigen_cpu.py::test_model_converges_and_measures_the_allowance (which prints it and fails when the cases outgrow the
constant), rounded up.  The GPU test allows 8 times it on top of the reported rho: the device's sums run in another order
than numpy's (the scheme of hessian_guard_cases.ALLOWANCE).

The bound on T (t_bound).  The device and q_lanczos_model run the same recurrence with sums in two orders.  With u = 2^-53,
N = |B|_inf >= |B|_2, a sum of L terms in any order within (L + 2) u of the sum of |terms|, and e_j the 2-norm of the
difference of the two v_j, to first order in the errors:
  r     = 4 (L + 2) u sqrt(L) N        what the roundings of one step (the product - |B|_F <= sqrt(L) N -, the two axpys, the
                                       projections, the norms), of both runs together, add to a vector or a scalar of the step
  e_0   = 2 (L + 3) u                  v_0 = f / |f|: the norm's sum and the division, twice
  a_j   = 2 N e_j + r                  alpha_j = v_j'B v_j
  d_j   = 4 N e_j + N e_{j-1} + d_{j-1} + 2 r    w - alpha_j v_j - beta_{j-1} v_{j-1} (|alpha|, beta <= N; the change of
                                       alpha_j and of beta_{j-1}); the projections of the second pass are of rounding size
  |beta_j - beta_j'| <= d_j,  e_{j+1} = 2 d_j / beta_j       v_{j+1} = w / beta_j
The bound grows by about 8 N / beta_j per step, so it says something for the first steps alone: T is compared at the steps
j where max(a_j, d_j) <= 2^-10 N, and step 0 is always one of them."""
import numpy as np

from hqp_amd import hessian_update as hu
from hqp_amd import ipmatrix, problems
import hessian_guard_cases as G

EPS = 2.0 ** -10  # the control's eps: theta = 2^-20 on every block without a floor of its own
U = 2.0 ** -53
SUB = 96
ALLOWANCE = 2.5
GK, THETA, STEPS, LO, HI, RHO, LAM, DK, NORMT, OUTCOME = range(10)
KINDS = ("indefinite", "rank2", "definite", "dominant")


def dense_block(kind, v, rng):
    return (G.indefinite_block(rng, v) if kind == "indefinite" else G.rank2_block(rng, v, 40.0) if kind == "rank2" else
            G.rank2_block(rng, v, 0.0) if kind == "definite" else G.dominant_block(rng, v))


def want_of(kind, v):
    """the outcomes a dense block of this kind and order may end with"""
    if kind == "definite":  # (3 I + 2 a a' is diagonally dominant by itself at tiny orders, and may be up to a handful)
        return (0,) if v < 4 else (0, 1) if v < 16 else (1,)
    return (0,) if kind == "dominant" else (2,)


def long_block(length, rng):
    """the sub-blocks of a long block: orders SUB, .., and the rest; the second one carries the eigenvalue near -30"""
    out = []
    for k, o in enumerate(range(0, length, SUB)):
        v = min(SUB, length - o)
        E = np.triu(rng.uniform(-1.0, 1.0, (v, v))) / np.sqrt(v)
        B = 10.0 * np.eye(v) + E + np.triu(E, 1).T
        if k == 1:
            u = rng.uniform(-1.0, 1.0, v)
            B = B - (40.0 / (u @ u)) * np.outer(u, u)
        out.append(B)
    return out


def program_of(blocks, seed=0):
    """(program, first, fine): Q from `blocks`, a list of blocks, each a list of decoupled dense sub-blocks whose upper
    triangles are stored; n // 4 equalities of two entries, n // 2 bounds"""
    qr, qc, qv, first, fine = [], [], [], [0], [0]
    for subs in blocks:
        for B in subs:
            i, j = np.triu_indices(B.shape[0])
            qr.append(fine[-1] + i), qc.append(fine[-1] + j), qv.append(B[i, j])
            fine.append(fine[-1] + B.shape[0])
        first.append(fine[-1])
    n = first[-1]
    return _program(n, problems._csr(np.concatenate(qr), np.concatenate(qc), np.concatenate(qv), n), seed), np.array(first), np.array(fine)


def _program(n, Q, seed):
    rng = np.random.default_rng(900 + seed)
    me, m = n // 4, n // 2
    A = problems._csr(np.repeat(np.arange(me), 2), np.stack([4 * np.arange(me), 4 * np.arange(me) + 2], 1).ravel(), rng.uniform(-1, 1, 2 * me), me)
    Cm = problems._csr(np.arange(m), 2 * np.arange(m), rng.uniform(0.5, 1.5, m), m)
    return problems.Program(n, me, m, Q, A, Cm, c=rng.uniform(-1, 1, n), b=np.zeros(me), d=-np.ones(m))


def dense_case(name, orders, turn, seed=0):
    """detected blocks: fully stored dense blocks of the given orders, each drawn from a seed of its order and kind alone (a
    permutation of `orders` moves the blocks and keeps their values), the kinds taking turns"""
    kinds = [KINDS[(k + turn) % 4] for k in range(len(orders))]
    blocks = [[dense_block(kind, v, np.random.default_rng(700 + 11 * v + KINDS.index(kind) + seed))] for kind, v in zip(kinds, orders)]
    prog, first, fine = program_of(blocks, seed)
    return dict(name=name, prog=prog, bsize=-1, first=first, fine=fine, want=[want_of(k, v) for k, v in zip(kinds, orders)])


def long_case(length, tail, bsize):
    rng = np.random.default_rng(3000 + length)
    blocks = [long_block(length, rng)] + ([[dense_block("indefinite", tail, rng)]] if tail else [])
    prog, first, fine = program_of(blocks, length)
    return dict(name="long%d" % length, prog=prog, bsize=bsize, first=first, fine=fine, want=[(2,)] * len(blocks))


def band_program(n=257, band=10, seed=0):
    rng = np.random.default_rng(4000 + n + seed)
    r = np.concatenate([np.arange(n - k) for k in range(band + 1)])
    c = np.concatenate([np.arange(k, n) for k in range(band + 1)])
    v = np.concatenate([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.0, 1.0, c.size - n)])
    return _program(n, problems._csr(r, c, v, n), seed)


def band_case(bsize):
    prog = band_program()
    first = hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, bsize)[0]
    nb = first.size - 1
    # a block of at most 64 runs until its Krylov space is the whole block; a longer one may stop at the cap of 64 steps
    want = [(2,) if first[b + 1] - first[b] <= 64 else (2, 3) for b in range(nb)]
    return dict(name="band%d" % bsize, prog=prog, bsize=bsize, first=first, fine=first, want=want)


def docp_program():
    base = problems.with_dense_hessian(problems.lq_docp(4, 3, 2))
    x = np.array(base.Q[2], dtype=np.float64)
    rows = np.repeat(np.arange(base.n), np.diff(base.Q[0]))
    x[np.asarray(base.Q[1]) == rows] -= 10.0
    return problems.Program(base.n, base.me, base.m, (base.Q[0], base.Q[1], x), base.A, base.C, base.c, base.b, base.d)


def docp_case():
    prog = docp_program()
    first = hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, -1)[0]
    return dict(name="docp", prog=prog, bsize=-1, first=first, fine=first, want=[(2,)] * (first.size - 1))


WAVE_ORDERS = (1, 2, 3, 63, 64, 8, 63, 5)
MIXED_ORDERS = (1, 2, 3, 63, 64, 65, 257)
SP = (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP)


def cases():
    out = [dense_case("wave", WAVE_ORDERS, 0), dense_case("mixed", MIXED_ORDERS, 2),
           long_case(4095, 65, 4095), long_case(4096, 0, 0), long_case(4097, 3, 4097), long_case(8193, 64, 8193),
           band_case(7), band_case(100), docp_case()]
    for k, c in enumerate(out):
        c["classes"] = SP + (ipmatrix.IpLQDOCP,) if c["name"] == "docp" else SP[k % 2: k % 2 + 1] if c["name"].startswith("long") else SP
    return out


def sub_blocks(Q_csr, case, b):
    """the dense sub-blocks of block b, from the values in Q_csr"""
    fine = case["fine"]
    ks = np.flatnonzero((fine[:-1] >= case["first"][b]) & (fine[:-1] < case["first"][b + 1]))
    return [hu.q_block_dense(Q_csr, fine, int(k)) for k in ks]


def block_facts(Q_csr, case, b, shift=0.0):
    """(smallest eigenvalue, |B|_inf, length) of block b, d added to its diagonal: the minimum and the maximum over its
    sub-blocks"""
    subs = sub_blocks(Q_csr, case, b)
    lam = min(float(np.linalg.eigvalsh(B + shift * np.eye(B.shape[0]))[0]) for B in subs)
    return lam, max(G.norm_inf(B) for B in subs), int(case["first"][b + 1] - case["first"][b])


def model(Q_csr, case, theta=EPS ** 2, max_steps=0):
    """q_lanczos_model and eigen_replay of every block: a list of the replay's dicts with g, steps and T added"""
    g, steps, T = hu.q_lanczos_model(Q_csr, case["first"], theta, max_steps)
    th = np.broadcast_to(np.asarray(theta, dtype=np.float64), g.shape)
    out = []
    for b in range(g.size):
        r = hu.eigen_replay(int(case["first"][b + 1] - case["first"][b]), g[b], th[b], steps[b], T[b])
        r.update(g=g[b], steps=int(steps[b]), T=T[b], theta=float(th[b]))
        out.append(r)
    return out


def t_bound(L, N, beta):
    """(a, d): the bounds on |alpha_j - alpha_j'| and |beta_j - beta_j'| of the module's docstring for a block of length L and
    norm N, from the betas of one of the two runs"""
    m = len(beta)
    r = 4.0 * (L + 2) * U * np.sqrt(L) * N
    a, d = np.zeros(m), np.zeros(m)
    e_prev, e, d_prev = 0.0, 2.0 * (L + 3) * U, 0.0
    with np.errstate(all="ignore"):
        for j in range(m):
            a[j] = 2.0 * N * e + r
            d[j] = 4.0 * N * e + N * e_prev + d_prev + 2.0 * r
            e_prev, e, d_prev = e, (2.0 * d[j] / beta[j] if beta[j] > 0.0 else np.inf), d[j]
    return a, d


def t_compare(L, N, T_dev, T_mod, steps):
    """the steps compared and the worst |difference| / bound over them: T of two runs of one block, at the steps where
    t_bound says something"""
    a, d = t_bound(L, N, T_mod[1][:steps])
    ok = np.maximum(a, d) <= 2.0 ** -10 * N
    worst = 0.0
    for j in np.flatnonzero(ok):
        worst = max(worst, abs(T_dev[0][j] - T_mod[0][j]) / a[j], abs(T_dev[1][j] - T_mod[1][j]) / d[j])
    return int(ok.sum()), worst
