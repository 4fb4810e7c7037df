"""Host side of the block-BFGS update of the dense stage Hessians: the terms that
``IpLQDOCP.update_stage_hessians`` (hqpkkt_update_stage_hessians) applies on the device.

Per diagonal block Q of the Hessian, with the step s and the change y of the Lagrangian's gradient over the block's
variables, the reference's damped BFGS update (Hqp_HL_BFGS::update_b_Q) is

    sv = s'y,  sQs = s'(Q s)
    gamma  = gamma_0                                   for gamma_0 >= 0,
             g + (1 - g)(1 - alpha) with g = -gamma_0  otherwise (damping adapted to the step length alpha)
    Powell's modification, where sv < gamma sQs:
        theta = (1 - gamma) sQs / (sQs - sv),  v = theta y + (1 - theta) Q s,  sv = s'v
    otherwise v = y
    Q+ = Q - (Q s)(Q s)' / sQs + v v' / sv,            and Q+ = Q where sv or sQs is zero.

``IpLQDOCP.bfgs_update_device`` (hqpkkt_bfgs_update_stage_hessians) forms the same terms on the device; ``bfgs_replay`` is its
numpy model, operation by operation from the sums the device reports.

The safeguards that read a block run on the device as well (staged_hess_guard.hip.h); their numpy models are here:
``restart_model`` (restart_Q, ``IpLQDOCP.restart_hessians``), ``gerschgorin_model`` (Hqp_HL_Gerschgorin::update,
``IpLQDOCP.gerschgorin_hessians``) and, of the eigenvalue control that the reference runs after the update
(``IpLQDOCP.eigen_control``: the smallest eigenvalue lambda of the block, and q_ii -= lambda - theta where that is negative),
``lanczos_model``, the device's recurrence in float64, and ``eigen_replay``, the device's evaluation of the tridiagonal T it
REPORTED, operation by operation.  The device estimates lambda from below by lo - rho (a bracket of T's smallest eigenvalue
and Lanczos' residual bound) where the reference calls symmeig.

The approximations that work on the sparse Q of the program itself (``Hqp_IpMatrix.q_gerschgorin``, ``q_dscale_setup``,
``q_dscale_update``; hqpkkt_q_*) have their models at the end: ``q_gerschgorin_model``, ``dscale_terms`` - Hqp_HL_DScale::update
with the reference's operations and sequential sums - and ``dscale_replay``, the device's decision and update from the sums
it REPORTED.

The reference's default, Hqp_HL_BFGS, on the sparse Q itself (``Hqp_IpMatrix.q_blocks``, ``q_bfgs_update``; hqpkkt_q_blocks,
hqpkkt_q_bfgs_update) closes the file: ``q_blocks_model`` is Hqp_HL_BFGS::next_block, ``q_bfgs_terms`` the update of every block
with the reference's operations and sequential sums - on the stored entries alone under ``pattern`` -, and ``q_bfgs_replay``
the device's decision and its two steps of every stored entry from the sums it REPORTED and the Q s it returned.

The y of all these updates is a difference of two gradients of the Lagrangian; ``grad_l_dense_model`` is grad L = c - A'y - C'z
for a program whose dynamics rows are dense blocks (``IpLQDOCP.lagrangian_gradient_staged``, hqpkkt_lagrangian_gradient_staged),
in longdouble, with the term counts and magnitudes its error bound needs.
"""
from __future__ import annotations

import numpy as np


def bfgs_terms(s, y, Qs, offsets, gamma=0.1, alpha=1.0):
    """(U, coef) of the damped BFGS update of every block: U = [v, Qs], two vectors of n, and coef of shape (blocks, 2)
    with the rows (1 / s'v, -1 / s'Qs), so that Q+ = Q + coef[k, 0] v_k v_k' + coef[k, 1] (Qs)_k (Qs)_k' over block k.
    ``offsets``: the blocks' first indices and n behind them (blocks + 1 ascending ints); ``Qs``: Q s over all blocks
    (``IpLQDOCP.hessian_product(s)``).  A block with s'v = 0 or s'Qs = 0 keeps its Q: both coefficients are exactly 0."""
    s, y, Qs = (np.ascontiguousarray(a, dtype=np.float64) for a in (s, y, Qs))
    offsets = np.asarray(offsets, dtype=np.int64)
    if not (s.shape == y.shape == Qs.shape == (int(offsets[-1]),)) or offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("bfgs_terms: s, y and Qs are vectors of offsets[-1] entries")
    if gamma < 0.0:  # damping adapted to the step length
        gamma = -gamma + (1.0 + gamma) * (1.0 - alpha)
    v = y.copy()
    coef = np.zeros((offsets.size - 1, 2))
    for k in range(offsets.size - 1):
        b = slice(int(offsets[k]), int(offsets[k + 1]))
        sv, sQs = float(s[b] @ y[b]), float(s[b] @ Qs[b])
        if sv < gamma * sQs:  # Powell's modification
            theta = (1.0 - gamma) * sQs / (sQs - sv)
            v[b] = theta * y[b] + (1.0 - theta) * Qs[b]
            sv = float(s[b] @ v[b])
        if sv != 0.0 and sQs != 0.0 and np.isfinite(sv) and np.isfinite(sQs):
            coef[k] = 1.0 / sv, -1.0 / sQs
    return [v, Qs], coef


def bfgs_replay(report, s, y, Qs, offsets):
    """(v, coef) of ``IpLQDOCP.bfgs_update_device`` (hqpkkt_bfgs_update_stage_hessians) repeated in numpy from the sums the
    device REPORTED: ``report`` is ``IpLQDOCP.bfgs_report()``, (blocks, 8), of which sy (0), sQs (1), gamma_eff (2) and sv
    (4) are read.  One numpy operation per rounded operation of k_hb_terms (staged_hess_bfgs.hip.h): the test
    sy < fl(gamma_eff sQs), theta = fl(fl((1 - gamma_eff) sQs) / fl(sQs - sy)), omt = fl(1 - theta),
    v_i = fl(fl(theta y_i) + fl(omt Qs_i)), c0 = fl(1 / sv), c1 = -fl(1 / sQs); v = y on a block that is not damped, both
    coefficients exactly 0 where sv or sQs is zero or not finite.  ``s`` is not read: the sums come from the report."""
    report = np.asarray(report, dtype=np.float64)
    y, Qs = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, Qs))
    offsets = np.asarray(offsets, dtype=np.int64)
    if report.shape != (offsets.size - 1, 8) or not (y.shape == Qs.shape == (int(offsets[-1]),)):
        raise ValueError("bfgs_replay: report of (blocks, 8), y and Qs vectors of offsets[-1] entries")
    v = y.copy()
    coef = np.zeros((offsets.size - 1, 2))
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for k in range(offsets.size - 1):
            b = slice(int(offsets[k]), int(offsets[k + 1]))
            sy, sQs, gamma, sv = (np.float64(report[k, j]) for j in (0, 1, 2, 4))
            if sy < gamma * sQs:
                theta = ((one - gamma) * sQs) / (sQs - sy)
                omt = one - theta
                v[b] = theta * y[b] + omt * Qs[b]
            else:
                sv = sy
            if sv != 0.0 and sQs != 0.0 and np.isfinite(sv) and np.isfinite(sQs):
                coef[k] = one / sv, -(one / sQs)
    return v, coef


EIG_MAX_STEPS = 128  # (HQPKKT_EIG_MAX_STEPS)
EIG_END_REL = 2.0 ** -40  # (HQPKKT_EIG_END_REL)


def restart_model(Q, eps):
    """restart_Q (hqp/Hqp_HL_BFGS.C:125-146): diag(min(max(eps, max_j |Q_ij|), 1 / eps)), the two comparisons in the
    reference's order."""
    Q = np.asarray(Q, dtype=np.float64)
    if Q.shape[0] == 0:
        return Q.copy()
    rm = np.abs(Q).max(axis=1)
    inv = np.float64(1.0) / np.float64(eps)
    t = np.where(eps > rm, np.float64(eps), rm)
    return np.diag(np.where(t < inv, t, inv))


def gerschgorin_model(Q, eps):
    """Hqp_HL_Gerschgorin::update (hqp/Hqp_HL_Gerschgorin.C:66-106) on a block: q_ii <- max(q_ii, sum_{j != i} |q_ij| + eps);
    every other entry stays."""
    Q = np.array(Q, dtype=np.float64)
    A = np.abs(Q)
    off = A.sum(axis=1) - np.diag(A) if Q.shape[0] else np.zeros(0)
    t = off + np.float64(eps)
    dg = np.diag(Q).copy()
    Q[np.diag_indices(Q.shape[0])] = np.where(t > dg, t, dg)
    return Q


def lanczos_start(order):
    """The start vector of stage order ``order`` before it is normalised: 1 + ((37 i + 11) mod 64) / 64."""
    i = np.arange(order, dtype=np.int64)
    return 1.0 + ((37 * i + 11) % 64) / 64.0


def lanczos_model(Q, theta, max_steps=0):
    """The device's recurrence on one block in float64 (k_he_start, k_he_step; numpy's sums run in another order than the
    device's).  Returns (g, steps, T): Gerschgorin's bound g = min_i (q_ii - sum_{j != i} |q_ij|), the steps taken - 0 where
    g >= theta or the order is 0: no recurrence runs - and T of shape (2, 128), alpha then beta."""
    Q = np.asarray(Q, dtype=np.float64)
    nz = Q.shape[0]
    T = np.zeros((2, EIG_MAX_STEPS))
    if nz == 0:
        return 0.0, 0, T
    A = np.abs(Q)
    g = float((np.diag(Q) - (A.sum(axis=1) - np.diag(A))).min())
    if g >= theta:
        return g, 0, T
    f = lanczos_start(nz)
    V = [f / np.sqrt(f @ f)]
    bprev, scale, steps = 0.0, 0.0, 0
    with np.errstate(all="ignore"):
        for j in range(min(max_steps if max_steps else 64, nz)):
            v = V[j]
            w = Q @ v
            alpha = float(v @ w)
            w = w - alpha * v
            if j > 0:
                w = w - bprev * V[j - 1]
            B = np.array(V)
            w = w - B.T @ (B @ w)  # (orthogonal to the whole basis once more: no second copies of a converged eigenvalue)
            beta = float(np.sqrt(w @ w))
            T[0, j], T[1, j] = alpha, beta
            steps = j + 1
            scale = max(scale, abs(alpha))
            if j + 1 >= nz or not beta > EIG_END_REL * scale:
                break
            scale = max(scale, beta)
            V.append(w / beta)
            bprev = beta
    return g, steps, T


def _nan_max(m, a):
    return a if (a > m or a != a) else m


def _nan_min(m, a):
    return a if (a < m or a != a) else m


def eigen_replay(order, g, theta, steps, T):
    """What the device does with one stage's T (k_he_ritz, staged_hess_guard.hip.h) repeated in numpy, one operation per
    device operation: from Gerschgorin's bound ``g``, the floor ``theta``, ``steps`` and ``T`` of shape (2, 128) as
    ``IpLQDOCP.eigen_report(with_T=True)`` returns them.  Returns a dict: lo, hi (the bracket of T's smallest eigenvalue by the
    Sturm count, 64 points per round), rho (Lanczos' residual bound from the twisted factorisation of T - lo I), lam = lo - rho, d (the shift),
    normT and the outcome 0 .. 5."""
    f8 = np.float64
    out = dict(lo=0.0, hi=0.0, rho=0.0, lam=0.0, d=0.0, normT=0.0, outcome=-1)
    if order == 0:
        out["outcome"] = 5
        return out
    if g >= theta:
        out["outcome"] = 0
        return out
    m = int(steps)
    al, be = np.asarray(T[0][:m], dtype=f8), np.asarray(T[1][:m], dtype=f8)
    with np.errstate(all="ignore"):
        b2 = be * be
        normT, gl, gu = f8(0.0), f8(np.inf), f8(-np.inf)
        for i in range(m):
            off = (abs(be[i - 1]) if i > 0 else f8(0.0)) + (abs(be[i]) if i < m - 1 else f8(0.0))
            normT = _nan_max(normT, abs(al[i]) + off)
            gl, gu = _nan_min(gl, al[i] - off), _nan_max(gu, al[i] + off)
        out["normT"] = float(normT)
        if not np.isfinite(normT):
            out["outcome"] = 4
            return out
        tol = f8(2.0 ** -50) * normT
        pivmin = max(f8(2.0 ** -104) * normT, f8(2.0 ** -1000))
        lo, hi = gl - tol, gu + tol
        c = np.arange(1, 65).astype(f8) / f8(65.0)
        rounds = 0
        while rounds < 32 and hi - lo > tol:
            x = lo + (hi - lo) * c
            p = al[0] - x
            cnt = (p < 0).astype(np.int64)
            for i in range(1, m):
                p = np.where(np.abs(p) < pivmin, np.where(p < 0, -pivmin, pivmin), p)
                p = (al[i] - x) - b2[i - 1] / p
                cnt += p < 0
            hit = cnt >= 1
            if not hit.any():
                lo = x[63]
            else:
                f = int(np.argmax(hit))
                hi = x[f]
                if f > 0:
                    lo = x[f - 1]
            rounds += 1
        pv = np.zeros(m)
        pv[0] = al[0] - lo
        for i in range(1, m + 1):
            p = pv[i - 1]
            if abs(p) < pivmin:
                p = -pivmin if p < 0 else pivmin
            pv[i - 1] = p
            if i < m:
                pv[i] = (al[i] - lo) - b2[i - 1] / p
        rv = np.zeros(m)
        rv[m - 1] = al[m - 1] - lo
        for i in range(m - 1, -1, -1):
            p = rv[i]
            if abs(p) < pivmin:
                p = -pivmin if p < 0 else pivmin
            rv[i] = p
            if i > 0:
                rv[i - 1] = (al[i - 1] - lo) - b2[i - 1] / p
        t, gmin = 0, f8(np.inf)
        for i in range(m):
            gam = abs((pv[i] + rv[i]) - (al[i] - lo))
            if gam < gmin:
                gmin, t = gam, i
        z = np.zeros(m)
        z[t] = 1.0
        for i in range(t - 1, -1, -1):
            z[i] = -((be[i] / pv[i]) * z[i + 1])
        for i in range(t, m - 1):
            z[i + 1] = -((be[i] / rv[i + 1]) * z[i])
        zz = f8(0.0)
        for i in range(m):
            zz = zz + z[i] * z[i]
        rho = abs(be[m - 1]) * (abs(z[m - 1]) / np.sqrt(zz))
        lam = lo - rho
        d, outcome = f8(0.0), 1
        if not np.isfinite(lam):
            outcome = 4
        elif lam < theta:
            d, outcome = f8(theta) - lam, 2 if rho <= f8(EIG_END_REL) * normT else 3
    out.update(lo=float(lo), hi=float(hi), rho=float(rho), lam=float(lam), d=float(d), outcome=outcome)
    return out


# ---- the approximations that work on the sparse Q of the program (Hqp_IpMatrix.q_gerschgorin, q_dscale_update) ----

def q_gerschgorin_model(Q, eps):
    """Hqp_HL_Gerschgorin::update = Hqp_HL::posdef on the sparse Q as ``Hqp_IpMatrix.q_gerschgorin`` applies it, on the CSR
    triple ``Q`` = (indptr, indices, data) of which the entries with col >= row exist: returns the new data,
    q_ii <- max(q_ii, fl(sum_{j != i} |q_ij| + eps)) with the reference's macro a > b ? a : b, the sum over row i of the
    symmetric image; every other value stays."""
    p, ix, x = (np.asarray(a) for a in Q)
    x = np.array(x, dtype=np.float64)
    n = p.size - 1
    rows = np.repeat(np.arange(n), np.diff(p))
    up = ix > rows
    off = np.zeros(n)
    np.add.at(off, rows[up], np.abs(x[up]))
    np.add.at(off, ix[up], np.abs(x[up]))
    t = off + np.float64(eps)
    dg = np.flatnonzero(ix == rows)
    q = x[dg]
    x[dg] = np.where(q > t[rows[dg]], q, t[rows[dg]])
    return x


def _dscale_blocks(n, bsize):
    B = int(bsize) if 0 < int(bsize) < n else n
    return [(o, min(o + B, n)) for o in range(0, n, B)] if n else []


def _seq_sums(keys, terms, size, start=0.0):
    """per key the sum of its terms in the order they stand, from +0.0 (in_prod); numpy's unbuffered add.at runs in order.
    ``start`` = -0.0: from the key's first term, whose sign a zero sum then keeps (-0.0 + t is t for every t)."""
    out = np.full(size, start)
    np.add.at(out, keys, terms)
    return out


def _damped(rep, of, y, Qs):
    """What the damped updates share - Hqp_HL_DScale::update_b_Q with Qs = fl(s q), Hqp_HL_BFGS::update_b_Q with Qs = Q s -
    from the sums in ``rep`` (columns 0 sy, 1 sQs, 2 gamma, 4 sv where damped), one numpy operation per rounded operation,
    all blocks at once: the decision, theta, v, sv as used, the blocks that are updated and the outcome codes.  ``of``: the
    block of every variable.  Returns (v, sqs, sv, ok, outcome, theta)."""
    one = np.float64(1.0)
    sy, sqs, gamma = (np.array(rep[:, j], dtype=np.float64) for j in (0, 1, 2))
    damp = sy < gamma * sqs
    theta = np.where(damp, ((one - gamma) * sqs) / (sqs - sy), one)
    omt = one - theta
    v = np.where(damp[of], theta[of] * y + omt[of] * Qs, y)
    sv = np.where(damp, rep[:, 4], sy)
    finite = np.isfinite(sv) & np.isfinite(sqs)
    ok = finite & (sv != 0.0) & (sqs != 0.0)
    outcome = np.where(~finite, 3, np.where(~ok, 2, np.where(damp, 1, 0))).astype(np.int64)
    return v, sqs, sv, ok, outcome, theta


def _dscale_apply(rep, s, y, q, blocks):
    """decision, theta, v and both steps of q of every block from the sums in ``rep``: ``_damped`` with fl(s q), then the
    two steps of the diagonal, one numpy operation per rounded operation of Hqp_HL_DScale::update_b_Q"""
    nb = len(blocks)
    if nb == 0:
        return y.copy(), q.copy(), np.zeros(0, dtype=np.int64), np.ones(0), np.zeros(0)
    of = np.repeat(np.arange(nb), [e - a for a, e in blocks])  # the block of every variable
    with np.errstate(all="ignore"):
        sq = s * q
        v, sqs, sv, ok, outcome, theta = _damped(rep, of, y, sq)
        t = q - (sq * sq) / sqs[of]
        qn = np.where(ok[of], t + (v * v) / sv[of], q)
    return v, qn, outcome, theta, sv


def dscale_terms(s, y, q, gamma=0.2, bsize=0):
    """Hqp_HL_DScale::update (hqp/Hqp_HL_DScale.C:92-176) on the diagonal ``q`` for the step ``s`` and the change ``y`` of the
    Lagrangian's gradient, block by block, with the reference's operations and its sequential sums (in_prod): returns
    (report, v, q_new), ``report`` in the layout of ``Hqp_IpMatrix.q_dscale_report`` - sy, sqs, gamma, theta, sv as used,
    first index, length, outcome.  As on the device a block whose sv or sqs is not finite is left alone (outcome 3; the
    reference would write NaN)."""
    s, y, q = (np.ascontiguousarray(a, dtype=np.float64) for a in (s, y, q))
    blocks = _dscale_blocks(s.size, bsize)
    nb = len(blocks)
    rep = np.zeros((nb, 8))
    one, g = np.float64(1.0), np.float64(gamma)
    if nb:
        of = np.repeat(np.arange(nb), [e - a for a, e in blocks])
        with np.errstate(all="ignore"):
            sq = s * q
            sy, sqs = _seq_sums(of, s * y, nb, -0.0), _seq_sums(of, sq * s, nb, -0.0)
            damp = sy < g * sqs
            theta = np.where(damp, ((one - g) * sqs) / (sqs - sy), one)
            sv = np.where(damp, _seq_sums(of, s * (theta[of] * y + (one - theta)[of] * sq), nb, -0.0), sy)
        rep[:, 0], rep[:, 1], rep[:, 2], rep[:, 4] = sy, sqs, g, sv
        rep[:, 5], rep[:, 6] = [a for a, _e in blocks], [e - a for a, e in blocks]
    v, qn, outcome, theta, sv = _dscale_apply(rep, s, y, q, blocks)
    rep[:, 3], rep[:, 4], rep[:, 7] = theta, sv, outcome
    return rep, v, qn


def dscale_replay(report, s, y, q, bsize=0):
    """(v, q_new, outcome) of ``Hqp_IpMatrix.q_dscale_update`` (hqpkkt_q_dscale_update) repeated in numpy from the sums the
    device REPORTED: of ``report``, (blocks, 8), sy (0), sqs (1), gamma (2) and - on a damped block - sv (4) are read.  One
    numpy operation per device operation: the test sy < fl(gamma sqs), theta = fl(fl((1 - gamma) sqs) / fl(sqs - sy)),
    v_i = fl(fl(theta y_i) + fl(fl(1 - theta) fl(s_i q_i))), q_i <- fl(q_i - fl(fl(sq_i sq_i) / sqs)), then
    q_i <- fl(q_i + fl(fl(v_i v_i) / sv)); v = y on a block that is not damped; q stays where sv or sqs is zero (outcome 2)
    or not finite (3)."""
    report = np.asarray(report, dtype=np.float64)
    s, y, q = (np.ascontiguousarray(a, dtype=np.float64) for a in (s, y, q))
    blocks = _dscale_blocks(s.size, bsize)
    if report.shape != (len(blocks), 8) or not (s.shape == y.shape == q.shape):
        raise ValueError("dscale_replay: report of (blocks, 8), s, y and q vectors of one length")
    v, qn, outcome, _theta, _sv = _dscale_apply(report, s, y, q, blocks)
    return v, qn, outcome


# ---- Hqp_HL_BFGS on the sparse Q of the program (Hqp_IpMatrix.q_blocks, q_bfgs_update) ----

def q_blocks_model(Qp, Qi, n, bsize):
    """Hqp_HL_BFGS::next_block (hqp/Hqp_HL_BFGS.C:257-292) on the pattern (Qp, Qi) of Q, rows ascending: returns (first, full),
    the blocks' first indices with n behind the last (empty for n = 0) and per block 1 where every (i, j), i <= j, of it is
    stored.  bsize < 0: a block grows while the last stored column of one of its rows reaches past its end; 0: one block;
    > 0: blocks of bsize, the last one shorter."""
    Qp, Qi = np.asarray(Qp, dtype=np.int64), np.asarray(Qi, dtype=np.int64)
    n, bsize = int(n), int(bsize)
    first = []
    b = 0
    while b < n:
        first.append(b)
        if bsize < 0:
            end = b
            while b <= end:
                last = int(Qi[Qp[b + 1] - 1]) if Qp[b + 1] > Qp[b] else b
                end = max(end, last)
                b += 1
        else:
            b += min(bsize, n - b) if bsize > 0 else n - b
    if n:
        first.append(n)
    first = np.array(first, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(Qp[: n + 1])) if n else np.zeros(0, dtype=np.int64)
    full = np.zeros(max(first.size - 1, 0), dtype=np.int64)
    for k in range(full.size):
        a, e = int(first[k]), int(first[k + 1])
        lo, hi = int(Qp[a]), int(Qp[e])
        c, r = Qi[lo:hi], rows[lo:hi]
        full[k] = int(((c >= r) & (c < e)).sum()) == (e - a) * (e - a + 1) // 2
    return first, full


def _q_bfgs_entries(Q_csr, first):
    """rows and columns of Q's entries, the block of every variable, and the mask of the entries an update may touch:
    col >= row, both in one block"""
    p, ix, x = (np.asarray(a) for a in Q_csr)
    n = p.size - 1
    first = np.asarray(first, dtype=np.int64)
    if n and (first.size < 2 or first[0] != 0 or first[-1] != n or (np.diff(first) <= 0).any()):
        raise ValueError("first: the blocks' first indices, ascending from 0, and n behind the last")
    rows = np.repeat(np.arange(n), np.diff(p))
    of = np.repeat(np.arange(max(first.size - 1, 0)), np.diff(first)) if n else np.zeros(0, dtype=np.int64)
    ix = ix.astype(np.int64)
    inb = (ix >= rows) & (of[rows] == of[ix]) if n else np.zeros(0, dtype=bool)
    return rows, ix, np.array(x, dtype=np.float64), of, inb


def _q_bfgs_apply(rep, rows, ix, x, of, inb, y, Qs):
    """decision, theta, v and both steps of every stored entry from the sums in ``rep``: ``_damped`` with Q s, then the two
    steps of the entries an update may touch, one numpy operation per rounded operation, all blocks at once"""
    nb = rep.shape[0]
    if nb == 0:
        return y.copy(), x.copy(), np.zeros(0, dtype=np.int64), np.ones(0), np.zeros(0)
    with np.errstate(all="ignore"):
        v, sqs, sv, ok, outcome, theta = _damped(rep, of, y, Qs)
        xn = x.copy()
        k = np.flatnonzero(inb)
        k = k[ok[of[rows[k]]]]
        r, c, b = rows[k], ix[k], of[rows[k]]
        t = x[k] - (Qs[r] * Qs[c]) / sqs[b]
        xn[k] = t + (v[r] * v[c]) / sv[b]
    return v, xn, outcome, theta, sv


def q_bfgs_terms(Q_csr, s, y, first, gamma=0.1, alpha=1.0, pattern=False):
    """Hqp_HL_BFGS::update (hqp/Hqp_HL_BFGS.C:150-251, without its eigenvalue control) on the CSR triple ``Q_csr`` = (indptr,
    indices, data), of which the entries with col >= row exist, for the blocks ``first`` (``q_blocks_model``): per block the
    reference's operations with its sequential sums - (Q s)_i over row i of the block's symmetric image by ascending column,
    s'y, s'(Q s), s'v by ascending index.  Returns (report, v, Qs, Qx_new): ``report`` in the layout of
    ``Hqp_IpMatrix.q_bfgs_report``, v as applied, the block-restricted Q s and the new data.  ``pattern``: the stored entries
    of a block alone are updated (the operator of Hqp_HL_Gangster); otherwise a block that is not fully stored raises
    ValueError.  As on the device a block whose sv or sQs is not finite is left alone (outcome 3)."""
    s, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (s, y))
    rows, ix, x, of, inb = _q_bfgs_entries(Q_csr, first)
    n, nb = s.size, max(np.asarray(first).size - 1, 0)
    first = np.asarray(first, dtype=np.int64)
    if not pattern:
        cnt = np.bincount(of[rows[inb]], minlength=nb) if nb else np.zeros(0)
        ln = np.diff(first) if nb else np.zeros(0)
        if (cnt != ln * (ln + 1) // 2).any():
            raise ValueError("q_bfgs_terms: a block is not fully stored (pattern=False)")
    if gamma < 0.0:  # damping adapted to the step length, as bfgs_terms forms it
        gamma = -gamma + (1.0 + gamma) * (1.0 - alpha)
    g = np.float64(gamma)
    rep = np.zeros((nb, 8))
    with np.errstate(all="ignore"):
        # the block's symmetric image, row by row in ascending column order
        st = inb & (ix > rows)
        r2, c2, v2 = np.concatenate([rows[inb], ix[st]]), np.concatenate([ix[inb], rows[st]]), np.concatenate([x[inb], x[st]])
        o = np.lexsort((c2, r2))
        Qs = _seq_sums(r2[o], v2[o] * s[c2[o]], n)
        sy, sqs = _seq_sums(of, s * y, nb), _seq_sums(of, s * Qs, nb)
        one = np.float64(1.0)
        damp = sy < g * sqs
        theta = np.where(damp, ((one - g) * sqs) / (sqs - sy), one)
        if nb:
            vd = theta[of] * y + (one - theta)[of] * Qs
            sv = np.where(damp, _seq_sums(of, s * vd, nb), sy)
            rep[:, 0], rep[:, 1], rep[:, 2], rep[:, 4], rep[:, 5], rep[:, 6] = sy, sqs, g, sv, first[:-1], np.diff(first)
    v, xn, outcome, theta, sv = _q_bfgs_apply(rep, rows, ix, x, of, inb, y, Qs)
    if nb:
        rep[:, 3], rep[:, 4], rep[:, 7] = theta, sv, outcome
    return rep, v, Qs, xn


def q_bfgs_replay(report, Q_csr, y, Qs, first):
    """(v, Qx_new, outcome) of ``Hqp_IpMatrix.q_bfgs_update`` (hqpkkt_q_bfgs_update) repeated in numpy from the sums the device
    REPORTED and the ``Qs`` it returned: of ``report``, (blocks, 8), sy (0), sQs (1), gamma_eff (2) and - on a damped block -
    sv (4) are read.  One numpy operation per device operation: the test sy < fl(gamma_eff sQs), theta = fl(fl((1 - gamma_eff)
    sQs) / fl(sQs - sy)), v_i = fl(fl(theta y_i) + fl(fl(1 - theta) Qs_i)), and for every stored (i, j), j >= i, inside an
    updated block q <- fl(q - fl(fl(Qs_i Qs_j) / sQs)), then q <- fl(q + fl(fl(v_i v_j) / sv)); v = y on a block that is not
    damped; a block stays where sv or sQs is zero (outcome 2) or not finite (3).  ``Q_csr`` holds the data before the update."""
    report = np.asarray(report, dtype=np.float64)
    y, Qs = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, Qs))
    rows, ix, x, of, inb = _q_bfgs_entries(Q_csr, first)
    if report.shape != (max(np.asarray(first).size - 1, 0), 8) or not (y.shape == Qs.shape == (np.asarray(Q_csr[0]).size - 1,)):
        raise ValueError("q_bfgs_replay: report of (blocks, 8), y and Qs vectors of n entries")
    v, xn, outcome, _theta, _sv = _q_bfgs_apply(report, rows, ix, x, of, inb, y, Qs)
    return v, xn, outcome


# ---- the eigenvalue control of Hqp_HL_BFGS on the blocks of the sparse Q (Hqp_IpMatrix.q_eigen_control) ----

def q_block_dense(Q_csr, first, b):
    """Block ``b`` of the partition ``first`` (``q_blocks_model``) as ``Hqp_IpMatrix.q_eigen_control`` sees it: the symmetric
    image of the stored entries of the CSR triple ``Q_csr`` with col >= row and both indices in the block (what
    symsp_extract_mat extracts), a dense matrix with zeros where nothing is stored."""
    rows, ix, x, of, inb = _q_bfgs_entries(Q_csr, first)
    a, e = int(first[b]), int(first[b + 1])
    k = np.flatnonzero(inb & (rows >= a) & (rows < e))
    B = np.zeros((e - a, e - a))
    B[rows[k] - a, ix[k] - a] = x[k]
    B[ix[k] - a, rows[k] - a] = x[k]
    return B


def q_lanczos_model(Q_csr, first, theta, max_steps=0):
    """``lanczos_model`` on every block of the partition ``first`` of the sparse Q, the products through the CSR triple - a
    block of 8193 needs no dense matrix.  ``theta``: one floor, or one per block.  Returns (g, steps, T): per block
    Gerschgorin's bound over the block's own entries, the steps taken (0 where g >= theta: no recurrence runs) and T of
    shape (blocks, 2, cap), alpha then beta, cap = min(max_steps or 64, longest block) - the stride of
    ``Hqp_IpMatrix.q_eigen_report(with_T=True)``.  numpy's sums run in another order than the device's."""
    rows, ix, x, of, inb = _q_bfgs_entries(Q_csr, first)
    first = np.asarray(first, dtype=np.int64)
    n, nb = np.asarray(Q_csr[0]).size - 1, max(first.size - 1, 0)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), (nb,))
    cap = int(min(max_steps if max_steps else 64, np.diff(first).max())) if nb else 0
    g, steps, T = np.zeros(nb), np.zeros(nb, dtype=np.int64), np.zeros((nb, 2, cap))
    # the blocks' symmetric image as one list of entries, and the diagonal
    st = inb & (ix > rows)
    r2, c2, v2 = np.concatenate([rows[inb], ix[st]]), np.concatenate([ix[inb], rows[st]]), np.concatenate([x[inb], x[st]])
    dg = np.zeros(n)
    dk = inb & (ix == rows)
    np.add.at(dg, rows[dk], x[dk])
    off = np.zeros(n)
    od = r2 != c2
    with np.errstate(all="ignore"):
        np.add.at(off, r2[od], np.abs(v2[od]))
    for b in range(nb):
        a, e = int(first[b]), int(first[b + 1])
        nz = e - a
        g[b] = (dg[a:e] - off[a:e]).min()  # (a NaN is kept)
        if g[b] >= theta[b]:
            continue
        k = np.flatnonzero((r2 >= a) & (r2 < e))
        rb, cb, vb = r2[k] - a, c2[k] - a, v2[k]

        def mult(v):
            w = np.zeros(nz)
            np.add.at(w, rb, vb * v[cb])
            return w

        f = lanczos_start(nz)
        V = [f / np.sqrt(f @ f)]
        bprev, scale = 0.0, 0.0
        with np.errstate(all="ignore"):
            for j in range(min(cap, nz)):
                v = V[j]
                w = mult(v)
                alpha = float(v @ w)
                w = w - alpha * v
                if j > 0:
                    w = w - bprev * V[j - 1]
                B = np.array(V)
                w = w - B.T @ (B @ w)
                beta = float(np.sqrt(w @ w))
                T[b, 0, j], T[b, 1, j] = alpha, beta
                steps[b] = j + 1
                scale = max(scale, abs(alpha))
                if j + 1 >= nz or not beta > EIG_END_REL * scale:
                    break
                scale = max(scale, beta)
                V.append(w / beta)
                bprev = beta
    return g, steps, T


def grad_l_dense_model(dq, c, y, z, dtype=np.longdouble):
    """(g, L, mag) of ``IpLQDOCP.lagrangian_gradient_staged`` (hqpkkt_lagrangian_gradient_staged) for a
    :class:`hqp_amd.problems.DenseDocp`: g = c - A'y - C'z in ``dtype`` (numpy longdouble; int64 for integer data), with the
    dynamics rows of A taken from the blocks - row li of stage k is [F_k[li], -1.0 at component li of x_{k+1}] - then
    the rows of E and C.  ``y`` in the reference's row order: the dynamics rows first, then the rows of E.  Per variable
    i also L_i, the number of terms of t_i = (A'y + C'z)_i - the rows of its stage's block, one for the -y of the row
    that produces a state of a stage k > 0, the stored entries of column i of E and of C - and mag_i, the sum of the
    terms' absolute values: a sum of those terms rounded in ANY order, each term rounded once, lies within
    (L_i + 3) 2^-53 (mag_i + |c_i|) of g_i once c_i has been subtracted."""
    nx, nu, K = dq.nx, dq.nu, dq.K
    n, ndyn = dq.n, dq.ndyn
    y, z, c = (np.asarray(a).astype(dtype) for a in (y, z, c))
    if c.shape != (n,) or y.shape != (dq.me,) or z.shape != (dq.m,):
        raise ValueError("grad_l_dense_model: c, y, z are vectors of n, me, m entries")
    t, mag = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    L = np.zeros(n, dtype=np.int64)
    col0 = row0 = 0
    for k in range(K + 1):
        if k > 0:  # the -1.0 of the rows that produce x_k
            prev = y[row0 - nx[k]: row0]
            t[col0: col0 + nx[k]] -= prev
            mag[col0: col0 + nx[k]] += np.abs(prev)
            L[col0: col0 + nx[k]] += 1
        if k == K:
            break
        nz, np_ = nx[k] + nu[k], nx[k + 1]
        F = np.asarray(dq.F[k].cpu().numpy() if hasattr(dq.F[k], "data_ptr") else dq.F[k])
        if F.shape != (np_, nz):
            raise ValueError("grad_l_dense_model: F[%d] is not nx[k+1] x (nx[k] + nu[k])" % k)
        terms = F.astype(dtype) * y[row0: row0 + np_, None]
        t[col0: col0 + nz] += terms.sum(axis=0)
        mag[col0: col0 + nz] += np.abs(terms).sum(axis=0)
        L[col0: col0 + nz] += np_
        col0 += nz
        row0 += np_
    for (p, ix, v), vec in ((dq.E, y[ndyn:]), (dq.C, z)):
        p, ix = np.asarray(p), np.asarray(ix)
        v = np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v)
        if v.size == 0:
            continue
        w = v.astype(dtype) * vec[np.repeat(np.arange(p.size - 1), np.diff(p))]
        np.add.at(t, ix, w), np.add.at(mag, ix, np.abs(w)), np.add.at(L, ix, 1)
    return c - t, L, mag
