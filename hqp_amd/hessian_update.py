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

The eigenvalue control that the reference can run after it (an eigenvalue decomposition per block, then a shift of the
diagonal) is not built; its effect, a diagonal shift, is ``update_stage_hessians(..., diag=shift)`` with beta = 1.

``IpLQDOCP.bfgs_update_device`` (hqpkkt_bfgs_update_stage_hessians) forms the same terms on the device; ``bfgs_replay`` is its
numpy model, operation by operation from the sums the device reports.
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
