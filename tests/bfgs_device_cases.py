"""Shapes and operands of the damped BFGS update of the dense stage Hessians on the device
(hqpkkt_bfgs_update_stage_hessians; test_staged_bfgs_device_cpu.py, test_gpu_staged_bfgs_device.py).

k_hb_terms gives a stage to one workgroup of 256 threads, thread t the entries t, t + 256, ..: the orders here lie around
that stride and its double - (255, 257, 512) one entry short of a trip, one into the second, two whole trips; (513, 1, 2) one
into the third, and stages of order 1 and 2, whose first columns are odd.  The tests add them to
hessian_update_cases.ORDERS, the orders at the edges of the update kernel's 128-wide tile."""
import numpy as np

import hessian_update_cases as H

ORDERS = [(255, 257, 512), (513, 1, 2)]
ALL_ORDERS = list(H.ORDERS) + ORDERS


def spd_blocks(rng, nz):
    """Positive-definite blocks with full mantissas, D (A A' + nz I) D with D = diag(10^[-1, 1]): entries over 10^+-2."""
    out = []
    for v in nz:
        A = rng.standard_normal((v, v))
        d = 10.0 ** rng.uniform(-1, 1, v)
        B = (A @ A.T + v * np.eye(v)) * np.outer(d, d)
        out.append(np.triu(B) + np.triu(B, 1).T)
    return out


def spread(rng, k):
    """Full mantissas, magnitudes over 10^+-2, no zero."""
    return rng.standard_normal(k) * 10.0 ** rng.uniform(-2, 2, k)


KINDS = ("undamped", "negative", "zero")


def chain_operands(nz, seed, shift=0):
    """(blocks, s, y, kinds) with one stage of each kind, stage k of kind KINDS[(k + shift) % 3]: y = 2 Qs + noise (s'y about
    2 s'Qs: not damped), y = -Qs + noise (s'y < 0: damped), y = 0 (damped, s'v = gamma s'Qs); Qs in numpy."""
    rng = np.random.default_rng(seed)
    off = H.offsets(nz)
    blocks = spd_blocks(rng, nz)
    s = spread(rng, int(off[-1]))
    y = np.zeros_like(s)
    kinds = []
    for k, B in enumerate(blocks):
        b = slice(int(off[k]), int(off[k + 1]))
        Qs = B @ s[b]
        kind = KINDS[(k + shift) % 3]
        kinds.append(kind)
        noise = 0.01 * np.abs(Qs) * rng.standard_normal(Qs.size)
        if kind == "undamped":
            y[b] = 2.0 * Qs + noise
        elif kind == "negative":
            y[b] = -Qs + noise
    return blocks, s, y, kinds


def dot_bound(a, b):
    """n 2^-53 sum |a_i||b_i|: the bound of an n-term dot product in any order, fused or not (longdouble)."""
    a, b = (np.abs(np.asarray(x)).astype(np.longdouble) for x in (a, b))
    return a.size * np.longdouble(2.0) ** -53 * (a @ b)


def gamma_eff(gamma, alpha):
    """The damping factor as hessian_update.bfgs_terms writes it."""
    if gamma < 0.0:
        gamma = -gamma + (1.0 + gamma) * (1.0 - alpha)
    return gamma


def int_operands(nz, seed):
    """(blocks, s, y, Q s) in int64: positive-definite integer blocks (int_blocks(spd=True)), s integers 1 <= |s| <= 2^6, y = 2 Q s + e
    with e in -2 .. 2 - s'y about 2 s'Qs, so no stage damps -, and every sum of the update below 2^53 (asserted in int64)."""
    rng = np.random.default_rng(seed)
    off = H.offsets(nz)
    blocks = H.int_blocks(rng, nz, spd=True)
    n = int(off[-1])
    s = rng.integers(1, 2 ** 6 + 1, n) * rng.choice([-1, 1], n)
    Qs = np.concatenate([B @ s[off[k]: off[k + 1]] for k, B in enumerate(blocks)])
    y = 2 * Qs + rng.integers(-2, 3, n)
    for k, B in enumerate(blocks):
        b = slice(int(off[k]), int(off[k + 1]))
        assert int((np.abs(B) @ np.abs(s[b])).max()) < 2 ** 53
        assert int(np.abs(s[b]) @ np.abs(y[b])) < 2 ** 53 and int(np.abs(s[b]) @ np.abs(Qs[b])) < 2 ** 53
    return blocks, s.astype(np.int64), y.astype(np.int64), Qs.astype(np.int64)
