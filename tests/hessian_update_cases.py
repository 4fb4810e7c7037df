"""Shapes, operands and host references of the in-place update of the dense stage Hessians
(hqpkkt_update_stage_hessians; test_staged_hessian_update_cpu.py, test_gpu_staged_hessian_update.py).

K = 2 stages handed over densely with empty E and C and small random F.  Block orders at the edges of the 128-wide tile:
(313, 384, 220) a ragged odd last tile, whole tiles, the smallest order that packs; (402, 311, 320) a middle stage that keeps
its dense block on a packed handle; (256, 129, 640) one row into a second tile, five tile rows; (2, 1, 3) tiny."""
import numpy as np

from hqp_amd import ipmatrix, problems

ORDERS = [(313, 384, 220), (402, 311, 320), (256, 129, 640), (2, 1, 3)]
up8 = lambda v: (v + 7) // 8 * 8


def sizes(nz):
    """(nx, nu) of K = 2 stages with Q_k of the given orders: one control where the order leaves room for a state."""
    nu = [1 if v > 1 else 0 for v in nz[:2]]
    return [nz[0] - nu[0], nz[1] - nu[1], nz[2]], nu


def block_docp(nz, blocks, seed=1, bounds=False):
    """The dense hand-over with the given blocks Q_k (None: no Hessians handed over).  bounds: -1 <= u <= 1 on every
    control as rows of C (an interior-point loop then has something to iterate on); c random."""
    nx, nu = sizes(nz)
    rng = np.random.default_rng(seed)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    F = [0.1 * rng.uniform(-1, 1, (nx[k + 1], nx[k] + nu[k])) for k in range(2)]
    n = sum(nz)
    Cm, m, d = empty(0), 0, None
    if bounds:
        off = offsets(nz)
        ucols = np.array([off[k] + nx[k] + j for k in range(2) for j in range(nu[k])], dtype=np.int32)
        m = 2 * ucols.size
        Cm = (np.arange(m + 1, dtype=np.int32), np.repeat(ucols, 2).astype(np.int32), np.tile([1.0, -1.0], ucols.size))
        d = np.ones(m)
    return problems.DenseDocp(nx, nu, empty(n), empty(0), Cm, F, 0, m, c=rng.uniform(-1, 1, n), d=d, Qd=blocks)


def offsets(nz):
    return np.concatenate([[0], np.cumsum(nz)]).astype(np.int64)


def handle(packed, **opts):
    return ipmatrix.IpLQDOCP(q_dense=True, q_packed=packed, **opts)


def analyze_only(M, nz):
    """hqpkkt_analyze_staged alone: no block has arrived."""
    import ctypes as C
    nx, nu = (np.asarray(a, dtype=np.int32) for a in sizes(nz))
    vp = lambda a: C.c_void_p(a.ctypes.data)
    code = M._L.hqpkkt_analyze_staged(M._h, 2, vp(nx), vp(nu), int(sum(nz)), 0, 0, None, None, None, None, None, None)
    M.n, M.me, M.m = int(sum(nz)), int(nx[1] + nx[2]), 0
    return code


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def padded(B):
    """A block as it lies in the arena: order x up8(order), +0.0 in the padding."""
    P = np.zeros((B.shape[0], up8(B.shape[0])))
    P[:, : B.shape[0]] = B
    return P


def int_blocks(rng, nz, spd=False):
    """Symmetric integer blocks, |q| <= 2^20; spd: |q| <= 2^8 off the diagonal and strictly diagonally dominant."""
    out = []
    for v in nz:
        hi = 2 ** 8 if spd else 2 ** 20
        U = np.triu(rng.integers(-hi, hi + 1, (v, v)))
        B = U + np.triu(U, 1).T
        if spd:
            B[np.diag_indices(v)] = np.abs(B).sum(axis=1) + 1
        out.append(B.astype(np.int64))
    return out


def int_update(rng, nz, r, beta, with_diag, positive=False):
    """(U, coef, beta, diag) of integers: |u| <= 2^10, c in -3 .. 3 (positive: 1 .. 3), d in -2^10 .. 2^10 (positive: >= 0)."""
    n = int(sum(nz))
    U = [rng.integers(-2 ** 10, 2 ** 10 + 1, n).astype(np.float64) for _ in range(r)]
    coef = (rng.integers(1, 4, (len(nz), r)) if positive else rng.integers(-3, 4, (len(nz), r))).astype(np.float64)
    diag = rng.integers(0 if positive else -2 ** 10, 2 ** 10 + 1, n).astype(np.float64) if with_diag else None
    return U, coef, np.asarray(beta, dtype=np.float64), diag


def apply(blocks, nz, U, coef, beta, diag, dtype):
    """beta_k Q_k + diag(d_k) + sum_j c_kj u_jk u_jk' per stage in the given dtype (int64: exact on integer operands;
    longdouble: the reference of the real-operand bound), skipping what the device skips: a block with beta_k = 0 and a
    term with c_kj = 0 do not enter.  Returns (blocks, scales): scale_ij = |beta||Q_ij| + |d_i| [i = j] + sum |c||u_i||u_j|."""
    off = offsets(nz)
    out, scales = [], []
    for k, B in enumerate(blocks):
        sl = slice(int(off[k]), int(off[k + 1]))
        b = 1.0 if beta is None else float(beta[k])
        if b == 0.0:
            R, S = np.zeros(B.shape, dtype=dtype), np.zeros(B.shape, dtype=np.longdouble)
        else:
            R = np.asarray(B).astype(dtype) * dtype(b)
            S = np.abs(np.asarray(B).astype(np.longdouble)) * abs(b)
        if diag is not None:
            dk = np.asarray(diag[sl])
            R = R + np.diag(dk.astype(dtype))
            S = S + np.diag(np.abs(dk.astype(np.longdouble)))
        for j, u in enumerate(U):
            c = float(coef[k][j])
            if c == 0.0:
                continue
            uk = np.asarray(u[sl]).astype(dtype)
            R = R + dtype(c) * np.outer(uk, uk)
            S = S + abs(c) * np.outer(np.abs(uk).astype(np.longdouble), np.abs(uk).astype(np.longdouble))
        out.append(R)
        scales.append(S)
    return out, scales
