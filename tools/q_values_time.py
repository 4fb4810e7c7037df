"""Times of the entries on the sparse Q against the round trip through hqpkkt_set_values (profiles/q_values_time.txt).

Handle: problems.grid_sparse_qp(gx, gy) with Hqp_IpRedSpBKP, ordering=2, device vectors - analysis and values alone, no
factorisation.  Per call by wall clock to a device synchronisation, mean of --reps after --warmup, the paths taking turns:
  (a) q_dscale_update, bsize 0      (b) the same, bsize 64      (c) q_gerschgorin      (d) q_product
  (e) lagrangian_gradient           (f) hqpkkt_set_values of a HOST-vector handle of the same program from its pinned
  hqpkkt_values_staging buffers - the route to the same change without these entries (the staging buffers are host
  memory: a device-vector handle does not take them)  (g) hqpkkt_set_values of the device handle from device arrays.
  (h) q_bfgs_update, blocks detected, on a second handle: a block-diagonal Q of --bfgs-blocks fully stored blocks of order
  --bfgs-order with n / 2 bounds      (i) q_bfgs_update, bsize 0, the stored entries alone (PATTERN), on the grid's handle.
Bytes: what the call must move at the least - every operand once per pass that needs it, and the regather of Q's image
behind a write - and the rate that makes at the measured time.

    python tools/q_values_time.py [--gx 1000 --gy 1000 --reps 20 --warmup 3 --out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hqp_amd import _lib, ipmatrix, problems  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gx", type=int, default=1000)
    ap.add_argument("--gy", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bfgs-blocks", type=int, default=125000)
    ap.add_argument("--bfgs-order", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    prog = problems.grid_sparse_qp(a.gx, a.gy)
    n, me, m = prog.dims
    t0 = time.perf_counter()
    M = ipmatrix.IpRedSpBKP(device_vectors=True, ordering=2)
    M.init(prog)
    Hh = ipmatrix.IpRedSpBKP(device_vectors=False, ordering=2)
    Hh.init(prog)
    t_init = time.perf_counter() - t0
    # the block-diagonal program of (h): SPD blocks, upper triangles stored
    nb, k = a.bfgs_blocks, a.bfgs_order
    rngb = np.random.default_rng(2)
    Bm = rngb.uniform(-1.0, 1.0, (nb, k, k))
    Bm = Bm @ Bm.transpose(0, 2, 1) / k + np.eye(k) * rngb.uniform(0.5, 1.5, (nb, k, 1))
    bi, bj = np.triu_indices(k)
    off = (np.arange(nb) * k)[:, None]
    nB = nb * k
    Qb = problems._csr((off + bi).ravel(), (off + bj).ravel(), Bm[:, bi, bj].ravel(), nB)
    none = problems._csr([], [], [], 0)
    Cb = problems._csr(np.arange(nB // 2), 2 * np.arange(nB // 2), np.ones(nB // 2), nB // 2)
    progb = problems.Program(nB, 0, nB // 2, Qb, none, Cb, d=-np.ones(nB // 2))
    t0 = time.perf_counter()
    Mb = ipmatrix.IpRedSpBKP(device_vectors=True, ordering=2)
    Mb.init(progb)
    t_initb = time.perf_counter() - t0
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    tens = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    p, ix, qx = (np.asarray(v) for v in prog.Q)
    rows = np.repeat(np.arange(n), np.diff(p))
    q = np.asarray(qx, dtype=np.float64)[ix == rows]
    s_h = rng.normal(size=n)
    s, y = tens(s_h), tens(1.1 * q * s_h)
    x, c, out, v = tens(rng.normal(size=n)), tens(prog.c), tens(np.zeros(n)), tens(np.zeros(n))
    yy, zz = tens(rng.normal(size=me)), tens(rng.normal(size=m))
    dQ, dA, dC = tens(prog.Q[2]), tens(prog.A[2]), tens(prog.C[2])
    sq, sa, sc = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.hqpkkt_values_staging(Hh._h, C.byref(sq), C.byref(sa), C.byref(sc)) == 0
    for ptr, val in ((sq, prog.Q[2]), (sa, prog.A[2]), (sc, prog.C[2])):
        val = np.ascontiguousarray(val, dtype=np.float64)
        if val.size:
            C.memmove(ptr.value, val.ctypes.data, val.nbytes)
    P = lambda t: C.c_void_p(t.data_ptr())
    sb_h = rngb.normal(size=nB)
    sb, yb = tens(sb_h), tens(1.1 * np.einsum("bij,bj->bi", Bm, sb_h.reshape(nb, k)).ravel())

    def bfgs(H, s_, y_, bsize, fill):
        u = _lib.QBfgsUpdate()
        u.s, u.y, u.gamma, u.alpha, u.bsize, u.fill = s_.data_ptr(), y_.data_ptr(), 0.1, 1.0, bsize, fill
        return lambda: L.hqpkkt_q_bfgs_update(H._h, C.byref(u))

    def dscale(bsize):
        u = _lib.DScaleUpdate()
        u.s, u.y, u.gamma, u.bsize = s.data_ptr(), y.data_ptr(), 0.2, bsize
        return lambda: L.hqpkkt_q_dscale_update(M._h, C.byref(u))

    paths = [
        ("a q_dscale_update bsize 0", dscale(0)),
        ("b q_dscale_update bsize 64", dscale(64)),
        ("c q_gerschgorin", lambda: L.hqpkkt_q_gerschgorin(M._h, 1e-3)),
        ("d q_product", lambda: L.hqpkkt_q_product(M._h, P(x), P(out))),
        ("e lagrangian_gradient", lambda: L.hqpkkt_lagrangian_gradient(M._h, P(c), P(yy), P(zz), None, P(out))),
        ("f set_values, host handle, pinned staging", lambda: L.hqpkkt_set_values(Hh._h, sq, sa, sc)),
        ("g set_values, device handle, device arrays", lambda: L.hqpkkt_set_values(M._h, P(dQ), P(dA), P(dC))),
        ("h q_bfgs_update detected blocks, block-diag Q", bfgs(Mb, sb, yb, -1, _lib.HQPKKT_QBFGS_FULL)),
        ("i q_bfgs_update bsize 0 PATTERN, the grid", bfgs(M, s, y, 0, _lib.HQPKKT_QBFGS_PATTERN)),
    ]
    nq, na, nc = len(prog.Q[2]), len(prog.A[2]), len(prog.C[2])
    nqf = 2 * nq - n  # entries of the symmetric image (every row has its diagonal)
    regather = nqf * (4 + 8 + 8)
    walk_q = nqf * 12 + (n + 1) * 4
    nqb = len(Qb[2])
    nqfb = 2 * nqb - nB

    def bfgs_bytes(n_, nq_, nqf_):
        # the row pass over the image with the block table, s in and Qs out; the sums read s, y, Qs; v out of y; the update per
        # stored entry: row, column, kind, the value in and out, Qs, v and the block table gathered; the regather of the image
        return nqf_ * 12 + (n_ + 1) * 4 + n_ * 4 + 2 * n_ * 8 + 3 * n_ * 8 + 2 * n_ * 8 + nq_ * (12 + 16) + 2 * n_ * 8 + n_ * 4 + nqf_ * (4 + 8 + 8)

    bytes_min = {
        "h": bfgs_bytes(nB, nqb, nqfb),
        "i": bfgs_bytes(n, nq, nqf),
        "a": 3 * n * 8 + 4 * n * 8 + 2 * n * 4 + regather,  # the sums read s, y, q; the update reads them again and writes q; the diagonal's index twice
        "b": 3 * n * 8 + 4 * n * 8 + 2 * n * 4 + regather,
        "c": walk_q + 2 * n * 8 + 2 * n * 8 + n * 4 + regather,  # the row pass, offsum out and in, the diagonal read and written
        "d": walk_q + 2 * n * 8,
        "e": (na + nc) * 12 + 2 * (n + 1) * 4 + (me + m) * 8 + 2 * n * 8,
        "f": (nq + na + nc) * 8 * 2 + (nqf + 2 * na + 2 * nc) * (4 + 8 + 8),  # the copy, every CSR copy gathered
        "g": (nq + na + nc) * 8 * 2 + (nqf + 2 * na + 2 * nc) * (4 + 8 + 8),
    }
    times = {nm: [] for nm, _f in paths}
    torch.cuda.synchronize()
    for r in range(a.warmup + a.reps):
        for nm, fn in paths:
            t = time.perf_counter()
            e = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            assert e == 0, (nm, e)
            if r >= a.warmup:
                times[nm].append(dt)
    lines = [f"grid_sparse_qp({a.gx}, {a.gy}), Hqp_IpRedSpBKP, ordering 2: n {n} me {me} m {m}, nnz Q {nq} A {na} C {nc}; "
             f"analysis + values of both handles {t_init:.1f} s",
             f"(h): {nb} full blocks of order {k}, Hqp_IpRedSpBKP, ordering 2: n {nB} me 0 m {nB // 2}, nnz Q {nqb}; analysis + values {t_initb:.1f} s",
             f"device {torch.cuda.get_device_name(0)}; mean of {a.reps} after {a.warmup}, wall clock to a device synchronisation",
             f"{'path':46s} {'mean us':>10s} {'min us':>10s} {'max us':>10s} {'MB at least':>12s} {'GB/s':>8s}"]
    for nm, _f in paths:
        t = np.array(times[nm])
        b = bytes_min[nm[0]]
        lines.append(f"{nm:46s} {t.mean() * 1e6:10.1f} {t.min() * 1e6:10.1f} {t.max() * 1e6:10.1f} {b / 1e6:12.2f} {b / t.mean() / 1e9:8.1f}")
    fm = np.mean(times[paths[5][0]])
    for k in (0, 2):
        tm = np.mean(times[paths[k][0]])
        lines.append(f"({paths[k][0][0]}) is {'below' if tm < fm else 'NOT below'} (f): {tm * 1e6:.1f} us against {fm * 1e6:.1f} us")
    gm = np.mean(times[paths[6][0]])
    for k2 in (7, 8):
        tm = np.mean(times[paths[k2][0]])
        lines.append(f"({paths[k2][0][0]}): {tm * 1e6:.1f} us against (f) {fm * 1e6:.1f} us and (g) {gm * 1e6:.1f} us"
                     + (" - (f) and (g) are the grid's, whose Q has other sizes" if k2 == 7 else ""))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
