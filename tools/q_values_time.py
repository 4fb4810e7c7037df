"""Times of the entries on the sparse Q against the round trip through hqpkkt_set_values (profiles/q_values_time.txt).

Handle: problems.grid_sparse_qp(gx, gy) with Hqp_IpRedSpBKP, ordering=2, device vectors - analysis and values alone, no
factorisation.  Per call by wall clock to a device synchronisation, mean of --reps after --warmup, the paths taking turns:
  (a) q_dscale_update, bsize 0      (b) the same, bsize 64      (c) q_gerschgorin      (d) q_product
  (e) lagrangian_gradient           (f) hqpkkt_set_values of a HOST-vector handle of the same program from its pinned
  hqpkkt_values_staging buffers - the route to the same change without these entries (the staging buffers are host
  memory: a device-vector handle does not take them)  (g) hqpkkt_set_values of the device handle from device arrays.
  (h) q_bfgs_update, blocks detected, on a second handle: a block-diagonal Q of --bfgs-blocks fully stored blocks of order
  --bfgs-order with n / 2 bounds      (i) q_bfgs_update, bsize 0, the stored entries alone (PATTERN), on the grid's handle.
  (j) q_eigen_control on the detected blocks of (h)'s handle (the cap is the blocks' order)      (k) q_eigen_control, bsize 0
  (one block of n, 64 steps), on a third handle of the grid whose diagonal is lowered by 8 so that Gerschgorin's bound does
  not settle the block; its values are set again, untimed, before every call.
  (m), (n) the route through the host that (k) and (j) replace, without the host's eigen-solver, which comes on top:
  hqpkkt_q_values out to host memory and hqpkkt_set_values in from the pinned staging buffers, on host-vector handles of
  the grid and of the block-diagonal program.
Bytes: what the call must move at the least - every operand once per pass that needs it, and the regather of Q's image
behind a write - and the rate that makes at the measured time.
  (s) --staged K NX NU: hqpkkt_lagrangian_gradient_staged on a handle of the dense hand-over, next to the residual's pass
  over the same F blocks (staged_gradient_rows below); a run of its own, appended to --out.

    python tools/q_values_time.py [--gx 1000 --gy 1000 --reps 20 --warmup 3 --out FILE]
    python tools/q_values_time.py --staged 200 5000 50 [--reps 20 --warmup 3 --out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hqp_amd import _lib, ipmatrix, problems  # noqa: E402


def staged_gradient_rows(K, nx, nu, reps, warmup):
    """(s) hqpkkt_lagrangian_gradient_staged on the headline's handle: bench.c4_dense(K, nx, nu) - the F blocks made on the
    device -, Hqp_IpLQDOCP, device vectors, analysis and values alone.  Next to it, on the same handle in the same
    session, the pass it shares its loads with: the residual's products with the dense dynamics rows, k_st_dyn_both +
    k_st_dyn_ax_finish (both products, one sweep over F).
    Times.  (s) by wall clock to a device synchronisation, as the rows above, and by the handle's events around its one
    launch (class "vector" of hqpkkt_set_profile).  The residual's pass by the events of its class "residual" over one
    hqpkkt_residual: the two kernels of the pass and the residual's own kernel over Q, E, C and the vectors - n + me + m
    rows against 40 GB of F at the headline.  hqpkkt_residual is what collects the events, so (s)'s event time is the
    class "vector" of (s) + a residual less that of a residual alone; the two kinds of round take turns.
    GB/s: the bytes of the F blocks over the time."""
    import torch
    from bench import c4_dense
    dq = c4_dense(K, nx, nu)
    fbytes = 8 * sum(int(blk.numel()) for blk in dq.F)
    t0 = time.perf_counter()
    M = ipmatrix.IpLQDOCP(device_vectors=True)
    M.init_dense(dq)
    t_init = time.perf_counter() - t0
    dq.F = None  # (the engine holds its own copy)
    torch.cuda.empty_cache()
    n, me, m = dq.dims
    L = _lib.lib()
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda k, lo=-1.0, hi=1.0: torch.empty(k, dtype=torch.float64, device="cuda").uniform_(lo, hi, generator=g)
    c, y, z, out = rnd(n), rnd(me), rnd(m), rnd(n)
    zz, ww = rnd(m, 0.1, 1.1), rnd(m, 0.1, 1.1)
    r = [rnd(k) for k in (n, me, m, m)]
    d = [rnd(k) for k in (n, me, m, m)]
    P = lambda t: C.c_void_p(t.data_ptr())
    res = C.c_double()
    grad = lambda: L.hqpkkt_lagrangian_gradient_staged(M._h, P(c), P(y), P(z), None, P(out))
    resid = lambda: L.hqpkkt_residual(M._h, P(zz), P(ww), *(P(t) for t in r), *(P(t) for t in d), C.byref(res))
    wall, ev = [], {"alone": [], "with": []}
    torch.cuda.synchronize()
    for rep in range(warmup + reps):
        t = time.perf_counter()
        e = grad()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        assert e == 0, e
        if rep >= warmup:
            wall.append(dt)
        for kind in ("alone", "with"):
            M.set_profile(True)
            assert (grad() if kind == "with" else 0) == 0 and resid() == 0
            torch.cuda.synchronize()
            p = M.profile()
            M.set_profile(False)
            if rep >= warmup:
                ev[kind].append((p["vector"][0], p["vector"][1], p["residual"][0], p["residual"][1]))
    a, w = np.array(ev["alone"]), np.array(ev["with"])
    wall = np.array(wall)
    g_ev = w[:, 0] - a[:, 0].mean()
    rs = np.concatenate([a[:, 2], w[:, 2]])
    gb = lambda ms: fbytes / (ms * 1e-3) / 1e9
    spread = rs.max() - rs.min()
    lines = [
        f"c4_dense({K}, {nx}, {nu}), Hqp_IpLQDOCP, dense hand-over, device vectors: n {n} me {me} m {m}, F {fbytes / 1e9:.2f} GB; analysis + values {t_init:.1f} s",
        f"device {torch.cuda.get_device_name(0)}; {reps} rounds after {warmup}; launches per call by class: (s) vector {int(w[0, 1] - a[0, 1])}, "
        f"hqpkkt_residual vector {int(a[0, 1])} residual {int(a[0, 3])}",
        f"{'path':58s} {'mean ms':>9s} {'min ms':>9s} {'max ms':>9s} {'GB/s of F':>10s}",
        f"{'s lagrangian_gradient_staged, wall clock to a synchronise':58s} {wall.mean() * 1e3:9.3f} {wall.min() * 1e3:9.3f} {wall.max() * 1e3:9.3f} {gb(wall.mean() * 1e3):10.1f}",
        f"{'s lagrangian_gradient_staged, events (k_st_grad_l)':58s} {g_ev.mean():9.3f} {g_ev.min():9.3f} {g_ev.max():9.3f} {gb(g_ev.mean()):10.1f}",
        f"{'residual class: k_st_dyn_both + k_st_dyn_ax_finish + k_residual':58s} {rs.mean():9.3f} {rs.min():9.3f} {rs.max():9.3f} {gb(rs.mean()):10.1f}",
        f"(s) by events is {'below' if g_ev.mean() < rs.mean() else 'NOT below'} the residual's pass: {g_ev.mean():.3f} ms against {rs.mean():.3f} ms, "
        f"whose spread over the rounds is {spread:.3f} ms",
    ]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--staged", type=int, nargs=3, metavar=("K", "NX", "NU"), default=None,
                    help="the rows of hqpkkt_lagrangian_gradient_staged at this DOCP alone (the headline: 200 5000 50); --out is appended to")
    ap.add_argument("--gx", type=int, default=1000)
    ap.add_argument("--gy", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bfgs-blocks", type=int, default=125000)
    ap.add_argument("--bfgs-order", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.staged:
        text = "\n".join(staged_gradient_rows(*a.staged, a.reps, a.warmup))
        print(text)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
        return
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
    Hb = ipmatrix.IpRedSpBKP(device_vectors=False, ordering=2)
    Hb.init(progb)
    t_initb = time.perf_counter() - t0
    # the grid with its diagonal lowered, for (k)
    pk, ixk, qxk = (np.asarray(v) for v in prog.Q)
    qlow = np.array(qxk, dtype=np.float64)
    qlow[ixk == np.repeat(np.arange(n), np.diff(pk))] -= 8.0
    progk = problems.Program(n, me, m, (prog.Q[0], prog.Q[1], qlow), prog.A, prog.C, prog.c, prog.b, prog.d)
    Mk = ipmatrix.IpRedSpBKP(device_vectors=True, ordering=2)
    Mk.init(progk)
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
    dQk = tens(qlow)

    def staging(H, pr):
        ptrs = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert L.hqpkkt_values_staging(H._h, *(C.byref(t) for t in ptrs)) == 0
        for ptr, val in zip(ptrs, (pr.Q[2], pr.A[2], pr.C[2])):
            val = np.ascontiguousarray(val, dtype=np.float64)
            if val.size:
                C.memmove(ptr.value, val.ctypes.data, val.nbytes)
        return ptrs

    sq, sa, sc = staging(Hh, prog)
    bq, ba, bc = staging(Hb, progb)
    qout, qoutb = np.zeros(len(prog.Q[2])), np.zeros(len(Qb[2]))
    P = lambda t: C.c_void_p(t.data_ptr())
    sb_h = rngb.normal(size=nB)
    sb, yb = tens(sb_h), tens(1.1 * np.einsum("bij,bj->bi", Bm, sb_h.reshape(nb, k)).ravel())

    def bfgs(H, s_, y_, bsize, fill):
        u = _lib.QBfgsUpdate()
        u.s, u.y, u.gamma, u.alpha, u.bsize, u.fill = s_.data_ptr(), y_.data_ptr(), 0.1, 1.0, bsize, fill
        return lambda: L.hqpkkt_q_bfgs_update(H._h, C.byref(u))

    def eigen(H, bsize):
        e = _lib.QEigenControl()
        e.eps, e.bsize, e.floor_from_bfgs, e.max_steps = 2.0 ** -10, bsize, 0, 0
        return lambda: L.hqpkkt_q_eigen_control(H._h, C.byref(e))

    def host_route(H, buf, ptrs):
        return lambda: L.hqpkkt_q_values(H._h, C.c_void_p(buf.ctypes.data)) or L.hqpkkt_set_values(H._h, *ptrs)

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
        ("j q_eigen_control detected blocks, block-diag Q", eigen(Mb, -1)),
        ("k q_eigen_control bsize 0, the grid lowered", eigen(Mk, 0)),
        ("m q_values out + set_values in, host, the grid", host_route(Hh, qout, (sq, sa, sc))),
        ("n q_values out + set_values in, host, block-diag", host_route(Hb, qoutb, (bq, ba, bc))),
    ]
    prep = {"k": lambda: L.hqpkkt_set_values(Mk._h, P(dQk), P(dA), P(dC))}  # (untimed: the same block before every control)
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

    def eigen_bytes(n_, nq_, nqf_, steps):
        # the row pass with the block table and the diagonals; per step the product (the image, the block table, v in, w out),
        # v'w (2 n), the residual (w in and out, v_j, v_{j-1}), the second pass (w in and out), the next vector (w in, v out) and
        # the basis read twice, j + 1 vectors each time; the basis cleared; the shift; the regather of the image
        walk = nqf_ * 12 + (n_ + 1) * 4 + n_ * 4
        return (walk + 3 * n_ * 8 + n_ * 4 + steps * (walk + 2 * n_ * 8 + 2 * n_ * 8 + 4 * n_ * 8 + 2 * n_ * 8 + 2 * n_ * 8)
                + 2 * n_ * 8 * steps * (steps + 1) // 2 + steps * n_ * 8 + 2 * n_ * 8 + 2 * n_ * 4 + nqf_ * (4 + 8 + 8))

    bytes_min = {
        "j": eigen_bytes(nB, nqb, nqfb, min(64, k)),
        "k": eigen_bytes(n, nq, nqf, 64),
        "m": nq * 8 * 2 + (nq + na + nc) * 8 * 2 + (nqf + 2 * na + 2 * nc) * (4 + 8 + 8),
        "n": nqb * 8 * 2 + (nqb + nB // 2) * 8 * 2 + (nqfb + 2 * (nB // 2)) * (4 + 8 + 8),
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
            if nm[0] in prep:
                assert prep[nm[0]]() == 0
                torch.cuda.synchronize()
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
    hm, hn = np.mean(times[paths[11][0]]), np.mean(times[paths[12][0]])
    for k2, host, H in ((9, hn, Mb), (10, hm, Mk)):
        tm = np.mean(times[paths[k2][0]])
        r_ = H.q_eigen_report()
        oc = {int(o): int((r_[:, 9] == o).sum()) for o in np.unique(r_[:, 9])}
        lines.append(f"({paths[k2][0][0]}): {tm * 1e6:.1f} us, {'below' if tm < host else 'NOT below'} the route through the host ({'n' if k2 == 9 else 'm'}) "
                     f"{host * 1e6:.1f} us; steps at most {int(r_[:, 2].max())}, blocks by outcome {oc}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
