"""The GPU checks of hqpkkt_lagrangian_gradient_staged (tests/test_gpu_grad_l_staged.py starts this once, as a child
process): every case runs on the device and the outcomes go to stdout as one JSON line, {check: "ok" | failures}.  A case
that ends in a device error ends the run: nothing more is started on the GPU.

Shapes, built directly as DenseDocp with per-stage sizes - the smallest at which each guard of k_st_grad_l can fail (a
workgroup takes 256 columns of a stage, wavefront w the rows w, w + 4, .., eight of them per trip):
  1  K = 1, nx = [3, 2], nu = [1]                  np = 2: two wavefronts have no row
  2  K = 3, nx = [5, 1, 70, 33], nu = [2, 1, 7]    np = 1; sizes change from stage to stage; np = 70 and 33: full trips and a tail
  3  K = 2, nx = [250, 37, 300], nu = [9, 3]       nz = 259: a second column block of 3 columns; np = 37 and 300, no multiples
                                                   of 32; the block-less last stage of 300 columns spans two column blocks
  4  K = 4, nx = nu = 64 throughout                exact multiples
  5  K = 2, nx = [3, 2, 2], nu = [1, 0]            a stage without controls (hqpkkt_analyze_staged accepts it); the gradient alone
Each shape with me_rest = 0 and me_rest > 0 (the rows that fix x_0 and one or two final-state rows), with m = 0 (z = NULL)
and m > 0 (a bound per control, one on the first state of every stage k >= 1, a row over three columns of stage 0 and one
over two of stage K), and over them four handles: (caller's ldF = nz, host vectors, sparse Q), (ldF = nz + 5, device
vectors, sparse Q), (ldF = nz, device vectors, q_dense), (ldF = nz + 5, host vectors, q_dense).

Bounds.  Integer operands (|values| <= 8, sums below 2^53): exact against int64, whatever the order.  Real operands: a sum
of L terms in ANY order, each term rounded once (fused or not), and the subtraction from c lie within
(L_i + 3) 2^-53 (sum |terms|_i + |c_i|) of the exact value - hessian_update.grad_l_dense_model gives the exact value in
longdouble, L_i and the sum; with minus the result is one rounded subtraction from the first, bit for bit."""
import ctypes as C
import json
import sys
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu

U = 2.0 ** -53
SHAPES = {
    1: ([3, 2], [1]),
    2: ([5, 1, 70, 33], [2, 1, 7]),
    3: ([250, 37, 300], [9, 3]),
    4: ([64] * 5, [64] * 4),
    5: ([3, 2, 2], [1, 0]),
}
# (extra columns of the caller's F rows, device vectors, q_dense)
HANDLES = ((0, False, False), (5, True, False), (0, True, True), (5, False, True))
C0, C1, OUTCOME = 5, 6, 7  # (columns of bfgs_report)


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def spd_blocks(rng, orders):
    out = []
    for v in orders:
        A = rng.uniform(-1.0, 1.0, (v, v))
        out.append(A @ A.T / max(v, 1) + np.diag(rng.uniform(0.5, 1.5, v)))
    return out


def make_docp(shape, with_e, with_c, integers, seed=0):
    """The DenseDocp of a shape: F, E, C, c with full mantissas (integers: nonzero integers |v| <= 8), a diagonal Q, and the
    stage Hessians Qd for the q_dense handles."""
    nx, nu = SHAPES[shape]
    K = len(nu)
    rng = np.random.default_rng(1000 * shape + 10 * seed + 2 * with_e + with_c + (100 if integers else 0))
    nz = [nx[k] + nu[k] for k in range(K)] + [nx[K]]
    col0 = np.concatenate([[0], np.cumsum(nz)])
    n = int(col0[-1])

    def vals(shape_):
        if integers:
            return (rng.integers(1, 9, shape_) * rng.choice([-1, 1], shape_)).astype(np.float64)
        return rng.uniform(0.25, 1.0, shape_) * rng.choice([-1.0, 1.0], shape_) * 10.0 ** rng.integers(-1, 2, shape_)

    F = [vals((nx[k + 1], nz[k])) for k in range(K)]
    er, ec = [], []
    if with_e:
        er, ec = list(range(nx[0])), list(range(nx[0]))  # x_0 fixed
        nf = 1 if sum(nu) < 2 else min(2, nx[K])  # final-state rows: no more than there are controls to meet them
        for j in range(nf):
            er.append(nx[0] + j), ec.append(int(col0[K]) + j)
    me_rest = (max(er) + 1) if er else 0
    E = problems._csr(np.array(er, dtype=int), np.array(ec, dtype=int), vals(len(er)), me_rest)
    cr, cc = [], []
    if with_c:
        row = 0
        for k in range(K):
            for j in range(nu[k]):
                cr.append(row), cc.append(int(col0[k]) + nx[k] + j)
                row += 1
        for k in range(1, K + 1):
            cr.append(row), cc.append(int(col0[k]))
            row += 1
        for c_ in sorted({0, nx[0] - 1, nx[0]} if nu[0] else {0, nx[0] - 1}):
            cr.append(row), cc.append(c_)
        row += 1
        for c_ in sorted({int(col0[K]), int(col0[K]) + nx[K] - 1}):
            cr.append(row), cc.append(c_)
        row += 1
    m = (max(cr) + 1) if cr else 0
    Cm = problems._csr(np.array(cr, dtype=int), np.array(cc, dtype=int), vals(len(cr)), m)
    Q = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), rng.uniform(0.5, 1.5, n))
    dq = problems.DenseDocp(nx, nu, Q, E, Cm, F, me_rest, m, c=vals(n), d=np.ones(m))
    dq.Qd_blocks = spd_blocks(rng, nz)
    return dq


def vectors(dq, integers, seed):
    rng = np.random.default_rng(seed)
    n, me, m = dq.dims
    if integers:
        return tuple(rng.integers(-8, 9, k).astype(np.float64) for k in (me, m, n))
    return rng.normal(size=me), rng.normal(size=m), rng.normal(size=n)


def program_from_dense(dq):
    """The same program in Hqp_Docp's CSR layout: row li of stage k = [F_k[li], -1.0 at component li of x_{k+1}], then E."""
    nx, nu, K = dq.nx, dq.nu, dq.K
    col0 = np.concatenate([[0], np.cumsum([nx[k] + nu[k] for k in range(K)])])
    ar, ac, av = [], [], []
    row = 0
    for k in range(K):
        np_, nz = nx[k + 1], nx[k] + nu[k]
        r = row + np.arange(np_)
        ar.append(np.repeat(r, nz)), ac.append(np.tile(col0[k] + np.arange(nz), np_)), av.append(np.asarray(dq.F[k]).ravel())
        ar.append(r), ac.append(col0[k + 1] + np.arange(np_)), av.append(np.full(np_, -1.0))
        row += np_
    p, ix, x = (np.asarray(a) for a in dq.E)
    ar.append(row + np.repeat(np.arange(p.size - 1), np.diff(p))), ac.append(ix), av.append(x)
    A = problems._csr(np.concatenate(ar).astype(int), np.concatenate(ac).astype(int), np.concatenate(av), dq.me)
    prog = problems.Program(dq.n, dq.me, dq.m, dq.Q, A, dq.C, c=dq.c, b=dq.b, d=dq.d)
    prog.nx, prog.nu = list(nx), list(nu)
    return prog


class Vecs:
    """numpy in, numpy out, whatever the handle's vectors are"""

    def __init__(self, device):
        self.device = device

    def to(self, a):
        if a is None or not self.device:
            return a
        import torch
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()

    @staticmethod
    def np(a):
        return None if a is None else (a.cpu().numpy() if hasattr(a, "data_ptr") else a)


def hand_over(M, dq, pad, device, q_dense):
    """update_dense with the caller's F rows `pad` columns longer than the block: views of wider arrays (device: torch
    tensors with a row stride; host: straight through hqpkkt_set_values_staged, which takes ldF)"""
    wide = []
    for blk in dq.F:
        w = np.full((blk.shape[0], blk.shape[1] + pad), np.nan)
        w[:, : blk.shape[1]] = blk
        wide.append(w)
    d2 = problems.DenseDocp(dq.nx, dq.nu, dq.Q, dq.E, dq.C, wide, dq.me_rest, dq.m, c=dq.c, b=dq.b, d=dq.d,
                            Qd=dq.Qd_blocks if q_dense else None)
    if device:
        import torch
        d2.F = [torch.as_tensor(w).cuda()[:, : w.shape[1] - pad] for w in wide]
        if q_dense:
            d2.Qd = [torch.as_tensor(np.ascontiguousarray(q)).cuda() for q in d2.Qd]
        return d2
    if pad == 0:
        return d2
    # host vectors, ldF > nz: update_dense would compact the views, so the blocks go through the ABI
    if q_dense:
        for k, blk in enumerate(d2.Qd):
            M.set_stage_hessian(k, blk)
    L = _lib.lib()
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in ((np.zeros(0) if q_dense else dq.Q[2]), dq.E[2], dq.C[2])]
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    fp, ld = (C.c_void_p * dq.K)(), (C.c_longlong * dq.K)()
    for k, w in enumerate(wide):
        fp[k], ld[k] = w.ctypes.data, w.shape[1]
    code = L.hqpkkt_set_values_staged(M._h, ptr(keep[0]), fp, ld, ptr(keep[1]), ptr(keep[2]))
    if code:
        raise ipmatrix.KktError(code, "set_values_staged")
    return None


def handle(dq, pad, device, q_dense):
    M = ipmatrix.IpLQDOCP(device_vectors=device, q_dense=q_dense)
    if not device and pad:
        d0 = problems.DenseDocp(dq.nx, dq.nu, dq.Q, dq.E, dq.C, dq.F, dq.me_rest, dq.m, Qd=dq.Qd_blocks if q_dense else None)
        M.init_dense(d0)  # (analysis and a first hand-over; the padded one replaces every value)
        hand_over(M, dq, pad, device, q_dense)
    else:
        M.init_dense(hand_over(M, dq, pad, device, q_dense))
    return M


def bound(L, mag, c):
    return (L + 3) * U * (mag + np.abs(np.asarray(c, dtype=np.longdouble)))


def solve_bits(M, V, dq, st, refactor):
    """factor (or not) + solve: the results, or the code of an entry that refuses (never a device error)"""
    out = []
    try:
        if refactor:
            M.factor(dq, V.to(st[0]), V.to(st[1]))
        d = [V.to(np.zeros(k)) for k in (dq.n, dq.me, dq.m, dq.m)]
        res = M.solve(dq, *(V.to(a) for a in st), *d)
        out += [V.np(a).copy() for a in d] + [np.float64(res)]
    except ipmatrix.KktError as e:
        if e.code == _lib.E_DEVICE:
            raise
        out.append(np.float64(-e.code))
    return out


# ------------------------------------------------------------------------------------------------ the cases
def case(shape, with_e, with_c, fail):
    """all checks of one (shape, me_rest, m) on its four handles; fail(check, tag, message) records a failure"""
    ld = np.longdouble
    dqi, dqr = make_docp(shape, with_e, with_c, True), make_docp(shape, with_e, with_c, False)
    yi, zi, mi = vectors(dqi, True, 7)
    yr, zr, mr = vectors(dqr, False, 11)
    gi, _L, _mag = hu.grad_l_dense_model(dqi, dqi.c, yi, zi, dtype=np.int64)
    want_i = gi.astype(np.float64)
    want_i2 = (gi - mi.astype(np.int64)).astype(np.float64)
    gr, Lr, magr = hu.grad_l_dense_model(dqr, dqr.c, yr, zr)
    bnd = bound(Lr, magr, dqr.c)
    # the CSR hand-over of the same two programs
    csr = {}
    for nm, dq, (y, z, mi_) in (("int", dqi, (yi, zi, mi)), ("real", dqr, (yr, zr, mr))):
        prog = program_from_dense(dq)
        Mc = ipmatrix.IpLQDOCP()
        Mc.set_stages(dq.nx, dq.nu)
        Mc.init(prog)
        csr[nm] = Mc.lagrangian_gradient(dq.c, y, z)
        if nm == "real":
            cnt = np.zeros(dq.n, dtype=np.int64)
            for Mx in (prog.A, prog.C):
                np.add.at(cnt, np.asarray(Mx[1]), 1)
            if not (cnt == Lr).all():
                fail("both_hand_overs", (shape, with_e, with_c), "the model's term counts are not the CSR columns' lengths")
    if not bits(csr["int"], want_i):
        fail("both_hand_overs", (shape, with_e, with_c), "the CSR entry is not exact on the integer program")
    ref_bits = {}
    for pad, device, q_dense in HANDLES:
        tag = (shape, with_e, with_c, pad, device, q_dense)
        V = Vecs(device)
        for nm, dq, (y, z, mi_) in (("int", dqi, (yi, zi, mi)), ("real", dqr, (yr, zr, mr))):
            M = handle(dq, pad, device, q_dense)
            zz = z if dq.m else None
            st = problems.ip_state(dq, seed=12, spread=1.0)
            before = solve_bits(M, V, dq, st, True) if (nm == "real" and shape != 5) else None
            g = V.np(M.lagrangian_gradient_staged(V.to(dq.c), V.to(y), V.to(zz)))
            g2 = V.np(M.lagrangian_gradient_staged(V.to(dq.c), V.to(y), V.to(zz), minus=V.to(mi_)))
            again = V.np(M.lagrangian_gradient_staged(V.to(dq.c), V.to(y), V.to(zz)))
            if not bits(g, again):
                fail("repeatable", tag, "two calls differ (%s)" % nm)
            if nm in ref_bits and not (bits(ref_bits[nm][0], g) and bits(ref_bits[nm][1], g2)):
                fail("repeatable", tag, "the bits differ from the first handle's (%s): host / device vectors, ldF, the form of Q" % nm)
            ref_bits.setdefault(nm, (g, g2))
            if nm == "int":
                if not bits(g, want_i):
                    fail("integers", tag, "not the int64 result at %s" % np.flatnonzero(g != want_i)[:8].tolist())
                if not bits(g2, want_i2):
                    fail("integers", tag, "with minus: not the int64 result at %s" % np.flatnonzero(g2 != want_i2)[:8].tolist())
                if not bits(g, csr["int"]):
                    fail("both_hand_overs", tag, "integer data: the two hand-overs differ")
            else:
                err = np.abs(g.astype(ld) - gr)
                worst = float((err / np.maximum(bnd, np.finfo(ld).tiny)).max())
                print(f"reals {tag}: largest error / bound {worst:.3f}", file=sys.stderr)
                if not (err <= bnd).all():
                    fail("reals", tag, "error above (L + 3) 2^-53 (sum |terms| + |c|) at %s, largest ratio %.3f" % (np.flatnonzero(err > bnd)[:8].tolist(), worst))
                if not bits(g2, g - mr):
                    fail("reals", tag, "with minus: not fl(g - minus)")
                if not (np.abs(g.astype(ld) - csr["real"].astype(ld)) <= 2 * bnd).all():
                    fail("both_hand_overs", tag, "the two hand-overs differ by more than the sum of their bounds")
                if before is not None:
                    after = solve_bits(M, V, dq, st, False)  # (the factorisation made before the calls)
                    fresh = solve_bits(M, V, dq, st, True)
                    for what, b in (("the same factorisation", after), ("a new factorisation", fresh)):
                        if len(before) != len(b) or not all(bits(p, q) for p, q in zip(before, b)):
                            fail("no_side_effects", tag, "factor + solve differ after the calls (%s)" % what)
                    if len(before) > 1 and not all(np.isfinite(a).all() for a in before):
                        fail("no_side_effects", tag, "the solve is not finite")


def check_refusals(fail):
    """HQPKKT_E_INTERN from the new entry on a STAGED handle of the CSR hand-over and on a FULL handle, both with values; the old
    entry still refuses the dense handle, and the new one serves it."""
    L = _lib.lib()
    prog = problems.lq_docp(4, 3, 2)
    n, me, m = prog.dims
    x, y, z = np.ones(n), np.ones(me), np.ones(m)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for cls in (ipmatrix.IpLQDOCP, ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):
        M = cls()
        M.init(prog)
        out = np.full(n, 7.0)
        code = L.hqpkkt_lagrangian_gradient_staged(M._h, vp(x), vp(y), vp(z), None, vp(out))
        if code != _lib.E_INTERN or not (out == 7.0).all():
            fail("refusals", cls.__name__, "code %d on a handle of the CSR hand-over" % code)
        M.lagrangian_gradient(x, y, z)  # (the entry for such a handle)
    Mc = ipmatrix.IpLQDOCP()
    Mc.init(prog)
    try:
        Mc.lagrangian_gradient_staged(x, y, z)
        fail("refusals", "method", "accepted on the CSR hand-over")
    except ipmatrix.KktError as e:
        if e.code != _lib.E_INTERN:
            fail("refusals", "method", "code %d" % e.code)
    D = ipmatrix.IpLQDOCP()
    D.init_dense(problems.dense_docp_from_program(prog, [3] * 5, [2] * 4))
    try:
        D.lagrangian_gradient(x, y, z)
        fail("refusals", "old entry", "accepted the dense handle")
    except ipmatrix.KktError as e:
        if e.code != _lib.E_INTERN:
            fail("refusals", "old entry", "code %d" % e.code)
    if not (np.abs(D.lagrangian_gradient_staged(x, y, z) - Mc.lagrangian_gradient(x, y, z)) <= 1e-12).all():
        fail("refusals", "dense handle", "the new entry does not serve it")
    if L.hqpkkt_lagrangian_gradient_staged(D._h, vp(x), None, vp(z), None, vp(x.copy())) != _lib.E_NULL:
        fail("refusals", "dense handle", "y = NULL with me > 0 is not HQPKKT_E_NULL")


def check_end_to_end(fail):
    """Shape 3, q_dense, host and device vectors: g_old with the old blocks, new F blocks and a new c handed over, y = g_new
    with minus = g_old, fed to bfgs_update_device.  y lies within the two gradients' bounds (and the subtraction's rounding)
    of the model's; where its bits are the model's y, rounded the same way, a second handle fed the model's y has the same
    blocks; either way the update is hessian_update.bfgs_replay's from the reported sums on the device's y: v and the
    coefficients bit for bit, and the blocks those of a fresh handle given update_stage_hessians([v, Qs], coefficients)."""
    ld = np.longdouble
    old, new = make_docp(3, True, True, False, seed=1), make_docp(3, True, True, False, seed=2)
    new.Qd_blocks = old.Qd_blocks
    y, z, _mi = vectors(old, False, 21)
    s = np.random.default_rng(22).normal(size=old.n)
    g0, L0, mag0 = hu.grad_l_dense_model(old, old.c, y, z)
    g1, L1, mag1 = hu.grad_l_dense_model(new, new.c, y, z)
    g0f, g1f = g0.astype(np.float64), g1.astype(np.float64)
    y_model = g1f - g0f
    bnd = bound(L0, mag0, old.c) + bound(L1, mag1, new.c)
    nz = [old.nx[k] + old.nu[k] for k in range(old.K)] + [old.nx[old.K]]
    off = np.concatenate([[0], np.cumsum(nz)])
    views = lambda M: [M.stage_hessian(k) for k in range(len(nz))]
    ref = None
    for pad, device in ((0, False), (5, True)):
        tag = ("end_to_end", pad, device)
        V = Vecs(device)
        M = handle(old, pad, device, True)
        g_old = M.lagrangian_gradient_staged(V.to(old.c), V.to(y), V.to(z))
        if not (np.abs(V.np(g_old).astype(ld) - g0) <= bound(L0, mag0, old.c)).all():
            fail("end_to_end", tag, "g_old outside its bound")
        d2 = hand_over(M, new, pad, device, True)
        if d2 is not None:
            M.update_dense(d2)
        y_dev = M.lagrangian_gradient_staged(V.to(new.c), V.to(y), V.to(z), minus=g_old)
        yd = V.np(y_dev).copy()
        err = np.abs(yd.astype(ld) - (g1 - g0))
        ybnd = bnd * (1 + U) + U * np.abs(g1 - g0)  # (the subtraction rounds a difference within bnd of g1 - g0)
        if not (err <= ybnd).all():
            fail("end_to_end", tag, "y outside the sum of the two gradients' bounds")
        Qs = V.np(M.hessian_product(V.to(s))).copy()
        v = V.np(M.bfgs_update_device(V.to(s), y_dev, want_v=True)).copy()
        rep = M.bfgs_report()
        if not set(rep[:, OUTCOME].tolist()) <= {0.0, 1.0}:
            fail("end_to_end", tag, "outcomes %s" % rep[:, OUTCOME].tolist())
        got = views(M)
        same = bits(yd, y_model)
        print(f"end_to_end {tag}: y differs from the model's in {int((yd != y_model).sum())} of {yd.size} entries, "
              f"largest error / bound {float((err / ybnd).max()):.3f}", file=sys.stderr)
        if same:
            R = handle(new, pad, device, True)
            R.bfgs_update_device(V.to(s), V.to(y_model))
            if not all(bits(a, b) for a, b in zip(got, views(R))):
                fail("end_to_end", tag, "the blocks differ from those of the update fed the model's y")
        vr, cr = hu.bfgs_replay(rep, s, yd, Qs, off)
        if not (bits(v, vr) and bits(rep[:, C0: C1 + 1], cr)):
            fail("end_to_end", tag, "v or the coefficients are not bfgs_replay's from the reported sums")
        R = handle(new, 0, False, True)
        R.update_stage_hessians([v, Qs], rep[:, C0: C1 + 1])
        want = views(R)
        if not all(np.isfinite(a).all() and bits(a, b) for a, b in zip(got, want)):
            fail("end_to_end", tag, "the blocks differ from update_stage_hessians([v, Qs], the reported coefficients)")
        if all(bits(a, b) for a, b in zip(got, views(handle(new, 0, False, True)))):
            fail("end_to_end", tag, "the blocks have not changed")
        if ref is not None and not (bits(ref[0], yd) and all(bits(a, b) for a, b in zip(ref[1], got))):
            fail("end_to_end", tag, "host and device vectors give different bits")
        ref = ref or (yd, got)


CHECKS = ("integers", "reals", "both_hand_overs", "repeatable", "no_side_effects", "refusals", "end_to_end")


def main():
    failures = {nm: [] for nm in CHECKS}
    dead = None

    def fail(check, tag, message):
        failures[check].append(f"{tag}: {message}")

    def run(what, fn, *args):
        nonlocal dead
        if dead:
            return
        try:
            fn(*args, fail)
        except ipmatrix.KktError as e:
            if e.code == _lib.E_DEVICE:
                dead = f"{what}: device error, nothing more was run\n{traceback.format_exc()}"
            else:
                for nm in CHECKS:
                    failures[nm].append(f"{what}: {traceback.format_exc()}")
        except Exception:
            for nm in CHECKS:
                failures[nm].append(f"{what}: {traceback.format_exc()}")

    for shape in SHAPES:
        for with_e in (False, True):
            for with_c in (False, True):
                run(f"case {(shape, with_e, with_c)}", case, shape, with_e, with_c)
    run("refusals", check_refusals)
    run("end_to_end", check_end_to_end)
    results = {}
    for nm in CHECKS:
        msgs = failures[nm] + ([dead] if dead else [])
        results[nm] = "ok" if not msgs else "\n".join(msgs)
    print("GRAD_L_STAGED_RESULTS " + json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
