"""The GPU checks of the entries on the sparse Q (tests/test_gpu_q_values.py starts this once, as a child process): every
check of CHECKS runs on the device and the outcomes go to stdout as one JSON line, {name: "ok" | traceback}.  A check that
ends in a device error ends the run: nothing more is started on the GPU.

Shapes: a diagonal Q plus a band of 2 at n = 1 .. 8193 (around the lanes of a row, a workgroup, a chunk of 4096 and two
chunks), random_sparse_qp(150, 40, 90, row_nnz=3), grid_sparse_qp(14, 11) and lq_docp(4, 3, 2); handles Hqp_IpSpBKP,
Hqp_IpRedSpBKP and - on lq_docp, which has the stage structure - Hqp_IpLQDOCP; host and device vectors.

Bounds.  Integer operands (|values| <= 8, sums below 2^53): exact against int64.  Real operands: a sum of L terms in ANY
order lies within (L + 2) 2^-53 sum |terms| of the exact sum (L - 1 additions and the rounding of each term, fused or not),
so products and reported sums are held to that against longdouble; everything behind the reported sums is held bit for
bit to hessian_update.dscale_replay."""
import ctypes as C
import json
import sys
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu

U = 2.0 ** -53
NS = (1, 2, 63, 64, 65, 255, 257, 4095, 4097, 8193)
SY, SQS, GAMMA, THETA, SV, FIRST, LEN, OUTCOME = range(8)


def band_qp(n, seed=0):
    """diagonal Q plus a band of 2 (upper entries), n // 4 equalities of two entries, n // 2 bounds"""
    rng = np.random.default_rng(1000 + n + seed)
    r = np.concatenate([np.arange(n), np.arange(max(n - 1, 0)), np.arange(max(n - 2, 0))])
    c = np.concatenate([np.arange(n), np.arange(1, n), np.arange(2, n)])
    v = np.concatenate([rng.uniform(4.0, 6.0, n), rng.uniform(-1.0, 1.0, c.size - n)])
    me, m = n // 4, n // 2
    A = problems._csr(np.repeat(np.arange(me), 2), np.stack([4 * np.arange(me), 4 * np.arange(me) + 2], 1).ravel(), rng.uniform(-1, 1, 2 * me), me)
    Cm = problems._csr(np.arange(m), 2 * np.arange(m), rng.uniform(0.5, 1.5, m), m)
    return problems.Program(n, me, m, problems._csr(r, c, v, n), A, Cm, c=rng.uniform(-1, 1, n), b=np.zeros(me), d=-np.ones(m))


def programs():
    out = [("band%d" % n, band_qp(n)) for n in NS]
    out.append(("random", problems.random_sparse_qp(150, 40, 90, row_nnz=3)))
    out.append(("grid", problems.grid_sparse_qp(14, 11)))
    out.append(("docp", problems.lq_docp(4, 3, 2)))
    return out


def classes(name):
    return (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP) + ((ipmatrix.IpLQDOCP,) if name == "docp" else ())


def with_q(prog, x):
    return problems.Program(prog.n, prog.me, prog.m, (prog.Q[0], prog.Q[1], np.asarray(x, dtype=np.float64)), prog.A, prog.C, prog.c, prog.b, prog.d)


def integer_program(prog, seed=3):
    """the same patterns with integer values |v| <= 8; the -1.0 of a staircase stays, and no stored value is 0"""
    rng = np.random.default_rng(seed)

    def ints(x, keep_minus_one=False):
        x = np.asarray(x, dtype=np.float64)
        v = rng.integers(1, 9, x.size).astype(np.float64) * rng.choice([-1.0, 1.0], x.size)
        return np.where(x == -1.0, -1.0, v) if keep_minus_one else v

    return problems.Program(prog.n, prog.me, prog.m, (prog.Q[0], prog.Q[1], ints(prog.Q[2])), (prog.A[0], prog.A[1], ints(prog.A[2], True)),
                            (prog.C[0], prog.C[1], ints(prog.C[2])), prog.c, prog.b, prog.d)


def with_lower_nan(prog):
    """the image (j, i) of every stored entry (i, j), j > i, added to Q's pattern with a NaN value - entries below the
    diagonal wherever the pattern allows one; returns (program, mask of the added entries)"""
    p, ix, x = (np.asarray(a) for a in prog.Q)
    n = prog.n
    rows = np.repeat(np.arange(n), np.diff(p))
    st = ix > rows
    r2 = np.concatenate([rows, ix[st]])
    c2 = np.concatenate([ix, rows[st]])
    v2 = np.concatenate([np.asarray(x, dtype=np.float64), np.full(int(st.sum()), np.nan)])
    Q = problems._csr(r2, c2, v2, n)
    return problems.Program(prog.n, prog.me, prog.m, Q, prog.A, prog.C, prog.c, prog.b, prog.d), np.isnan(Q[2])


def rows_of(csr):
    p = np.asarray(csr[0])
    return np.repeat(np.arange(p.size - 1), np.diff(p))


def sym_terms(Q, x, dtype):
    """per row of the symmetric image of Q's upper entries: (sum q_ij x_j, sum |q_ij x_j|, sum_{j != i} |q_ij|, terms) in dtype"""
    p, ix, v = (np.asarray(a) for a in Q)
    n = p.size - 1
    r = rows_of(Q)
    up, st = ix >= r, ix > r
    v, x = v.astype(dtype), np.asarray(x).astype(dtype)
    y, mag, off, cnt = (np.zeros(n, dtype=dtype) for _ in range(4))
    np.add.at(y, r[up], v[up] * x[ix[up]]), np.add.at(y, ix[st], v[st] * x[r[st]])
    np.add.at(mag, r[up], np.abs(v[up] * x[ix[up]])), np.add.at(mag, ix[st], np.abs(v[st] * x[r[st]]))
    np.add.at(off, r[st], np.abs(v[st])), np.add.at(off, ix[st], np.abs(v[st]))
    np.add.at(cnt, r[up], 1), np.add.at(cnt, ix[st], 1)
    return y, mag, off, cnt


def grad_terms(prog, y, z, dtype):
    """(A'y + C'z, sum of |terms|, terms per row) in dtype"""
    n = prog.n
    t, mag, cnt = (np.zeros(n, dtype=dtype) for _ in range(3))
    for M, vec in ((prog.A, y), (prog.C, z)):
        ix, v = np.asarray(M[1]), np.asarray(M[2]).astype(dtype)
        if v.size == 0:
            continue
        w = v * np.asarray(vec).astype(dtype)[rows_of(M)]
        np.add.at(t, ix, w), np.add.at(mag, ix, np.abs(w)), np.add.at(cnt, ix, 1)
    return t, mag, cnt


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


def handle(cls, prog, device=False, **kw):
    M = cls(device_vectors=device, **kw)
    M.init(prog)
    return M


def bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def diag_index(prog):
    r = rows_of(prog.Q)
    return np.flatnonzero(np.asarray(prog.Q[1]) == r)


# ------------------------------------------------------------------------------------------------ the checks
def check_integers():
    """q_product, q_row_stats, lagrangian_gradient with and without minus, q_set_diagonal and q_gerschgorin (eps = 1) exact
    against int64 on every shape, plugin and kind of vector."""
    for name, base in programs():
        prog = integer_program(base)
        n, me, m = prog.dims
        rng = np.random.default_rng(7)
        x, c, mi, d = (rng.integers(-8, 9, n).astype(np.float64) for _ in range(4))
        y, z = rng.integers(-8, 9, me).astype(np.float64), rng.integers(-8, 9, m).astype(np.float64)
        qx_y, _mag, off, _cnt = sym_terms(prog.Q, x, np.int64)
        t, _m, _c = grad_terms(prog, y, z, np.int64)
        di = diag_index(prog)
        r, ix = rows_of(prog.Q), np.asarray(prog.Q[1])
        for cls in classes(name):
            for device in (False, True):
                V = Vecs(device)
                M = handle(cls, prog, device)
                tag = (name, cls.__name__, device)
                assert bits(V.np(M.q_values()), prog.Q[2]), tag
                assert bits(V.np(M.q_product(V.to(x))), qx_y.astype(np.float64)), tag
                dg, os_ = M.q_row_stats()
                assert bits(V.np(dg), np.asarray(prog.Q[2])[di]) and bits(V.np(os_), off.astype(np.float64)), tag
                only = M.q_row_stats(want_diag=False)
                assert only[0] is None and bits(V.np(only[1]), off.astype(np.float64)), tag
                g = V.np(M.lagrangian_gradient(V.to(c), V.to(y), V.to(z)))
                assert bits(g, (c.astype(np.int64) - t).astype(np.float64)), tag
                g2 = V.np(M.lagrangian_gradient(V.to(c), V.to(y), V.to(z), minus=V.to(mi)))
                assert bits(g2, (c.astype(np.int64) - t - mi.astype(np.int64)).astype(np.float64)), tag
                M.q_gerschgorin(1.0)
                want = np.array(prog.Q[2], dtype=np.float64)
                want[di] = np.maximum(want[di], off.astype(np.float64) + 1.0)
                assert bits(V.np(M.q_values()), want), tag
                assert bits(want, hu.q_gerschgorin_model(prog.Q, 1.0)), tag
                M.q_set_diagonal(V.to(d))
                want = np.where(ix > r, 0.0, want)
                want[di] = d
                got = V.np(M.q_values())
                assert bits(got, want) and not np.signbit(got[ix > r]).any(), tag
                assert bits(V.np(M.q_product(V.to(x))), d * x + 0.0), tag  # (a row's sum starts from +0.0)


def _dscale_case(prog, seed):
    """s and y over the diagonal q of prog: the first half of the variables not damped (y = 1.1 q s), the second damped"""
    rng = np.random.default_rng(seed)
    n = prog.n
    q = np.asarray(prog.Q[2], dtype=np.float64)[diag_index(prog)]
    s = rng.normal(size=n) * rng.choice([1e-2, 1.0, 1e2], n)
    s[s == 0.0] = 1.0
    f = np.where(np.arange(n) < (n + 1) // 2, 1.1, -0.5) * rng.uniform(0.9, 1.1, n)
    return s, f * q * s, q


def _check_dscale(M, V, prog, s, y, bsize, tag):
    """one update on the handle's current Q (its diagonal read first): sums against longdouble, the rest against the replay;
    returns (report, new diagonal)"""
    n = prog.n
    di = diag_index(prog)
    before = V.np(M.q_values()).copy()
    q = before[di]
    v = V.np(M.q_dscale_update(V.to(s), V.to(y), gamma=0.2, bsize=bsize, want_v=True))
    rep = M.q_dscale_report()
    after = V.np(M.q_values())
    B = bsize if 0 < bsize < n else n
    first = np.arange(0, n, B)
    assert rep.shape == (first.size, 8) and bits(rep[:, FIRST], first) and bits(rep[:, LEN], np.minimum(first + B, n) - first), tag
    assert (rep[:, GAMMA] == 0.2).all(), tag
    ld = np.longdouble
    sq = s * q
    ln = rep[:, LEN]
    for col, terms in ((SY, s.astype(ld) * y.astype(ld)), (SQS, sq.astype(ld) * s.astype(ld))):
        exact, mag = np.add.reduceat(terms, first), np.add.reduceat(np.abs(terms), first)
        fin = np.isfinite(exact)  # (a NaN in a block's y: its sum is NaN, and its alone)
        assert (np.abs(rep[:, col].astype(ld) - exact) <= (ln + 2) * U * mag)[fin].all() and np.isnan(rep[~fin, col]).all(), (tag, col)
    v_r, q_r, out_r = hu.dscale_replay(rep, s, y, q, bsize=bsize)
    assert bits(v, v_r) and bits(after[di], q_r), tag
    assert bits(rep[:, OUTCOME], out_r), tag
    damp = rep[:, SY] < 0.2 * rep[:, SQS]
    assert ((rep[:, THETA] != 1.0) == damp).all() and bits(rep[~damp, SV], rep[~damp, SY]), tag
    terms = s.astype(ld) * v_r.astype(ld)
    exact, mag = np.add.reduceat(terms, first), np.add.reduceat(np.abs(terms), first)
    assert (np.abs(rep[:, SV].astype(ld) - exact) <= (ln + 2) * U * mag)[damp].all(), tag
    off = np.ones(before.size, dtype=bool)
    off[di] = False
    assert bits(after[off], before[off]), tag
    return rep, after[di]


def check_reals():
    """q_product and lagrangian_gradient against longdouble within (L_i + 2) 2^-53 sum |terms|; q_dscale_update for every
    bsize: the reported sums against longdouble, decision, theta, v and the new diagonal bit for bit dscale_replay, the
    outcome codes, the off-diagonal values untouched."""
    ld = np.longdouble
    for name, prog in programs():
        n, me, m = prog.dims
        rng = np.random.default_rng(11)
        x, c, mi = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)
        y, z = rng.normal(size=me), rng.normal(size=m)
        qx, qmag, _off, qcnt = sym_terms(prog.Q, x, ld)
        t, tmag, tcnt = grad_terms(prog, y, z, ld)
        s, yy, _q = _dscale_case(prog, 5)
        for cls in classes(name):
            for device in (False, True):
                V = Vecs(device)
                M = handle(cls, prog, device)
                tag = (name, cls.__name__, device)
                got = V.np(M.q_product(V.to(x)))
                assert (np.abs(got.astype(ld) - qx) <= (qcnt + 2) * U * qmag).all(), tag
                g = V.np(M.lagrangian_gradient(V.to(c), V.to(y), V.to(z)))
                # (c_i - t_i: one more term and one more rounding)
                assert (np.abs(g.astype(ld) - (c.astype(ld) - t)) <= (tcnt + 3) * U * (tmag + np.abs(c))).all(), tag
                g2 = V.np(M.lagrangian_gradient(V.to(c), V.to(y), V.to(z), minus=V.to(mi)))
                assert bits(g2, g - mi), tag  # (the last subtraction is one rounded operation on the first result)
                seen = set()
                for bsize in (0, 1, 7, 256, 4096, n - 1):
                    M.update(prog)
                    rep, _d = _check_dscale(M, V, prog, s, yy, bsize, tag + (bsize,))
                    seen |= set(rep[:, OUTCOME].astype(int).tolist())
                assert seen == ({0, 1} if n > 1 else {0}), (tag, seen)
                # the reference's sequence on top of each other: setup, two updates, Gerschgorin
                M.update(prog)
                M.q_dscale_setup(1e-8)
                r = rows_of(prog.Q)
                want = np.where(np.asarray(prog.Q[1]) > r, 0.0, np.asarray(prog.Q[2], dtype=np.float64))
                assert bits(V.np(M.q_values()), want), tag
                progd = with_q(prog, want)
                _check_dscale(M, V, progd, s, yy, 7, tag)
                _check_dscale(M, V, progd, yy, s, 0, tag)


def check_lower_entries_and_skips():
    """Entries with col < row hold NaN: every result is what it is without them and they still hold NaN afterwards.  A block
    with s = 0 is left alone (2); a NaN in one block's y gives 3 there and the other blocks' bits are as without it."""
    for name, base in programs():
        if base.n < 2:
            continue
        prog, low = with_lower_nan(base)
        n = base.n
        di_b, di = diag_index(base), diag_index(prog)
        rng = np.random.default_rng(13)
        x = rng.normal(size=n)
        s, y, _q = _dscale_case(base, 9)
        B = 7
        nb = (n + B - 1) // B
        for cls in classes(name):
            V = Vecs(False)
            Mb, M = handle(cls, base), handle(cls, prog)
            tag = (name, cls.__name__)
            assert bits(M.q_product(x), Mb.q_product(x)), tag
            for a, b in zip(M.q_row_stats(), Mb.q_row_stats()):
                assert bits(a, b), tag
            for H in (Mb, M):
                H.q_dscale_setup(1e-8)
                H.q_dscale_update(s, y, bsize=B)
                H.q_gerschgorin(0.5)
            got, ref = M.q_values(), Mb.q_values()
            assert np.isnan(got[low]).all() and bits(got[~low], ref), tag
            assert bits(M.q_dscale_report(), Mb.q_dscale_report()), tag
            M.q_set_diagonal(x)
            got = M.q_values()
            assert np.isnan(got[low]).all() and bits(got[di], x), tag
            # the skipped blocks, on the handle without the extra entries
            Mb.update(base)
            rep0, d0 = _check_dscale(Mb, V, base, s, y, B, tag)
            if nb < 3:
                continue
            s2, y2 = s.copy(), y.copy()
            s2[B: 2 * B] = 0.0
            y2[min(2 * B + 3, n - 1)] = np.nan
            Mb.update(base)
            rep, d1 = _check_dscale(Mb, V, base, s2, y2, B, tag)
            assert rep[1, OUTCOME] == 2 and rep[2, OUTCOME] == 3, (tag, rep[:3])
            q0 = np.asarray(base.Q[2], dtype=np.float64)[di_b]
            assert bits(d1[B: 3 * B], q0[B: 3 * B]), tag
            keep = np.ones(n, dtype=bool)
            keep[B: 3 * B] = False
            assert bits(d1[keep], d0[keep]) and bits(np.delete(rep, (1, 2), 0), np.delete(rep0, (1, 2), 0)), tag


def check_reproducible():
    """Two calls on equal inputs give equal bits; the three plugins - and host and device vectors - give the same diagonal bits
    for the same Q, s, y and bsize; and a block's bits do not depend on bsize's cut of the OTHER variables."""
    for name, prog in programs():
        n = prog.n
        s, y, _q = _dscale_case(prog, 21)
        x = np.random.default_rng(2).normal(size=n)
        handles = [(cls, device, handle(cls, prog, device)) for cls in classes(name) for device in (False, True)]
        for bsize in (0, 1, 7, 256, 4096, n - 1):
            ref = None
            for cls, device, M in handles:
                V = Vecs(device)
                res = []
                for _ in range(2):
                    M.update(prog)
                    v = V.np(M.q_dscale_update(V.to(s), V.to(y), bsize=bsize, want_v=True))
                    res.append((v, M.q_dscale_report(), V.np(M.q_values()), V.np(M.q_product(V.to(x))), V.np(M.q_row_stats()[1])))
                ref = ref or res[0]
                for r in res:
                    assert all(bits(a, b) for a, b in zip(r, ref)), (name, cls.__name__, device, bsize)
    # the order of a block's sums is fixed by its length alone: a block of 300 at the front of n = 8193 (bsize 300) and the
    # same 300 variables as a program of their own (one block); and the 7 variables behind 4096 others (bsize 4096: a
    # workgroup sums them) as a program of their own (a wavefront sums them)
    for nbig, bsize, lo, ln in ((8193, 300, 0, 300), (4103, 4096, 4096, 7)):
        big, small = band_qp(nbig), band_qp(ln)
        s, y, _q = _dscale_case(big, 4)
        qb = np.asarray(big.Q[2], dtype=np.float64)[diag_index(big)][lo: lo + ln]
        y[lo: lo + ln] = -0.5 * qb * s[lo: lo + ln]  # (damped, so that s'v is compared too)
        vals = np.array(small.Q[2], dtype=np.float64)
        vals[diag_index(small)] = qb
        small = with_q(small, vals)
        Mb, Ms = handle(ipmatrix.IpRedSpBKP, big), handle(ipmatrix.IpSpBKP, small)
        Mb.q_dscale_update(s, y, bsize=bsize)
        Ms.q_dscale_update(s[lo: lo + ln], y[lo: lo + ln], bsize=0)
        rb, rs = Mb.q_dscale_report()[lo // bsize], Ms.q_dscale_report()[0]
        assert bits(rb[:5], rs[:5]) and rb[OUTCOME] == rs[OUTCOME] == 1, (nbig, rb, rs)
        assert bits(Mb.q_values()[diag_index(big)][lo: lo + ln], Ms.q_values()[diag_index(small)]), nbig


def _state_bits(M, prog, st):
    """factor, step, residuum, solve and a Mehrotra run of the handle: everything that must agree bit for bit (an entry
    that ends in an error counts with its code)"""
    from common import new_d
    out = []

    def run(fn):
        try:
            r = fn()
            out.append(np.float64(0.0 if r is None else r))
        except ipmatrix.KktError as e:
            assert e.code != _lib.E_DEVICE
            out.append(np.float64(-e.code))

    run(lambda: M.factor(prog, st[0], st[1]))
    d = new_d(prog)
    run(lambda: M.step(prog, *st, *d))
    out.extend(a.copy() for a in d)
    run(lambda: M.residuum(prog, *st, *d))
    d = new_d(prog)
    run(lambda: M.solve(prog, *st, *d))
    out.extend(d)
    try:
        x, y, z, w, info = M.mehrotra(prog, max_iters=30)
        out += [x, y, z, w, np.float64(info["iters"]), np.float64(info["result"])]
    except ipmatrix.KktError as e:
        assert e.code != _lib.E_DEVICE
        out.append(np.float64(-e.code))
    return out


def check_handle_afterwards():
    """After q_dscale_setup -> q_dscale_update -> q_gerschgorin: q_values, then a FRESH handle of the same class given those
    values by hqpkkt_set_values - factor, step, residuum, solve and the iterates and iteration count of hqpkkt_mehrotra are
    bit-identical; the updated handle is not factored before its factor.  Once more with zd_policy = -1 on a handle whose
    update (q_set_diagonal with small entries) makes diagonals weak."""
    from common import new_d
    cases = [("random", problems.random_sparse_qp(150, 40, 90, row_nnz=3)), ("grid", problems.grid_sparse_qp(14, 11)),
             ("docp", problems.lq_docp(4, 3, 2))]
    for name, prog in cases:
        st = problems.ip_state(prog, seed=12, spread=1.0)
        s, y, _q = _dscale_case(prog, 31)
        for cls in classes(name):
            for weak in (False, True):
                if weak and cls is ipmatrix.IpLQDOCP:
                    continue  # (the STAGED engine has no zero-diagonal placement)
                tag = (name, cls.__name__, weak)
                M = handle(cls, prog, zd_policy=-1)
                M.factor(prog, st[0], st[1])  # (factored - and not any more after the update)
                if weak:
                    d = np.where(np.arange(prog.n) % 3 == 0, 1e-4, 1.0)
                    M.q_set_diagonal(d)
                    assert M.debug(30)[1] == 1, tag
                else:
                    M.q_dscale_setup(1e-8)
                    M.q_dscale_update(s, y, bsize=7)
                    M.q_gerschgorin(1e-3)
                with np.testing.assert_raises(ipmatrix.KktError) as e:
                    M.solve(prog, *st, *new_d(prog))
                assert e.exception.code == _lib.E_INTERN, tag
                qx = M.q_values()
                assert not bits(qx, prog.Q[2]), tag
                prog2 = with_q(prog, qx)
                F = handle(cls, prog2, zd_policy=-1)
                assert (F.debug(30) == M.debug(30)).all(), tag
                a, b = _state_bits(M, prog2, st), _state_bits(F, prog2, st)
                assert len(a) == len(b) and all(bits(p, q) for p, q in zip(a, b)), tag
                assert a[0] == 0.0 and np.isfinite(a[1]).all(), tag  # (the factorisation went through)


def check_refused_handles():
    """hqpkkt_lagrangian_gradient is HQPKKT_E_INTERN on a dense hand-over (init_dense) handle; every hqpkkt_q_* entry on dense
    stage Hessians; and the diagonal rule is HQPKKT_E_FORMAT where the values have arrived."""
    prog = problems.lq_docp(4, 3, 2)
    n, me, m = prog.dims
    M = ipmatrix.IpLQDOCP()
    M.init_dense(problems.dense_docp_from_program(prog, [3] * 5, [2] * 4))
    x = np.ones(n)
    for call in (lambda: M.lagrangian_gradient(x, np.ones(me), np.ones(m)),):
        try:
            call()
            raise AssertionError("accepted")
        except ipmatrix.KktError as e:
            assert e.code == _lib.E_INTERN
    assert bits(M.q_product(x), handle(ipmatrix.IpLQDOCP, prog).q_product(x))  # (Q is in CSR form there: accepted)
    D = ipmatrix.IpLQDOCP(q_dense=True)
    D.init(prog)
    for call in (D.q_values, lambda: D.q_product(x), D.q_row_stats, lambda: D.q_set_diagonal(x), lambda: D.q_gerschgorin(1.0),
                 lambda: D.q_dscale_setup(1.0), lambda: D.q_dscale_update(x, x), D.q_dscale_report):
        try:
            call()
            raise AssertionError("accepted")
        except ipmatrix.KktError as e:
            assert e.code == _lib.E_INTERN
    g = D.lagrangian_gradient(x, np.ones(me), np.ones(m))
    assert bits(g, handle(ipmatrix.IpSpBKP, prog).lagrangian_gradient(x, np.ones(me), np.ones(m)))
    # the diagonal rule
    base = problems.banded_qp(40, 3)
    p, ix, v = (np.array(a) for a in base.Q)
    k = int(p[7])
    assert ix[k] == 7
    p[8:] -= 1
    bad = problems.Program(base.n, base.me, base.m, (p, np.delete(ix, k), np.delete(v, k)), base.A, base.C, base.c, base.b, base.d)
    for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):
        B = handle(cls, bad)
        one = np.ones(bad.n)
        for call in (lambda: B.q_set_diagonal(one), lambda: B.q_gerschgorin(1.0), lambda: B.q_dscale_setup(1.0), lambda: B.q_dscale_update(one, one)):
            try:
                call()
                raise AssertionError("accepted")
            except ipmatrix.KktError as e:
                assert e.code == _lib.E_FORMAT
        dg, off = B.q_row_stats()
        assert dg[7] == 0.0 and off[7] > 0.0
        assert bits(B.q_values(), bad.Q[2])  # (nothing was written)
        B.q_product(one)
        # before the first update since the analysis the report has nothing to tell
        k2 = C.c_longlong()
        out = np.zeros(8)
        assert _lib.lib().hqpkkt_q_dscale_report(B._h, C.c_void_p(out.ctypes.data), 1, C.byref(k2)) == _lib.E_INTERN
    G = handle(ipmatrix.IpSpBKP, base)
    G.q_dscale_update(np.ones(base.n), np.ones(base.n), bsize=7)
    k2 = C.c_longlong()
    out = np.zeros(8)
    assert _lib.lib().hqpkkt_q_dscale_report(G._h, C.c_void_p(out.ctypes.data), 1, C.byref(k2)) == _lib.E_RANGE and k2.value == 6


def check_shared_plans():
    """A DScale update and a BFGS update (PATTERN) with the same bsize use one partition: neither touches the other's report,
    whatever ran in between, and the DScale update's bits do not depend on a BFGS update having made the partition's tables
    first; the eigenvalue control's floor_from_bfgs still reads the BFGS update's words behind a DScale update.  band_qp(65) with bsize 64 (blocks of 64 and 1: a wavefront per unit) and band_qp(4097) with bsize 0 (one block of
    two chunks: a workgroup per unit)."""
    for n, bsize in ((65, 64), (4097, 0)):
        prog = band_qp(n)
        di = diag_index(prog)
        s, y, _q = _dscale_case(prog, 17)
        s2, y2, _q = _dscale_case(prog, 18)
        for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):
            tag = (n, bsize, cls.__name__)
            M = handle(cls, prog)
            M.q_bfgs_update(s, y, bsize=bsize, pattern=True)
            R = M.q_bfgs_report()
            q_mid = M.q_values().copy()
            v = M.q_dscale_update(s2, y2, bsize=bsize, want_v=True).copy()
            D = M.q_dscale_report()
            d_after = M.q_values()[di].copy()
            assert D.shape == R.shape == ((n + 63) // 64 if bsize else 1, 8), tag
            assert bits(M.q_bfgs_report(), R), tag  # (a)
            M.q_bfgs_update(s2, y2, bsize=bsize, pattern=True)
            assert not bits(M.q_bfgs_report(), R), tag  # (the other update did write its own words)
            assert bits(M.q_dscale_report(), D), tag  # (b)
            F = handle(cls, prog)  # (c): it has never made a BFGS update
            F.update(with_q(prog, q_mid))
            vf = F.q_dscale_update(s2, y2, bsize=bsize, want_v=True)
            assert bits(vf, v) and bits(F.q_dscale_report(), D) and bits(F.q_values()[di], d_after), tag
            # the eigenvalue control's floor_from_bfgs reads the BFGS update's words behind a DScale update on the same
            # partition: as on a handle with the same BFGS words and the same Q that has no DScale report
            A, G = handle(cls, prog), handle(cls, prog)
            for H in (A, G):
                H.q_bfgs_update(s, y, bsize=bsize, pattern=True)
            assert bits(A.q_bfgs_report(), R) and bits(G.q_bfgs_report(), R), tag
            A.q_dscale_update(s2, y2, bsize=bsize)
            G.update(with_q(prog, A.q_values()))
            res = []
            for H in (A, G):
                H.q_eigen_control(1.0, bsize=bsize, from_bfgs=True, max_steps=4)
                rep, T = H.q_eigen_report(with_T=True)
                res.append((rep, T, H.q_values()))
            assert all(bits(a, b) for a, b in zip(*res)), tag


CHECKS = {f.__name__[6:]: f for f in (check_integers, check_reals, check_lower_entries_and_skips, check_reproducible,
                                       check_handle_afterwards, check_refused_handles, check_shared_plans)}


def main():
    results = {}
    dead = False
    for name, fn in CHECKS.items():
        if dead:
            results[name] = "not run: an earlier check ended in a device error"
            continue
        try:
            fn()
            results[name] = "ok"
        except ipmatrix.KktError as e:
            results[name] = traceback.format_exc()
            dead = e.code == _lib.E_DEVICE
        except Exception:
            results[name] = traceback.format_exc()
    print("Q_VALUES_RESULTS " + json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
