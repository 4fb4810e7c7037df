"""The GPU checks of hqpkkt_q_blocks / hqpkkt_q_bfgs_update / hqpkkt_q_bfgs_report (tests/test_gpu_q_bfgs.py starts this once, as a
child process): every check of CHECKS runs on the device and the outcomes go to stdout as one JSON line, {name: "ok" |
traceback}.  A check that ends in a device error ends the run: nothing more is started on the GPU.  The programs and the
bound of the secant check are used by tests/test_q_bfgs_cpu.py as well.

Programs.  P1: a block-diagonal Q of fully stored SPD blocks of orders (1, 2, 63, 64, 65, 255, 257), n = 707, equalities and
bounds as q_values_worker.band_qp makes them; Hqp_IpSpBKP and Hqp_IpRedSpBKP.  P2: with_dense_hessian(lq_docp(4, 3, 2)) on
all three plugins, detected blocks.  P3: band_qp(n), n = 1 .. 8193 (around a wavefront, a workgroup, a chunk of 4096 and two
chunks), the stored entries alone (PATTERN): bsize 0 is one long block, 7 and 256 cut the band - entries that cross blocks
-, n - 1 leaves a block of one.  P4: random_sparse_qp(150, 40, 90, row_nnz=3) and grid_sparse_qp(14, 11), PATTERN, one block:
the update of Hqp_HL_Gangster.

Bounds.  Integer operands (|values| <= 8, every sum below 2^53): Qs, sy and sQs exact against int64.  Real operands: a sum of
L terms in ANY order lies within (L + 2) 2^-53 sum |terms| of the exact sum (L - 1 additions and the rounding of each term,
fused or not), so Qs - L the entries of the row inside its block - and the reported sums - L the block's length, the terms
those of the vectors the device itself summed - are held to that against longdouble.  Everything behind the sums is held
bit for bit to hessian_update.q_bfgs_replay.

The secant equation (secant_excess).  With w the returned Qs, sigma = sQs and tau = sv as reported, u = 2^-53, L the block's
length, e_i = w_i - (Q s)_i, eps1 = s'w - sigma, eps2 = s'v - tau: the matrix Q - w w'/sigma + v v'/tau maps s to
v - e - w eps1 / sigma + v eps2 / tau.  An updated entry differs from that matrix's by at most 2u|q| + 4u|a| + 3u|b| to first
order (a = w_i w_j / sigma, b = v_i v_j / tau: two roundings each, then fl(q - a'), then fl(t + b')), taken as 5u(|q| + |a| +
|b|); and the product afterwards is a sum of L terms.  So, row by row of an updated block,
  |(Q+ s)_i - v_i| <= (L + 2) u [sum_j |q_ij s_j| + |w_i| sum |s w| / |sigma| + |v_i| sum |s v| / |tau| + sum_j |q+_ij s_j|]
                     + 5u sum_j (|q_ij| + |a_ij| + |b_ij|) |s_j|."""
import ctypes as C
import json
import sys
import traceback

import numpy as np

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu
from q_values_worker import Vecs, band_qp, bits, handle, integer_program, rows_of, with_lower_nan, with_q

U = 2.0 ** -53
ORDERS = (1, 2, 63, 64, 65, 255, 257)
NS = (1, 2, 63, 64, 65, 255, 257, 4095, 4097, 8193)
SY, SQS, GAMMA, THETA, SV, FIRST, LEN, OUTCOME = range(8)
ld = np.longdouble


def block_diag_qp(orders=ORDERS, seed=0):
    """P1: fully stored SPD blocks M M' / k + diag(U(0.5, 1.5)) of the given orders, each drawn from a seed of its order alone
    (a permutation of ``orders`` moves the blocks and keeps their values); n // 4 equalities of two entries, n // 2 bounds"""
    n = int(sum(orders))
    qr, qc, qv = [], [], []
    off = 0
    for k in orders:
        rng = np.random.default_rng(500 + 7 * k + seed)
        M = rng.uniform(-1.0, 1.0, (k, k))
        B = M @ M.T / k + np.diag(rng.uniform(0.5, 1.5, k))
        i, j = np.triu_indices(k)
        qr.append(off + i), qc.append(off + j), qv.append(B[i, j])
        off += k
    rng = np.random.default_rng(900 + seed)
    me, m = n // 4, n // 2
    A = problems._csr(np.repeat(np.arange(me), 2), np.stack([4 * np.arange(me), 4 * np.arange(me) + 2], 1).ravel(), rng.uniform(-1, 1, 2 * me), me)
    Cm = problems._csr(np.arange(m), 2 * np.arange(m), rng.uniform(0.5, 1.5, m), m)
    Q = problems._csr(np.concatenate(qr), np.concatenate(qc), np.concatenate(qv), n)
    return problems.Program(n, me, m, Q, A, Cm, c=rng.uniform(-1, 1, n), b=np.zeros(me), d=-np.ones(m))


def docp_qp():
    return problems.with_dense_hessian(problems.lq_docp(4, 3, 2))


def blocks_of(prog, bsize):
    return hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, bsize)[0]


def cases():
    """(name, program, classes, bsize, pattern) of P1 .. P4"""
    sp = (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP)
    out = [("P1", block_diag_qp(), sp, -1, False), ("P2", docp_qp(), sp + (ipmatrix.IpLQDOCP,), -1, False)]
    for n in NS:
        for bsize in sorted({0, 7, 256, n - 1}):
            if n == 1 and bsize != 0:
                continue
            out.append(("P3_%d" % n, band_qp(n), sp[n % 2: n % 2 + 1], bsize, True))
    out.append(("P4_random", problems.random_sparse_qp(150, 40, 90, row_nnz=3), sp, 0, True))
    out.append(("P4_grid", problems.grid_sparse_qp(14, 11), sp, 0, True))
    return out


def restricted_product(Q, x, first, dtype):
    """per row of the symmetric image of Q's upper entries INSIDE the blocks: (sum q_ij x_j, sum |q_ij x_j|, terms) in dtype,
    and whether a stored upper entry crosses two blocks"""
    p, ix, v = (np.asarray(a) for a in Q)
    n = p.size - 1
    r = rows_of(Q)
    of = np.repeat(np.arange(len(first) - 1), np.diff(first)) if n else np.zeros(0, dtype=np.int64)
    same = of[r] == of[ix]
    up, st = (ix >= r) & same, (ix > r) & same
    v, x = v.astype(dtype), np.asarray(x).astype(dtype)
    y, mag, cnt = (np.zeros(n, dtype=dtype) for _ in range(3))
    np.add.at(y, r[up], v[up] * x[ix[up]]), np.add.at(y, ix[st], v[st] * x[r[st]])
    np.add.at(mag, r[up], np.abs(v[up] * x[ix[up]])), np.add.at(mag, ix[st], np.abs(v[st] * x[r[st]]))
    np.add.at(cnt, r[up], 1), np.add.at(cnt, ix[st], 1)
    return y, mag, cnt, bool(((ix > r) & ~same).any())


def mixed_inputs(prog, first, seed, damp_every=3):
    """s and y over the blocks: y = f Qs with f about 1.1 (not damped where s'Qs > 0) and, on every third block, about -0.5
    (damped)"""
    rng = np.random.default_rng(seed)
    n = prog.n
    s = rng.normal(size=n) * rng.choice([1e-2, 1.0, 1e2], n)
    s[s == 0.0] = 1.0
    Qs = restricted_product(prog.Q, s, first, np.float64)[0]
    nb = len(first) - 1
    of = np.repeat(np.arange(nb), np.diff(first))
    f = np.where((np.arange(nb) + seed) % damp_every == 0, -0.5, 1.1)[of] * rng.uniform(0.9, 1.1, n)
    return s, f * Qs


def secant_inputs(prog, first, seed):
    """s_i y_i > 0 everywhere; every third block with a y so short that it is damped"""
    rng = np.random.default_rng(seed)
    n = prog.n
    s = rng.normal(size=n)
    s[s == 0.0] = 1.0
    nb = len(first) - 1
    of = np.repeat(np.arange(nb), np.diff(first))
    y = s * rng.uniform(0.5, 1.5, n) * np.where(np.arange(nb) % 3 == 1, 0.01, 1.0)[of]
    return s, y


def secant_excess(Q_before, x_after, s, v, w, rep, first, p_after):
    """max over the rows of updated blocks of |p_after_i - v_i| / bound_i (the module's docstring), and the rows counted"""
    p, ix, x0 = (np.asarray(a) for a in Q_before)
    n = p.size - 1
    r = rows_of(Q_before)
    nb = len(first) - 1
    of = np.repeat(np.arange(nb), np.diff(first))
    ln = np.diff(first).astype(ld)[of]
    same = of[r] == of[ix]
    up, st = (ix >= r) & same, (ix > r) & same
    rr, cc = np.concatenate([r[up], ix[st]]), np.concatenate([ix[up], r[st]])
    q0 = np.concatenate([x0[up], x0[st]]).astype(ld)
    q1 = np.concatenate([np.asarray(x_after)[up], np.asarray(x_after)[st]]).astype(ld)
    sl, vl, wl = s.astype(ld), v.astype(ld), w.astype(ld)
    sig, tau = rep[:, SQS].astype(ld)[of], rep[:, SV].astype(ld)[of]
    sw, svm = np.add.reduceat(np.abs(sl * wl), first[:-1]).astype(ld)[of], np.add.reduceat(np.abs(sl * vl), first[:-1]).astype(ld)[of]

    def rowsum(t):
        out = np.zeros(n, dtype=ld)
        np.add.at(out, rr, t)
        return out

    a = np.abs(wl[rr] * wl[cc] / sig[rr])
    b = np.abs(vl[rr] * vl[cc] / tau[rr])
    bound = (ln + 2) * U * (rowsum(np.abs(q0 * sl[cc])) + np.abs(wl) * sw / np.abs(sig) + np.abs(vl) * svm / np.abs(tau) + rowsum(np.abs(q1 * sl[cc]))) \
        + 5 * U * rowsum((np.abs(q0) + a + b) * np.abs(sl[cc]))
    done = (rep[:, OUTCOME] < 2)[of]
    ratio = np.abs(np.asarray(p_after).astype(ld) - vl)[done] / bound[done]
    return float(ratio.max()), int(done.sum())


def update(M, V, s, y, bsize, pattern, gamma=0.1, alpha=1.0):
    """one update: (v, Qs, report, q_values before, q_values after) as numpy"""
    before = V.np(M.q_values()).copy()
    v, Qs = M.q_bfgs_update(V.to(s), V.to(y), gamma=gamma, alpha=alpha, bsize=bsize, pattern=pattern, want_v=True, want_Qs=True)
    rep = M.q_bfgs_report()
    return V.np(v), V.np(Qs), rep, before, V.np(M.q_values())


def check_against_replay(prog, first, s, y, res, tag, gamma_eff=0.1):
    """the sums of one update against longdouble, everything behind them against q_bfgs_replay; returns the outcomes"""
    v, Qs, rep, before, after = res
    nb = len(first) - 1
    assert rep.shape == (nb, 8) and bits(rep[:, FIRST], first[:-1]) and bits(rep[:, LEN], np.diff(first)), tag
    assert (rep[:, GAMMA] == gamma_eff).all(), tag
    assert bits(before, prog.Q[2]), tag
    qs, qmag, qcnt, _cross = restricted_product(prog.Q, s, first, ld)
    fin = np.isfinite(qs)
    assert (np.abs(Qs.astype(ld) - qs) <= (qcnt + 2) * U * qmag)[fin].all() and np.isnan(Qs[~fin]).all(), tag
    ln = rep[:, LEN]
    v_r, x_r, out_r = hu.q_bfgs_replay(rep, prog.Q, y, Qs, first)
    damp = rep[:, SY] < gamma_eff * rep[:, SQS]
    for col, terms, rows in ((SY, s.astype(ld) * y.astype(ld), slice(None)), (SQS, s.astype(ld) * Qs.astype(ld), slice(None)),
                             (SV, s.astype(ld) * v_r.astype(ld), damp)):
        exact, mag = np.add.reduceat(terms, first[:-1]), np.add.reduceat(np.abs(terms), first[:-1])
        fin = np.isfinite(exact)  # (a NaN in a block's y: its sums are NaN, and its alone)
        ok = (np.abs(rep[:, col].astype(ld) - exact) <= (ln + 2) * U * mag) | ~fin
        assert ok[rows].all() and (col == SV or np.isnan(rep[~fin, col]).all()), (tag, col)
    assert bits(v, v_r) and bits(rep[:, OUTCOME], out_r), tag
    assert bits(after, x_r), tag
    assert ((rep[:, THETA] != 1.0) == damp).all() and bits(rep[~damp, SV], rep[~damp, SY]), tag
    return rep[:, OUTCOME].astype(int)


# ------------------------------------------------------------------------------------------------ the checks
def check_integers():
    """Integer Q, s, y (|values| <= 8): the returned Qs and the reported sy, sQs are exact against int64, on every program,
    plugin and kind of vector; hqpkkt_q_blocks is q_blocks_model."""
    for name, base, classes, bsize, pattern in cases():
        prog = integer_program(base)
        n = prog.n
        first, full = hu.q_blocks_model(prog.Q[0], prog.Q[1], n, bsize)
        rng = np.random.default_rng(7)
        s, y = (rng.integers(-8, 9, n).astype(np.float64) for _ in range(2))
        qs = restricted_product(prog.Q, s, first, np.int64)[0]
        si, yi = s.astype(np.int64), y.astype(np.int64)
        for cls in classes:
            for device in (False, True):
                V = Vecs(device)
                M = handle(cls, prog, device)
                tag = (name, cls.__name__, device, bsize)
                f2, fl2 = M.q_blocks(bsize)
                assert (f2 == first).all() and (fl2 == full).all(), tag
                v, Qs, rep, _b, _a = update(M, V, s, y, bsize, pattern)
                assert bits(Qs, qs.astype(np.float64)), tag
                assert bits(rep[:, SY], np.add.reduceat(si * yi, first[:-1]).astype(np.float64)), tag
                assert bits(rep[:, SQS], np.add.reduceat(si * qs, first[:-1]).astype(np.float64)), tag


def check_reals():
    """Qs and the reported sums against longdouble within (L + 2) 2^-53 sum |terms|; outcome, theta, v, sv given v and every
    stored value afterwards bit for bit q_bfgs_replay; about a third of the blocks damped; a negative gamma is adapted to
    alpha on the host."""
    seen, damped, total = set(), 0, 0
    for k, (name, prog, classes, bsize, pattern) in enumerate(cases()):
        first = blocks_of(prog, bsize)
        s, y = mixed_inputs(prog, first, 5 + k)
        for cls in classes:
            for device in (False, True):
                V = Vecs(device)
                M = handle(cls, prog, device)
                tag = (name, cls.__name__, device, bsize)
                out = check_against_replay(prog, first, s, y, update(M, V, s, y, bsize, pattern), tag)
                seen |= set(out.tolist())
                if name in ("P1", "P2") or bsize == 7:
                    damped, total = damped + int((out == 1).sum()), total + out.size
        if name == "P1":  # damping adapted to the step length: gamma_eff = 0.2 + 0.8 * 0.5 formed as the model forms it
            M = handle(classes[0], prog)
            g = -(-0.2) + (1.0 + -0.2) * (1.0 - 0.5)
            check_against_replay(prog, first, s, y, update(M, Vecs(False), s, y, bsize, pattern, gamma=-0.2, alpha=0.5), (name, "adapted"), gamma_eff=g)
    assert seen == {0, 1}, seen
    assert 0.25 * total <= damped <= 0.45 * total, (damped, total)


def check_product_bits():
    """Where no stored entry crosses a block the returned Qs has the bits of q_product(s)."""
    n_same = 0
    for k, (name, prog, classes, bsize, pattern) in enumerate(cases()):
        first = blocks_of(prog, bsize)
        if restricted_product(prog.Q, np.ones(prog.n), first, np.float64)[3]:
            continue
        s, y = mixed_inputs(prog, first, 40 + k)
        for cls in classes:
            M = handle(cls, prog)
            want = M.q_product(s)
            _v, Qs = M.q_bfgs_update(s, y, bsize=bsize, pattern=pattern, want_Qs=True)
            assert bits(Qs, want), (name, cls.__name__, bsize)
            n_same += 1
    assert n_same >= 20, n_same


def check_secant():
    """P1, SPD blocks, s_i y_i > 0: q_product(s) after the update is v on every updated block within secant_excess's bound."""
    prog = block_diag_qp()
    first = blocks_of(prog, -1)
    s, y = secant_inputs(prog, first, 77)
    for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):
        M = handle(cls, prog)
        v, Qs, rep, before, after = update(M, Vecs(False), s, y, -1, False)
        assert set(rep[:, OUTCOME].astype(int).tolist()) == {0, 1}, rep[:, OUTCOME]
        worst, rows = secant_excess(prog.Q, after, s, v, Qs, rep, first, M.q_product(s))
        assert rows == prog.n and worst <= 1.0, (cls.__name__, worst)


def check_untouched_and_skips():
    """NaN below the diagonal is never read or written; NaN in the entries that cross two blocks stays there and reaches
    nothing; a block with s = 0 gives outcome 2, one with a NaN in y outcome 3, both keep their bits and reach no other
    block; under FULL a pattern with one entry of one block missing is HQPKKT_E_FORMAT and nothing changes."""
    for name, base, cls, bsize, pattern in (("P1", block_diag_qp(), ipmatrix.IpSpBKP, -1, False), ("band257", band_qp(257), ipmatrix.IpRedSpBKP, 7, True),
                                            ("band4097", band_qp(4097), ipmatrix.IpSpBKP, 256, True)):
        n = base.n
        first = blocks_of(base, bsize)
        nb = len(first) - 1
        of = np.repeat(np.arange(nb), np.diff(first))
        s, y = mixed_inputs(base, first, 9)
        V = Vecs(False)
        ref = update(handle(cls, base), V, s, y, bsize, pattern)
        # below the diagonal
        prog, low = with_lower_nan(base)
        assert (blocks_of(prog, bsize) == first).all(), name  # (a row's LAST column decides, and it is unchanged)
        got = update(handle(cls, prog), V, s, y, bsize, pattern)
        assert np.isnan(got[4][low]).all() and bits(got[4][~low], ref[4]), name
        assert all(bits(a, b) for a, b in zip(got[:3], ref[:3])), name
        # across two blocks
        r, ix = rows_of(base.Q), np.asarray(base.Q[1])
        cross = of[r] != of[ix]
        if cross.any():
            x = np.array(base.Q[2], dtype=np.float64)
            x[cross] = np.nan
            got = update(handle(cls, with_q(base, x)), V, s, y, bsize, pattern)
            assert np.isnan(got[4][cross]).all() and bits(got[4][~cross], ref[4][~cross]) and bits(ref[4][cross], np.asarray(base.Q[2])[cross]), name
            assert all(bits(a, b) for a, b in zip(got[:3], ref[:3])), name
        # the skipped blocks
        s2, y2 = s.copy(), y.copy()
        b0, b1 = 2, 4
        s2[first[b0]: first[b0 + 1]] = 0.0
        y2[first[b1] + (first[b1 + 1] - first[b1]) // 2] = np.nan
        M = handle(cls, base)
        got = update(M, V, s2, y2, bsize, pattern)
        out = check_against_replay(base, first, s2, y2, got, name)
        assert out[b0] == 2 and out[b1] == 3, (name, out[:6])
        skipped = (of[r] == b0) | (of[r] == b1)
        assert bits(got[4][skipped], np.asarray(base.Q[2])[skipped]) and bits(got[4][~skipped], ref[4][~skipped]), name
        assert bits(np.delete(got[2], (b0, b1), 0), np.delete(ref[2], (b0, b1), 0)), name
    # one entry of one block missing
    base = block_diag_qp()
    p, ix, x = (np.array(a) for a in base.Q)
    k = int(p[300]) + 5  # (row 300 lies in the block of 255; its sixth stored entry)
    assert ix[k] > 300
    p[301:] -= 1
    bad = problems.Program(base.n, base.me, base.m, (p, np.delete(ix, k), np.delete(x, k)), base.A, base.C, base.c, base.b, base.d)
    first = blocks_of(bad, -1)
    s, y = mixed_inputs(bad, first, 9)
    for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):
        M = handle(cls, bad)
        f2, full = M.q_blocks(-1)
        assert (f2 == first).all() and full.tolist() == [1, 1, 1, 1, 1, 0, 1], full
        try:
            M.q_bfgs_update(s, y)
            raise AssertionError("accepted")
        except ipmatrix.KktError as e:
            assert e.code == _lib.E_FORMAT
        assert bits(M.q_values(), bad.Q[2])
        check_against_replay(bad, first, s, y, update(M, Vecs(False), s, y, -1, True), "one entry missing")


def check_reproducible():
    """Equal bits from call to call, over the plugins and over host and device vectors; and for a full block of 257 wherever
    it lies: P1 with its blocks permuted."""
    for name, prog, classes, bsize, pattern in cases():
        if name.startswith("P3") and prog.n not in (65, 4097):
            continue
        first = blocks_of(prog, bsize)
        s, y = mixed_inputs(prog, first, 21)
        ref = None
        for cls in classes:
            for device in (False, True):
                V = Vecs(device)
                M = handle(cls, prog, device)
                for _ in range(2):
                    M.update(prog)
                    res = update(M, V, s, y, bsize, pattern)
                    ref = ref or res
                    assert all(bits(a, b) for a, b in zip(res, ref)), (name, cls.__name__, device, bsize)
    base = block_diag_qp()
    f0 = blocks_of(base, -1)
    s0, y0 = mixed_inputs(base, f0, 4)
    y0[f0[6]: f0[7]] *= -0.5 / 1.1 if (6 + 4) % 3 else 1.0  # (the block of 257 damped, so that s'v is compared too)
    r0 = update(handle(ipmatrix.IpSpBKP, base), Vecs(False), s0, y0, -1, False)
    assert r0[2][6, OUTCOME] == 1
    d0 = rows_of(base.Q) >= f0[6]
    for orders in ((257, 1, 2, 63, 64, 65, 255), (64, 65, 257, 255, 1, 2, 63)):
        prog = block_diag_qp(orders)
        first = blocks_of(prog, -1)
        at = orders.index(257)
        assert first[at + 1] - first[at] == 257
        s, y = mixed_inputs(prog, first, 8)
        s[first[at]: first[at + 1]], y[first[at]: first[at + 1]] = s0[f0[6]:], y0[f0[6]:]
        res = update(handle(ipmatrix.IpRedSpBKP, prog), Vecs(False), s, y, -1, False)
        assert bits(res[2][at, :5], r0[2][6, :5]) and res[2][at, OUTCOME] == 1, orders
        r = rows_of(prog.Q)
        d = (r >= first[at]) & (r < first[at + 1])
        assert bits(res[3][d], r0[3][d0]) and bits(res[4][d], r0[4][d0]), orders
        assert bits(res[0][first[at]: first[at + 1]], r0[0][f0[6]:]) and bits(res[1][first[at]: first[at + 1]], r0[1][f0[6]:]), orders


def check_handle_afterwards():
    """After the update the handle is not factored; then factor, step, residuum, solve and hqpkkt_mehrotra are bit-identical
    to a FRESH handle of the same class given the new q_values() through hqpkkt_set_values.  Once more under zd_policy -1
    with a Q so small that its diagonals are weak before and after the update."""
    from common import new_d
    from q_values_worker import _state_bits
    sp = (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP)
    todo = [("random", problems.random_sparse_qp(150, 40, 90, row_nnz=3), sp, 0, True, (False, True)),
            ("grid", problems.grid_sparse_qp(14, 11), sp, 0, True, (False,)),
            ("docp", docp_qp(), sp + (ipmatrix.IpLQDOCP,), -1, False, (False,))]
    for name, base, classes, bsize, pattern, weaks in todo:
        st = problems.ip_state(base, seed=12, spread=1.0)
        for cls in classes:
            for weak in weaks:
                prog = with_q(base, 1e-4 * np.asarray(base.Q[2])) if weak else base
                first = blocks_of(prog, bsize)
                s, y = mixed_inputs(prog, first, 31, damp_every=10 ** 6)
                tag = (name, cls.__name__, weak)
                M = handle(cls, prog, zd_policy=-1)
                M.factor(prog, st[0], st[1])  # (factored - and not any more after the update)
                M.q_bfgs_update(s, y, bsize=bsize, pattern=pattern)
                if weak:
                    assert M.debug(30)[1] == 1, tag
                with np.testing.assert_raises(ipmatrix.KktError) as e:
                    M.solve(prog, *st, *new_d(prog))
                assert e.exception.code == _lib.E_INTERN, tag
                qx = M.q_values()
                assert not bits(qx, prog.Q[2]) and np.isfinite(qx).all(), tag
                prog2 = with_q(prog, qx)
                F = handle(cls, prog2, zd_policy=-1)
                assert (F.debug(30) == M.debug(30)).all(), tag
                a, b = _state_bits(M, prog2, st), _state_bits(F, prog2, st)
                assert len(a) == len(b) and all(bits(p, q) for p, q in zip(a, b)), tag
                if not weak:
                    assert a[0] == 0.0 and np.isfinite(a[1]).all(), tag  # (the factorisation went through)


def check_refused_handles():
    """HQPKKT_E_INTERN on dense stage Hessians and before values; hqpkkt_q_bfgs_report: HQPKKT_E_INTERN before an update,
    HQPKKT_E_RANGE with *n_blocks set on a short cap."""
    L = _lib.lib()
    prog = docp_qp()
    x = np.ones(prog.n)
    D = ipmatrix.IpLQDOCP(q_dense=True)
    D.init(prog)
    N = ipmatrix.IpSpBKP()
    N.analyze(prog)
    for H in (D, N):
        for call in (lambda: H.q_bfgs_update(x, x), lambda: H.q_bfgs_update(x, x, pattern=True), H.q_bfgs_report):
            try:
                call()
                raise AssertionError("accepted")
            except ipmatrix.KktError as e:
                assert e.code == _lib.E_INTERN
    assert (N.q_blocks(-1)[0] == blocks_of(prog, -1)).all()  # (the analysis is all it needs)
    G = handle(ipmatrix.IpSpBKP, prog)
    k = C.c_longlong()
    out = np.zeros(8)
    assert L.hqpkkt_q_bfgs_report(G._h, C.c_void_p(out.ctypes.data), 1, C.byref(k)) == _lib.E_INTERN
    G.q_dscale_update(x, x, bsize=7)  # (another entry's report is not this one's)
    assert L.hqpkkt_q_bfgs_report(G._h, C.c_void_p(out.ctypes.data), 1, C.byref(k)) == _lib.E_INTERN
    G.q_bfgs_update(x, x)
    assert L.hqpkkt_q_bfgs_report(G._h, C.c_void_p(out.ctypes.data), 1, C.byref(k)) == _lib.E_RANGE and k.value == 5
    assert G.q_bfgs_report().shape == (5, 8)
    G.q_bfgs_update(x, x, bsize=4, pattern=True)
    assert G.q_bfgs_report().shape == (6, 8) and G.q_dscale_report().shape == (4, 8)


CHECKS = {f.__name__[6:]: f for f in (check_integers, check_reals, check_product_bits, check_secant, check_untouched_and_skips,
                                       check_reproducible, check_handle_afterwards, check_refused_handles)}


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
    print("Q_BFGS_RESULTS " + json.dumps(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
