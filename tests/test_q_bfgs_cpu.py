"""CPU tests of hqpkkt_q_blocks, hqpkkt_q_bfgs_update and hqpkkt_q_bfgs_report: the exported symbols and the struct, the partition
of hqpkkt_q_blocks - host code, complete without a device - against hessian_update.q_blocks_model, the return codes a
host-only run reaches in the header's order, and the numpy models: q_bfgs_replay against q_bfgs_terms bit for bit,
q_bfgs_terms against the dense formula of bfgs_terms, and the secant bound of tests/q_bfgs_worker.py on the model alone.

A handle gets its values through the device alone, so on a host without one "no values yet" (HQPKKT_E_INTERN) answers
before HQPKKT_E_FORMAT can, as in test_q_values_cpu.py; tests/test_gpu_q_bfgs.py reaches the rest."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hqp_amd import _lib, ipmatrix, problems  # noqa: E402
from hqp_amd import hessian_update as hu  # noqa: E402
import q_bfgs_worker as W  # noqa: E402


def vp(a):
    return C.c_void_p(a.ctypes.data)


def _upd(s, y, gamma=0.1, alpha=1.0, bsize=-1, fill=0):
    u = _lib.QBfgsUpdate()
    u.s, u.y, u.gamma, u.alpha, u.bsize, u.fill = s.ctypes.data, y.ctypes.data, gamma, alpha, bsize, fill
    return u


def test_symbols_constants_and_struct():
    L = _lib.lib()
    names = ("hqpkkt_q_blocks", "hqpkkt_q_bfgs_update", "hqpkkt_q_bfgs_report")
    assert set(names) <= set(_lib.SYMBOLS)
    for nm in names:
        assert getattr(L, nm) is not None
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "hqpkkt.h")).read()
    assert "#define HQPKKT_QBFGS_FULL 0" in hdr and _lib.HQPKKT_QBFGS_FULL == 0
    assert "#define HQPKKT_QBFGS_PATTERN 1" in hdr and _lib.HQPKKT_QBFGS_PATTERN == 1
    assert "#define HQPKKT_QBFGS_REPORT 8" in hdr and _lib.HQPKKT_QBFGS_REPORT == 8
    # two pointers, two doubles, two ints, two pointers on an LP64 host
    S = _lib.QBfgsUpdate
    assert C.sizeof(S) == 56
    assert (S.s.offset, S.y.offset, S.gamma.offset, S.alpha.offset, S.bsize.offset, S.fill.offset, S.v.offset, S.Qs.offset) == (0, 8, 16, 24, 32, 36, 40, 48)
    for nm in ("q_blocks", "q_bfgs_update", "q_bfgs_report"):
        assert callable(getattr(ipmatrix.Hqp_IpMatrix, nm))


def _gaps_qp():
    """n = 12: row 3 without entries, row 7 holding a sub-diagonal entry alone, the others a diagonal and here and there a
    reach of one or two"""
    rows = [0, 0, 1, 2, 4, 4, 5, 6, 7, 8, 8, 9, 10, 11]
    cols = [0, 1, 1, 2, 4, 6, 5, 6, 5, 8, 9, 9, 10, 11]
    n = 12
    Q = problems._csr(rows, cols, np.arange(1.0, len(rows) + 1), n)
    e = problems._csr([], [], [], 0)
    return problems.Program(n, 0, 0, Q, e, e)


def _block_programs():
    band = W.band_qp(40)
    return [("blockdiag", W.block_diag_qp()), ("docp", W.docp_qp()), ("band", band), ("gaps", _gaps_qp())]


@pytest.mark.parametrize("which", range(4))
def test_q_blocks_against_model(which):
    name, prog = _block_programs()[which]
    n = prog.n
    L = _lib.lib()
    M = ipmatrix.IpSpBKP()
    k = C.c_longlong(-1)
    assert L.hqpkkt_q_blocks(M._h, -1, None, None, 0, C.byref(k)) == _lib.E_INTERN  # (before the analysis)
    assert L.hqpkkt_q_blocks(None, -1, None, None, 0, C.byref(k)) == L.hqpkkt_q_blocks(M._h, -1, None, None, 0, None) == _lib.E_NULL
    M.analyze(prog)
    for bsize in (-1, 0, 1, 7, n - 1, n, n + 5):
        first, full = hu.q_blocks_model(prog.Q[0], prog.Q[1], n, bsize)
        f2, fl2 = M.q_blocks(bsize)
        assert f2.tolist() == first.tolist() and fl2.tolist() == full.tolist(), (name, bsize)
        assert first[0] == 0 and first[-1] == n and (np.diff(first) > 0).all()
        # the protocol: the count alone; a cap too small; a cap that fits, without full
        nb = len(full)
        assert L.hqpkkt_q_blocks(M._h, bsize, None, None, 0, C.byref(k)) == _lib.OK and k.value == nb
        buf = np.full(nb + 1, -7, dtype=np.int32)
        k.value = -1
        assert L.hqpkkt_q_blocks(M._h, bsize, vp(buf), None, nb - 1, C.byref(k)) == _lib.E_RANGE and k.value == nb
        assert (buf == -7).all()
        assert L.hqpkkt_q_blocks(M._h, bsize, vp(buf), None, nb, C.byref(k)) == _lib.OK and buf.tolist() == first.tolist()
    # what the partitions are
    det, dfull = hu.q_blocks_model(prog.Q[0], prog.Q[1], n, -1)
    if name == "blockdiag":
        assert np.diff(det).tolist() == list(W.ORDERS) and dfull.all()
        assert hu.q_blocks_model(prog.Q[0], prog.Q[1], n, 0)[1].tolist() == [0]
        assert hu.q_blocks_model(prog.Q[0], prog.Q[1], n, 1)[1].all()
    elif name == "docp":
        assert np.diff(det).tolist() == [5, 5, 5, 5, 3] and dfull.all()
    elif name == "band":
        assert det.tolist() == [0, n] and dfull.tolist() == [0]
        assert not hu.q_blocks_model(prog.Q[0], prog.Q[1], n, 7)[1].any() and hu.q_blocks_model(prog.Q[0], prog.Q[1], n, 2)[1].all()
    else:
        assert det.tolist() == [0, 2, 3, 4, 7, 8, 10, 11, 12], det
        assert dfull.tolist() == [1, 1, 0, 0, 0, 1, 1, 1], dfull


def test_q_blocks_of_nothing():
    """n = 0: no blocks.  hqpkkt_analyze itself refuses a program without variables (HQPKKT_E_SIZES), so through the ABI the
    entry stays at "not analysed"; the model answers for the partition."""
    e = problems._csr([], [], [], 0)
    prog = problems.Program(0, 0, 0, e, e, e)
    for bsize in (-1, 0, 3):
        first, full = hu.q_blocks_model(prog.Q[0], prog.Q[1], 0, bsize)
        assert first.size == 0 and full.size == 0
    M = ipmatrix.IpSpBKP()
    with pytest.raises(ipmatrix.KktError) as ex:
        M.analyze(prog)
    assert ex.value.code == _lib.E_SIZES
    k = C.c_longlong(-1)
    assert _lib.lib().hqpkkt_q_blocks(M._h, -1, None, None, 0, C.byref(k)) == _lib.E_INTERN


@pytest.mark.parametrize("cls", [ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP, ipmatrix.IpLQDOCP])
def test_null_then_range_then_intern(cls):
    L = _lib.lib()
    M = cls()
    a, b = np.ones(8), np.ones(8)
    k = C.c_longlong()
    # E_NULL first
    assert L.hqpkkt_q_bfgs_update(None, C.byref(_upd(a, b))) == L.hqpkkt_q_bfgs_update(M._h, None) == _lib.E_NULL
    for gone in ("s", "y"):
        u = _upd(a, b, gamma=float("nan"))  # (with a RANGE error behind it E_NULL still answers first)
        setattr(u, gone, None)
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(u)) == _lib.E_NULL
    assert L.hqpkkt_q_bfgs_report(None, vp(a), 1, C.byref(k)) == L.hqpkkt_q_bfgs_report(M._h, None, 1, C.byref(k)) == _lib.E_NULL
    assert L.hqpkkt_q_bfgs_report(M._h, vp(a), 1, None) == _lib.E_NULL
    # E_RANGE next, before the call order is looked at: gamma not finite; gamma < 0 with alpha not finite; fill
    for gamma in (float("inf"), float("nan"), -float("inf")):
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(a, b, gamma=gamma))) == _lib.E_RANGE
    for alpha in (float("inf"), float("nan")):
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(a, b, gamma=-0.2, alpha=alpha))) == _lib.E_RANGE
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(a, b, gamma=0.2, alpha=alpha))) == _lib.E_INTERN  # (alpha is not read)
    for fill in (-1, 2, 8):
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(a, b, fill=fill))) == _lib.E_RANGE
    # E_INTERN: before analyse - a negative gamma is valid - and before values
    for fill in (0, 1):
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(a, b, gamma=-0.2, alpha=0.5, fill=fill))) == _lib.E_INTERN
    assert L.hqpkkt_q_bfgs_report(M._h, vp(a), 1, C.byref(k)) == _lib.E_INTERN
    prog = problems.lq_docp(4, 3, 2) if cls is ipmatrix.IpLQDOCP else W.band_qp(40)
    M.analyze(prog)
    s, y = np.ones(prog.n), np.ones(prog.n)
    for fill in (0, 1):  # (band_qp is not fully stored: "no values yet" answers before HQPKKT_E_FORMAT)
        assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(s, y, fill=fill))) == _lib.E_INTERN
    assert L.hqpkkt_q_bfgs_report(M._h, vp(np.zeros(8 * prog.n)), prog.n, C.byref(k)) == _lib.E_INTERN
    assert L.hqpkkt_q_bfgs_update(M._h, C.byref(_upd(s, y, gamma=float("nan")))) == _lib.E_RANGE


def _dense_block(ln, rng):
    M = rng.uniform(-1.0, 1.0, (ln, ln))
    return M @ M.T / ln + np.diag(rng.uniform(0.5, 1.5, ln))


def _upper_csr(B):
    i, j = np.triu_indices(B.shape[0])
    return problems._csr(i, j, B[i, j], B.shape[0])


def test_replay_reproduces_terms():
    """200 random full blocks of 1 .. 300 variables, a third of them damped: q_bfgs_replay fed the sums and the Qs of
    q_bfgs_terms gives its v, its new values and its outcomes bit for bit; and the terms are the dense formula of bfgs_terms,
    Q + c0 v v' + c1 Qs Qs', to rounding."""
    rng = np.random.default_rng(20241)
    damped = 0
    for case in range(200):
        ln = 1 + case * 299 // 199
        B = _dense_block(ln, rng)
        Q = _upper_csr(B)
        s = rng.normal(size=ln)
        if case % 3 == 0:  # y against the curvature: s'y < gamma s'Qs
            y = -0.5 * (B @ s) + 0.01 * rng.normal(size=ln)
        else:
            y = (B @ s) * rng.uniform(0.9, 1.3, size=ln)
        first = np.array([0, ln])
        rep, v, Qs, xn = hu.q_bfgs_terms(Q, s, y, first, gamma=0.1)
        assert rep.shape == (1, 8) and rep[0, 5] == 0 and rep[0, 6] == ln and rep[0, 2] == 0.1
        damped += rep[0, 7] == 1
        if case % 3 == 0:
            assert rep[0, 7] == 1 and rep[0, 0] < 0.1 * rep[0, 1] and rep[0, 3] != 1.0
        else:
            assert rep[0, 7] == 0 and rep[0, 3] == 1.0 and rep[0, 4] == rep[0, 0] and (v == y).all()
        v2, x2, out = hu.q_bfgs_replay(rep, Q, y, Qs, first)
        assert v2.tobytes() == v.tobytes() and x2.tobytes() == xn.tobytes() and out[0] == rep[0, 7]
        assert (xn != Q[2]).all()
        # the dense formula
        (vd, Qsd), coef = hu.bfgs_terms(s, y, B @ s, first, gamma=0.1)
        want = B + coef[0, 0] * np.outer(vd, vd) + coef[0, 1] * np.outer(Qsd, Qsd)
        i, j = np.triu_indices(ln)
        scale = np.abs(B).max() + abs(coef[0, 0]) * np.abs(vd).max() ** 2 + abs(coef[0, 1]) * np.abs(Qsd).max() ** 2
        assert np.abs(xn - want[i, j]).max() <= 64 * ln * 2.0 ** -53 * scale, (case, ln)
    assert damped == 67


def test_pattern_is_the_masked_dense_formula():
    """Under ``pattern`` the stored entries of a block get the dense formula's values - with Q s over the stored symmetric image
    - and nothing else exists; blocks have sums of their own; entries across two blocks and below the diagonal stay; a
    block with s = 0 is left alone (2), one with a NaN in y as well (3), and neither reaches another block; pattern=False
    refuses a block that is not full; gamma < 0 is adapted to alpha."""
    for prog in (W.band_qp(23), problems.random_sparse_qp(30, 5, 8, row_nnz=3), problems.grid_sparse_qp(5, 4)):
        n = prog.n
        p, ix, x = (np.asarray(a) for a in prog.Q)
        r = W.rows_of(prog.Q)
        D = np.zeros((n, n))
        D[r[ix >= r], ix[ix >= r]] = x[ix >= r]
        D = D + np.triu(D, 1).T
        rng = np.random.default_rng(3)
        s = rng.normal(size=n)
        y = (D @ s) * 1.1
        rep, v, Qs, xn = hu.q_bfgs_terms(prog.Q, s, y, [0, n], pattern=True)
        (vd, Qsd), coef = hu.bfgs_terms(s, y, D @ s, [0, n], gamma=0.1)
        want = D + coef[0, 0] * np.outer(vd, vd) + coef[0, 1] * np.outer(Qsd, Qsd)
        up = ix >= r
        assert np.abs(Qs - D @ s).max() <= 64 * n * 2.0 ** -53 * np.abs(D).max() * np.abs(s).max()
        assert np.abs(xn[up] - want[r[up], ix[up]]).max() <= 64 * n * 2.0 ** -53 * (np.abs(want).max() + np.abs(D).max()) and rep[0, 7] in (0, 1)
        assert xn[~up].tobytes() == x[~up].tobytes()
        with pytest.raises(ValueError):
            hu.q_bfgs_terms(prog.Q, s, y, [0, n], pattern=False)
    prog = W.band_qp(23)
    n = 23
    first = hu.q_blocks_model(prog.Q[0], prog.Q[1], n, 7)[0]
    assert first.tolist() == [0, 7, 14, 21, 23]
    s, y = W.mixed_inputs(prog, first, 1)
    rep, v, Qs, xn = hu.q_bfgs_terms(prog.Q, s, y, first, pattern=True)
    r, ix = W.rows_of(prog.Q), np.asarray(prog.Q[1])
    of = np.repeat(np.arange(4), np.diff(first))
    cross = of[r] != of[ix]
    assert cross.any() and xn[cross].tobytes() == np.asarray(prog.Q[2])[cross].tobytes() and (xn[~cross] != np.asarray(prog.Q[2])[~cross]).all()
    assert sorted(set(rep[:, 7].tolist())) == [0, 1]
    for k in range(4):  # a block of its own gives the same bits
        a, e = first[k], first[k + 1]
        sub = W.band_qp(e - a)
        inside = (of[r] == k) & ~cross
        sub = W.with_q(sub, np.asarray(prog.Q[2])[inside])
        assert (np.asarray(sub.Q[1]) == ix[inside] - a).all()
        r1, v1, q1, x1 = hu.q_bfgs_terms(sub.Q, s[a:e], y[a:e], [0, e - a], pattern=True)
        assert r1[0, :5].tobytes() == rep[k, :5].tobytes() and x1.tobytes() == xn[inside].tobytes() and q1.tobytes() == Qs[a:e].tobytes()
    s2, y2 = s.copy(), y.copy()
    s2[7:14] = 0.0
    y2[16] = np.nan
    rep2, v2, Qs2, xn2 = hu.q_bfgs_terms(prog.Q, s2, y2, first, pattern=True)
    assert rep2[:, 7].tolist() == [rep[0, 7], 2, 3, rep[3, 7]]
    mid = (of[r] == 1) | (of[r] == 2)
    assert xn2[mid].tobytes() == np.asarray(prog.Q[2])[mid].tobytes() and xn2[~mid].tobytes() == xn[~mid].tobytes()
    assert hu.q_bfgs_replay(rep2, prog.Q, y2, Qs2, first)[1].tobytes() == xn2.tobytes()
    prog_nan, low = W.with_lower_nan(prog)
    xn3 = hu.q_bfgs_terms(prog_nan.Q, s, y, first, pattern=True)[3]
    assert np.isnan(xn3[low]).all() and xn3[~low].tobytes() == xn.tobytes()
    repa = hu.q_bfgs_terms(prog.Q, s, y, first, gamma=-0.2, alpha=0.5, pattern=True)[0]
    assert (repa[:, 2] == 0.2 + 0.8 * 0.5).all()


def test_secant_bound_holds_for_the_model():
    """q_bfgs_terms alone - sequential sums, every operation rounded once - stays inside the bound that the GPU check
    `secant` holds the device to, on that check's inputs."""
    prog = W.block_diag_qp()
    first = W.blocks_of(prog, -1)
    s, y = W.secant_inputs(prog, first, 77)
    rep, v, Qs, xn = hu.q_bfgs_terms(prog.Q, s, y, first)
    assert sorted(set(rep[:, 7].tolist())) == [0, 1] and (s * y > 0).all()
    after = W.restricted_product(W.with_q(prog, xn).Q, s, first, np.float64)[0]
    worst, rows = W.secant_excess(prog.Q, xn, s, v, Qs, rep, first, after)
    assert rows == prog.n and 0.0 < worst <= 1.0, worst
