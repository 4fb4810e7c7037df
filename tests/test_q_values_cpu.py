"""CPU tests of the entries on the sparse Q (hqpkkt_q_values .. hqpkkt_q_dscale_report, hqpkkt_lagrangian_gradient): the
exported symbols, the return codes in the header's order, and the numpy models of hessian_update - dscale_replay against
dscale_terms, q_gerschgorin_model against a dense restatement.

What a host-only run reaches: a handle gets its values through the device alone, so on a host without one "no values yet"
(HQPKKT_E_INTERN, third in the order) answers before the diagonal rule (HQPKKT_E_FORMAT, fourth) and the device
(HQPKKT_E_DEVICE, last) can.  The two cases of the diagonal rule are written for both kinds of host: where the values
arrive they must give HQPKKT_E_FORMAT, where hqpkkt_set_values itself ends in HQPKKT_E_DEVICE they give HQPKKT_E_INTERN;
tests/test_gpu_q_values.py runs them on the device as well.  A diagonal entry stored twice is no sorted CSR row:
hqpkkt_analyze answers HQPKKT_E_FORMAT itself, and the entries' own test for it is a second line."""
import ctypes as C
import os

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu

NAMES = ("hqpkkt_q_values", "hqpkkt_q_product", "hqpkkt_q_row_stats", "hqpkkt_q_set_diagonal", "hqpkkt_q_gerschgorin",
         "hqpkkt_q_dscale_setup", "hqpkkt_q_dscale_update", "hqpkkt_q_dscale_report", "hqpkkt_lagrangian_gradient")


def vp(a):
    return C.c_void_p(a.ctypes.data)


def _upd(s, y, gamma=0.2, bsize=0):
    u = _lib.DScaleUpdate()
    u.s, u.y, u.gamma, u.bsize = s.ctypes.data, y.ctypes.data, gamma, bsize
    return u


def _give_values(M, prog):
    """init(): True where the values arrived, False where the host has no device for them."""
    M.analyze(prog)
    try:
        M.update(prog)
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_DEVICE
        return False
    return True


def _calls(M, n, me, m):
    """every entry with arguments that pass its NULL and RANGE tests: name -> code"""
    L = _lib.lib()
    a, b = np.ones(n), np.ones(n)
    y, z = np.ones(max(me, 1)), np.ones(max(m, 1))
    u = _upd(a, b)
    k = C.c_longlong()
    rep = np.zeros((n, 8))
    qx = np.zeros(4096)
    return {
        "q_values": L.hqpkkt_q_values(M._h, vp(qx)),
        "q_product": L.hqpkkt_q_product(M._h, vp(a), vp(b)),
        "q_row_stats": L.hqpkkt_q_row_stats(M._h, vp(a), None),
        "q_set_diagonal": L.hqpkkt_q_set_diagonal(M._h, vp(a)),
        "q_gerschgorin": L.hqpkkt_q_gerschgorin(M._h, 1.0),
        "q_dscale_setup": L.hqpkkt_q_dscale_setup(M._h, 1e-8),
        "q_dscale_update": L.hqpkkt_q_dscale_update(M._h, C.byref(u)),
        "q_dscale_report": L.hqpkkt_q_dscale_report(M._h, vp(rep), n, C.byref(k)),
        "lagrangian_gradient": L.hqpkkt_lagrangian_gradient(M._h, vp(a), vp(y), vp(z), None, vp(b)),
    }


WRITERS = ("q_set_diagonal", "q_gerschgorin", "q_dscale_setup", "q_dscale_update")


def test_symbols_constant_and_struct():
    L = _lib.lib()
    assert set(NAMES) <= set(_lib.SYMBOLS)
    for nm in NAMES:
        assert getattr(L, nm) is not None
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "hqpkkt.h")).read()
    assert "#define HQPKKT_DSCALE_REPORT 8" in hdr and _lib.HQPKKT_DSCALE_REPORT == 8
    assert "the reference's Hqp_HL_DScale. */" not in hdr  # (the "Not built" line has lost it)
    # two pointers, double, int (+ 4), pointer on an LP64 host
    assert C.sizeof(_lib.DScaleUpdate) == 40
    assert _lib.DScaleUpdate.gamma.offset == 16 and _lib.DScaleUpdate.bsize.offset == 24 and _lib.DScaleUpdate.v.offset == 32
    for nm in ("q_values", "q_product", "q_row_stats", "q_set_diagonal", "q_gerschgorin", "q_dscale_setup", "q_dscale_update",
               "q_dscale_report", "lagrangian_gradient"):
        assert callable(getattr(ipmatrix.Hqp_IpMatrix, nm))


@pytest.mark.parametrize("cls", [ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP, ipmatrix.IpLQDOCP])
def test_null_then_range_then_intern(cls):
    L = _lib.lib()
    M = cls()
    a, b = np.ones(8), np.ones(8)
    k = C.c_longlong()
    # E_NULL first: no handle, or a vector the entry cannot do without
    assert L.hqpkkt_q_values(None, vp(a)) == L.hqpkkt_q_values(M._h, None) == _lib.E_NULL
    assert L.hqpkkt_q_product(None, vp(a), vp(b)) == L.hqpkkt_q_product(M._h, None, vp(b)) == L.hqpkkt_q_product(M._h, vp(a), None) == _lib.E_NULL
    assert L.hqpkkt_q_row_stats(None, vp(a), vp(b)) == L.hqpkkt_q_row_stats(M._h, None, None) == _lib.E_NULL
    assert L.hqpkkt_q_set_diagonal(None, vp(a)) == L.hqpkkt_q_set_diagonal(M._h, None) == _lib.E_NULL
    assert L.hqpkkt_q_gerschgorin(None, 1.0) == L.hqpkkt_q_dscale_setup(None, 1.0) == _lib.E_NULL
    assert L.hqpkkt_q_dscale_update(None, C.byref(_upd(a, b))) == L.hqpkkt_q_dscale_update(M._h, None) == _lib.E_NULL
    u = _upd(a, b)
    u.s = None
    assert L.hqpkkt_q_dscale_update(M._h, C.byref(u)) == _lib.E_NULL
    u = _upd(a, b)
    u.y = None
    assert L.hqpkkt_q_dscale_update(M._h, C.byref(u)) == _lib.E_NULL
    assert L.hqpkkt_q_dscale_report(None, vp(a), 1, C.byref(k)) == L.hqpkkt_q_dscale_report(M._h, None, 1, C.byref(k)) == _lib.E_NULL
    assert L.hqpkkt_q_dscale_report(M._h, vp(a), 1, None) == _lib.E_NULL
    assert L.hqpkkt_lagrangian_gradient(None, vp(a), vp(a), vp(a), None, vp(b)) == _lib.E_NULL
    assert L.hqpkkt_lagrangian_gradient(M._h, None, vp(a), vp(a), None, vp(b)) == _lib.E_NULL
    assert L.hqpkkt_lagrangian_gradient(M._h, vp(a), vp(a), vp(a), None, None) == _lib.E_NULL
    # E_RANGE next - with a NULL behind it E_NULL still answers first
    for eps in (0.0, float("nan"), -1.0, float("inf")):
        assert L.hqpkkt_q_gerschgorin(M._h, eps) == L.hqpkkt_q_dscale_setup(M._h, eps) == _lib.E_RANGE
        assert L.hqpkkt_q_gerschgorin(None, eps) == _lib.E_NULL
    for gamma in (-0.1, float("inf"), float("nan")):
        assert L.hqpkkt_q_dscale_update(M._h, C.byref(_upd(a, b, gamma=gamma))) == _lib.E_RANGE
    # E_INTERN: before analyse ...
    assert set(_calls(M, 8, 2, 2).values()) == {_lib.E_INTERN}
    # ... and before values; a missing multiplier vector is E_NULL once the sizes are known
    prog = problems.lq_docp(4, 3, 2) if cls is ipmatrix.IpLQDOCP else problems.banded_qp(40, 3)
    M.analyze(prog)
    assert set(_calls(M, prog.n, prog.me, prog.m).values()) == {_lib.E_INTERN}
    x = np.ones(prog.n)
    assert L.hqpkkt_lagrangian_gradient(M._h, vp(x), None, vp(np.ones(prog.m)), None, vp(x)) == _lib.E_NULL
    for eps in (0.0, float("nan")):
        assert L.hqpkkt_q_gerschgorin(M._h, eps) == _lib.E_RANGE  # (before the call order is looked at)


def test_intern_on_dense_stage_hessians():
    """The Hessians of a q_dense=True handle are the blocks: every hqpkkt_q_* entry refuses; hqpkkt_lagrangian_gradient does not
    touch Q and is accepted where the values have arrived."""
    prog = problems.lq_docp(4, 3, 2)
    M = ipmatrix.IpLQDOCP(q_dense=True)
    have = _give_values(M, prog)
    codes = _calls(M, prog.n, prog.me, prog.m)
    for nm, code in codes.items():
        if nm == "lagrangian_gradient":
            assert code == (_lib.OK if have else _lib.E_INTERN)
        else:
            assert code == _lib.E_INTERN, nm


def _without_diagonal(prog, row):
    p, ix, x = (np.array(a) for a in prog.Q)
    k = int(p[row] + np.flatnonzero(ix[p[row]: p[row + 1]] == row)[0])
    p[row + 1:] -= 1
    return problems.Program(prog.n, prog.me, prog.m, (p, np.delete(ix, k), np.delete(x, k)), prog.A, prog.C, prog.c, prog.b, prog.d)


def _diagonal_twice(prog, row):
    p, ix, x = (np.array(a) for a in prog.Q)
    k = int(p[row] + np.flatnonzero(ix[p[row]: p[row + 1]] == row)[0])
    p[row + 1:] += 1
    return problems.Program(prog.n, prog.me, prog.m, (p, np.insert(ix, k, row), np.insert(x, k, 1.0)), prog.A, prog.C, prog.c, prog.b, prog.d)


@pytest.mark.parametrize("cls", [ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP])
def test_format_by_the_diagonal_rule_and_device_last(cls):
    """banded_qp(40, 3) without the stored diagonal of row 7: the entries that write the diagonal answer HQPKKT_E_FORMAT, the
    others work; on a host without a device everything stops at "no values yet".  On the complete pattern HQPKKT_E_DEVICE
    is what is left to a host without a device - of hqpkkt_set_values itself."""
    base = problems.banded_qp(40, 3)
    prog = _without_diagonal(base, 7)
    M = cls()
    have = _give_values(M, prog)
    codes = _calls(M, prog.n, prog.me, prog.m)
    for nm, code in codes.items():
        if not have:
            assert code == _lib.E_INTERN, nm
        elif nm in WRITERS:
            assert code == _lib.E_FORMAT, nm
        elif nm == "q_dscale_report":
            assert code == _lib.E_INTERN  # (no update has run)
        else:
            assert code == _lib.OK, nm
    if have:  # the statistics of the row without a diagonal
        dg, _off = M.q_row_stats()
        assert dg[7] == 0.0 and (np.delete(dg, 7) != 0.0).all()
    M2 = cls()
    have2 = _give_values(M2, base)
    assert have2 == have
    for nm, code in _calls(M2, base.n, base.me, base.m).items():
        assert code == (_lib.OK if have else _lib.E_INTERN), nm


def test_format_for_a_diagonal_stored_twice():
    prog = _diagonal_twice(problems.banded_qp(40, 3), 7)
    M = ipmatrix.IpSpBKP()
    with pytest.raises(ipmatrix.KktError) as e:
        M.analyze(prog)
    assert e.value.code == _lib.E_FORMAT
    assert set(_calls(M, prog.n, prog.me, prog.m).values()) == {_lib.E_INTERN}


def test_dscale_replay_reproduces_dscale_terms():
    """200 random blocks of 1 .. 300 variables, a third of them damped: dscale_replay fed the sums of dscale_terms gives its
    v, its new diagonal and its outcomes bit for bit."""
    rng = np.random.default_rng(20240)
    damped = 0
    for case in range(200):
        ln = 1 + case * 299 // 199
        s = rng.normal(size=ln)
        q = rng.uniform(0.5, 2.0, size=ln)
        if case % 3 == 0:  # y against the curvature: s'y < gamma s'Qs
            y = -0.5 * s * q + 0.01 * rng.normal(size=ln)
        else:
            y = s * q * rng.uniform(0.5, 1.5, size=ln)
        rep, v, qn = hu.dscale_terms(s, y, q, gamma=0.2)
        assert rep.shape == (1, 8) and rep[0, 5] == 0 and rep[0, 6] == ln
        damped += rep[0, 7] == 1
        if case % 3 == 0:
            assert rep[0, 7] == 1 and rep[0, 0] < 0.2 * rep[0, 1] and rep[0, 3] != 1.0
        else:
            assert rep[0, 7] == 0 and rep[0, 3] == 1.0 and rep[0, 4] == rep[0, 0] and (v == y).all()
        v2, q2, out = hu.dscale_replay(rep, s, y, q)
        assert v2.tobytes() == v.tobytes() and q2.tobytes() == qn.tobytes() and out[0] == rep[0, 7]
        assert (qn != q).any()
    assert damped == 67


def test_dscale_terms_blocks_and_skips():
    """bsize cuts the variables into blocks with sums of their own; a block with s = 0 is left alone (2), one with a NaN in
    y as well (3), and neither reaches another block."""
    rng = np.random.default_rng(5)
    n = 23
    s, q = rng.normal(size=n), rng.uniform(0.5, 2.0, size=n)
    y = s * q * 1.1
    rep, v, qn = hu.dscale_terms(s, y, q, bsize=7)
    assert rep.shape == (4, 8) and rep[:, 5].tolist() == [0, 7, 14, 21] and rep[:, 6].tolist() == [7, 7, 7, 2]
    for k, (a, e) in enumerate(((0, 7), (7, 14), (14, 21), (21, 23))):
        r1, _v1, q1 = hu.dscale_terms(s[a:e], y[a:e], q[a:e])
        assert r1[0, :5].tobytes() == rep[k, :5].tobytes() and q1.tobytes() == qn[a:e].tobytes()
    s2, y2 = s.copy(), y.copy()
    s2[7:14] = 0.0
    y2[16] = np.nan
    rep2, v2, qn2 = hu.dscale_terms(s2, y2, q, bsize=7)
    assert rep2[:, 7].tolist() == [0, 2, 3, 0]
    assert qn2[7:21].tobytes() == q[7:21].tobytes()
    assert qn2[:7].tobytes() == qn[:7].tobytes() and qn2[21:].tobytes() == qn[21:].tobytes()
    assert hu.dscale_replay(rep2, s2, y2, q, bsize=7)[1].tobytes() == qn2.tobytes()
    assert hu.dscale_terms(s, y, q, bsize=n + 5)[0].shape == (1, 8)  # (a bsize beyond n: one block)


def test_q_gerschgorin_model_against_dense():
    for prog in (problems.banded_qp(40, 3), problems.random_sparse_qp(30, 5, 8, row_nnz=3), problems.grid_sparse_qp(5, 4)):
        p, ix, x = (np.asarray(a) for a in prog.Q)
        x = np.array(x, dtype=np.float64)
        n = prog.n
        rows = np.repeat(np.arange(n), np.diff(p))
        x[ix < rows] = np.nan  # (entries below the diagonal do not exist for the model)
        x[(ix > rows)] = np.round(x[ix > rows] * 8)
        x[ix == rows] = np.round(x[ix == rows])
        x[np.flatnonzero(ix == rows)[::3]] = -2.0  # (diagonals the bound has to lift)
        x[np.flatnonzero(ix == rows)[1::3]] = 1000.0  # (... and diagonals that stay)
        up = ix >= rows
        D = np.zeros((n, n))
        D[rows[up], ix[up]] = x[up]
        D = D + np.triu(D, 1).T
        want = hu.gerschgorin_model(D, 1.0)  # (the dense model of the stage blocks: integers, no rounding)
        got = hu.q_gerschgorin_model((p, ix, x), 1.0)
        dg = ix == rows
        assert (got[dg] == np.diag(want)[rows[dg]]).all()
        assert got[~dg & up].tobytes() == x[~dg & up].tobytes() and np.isnan(got[~up]).all()
        assert (got[dg] > x[dg]).any() and (got[dg] == x[dg]).any()
