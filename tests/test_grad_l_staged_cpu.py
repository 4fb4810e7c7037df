"""CPU tests of hqpkkt_lagrangian_gradient_staged (grad L on a handle of the dense hand-over): the exported symbol, the
return codes a host without a device reaches in the header's order - HQPKKT_E_NULL, then HQPKKT_E_INTERN for a handle that
is not analysed or whose hand-over has not ended - and the numpy model hessian_update.grad_l_dense_model against
c - A'y - C'z formed from the CSR program.  tests/test_gpu_grad_l_staged.py runs the entry on the device."""
import ctypes as C

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu


def vp(a):
    return C.c_void_p(a.ctypes.data)


def analyze_staged(M, dq):
    """hqpkkt_analyze_staged alone: the handle is analysed and has no values"""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    nx, nu = i32(dq.nx), i32(dq.nu)
    arrs = []
    for (p, i, _x) in (dq.Q, dq.E, dq.C):
        arrs += [i32(p), i32(i)]
    ptrs = [vp(a) if a.size else None for a in arrs]
    code = _lib.lib().hqpkkt_analyze_staged(M._h, dq.K, vp(nx), vp(nu), dq.n, dq.me_rest, dq.m, *ptrs)
    return code, arrs + [nx, nu]


def test_symbol_and_method():
    assert "hqpkkt_lagrangian_gradient_staged" in _lib.SYMBOLS
    assert _lib.lib().hqpkkt_lagrangian_gradient_staged is not None
    assert callable(ipmatrix.Hqp_IpLQDOCP.lagrangian_gradient_staged)
    assert callable(hu.grad_l_dense_model)


def test_null_first():
    L = _lib.lib()
    M = ipmatrix.IpLQDOCP()
    a, b = np.ones(8), np.ones(8)
    f = L.hqpkkt_lagrangian_gradient_staged
    assert f(None, vp(a), vp(a), vp(a), None, vp(b)) == _lib.E_NULL
    assert f(M._h, None, vp(a), vp(a), None, vp(b)) == _lib.E_NULL
    assert f(M._h, vp(a), vp(a), vp(a), None, None) == _lib.E_NULL
    assert f(None, None, None, None, None, None) == _lib.E_NULL


def test_intern_on_an_unanalysed_handle():
    L = _lib.lib()
    a, b = np.ones(8), np.ones(8)
    for cls in (ipmatrix.IpLQDOCP, ipmatrix.IpSpBKP):
        M = cls()
        assert L.hqpkkt_lagrangian_gradient_staged(M._h, vp(a), vp(a), vp(a), None, vp(b)) == _lib.E_INTERN
        assert L.hqpkkt_lagrangian_gradient_staged(M._h, vp(a), None, None, vp(a), vp(b)) == _lib.E_INTERN  # (sizes unknown: y, z not asked for)


@pytest.mark.parametrize("q_dense", [False, True])
def test_intern_before_values_and_null_once_sizes_are_known(q_dense):
    L = _lib.lib()
    prog = problems.lq_docp(4, 3, 2, final_eq=2)
    dq = problems.dense_docp_from_program(prog, [3] * 5, [2] * 4, dense_hessian=q_dense)
    M = ipmatrix.IpLQDOCP(q_dense=q_dense)
    code, _keep = analyze_staged(M, dq)
    assert code == _lib.OK
    n, me, m = dq.dims
    c, y, z, out = np.ones(n), np.ones(me), np.ones(m), np.zeros(n)
    f = L.hqpkkt_lagrangian_gradient_staged
    assert f(M._h, vp(c), vp(y), vp(z), None, vp(out)) == _lib.E_INTERN
    assert f(M._h, vp(c), vp(y), vp(z), vp(c), vp(out)) == _lib.E_INTERN
    # a missing multiplier vector is E_NULL once the sizes are known, ahead of "no values yet"
    assert f(M._h, vp(c), None, vp(z), None, vp(out)) == _lib.E_NULL
    assert f(M._h, vp(c), vp(y), None, None, vp(out)) == _lib.E_NULL
    assert (out == 0.0).all()


def test_intern_on_csr_hand_over_before_values():
    """A handle analysed by hqpkkt_analyze (CSR hand-over), STAGED or FULL: refused - here, without values, and with them
    (tests/test_gpu_grad_l_staged.py)."""
    L = _lib.lib()
    prog = problems.lq_docp(4, 3, 2)
    for cls in (ipmatrix.IpLQDOCP, ipmatrix.IpSpBKP):
        M = cls()
        M.analyze(prog)
        c, y, z = np.ones(prog.n), np.ones(prog.me), np.ones(prog.m)
        assert L.hqpkkt_lagrangian_gradient_staged(M._h, vp(c), vp(y), vp(z), None, vp(np.zeros(prog.n))) == _lib.E_INTERN


def csr_gradient(prog, c, y, z, dtype):
    """c - A'y - C'z from the CSR program in dtype"""
    t = np.zeros(prog.n, dtype=dtype)
    for (p, ix, v), vec in ((prog.A, y), (prog.C, z)):
        rows = np.repeat(np.arange(len(p) - 1), np.diff(p))
        np.add.at(t, np.asarray(ix), np.asarray(v).astype(dtype) * np.asarray(vec).astype(dtype)[rows])
    return np.asarray(c).astype(dtype) - t


@pytest.mark.parametrize("kw", [dict(), dict(x0_fixed=False), dict(final_eq=2, x_bounds=2), dict(path_eq=1, path_eq_every=2, final_eq=1)])
def test_model_equals_the_csr_gradient(kw):
    K, nx, nu = 5, 4, 3
    prog = problems.lq_docp(K, nx, nu, **kw)
    dq = problems.dense_docp_from_program(prog, [nx] * (K + 1), [nu] * K)
    rng = np.random.default_rng(3)
    n, me, m = prog.dims
    c, y, z = rng.normal(size=n), rng.normal(size=me), rng.normal(size=m)
    ld = np.longdouble
    g, L, mag = hu.grad_l_dense_model(dq, c, y, z)
    want = csr_gradient(prog, c, y, z, ld)
    eps = np.finfo(ld).eps
    assert g.dtype == ld and (np.abs(g - want) <= (L + 3) * eps * (mag + np.abs(c))).all()
    # the counts: the stored entries of column i of A and C (lq_docp's blocks are full, its -1.0 are stored)
    cnt = np.zeros(n, dtype=np.int64)
    for M_ in (prog.A, prog.C):
        np.add.at(cnt, np.asarray(M_[1]), 1)
    assert (L == cnt).all()
    # integer data: exact
    ci, yi, zi = (rng.integers(-8, 9, k) for k in (n, me, m))
    av = np.asarray(prog.A[2])
    ip = problems.Program(n, me, m, prog.Q, (prog.A[0], prog.A[1], np.where(av == -1.0, -1.0, np.round(av * 8))),  # (the staircase stays)
                          (prog.C[0], prog.C[1], np.round(np.asarray(prog.C[2]) * 8)))
    di = problems.dense_docp_from_program(ip, [nx] * (K + 1), [nu] * K)
    gi, _L, _mag = hu.grad_l_dense_model(di, ci, yi, zi, dtype=np.int64)
    assert gi.dtype == np.int64 and (gi == csr_gradient(ip, ci, yi, zi, np.int64)).all()


def test_model_checks_its_sizes():
    prog = problems.lq_docp(2, 2, 1)
    dq = problems.dense_docp_from_program(prog, [2] * 3, [1] * 2)
    with pytest.raises(ValueError):
        hu.grad_l_dense_model(dq, np.ones(prog.n), np.ones(prog.me + 1), np.ones(prog.m))
