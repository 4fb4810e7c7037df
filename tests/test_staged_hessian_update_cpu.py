"""CPU tests of the in-place update of the dense stage Hessians (hqpkkt_update_stage_hessians, hqpkkt_hessian_product): the
exported symbols, every return code that is reachable without a device - the arguments are checked before the device is
asked for -, and hessian_update.bfgs_terms against a restatement of the block formula evaluated in longdouble."""
import ctypes as C
import os

import numpy as np
import pytest

import hessian_update_cases as H
from dense_hessian_cases import CASES
from hqp_amd import _lib, ipmatrix, problems
from hqp_amd.hessian_update import bfgs_terms

NZ = (5, 4, 6)
N = sum(NZ)


def _update(r=1, U="vectors", coef=None, beta=None, diag=None):
    """(hqpkkt_hess_update, what keeps its arrays alive) over N variables and three stages."""
    keep = [np.arange(1.0, N + 1.0) for _ in range(max(r, 0))]
    up = (C.c_void_p * 4)(*[v.ctypes.data for v in keep[:4]])
    u = _lib.HessUpdate()
    u.r = r
    u.U = C.cast(up, C.POINTER(C.c_void_p)) if U == "vectors" else None
    coef = np.ones((3, max(r, 1))) if coef is None else np.asarray(coef, dtype=np.float64)
    u.coef = coef.ctypes.data
    keep += [up, coef]
    for name, a in (("beta", beta), ("diag", diag)):
        if a is not None:
            a = np.asarray(a, dtype=np.float64)
            setattr(u, name, a.ctypes.data)
            keep.append(a)
    return u, keep


def _call(M, u):
    return _lib.lib().hqpkkt_update_stage_hessians(M._h if M is not None else None, C.byref(u) if u is not None else None)


def _dense_handle():
    M = H.handle(False)
    assert H.analyze_only(M, NZ) == 0
    return M


def test_symbols_and_constant():
    L = _lib.lib()
    assert L.hqpkkt_update_stage_hessians is not None and L.hqpkkt_hessian_product is not None
    assert {"hqpkkt_update_stage_hessians", "hqpkkt_hessian_product"} <= set(_lib.SYMBOLS)
    assert _lib.HQPKKT_HESS_UPDATE_RANK == 4
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "hqpkkt.h")).read()
    assert "#define HQPKKT_HESS_UPDATE_RANK 4" in hdr


def test_argument_checks_come_before_the_device():
    M = _dense_handle()
    u, keep = _update()
    assert _call(None, u) == _lib.E_NULL
    assert _call(M, None) == _lib.E_NULL
    for r in (5, -1):
        u, keep = _update(r=r)
        assert _call(M, u) == _lib.E_RANGE, r
    u, keep = _update(r=1, U=None)
    assert _call(M, u) == _lib.E_NULL
    u, keep = _update(r=2)
    u.coef = None
    assert _call(M, u) == _lib.E_NULL
    u, keep = _update(r=2)
    C.cast(u.U, C.POINTER(C.c_void_p))[1] = None  # (U[1] null)
    assert _call(M, u) == _lib.E_NULL
    u, keep = _update(r=1, coef=[[1.0], [np.nan], [1.0]], beta=[0.0, 0.0, 0.0])
    assert _call(M, u) == _lib.E_RANGE
    u, keep = _update(r=1, beta=[0.0, np.inf, 0.0])
    assert _call(M, u) == _lib.E_RANGE
    u, keep = _update(r=0, beta=[0.0, -np.inf, 0.0])
    assert _call(M, u) == _lib.E_RANGE


def test_handles_that_are_refused():
    u, keep = _update(beta=[0.0, 0.0, 0.0])
    assert _call(ipmatrix.IpSpBKP(), u) == _lib.E_INTERN  # (the tree engine)
    M = H.handle(False)
    assert _call(M, u) == _lib.E_INTERN  # (not analysed)
    prog = CASES["nx70"]()

    def analyzed(M):
        arrs = []
        for (p, i, _x) in (prog.Q, prog.A, prog.C):
            arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
        sbw = C.c_int()
        assert M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *[C.c_void_p(a.ctypes.data) if a.size else None for a in arrs], C.byref(sbw)) == 0
        return M, arrs

    K1 = len(prog.nx)
    vecs = [np.ones(prog.n)]
    up = (C.c_void_p * 1)(vecs[0].ctypes.data)
    coef, beta = np.ones((K1, 1)), np.zeros(K1)
    u = _lib.HessUpdate()
    u.r, u.U, u.coef, u.beta = 1, C.cast(up, C.POINTER(C.c_void_p)), coef.ctypes.data, beta.ctypes.data
    M, arrs = analyzed(ipmatrix.IpLQDOCP())  # STAGED with HQPKKT_HESS_CSR
    assert _call(M, u) == _lib.E_INTERN
    M, arrs = analyzed(ipmatrix.IpLQDOCP(q_dense=True))  # dense Hessians by the CSR hand-over
    assert len(M.hessian_layout()) == K1
    assert _call(M, u) == _lib.E_INTERN
    y = np.zeros(prog.n)
    assert M._L.hqpkkt_hessian_product(M._h, C.c_void_p(vecs[0].ctypes.data), C.c_void_p(y.ctypes.data)) == _lib.E_INTERN  # (not uploaded)
    assert M._L.hqpkkt_hessian_product(None, C.c_void_p(vecs[0].ctypes.data), C.c_void_p(y.ctypes.data)) == _lib.E_NULL


def test_a_valid_call_asks_for_the_device_last():
    """Every block made on the device (beta = 0, a diagonal): nothing is wrong with the call, so without a gfx950 device it
    ends in HQPKKT_E_DEVICE; with beta = 1 the hand-over rule answers first."""
    M = _dense_handle()
    u, keep = _update(r=2, beta=[0.0, 0.0, 0.0], diag=np.ones(N))
    assert _call(M, u) == _lib.E_DEVICE
    u, keep = _update(r=2, beta=[0.0, 1.0, 0.0], diag=np.ones(N))
    assert _call(M, u) == _lib.E_INTERN  # (block 1 has not arrived since the analysis)
    with pytest.raises(ipmatrix.KktError) as e:
        M.update_stage_hessians([np.ones(N)], np.ones((3, 1)), beta=np.zeros(3))
    assert e.value.code == _lib.E_DEVICE


def _restatement(Q, s, y, gamma, alpha):
    """Q+ of one block in longdouble from the formula, (Q+, per-entry scale); sv and sQs in longdouble too."""
    L = np.longdouble
    Q, s, y = Q.astype(L), s.astype(L), y.astype(L)
    Qs = Q @ s
    sv, sQs = s @ y, s @ Qs
    g = L(gamma) if gamma >= 0 else -L(gamma) + (1 + L(gamma)) * (1 - L(alpha))
    damped = bool(sv < g * sQs)
    v = y
    if damped:
        theta = (1 - g) * sQs / (sQs - sv)
        v = theta * y + (1 - theta) * Qs
        sv = s @ v
    if sv == 0 or sQs == 0:
        return Q, np.abs(Q), damped
    t1, t2 = np.outer(Qs, Qs) / sQs, np.outer(v, v) / sv
    return Q - t1 + t2, np.abs(Q) + np.abs(t1) + np.abs(t2), damped


@pytest.mark.parametrize("gamma,alpha", [(0.1, 1.0), (-0.2, 0.6)])
def test_bfgs_terms_against_the_block_formula(gamma, alpha):
    """Three blocks of orders 5, 17 and 40: the first plain, the second takes the damped branch (s'y small against s'Qs),
    the third has s'y = 0 exactly (a zero step) and stays as it is, coefficients exactly 0.  Q + sum c u u' formed in numpy from the
    returned terms against the formula in longdouble, entry by entry within 16 * 2^-53 of the sum of the three terms'
    magnitudes: the same algebra in another order of at most a dozen roundings."""
    rng = np.random.default_rng(7)
    nz = [5, 17, 40]
    off = H.offsets(nz)
    Q = []
    for v in nz:
        A = rng.standard_normal((v, v))
        Q.append(A @ A.T + v * np.eye(v))
    s = rng.standard_normal(int(off[-1]))
    y = np.concatenate([Q[0] @ s[:5] + 0.3 * rng.standard_normal(5),  # s'y about s'Qs: no damping
                        1e-3 * s[5:22],                              # s'y far below gamma s'Qs: damped
                        rng.standard_normal(40)])
    s[22:] = 0.0  # the third block did not move: s'y = 0 and s'Qs = 0 (with s'Qs > 0 the damped branch would replace y)
    Qs = np.concatenate([Q[k] @ s[off[k]: off[k + 1]] for k in range(3)])
    U, coef = bfgs_terms(s, y, Qs, off, gamma=gamma, alpha=alpha)
    assert len(U) == 2 and coef.shape == (3, 2) and U[1] is not None and np.array_equal(U[1], Qs)
    branches = []
    for k in range(3):
        b = slice(int(off[k]), int(off[k + 1]))
        want, scale, damped = _restatement(Q[k], s[b], y[b], gamma, alpha)
        branches.append(damped)
        got = Q[k] + coef[k, 0] * np.outer(U[0][b], U[0][b]) + coef[k, 1] * np.outer(U[1][b], U[1][b])
        err = np.abs(got.astype(np.longdouble) - want)
        bound = 16 * 2.0 ** -53 * scale
        print(f"block {k} (order {nz[k]}, damped {damped}): largest error {float((err / bound).max()):.3f} of the bound")
        assert (err <= bound).all(), (k, float((err / bound).max()))
        assert coef[k, 0] > 0 > coef[k, 1] if k < 2 else True
    assert branches[:2] == [False, True]
    assert (coef[2] == 0.0).all() and np.array_equal(U[0][22:], y[22:])
    got = Q[2] + coef[2, 0] * np.outer(U[0][22:], U[0][22:]) + coef[2, 1] * np.outer(U[1][22:], U[1][22:])
    assert np.array_equal(got, Q[2])  # (the block is unchanged)
