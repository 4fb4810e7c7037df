"""CPU tests of the safeguards of the dense stage Hessians (hqpkkt_hessian_row_stats, hqpkkt_restart_stage_hessians,
hqpkkt_gerschgorin_stage_hessians, hqpkkt_eigen_control_stage_hessians, hqpkkt_eigen_report): the exported symbols, the
return codes a host-only run reaches - the arguments are checked before the device is asked for -, the numpy models of
restart_Q and Gerschgorin against hand-written blocks, and the model of the eigenvalue control (lanczos_model +
eigen_replay) against numpy.linalg.eigvalsh on every case of the GPU test.

HQPKKT_E_DEVICE is the one code no host-only run reaches: it stands behind the hand-over rule, and a block arrives through
the device alone.  Outcome 5 (a stage of order 0) is reached by the model alone: hqpkkt_analyze_staged refuses a stage
without a state (nx[k] >= 1), so no handle has such a stage."""
import ctypes as C
import os

import numpy as np
import pytest

import hessian_guard_cases as G
import hessian_update_cases as H
from hqp_amd import _lib, ipmatrix
from hqp_amd import hessian_update as hu

NZ = (5, 4, 6)
N = sum(NZ)


def _dense_handle():
    M = H.handle(False)
    assert H.analyze_only(M, NZ) == 0
    return M


def _ctl(eps=1e-3, from_bfgs=0, floor=None, max_steps=0):
    c = _lib.EigenControl()
    c.eps, c.floor_from_bfgs, c.max_steps = eps, from_bfgs, max_steps
    keep = None
    if floor is not None:
        keep = np.ascontiguousarray(floor, dtype=np.float64)
        c.floor = keep.ctypes.data
    return c, keep


def _eig(M, c):
    return _lib.lib().hqpkkt_eigen_control_stage_hessians(M._h if M is not None else None, C.byref(c) if c is not None else None)


def test_symbols_constants_and_struct():
    L = _lib.lib()
    names = {"hqpkkt_hessian_row_stats", "hqpkkt_restart_stage_hessians", "hqpkkt_gerschgorin_stage_hessians",
             "hqpkkt_eigen_control_stage_hessians", "hqpkkt_eigen_report"}
    assert names <= set(_lib.SYMBOLS)
    for nm in names:
        assert getattr(L, nm) is not None
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "hqpkkt.h")).read()
    assert "#define HQPKKT_EIG_MAX_STEPS 128" in hdr and _lib.HQPKKT_EIG_MAX_STEPS == 128 == hu.EIG_MAX_STEPS
    assert "#define HQPKKT_EIG_REPORT 10" in hdr and _lib.HQPKKT_EIG_REPORT == 10
    assert "#define HQPKKT_EIG_END_REL 9.094947017729282e-13" in hdr and _lib.HQPKKT_EIG_END_REL == 2.0 ** -40 == 9.094947017729282e-13
    # double, int, pointer, int on an LP64 host: 8 + 4 (+ 4) + 8 + 4 (+ 4)
    assert C.sizeof(_lib.EigenControl) == 32
    assert _lib.EigenControl.floor.offset == 16 and _lib.EigenControl.max_steps.offset == 24


def test_checks_in_their_order_before_the_device():
    """NULL, then RANGE, then INTERN; on an analysed handle whose blocks have not arrived the last is the hand-over rule."""
    L = _lib.lib()
    M = _dense_handle()
    out = np.zeros(N)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    # row statistics
    assert L.hqpkkt_hessian_row_stats(None, vp(out), vp(out)) == _lib.E_NULL
    assert L.hqpkkt_hessian_row_stats(M._h, None, None) == _lib.E_NULL
    assert L.hqpkkt_hessian_row_stats(M._h, vp(out), None) == _lib.E_INTERN  # (no block has arrived)
    # restart and Gerschgorin: eps
    assert L.hqpkkt_restart_stage_hessians(None, 1e-3, None) == _lib.E_NULL
    assert L.hqpkkt_gerschgorin_stage_hessians(None, 1e-3) == _lib.E_NULL
    for eps in (0.0, -1.0, np.nan, np.inf):
        assert L.hqpkkt_restart_stage_hessians(M._h, eps, None) == _lib.E_RANGE, eps
        assert L.hqpkkt_gerschgorin_stage_hessians(M._h, eps) == _lib.E_RANGE, eps
        assert L.hqpkkt_restart_stage_hessians(ipmatrix.IpSpBKP()._h, eps, None) == _lib.E_RANGE  # (RANGE comes before INTERN)
    assert L.hqpkkt_restart_stage_hessians(M._h, 1e-3, None) == _lib.E_INTERN
    none = np.zeros(3, dtype=np.uint8)
    one = np.array([0, 1, 0], dtype=np.uint8)
    assert L.hqpkkt_restart_stage_hessians(M._h, 1e-3, vp(one)) == _lib.E_INTERN  # (a chosen block is read)
    assert L.hqpkkt_gerschgorin_stage_hessians(M._h, 1e-3) == _lib.E_INTERN
    del none
    # the control
    c, keep = _ctl()
    assert _eig(None, c) == _lib.E_NULL and _eig(M, None) == _lib.E_NULL
    for eps in (0.0, -1.0, np.nan, np.inf):
        c, keep = _ctl(eps=eps)
        assert _eig(M, c) == _lib.E_RANGE, eps
    for ms in (-1, 129):
        c, keep = _ctl(max_steps=ms)
        assert _eig(M, c) == _lib.E_RANGE, ms
        assert _eig(ipmatrix.IpSpBKP(), c) == _lib.E_RANGE
    for bad in (np.nan, np.inf):
        c, keep = _ctl(floor=[0.0, bad, 0.0])
        assert _eig(M, c) == _lib.E_RANGE, bad
        assert _eig(ipmatrix.IpSpBKP(), c) == _lib.E_INTERN  # (the floors are K + 1 values: the handle's form comes first)
    for ms in (0, 1, 128):
        c, keep = _ctl(max_steps=ms, floor=[0.0, 1.0, -1.0])
        assert _eig(M, c) == _lib.E_INTERN, ms  # (valid arguments: the hand-over rule answers)
    c, keep = _ctl(from_bfgs=1)
    assert _eig(M, c) == _lib.E_INTERN
    # the report
    rep = np.zeros(3 * 10)
    assert L.hqpkkt_eigen_report(None, vp(rep), None) == _lib.E_NULL
    assert L.hqpkkt_eigen_report(M._h, None, None) == _lib.E_NULL
    assert L.hqpkkt_eigen_report(M._h, vp(rep), None) == _lib.E_INTERN


def test_handles_that_are_refused():
    L = _lib.lib()
    out = np.zeros(N)
    c, keep = _ctl()
    for M in (ipmatrix.IpSpBKP(), H.handle(False), ipmatrix.IpLQDOCP()):  # the tree engine; not analysed; HQPKKT_HESS_CSR, not analysed
        assert L.hqpkkt_hessian_row_stats(M._h, C.c_void_p(out.ctypes.data), None) == _lib.E_INTERN
        assert L.hqpkkt_restart_stage_hessians(M._h, 1e-3, None) == _lib.E_INTERN
        assert L.hqpkkt_gerschgorin_stage_hessians(M._h, 1e-3) == _lib.E_INTERN
        assert _eig(M, c) == _lib.E_INTERN


def test_wrappers_raise_the_codes():
    M = _dense_handle()
    for call in (lambda: M.hessian_row_stats(), lambda: M.restart_hessians(1e-3), lambda: M.gerschgorin_hessians(1e-3),
                 lambda: M.eigen_control(1e-3), lambda: M.eigen_report(), lambda: M.eigen_report(with_T=True)):
        with pytest.raises(ipmatrix.KktError) as e:
            call()
        assert e.value.code == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as e:
        M.restart_hessians(0.0, stages=[1, 0, 1])
    assert e.value.code == _lib.E_RANGE
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_control(1e-3, max_steps=200)
    assert e.value.code == _lib.E_RANGE


def test_restart_model_by_hand():
    Q = np.array([[0.0, 0.0, 0.0], [0.0, -3.0, 2.0], [0.0, 2.0, 100.0]])
    # eps = 1/8: the row of zeros is raised to eps, the row with 100 > 1 / eps = 8 is cut, the middle row keeps its |-3|
    assert H.bits(hu.restart_model(Q, 0.125), np.diag([0.125, 3.0, 8.0]))
    assert H.bits(hu.restart_model(Q, 1e-3), np.diag([1e-3, 3.0, 100.0]))
    assert hu.restart_model(np.zeros((0, 0)), 0.5).shape == (0, 0)
    assert H.bits(hu.restart_model(np.array([[-7.0]]), 0.5), np.array([[2.0]]))


def test_gerschgorin_model_by_hand():
    Q = np.array([[1.0, -2.0, 3.0], [-2.0, 10.0, 1.0], [3.0, 1.0, 4.0]])
    # off-diagonal sums 5, 3, 4; eps = 0.5: rows 0 and 2 are raised to 5.5 and 4.5, row 1 is dominant already
    want = Q.copy()
    want[0, 0], want[2, 2] = 5.5, 4.5
    assert H.bits(hu.gerschgorin_model(Q, 0.5), want)
    assert H.bits(hu.gerschgorin_model(want, 0.5), want)  # (dominant: unchanged)
    assert H.bits(hu.gerschgorin_model(np.array([[-1.0]]), 0.25), np.array([[0.25]]))


def test_sturm_count_of_the_cases_file():
    # T = [[2, 1], [1, 2]]: eigenvalues 1 and 3 (the last beta is the residual's norm and not part of T)
    for x, want in ((0.5, 0), (1.5, 1), (3.5, 2)):
        assert G.sturm_count([2.0, 2.0], [1.0, 9.0], x) == want


def test_replay_of_order_zero_and_of_a_dominant_block():
    assert hu.eigen_replay(0, 0.0, 1e-6, 0, np.zeros((2, 128)))["outcome"] == 5
    r = G.model(np.array([[4.0, 1.0], [1.0, 4.0]]), 1e-6)
    assert r["outcome"] == 0 and r["steps"] == 0 and r["g"] == 3.0 and r["d"] == 0.0
    r = G.model(np.array([[np.nan, 1.0], [1.0, 4.0]]), 1e-6)
    assert r["outcome"] == 4 and r["d"] == 0.0


def test_model_converges_and_measures_the_allowance():
    """Every block of every GPU eigen case: the model converges within the default cap of 64 steps (rho <= 2^-40 |T|),
    takes the Gerschgorin exit on the dominant blocks alone (and on orders so small that the block is dominant by itself),
    its bracket is honest, and lambda_est agrees with eigvalsh.  Prints the measured allowance."""
    theta = G.EPS ** 2
    worst, outcomes = 0.0, set()
    for nz, kinds, blocks in G.eigen_cases():
        for kind, Q in zip(kinds, blocks):
            v = Q.shape[0]
            r = G.model(Q, theta)
            lam = float(np.linalg.eigvalsh(Q)[0])
            outcomes.add(r["outcome"])
            if kind == "dominant" or (kind == "definite" and v < 4):
                assert r["outcome"] == 0 and r["g"] >= theta and lam >= r["g"], (nz, kind)
                continue
            assert r["outcome"] in ((1,) if kind == "definite" else (2,)), (nz, kind, r["outcome"])
            assert r["g"] < theta and 1 <= r["steps"] <= min(64, v)
            assert r["rho"] <= 2.0 ** -40 * r["normT"], (nz, kind, r["rho"])
            assert r["hi"] - r["lo"] <= 2.0 ** -50 * r["normT"]
            if r["steps"] <= 8:  # (the exact count is quadratic in the order of T with growing rationals: the short ones)
                al, be, gg = r["T"][0][: r["steps"]], r["T"][1][: r["steps"]], 8 * 2.0 ** -53 * r["normT"]
                assert G.sturm_count(al, be, r["lo"] - gg) == 0 and G.sturm_count(al, be, r["hi"] + gg) >= 1
            a = abs(r["lam"] - lam) / (2.0 ** -53 * v * G.norm_inf(Q))
            worst = max(worst, a)
            assert (r["d"] > 0.0) == (lam < theta), (nz, kind)
            if r["d"] > 0.0:  # the shifted block is not below the floor
                assert float(np.linalg.eigvalsh(Q + r["d"] * np.eye(v))[0]) >= theta - 8 * G.ALLOWANCE * 2.0 ** -53 * v * G.norm_inf(Q)
    print(f"measured allowance {worst:.3f} (hessian_guard_cases.ALLOWANCE = {G.ALLOWANCE})")
    assert worst <= G.ALLOWANCE
    assert outcomes == {0, 1, 2}


def test_model_of_one_step_is_not_converged_but_conservative():
    """max_steps = 1 on a block whose smallest eigenvector is nearly the start vector: T = [alpha_0], rho = beta_0, and
    alpha_0 - beta_0 lies below the smallest eigenvalue, within rho of it."""
    for v in (220, 65):
        Q = G.aligned_block(np.random.default_rng(3), v)
        r = G.model(Q, G.EPS ** 2, max_steps=1)
        lam = float(np.linalg.eigvalsh(Q)[0])
        assert r["outcome"] == 3 and r["steps"] == 1 and r["rho"] > 2.0 ** -40 * r["normT"]
        assert r["lam"] <= lam <= r["lam"] + r["rho"] + G.ALLOWANCE * 2.0 ** -53 * v * G.norm_inf(Q)
