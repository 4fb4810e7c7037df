"""CPU tests of hqpkkt_q_eigen_control and hqpkkt_q_eigen_report: the exported symbols, the struct and the constant, the return
codes a host-only run reaches in the header's order, the report's cap protocol before a control, and the numpy models -
q_block_dense and q_lanczos_model against lanczos_model on the dense block, the condition on the cases of q_eigen_cases.py
(every block meant to end "shifted, converged" does so in the model within 64 steps) and the measured allowance.

A handle gets its values through the device alone, so on a host without one "no values yet" (HQPKKT_E_INTERN) answers
before HQPKKT_E_FORMAT can, as in test_q_values_cpu.py; tests/test_gpu_q_eigen.py reaches the rest."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hqp_amd import _lib, ipmatrix, problems  # noqa: E402
from hqp_amd import hessian_update as hu  # noqa: E402
import hessian_guard_cases as G  # noqa: E402
import q_eigen_cases as E  # noqa: E402

NAN, INF = float("nan"), float("inf")


def vp(a):
    return C.c_void_p(a.ctypes.data)


def _ctl(eps=E.EPS, bsize=-1, from_bfgs=0, floor=None, max_steps=0):
    e = _lib.QEigenControl()
    e.eps, e.bsize, e.floor_from_bfgs, e.max_steps = eps, bsize, from_bfgs, max_steps
    e.floor = None if floor is None else floor.ctypes.data
    return e


def _report(L, M, cap=1):
    k, ts = C.c_longlong(-1), C.c_int(-1)
    out = np.zeros((max(cap, 1), 10))
    return L.hqpkkt_q_eigen_report(M._h, vp(out), None, cap, C.byref(k), C.byref(ts)), k.value, ts.value


def test_symbols_constants_and_struct():
    L = _lib.lib()
    names = ("hqpkkt_q_eigen_control", "hqpkkt_q_eigen_report")
    assert set(names) <= set(_lib.SYMBOLS)
    for nm in names:
        assert getattr(L, nm) is not None
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "hqpkkt.h")).read()
    assert "#define HQPKKT_EIG_REPORT 10" in hdr and _lib.HQPKKT_EIG_REPORT == 10
    assert "#define HQPKKT_EIG_MAX_STEPS 128" in hdr and _lib.HQPKKT_EIG_MAX_STEPS == 128
    assert "hqpkkt_q_eigen_control_args" in hdr
    # a double, two ints, a pointer, an int and its padding on an LP64 host
    S = _lib.QEigenControl
    assert C.sizeof(S) == 32
    assert (S.eps.offset, S.bsize.offset, S.floor_from_bfgs.offset, S.floor.offset, S.max_steps.offset) == (0, 8, 12, 16, 24)
    for nm in ("q_eigen_control", "q_eigen_report"):
        assert callable(getattr(ipmatrix.Hqp_IpMatrix, nm))
    import inspect
    assert "eigen_control" in inspect.signature(ipmatrix.Hqp_IpMatrix.q_bfgs_update).parameters


@pytest.mark.parametrize("cls", [ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP, ipmatrix.IpLQDOCP])
def test_null_then_range_then_intern(cls):
    L = _lib.lib()
    M = cls()
    out = np.zeros(10)
    k, ts = C.c_longlong(), C.c_int()
    # E_NULL first, also with a RANGE error behind it
    assert L.hqpkkt_q_eigen_control(None, C.byref(_ctl(eps=NAN))) == L.hqpkkt_q_eigen_control(M._h, None) == _lib.E_NULL
    assert L.hqpkkt_q_eigen_report(None, vp(out), None, 1, C.byref(k), C.byref(ts)) == _lib.E_NULL
    assert L.hqpkkt_q_eigen_report(M._h, None, None, 1, C.byref(k), C.byref(ts)) == _lib.E_NULL
    assert L.hqpkkt_q_eigen_report(M._h, vp(out), None, 1, None, C.byref(ts)) == _lib.E_NULL
    assert L.hqpkkt_q_eigen_report(M._h, vp(out), None, 1, C.byref(k), None) == _lib.E_NULL

    def ranges():
        for eps in (NAN, INF, -INF, 0.0, -1.0):
            assert L.hqpkkt_q_eigen_control(M._h, C.byref(_ctl(eps=eps))) == _lib.E_RANGE, eps
        for ms in (-1, 129, 1 << 20):
            assert L.hqpkkt_q_eigen_control(M._h, C.byref(_ctl(max_steps=ms))) == _lib.E_RANGE, ms
        for fb in (-1, 2, 7):
            assert L.hqpkkt_q_eigen_control(M._h, C.byref(_ctl(from_bfgs=fb))) == _lib.E_RANGE, fb

    # E_RANGE next, before the call order is looked at
    ranges()
    # E_INTERN: before the analysis - every valid combination, the caps included
    for c in (_ctl(), _ctl(max_steps=128), _ctl(max_steps=1, bsize=0), _ctl(from_bfgs=1), _ctl(bsize=7, floor=np.full(3, NAN))):
        assert L.hqpkkt_q_eigen_control(M._h, C.byref(c)) == _lib.E_INTERN
    assert _report(L, M)[0] == _lib.E_INTERN
    # ... and before values: the floors are not looked at yet (their count is known behind the call order alone)
    prog = problems.lq_docp(4, 3, 2) if cls is ipmatrix.IpLQDOCP else E.band_program(40)
    M.analyze(prog)
    for c in (_ctl(), _ctl(from_bfgs=1), _ctl(bsize=7, floor=np.full(prog.n, NAN))):
        assert L.hqpkkt_q_eigen_control(M._h, C.byref(c)) == _lib.E_INTERN
    assert _report(L, M, prog.n)[0] == _lib.E_INTERN
    ranges()


def _give_values(M, prog):
    """init(): True where the values arrived, False where the host has no device for them."""
    M.analyze(prog)
    try:
        M.update(prog)
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_DEVICE
        return False
    return True


def _without_diagonal(prog, row):
    p, ix, x = (np.array(a) for a in prog.Q)
    k = int(p[row] + np.flatnonzero(ix[p[row]: p[row + 1]] == row)[0])
    p[row + 1:] -= 1
    return problems.Program(prog.n, prog.me, prog.m, (p, np.delete(ix, k), np.delete(x, k)), prog.A, prog.C, prog.c, prog.b, prog.d)


@pytest.mark.parametrize("cls", [ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP])
def test_intern_floor_range_then_format(cls):
    """Where the values can arrive: HQPKKT_E_INTERN for from_bfgs without an update, HQPKKT_E_RANGE for a floor that is not
    finite - ahead of HQPKKT_E_FORMAT for the row without a diagonal - and the report's cap protocol before a control
    (HQPKKT_E_INTERN).  On a host without a device everything stops at "no values yet"."""
    L = _lib.lib()
    prog = _without_diagonal(E.band_program(40), 7)
    M = cls()
    have = _give_values(M, prog)
    nb = 6  # blocks of 7 in 40
    bad = np.ones(nb)
    bad[4] = INF
    codes = [L.hqpkkt_q_eigen_control(M._h, C.byref(c)) for c in (_ctl(bsize=7, from_bfgs=1), _ctl(bsize=7, floor=bad), _ctl(bsize=7, floor=np.ones(nb)), _ctl(bsize=7))]
    assert codes == ([_lib.E_INTERN, _lib.E_RANGE, _lib.E_FORMAT, _lib.E_FORMAT] if have else [_lib.E_INTERN] * 4)
    assert _report(L, M, 0)[0] == _lib.E_INTERN and _report(L, M, nb)[0] == _lib.E_INTERN


def test_refused_on_dense_stage_hessians():
    """A STAGED handle with HQPKKT_HESS_DENSE keeps its Hessians as blocks: every hqpkkt_q_* entry is HQPKKT_E_INTERN there,
    with or without values."""
    L = _lib.lib()
    prog = problems.with_dense_hessian(problems.lq_docp(4, 3, 2))
    D = ipmatrix.IpLQDOCP(q_dense=True)
    D.analyze(prog)
    try:
        D.update(prog)
    except ipmatrix.KktError as e:
        assert e.code == _lib.E_DEVICE
    assert L.hqpkkt_q_eigen_control(D._h, C.byref(_ctl())) == _lib.E_INTERN
    assert _report(L, D, 8)[0] == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as ex:
        D.q_eigen_control(E.EPS)
    assert ex.value.code == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as ex:
        D.q_eigen_report()
    assert ex.value.code == _lib.E_INTERN


# ---- the models

def _upper_csr(B, keep=None):
    i, j = np.triu_indices(B.shape[0])
    if keep is not None:
        k = keep(i, j)
        i, j = i[k], j[k]
    return problems._csr(i, j, B[i, j], B.shape[0])


def _patterns():
    """(name, CSR triple, partition): a full block; a band of 6 in one block; a band of 6 cut by blocks of 5 (entries across
    blocks, which no block sees)"""
    rng = np.random.default_rng(5)
    full = G.indefinite_block(rng, 37)
    band = np.triu(rng.uniform(-1, 1, (41, 41)))
    band = band + np.triu(band, 1).T - 2.0 * np.eye(41)
    bq = _upper_csr(band, lambda i, j: j - i <= 6)
    return [("full", _upper_csr(full), np.array([0, 37])), ("band", bq, np.array([0, 41])),
            ("cut", bq, np.array(list(range(0, 41, 5)) + [41]))]


@pytest.mark.parametrize("which", range(3))
def test_models_against_the_dense_model(which):
    """q_block_dense is the symmetric image of the stored upper entries inside the block - nothing of another block -, and
    q_lanczos_model is lanczos_model on it: the same g and steps, T within t_bound (two orders of summation)."""
    name, Q, first = _patterns()[which]
    p, ix, x = (np.asarray(a) for a in Q)
    n = p.size - 1
    rows = np.repeat(np.arange(n), np.diff(p))
    D = np.zeros((n, n))
    D[rows, ix] = x
    D = D + np.triu(D, 1).T
    theta = E.EPS ** 2
    g, steps, T = hu.q_lanczos_model(Q, first, theta)
    cap = int(min(64, np.diff(first).max()))
    assert T.shape == (first.size - 1, 2, cap)
    compared = 0
    for b in range(first.size - 1):
        a, e = int(first[b]), int(first[b + 1])
        B = hu.q_block_dense(Q, first, b)
        assert (B == D[a:e, a:e]).all() and (B == B.T).all(), (name, b)
        g0, s0, T0 = hu.lanczos_model(B, theta)
        assert s0 == steps[b] and abs(g0 - g[b]) <= 4 * (e - a) * E.U * G.norm_inf(B), (name, b)
        assert (T[b][:, steps[b]:] == 0.0).all()
        k, worst = E.t_compare(e - a, G.norm_inf(B), T[b], T0, int(steps[b]))
        assert k >= 1 and worst <= 1.0, (name, b, k, worst)
        compared += k
    assert compared >= 3 * (first.size - 1) or name == "cut", (name, compared)
    if name == "cut":  # the entries across blocks change nothing
        x2 = np.array(x)
        of = np.repeat(np.arange(first.size - 1), np.diff(first))
        x2[of[rows] != of[ix]] = np.nan
        g2, s2, T2 = hu.q_lanczos_model((p, ix, x2), first, theta)
        assert g2.tobytes() == g.tobytes() and (s2 == steps).all() and T2.tobytes() == T.tobytes()


def test_fine_partitions_hold_every_entry_of_a_block():
    for c in E.cases():
        prog, first, fine = c["prog"], c["first"], c["fine"]
        assert (hu.q_blocks_model(prog.Q[0], prog.Q[1], prog.n, c["bsize"])[0] == first).all(), c["name"]
        assert set(first.tolist()) <= set(fine.tolist()) and len(c["want"]) == first.size - 1
        rows = np.repeat(np.arange(prog.n), np.diff(prog.Q[0]))
        ix = np.asarray(prog.Q[1])
        of = np.repeat(np.arange(first.size - 1), np.diff(first))
        ff = np.repeat(np.arange(fine.size - 1), np.diff(fine))
        inb = of[rows] == of[ix]
        assert (ff[rows[inb]] == ff[ix[inb]]).all(), c["name"]
        assert np.diff(fine).max() <= 300
    lens = set()
    for c in E.cases():
        lens |= set(np.diff(c["first"]).tolist())
    assert lens >= {1, 2, 3, 63, 64, 65, 257, 4095, 4096, 4097, 8193}
    assert max(E.WAVE_ORDERS) <= 64 < max(E.MIXED_ORDERS)


def test_model_converges_and_measures_the_allowance():
    """Every block of every GPU case: where the case means "shifted, converged" the model reaches outcome 2 within the
    default cap of 64 steps; the outcome is one the case allows; lambda_est agrees with eigvalsh within rho and the
    allowance; a shifted block is not below its floor.  Prints the measured allowance."""
    theta = E.EPS ** 2
    worst, outcomes = 0.0, set()
    for c in E.cases():
        res = E.model(c["prog"].Q, c)
        for b, r in enumerate(res):
            lam, N, ln = E.block_facts(c["prog"].Q, c, b)
            unit = E.U * ln * N
            outcomes.add(r["outcome"])
            assert r["outcome"] in c["want"][b], (c["name"], b, r["outcome"], c["want"][b])
            if c["want"][b] == (2,):
                assert r["outcome"] == 2 and 1 <= r["steps"] <= min(64, ln) and r["rho"] <= 2.0 ** -40 * r["normT"], (c["name"], b)
            if r["outcome"] == 0:
                assert r["g"] >= theta and lam >= r["g"] - 4 * unit
                continue
            assert r["hi"] - r["lo"] <= 2.0 ** -50 * r["normT"]
            if r["outcome"] in (1, 2):
                a = abs(r["lam"] - lam) / unit
                worst = max(worst, a)
            else:
                assert r["outcome"] == 3 and abs(r["lam"] - lam) <= r["rho"] + E.ALLOWANCE * unit
            assert (r["d"] > 0.0) == (r["lam"] < theta)
            if r["d"] > 0.0:
                assert E.block_facts(c["prog"].Q, c, b, shift=r["d"])[0] >= theta - 8 * E.ALLOWANCE * unit, (c["name"], b)
    print(f"measured allowance {worst:.3f} (q_eigen_cases.ALLOWANCE = {E.ALLOWANCE})")
    assert worst <= E.ALLOWANCE
    assert outcomes >= {0, 1, 2}
