"""CPU tests of the dense stage Hessians of the STAGED engine (hqpkkt_set_hessian_form): the setters' return codes and
call order, the layout of the blocks Q_k, hqpkkt_stats.bytes_panels and the H terms left in the lists
(hqpkkt_debug_get 45) against numpy on both hand-overs, the refusal on a sharded handle, form 0 against a handle that
never asked, and the analysis of the headline's sizes without a pattern of Q.  The analysis is host-only: no GPU needed."""
import ctypes as C
import time

import numpy as np
import pytest

from dense_hessian_cases import CASES, DENSE_HANDOVER, OPTIONS, arena_bytes, orders, terms_left, up8
from hqp_amd import _lib, ipmatrix, problems

PLAN_ITEMS = (20, 21, 22, 23, 24, 25, 26, 36, 37, 39, 41, 42, 43)


def _ptrs(triples):
    arrs = []
    for (p, i, _x) in triples:
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    return arrs, [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]


def _analyze(M, prog):
    keep, ptrs = _ptrs((prog.Q, prog.A, prog.C))
    sbw = C.c_int()
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *ptrs, C.byref(sbw))


def _analyze_staged(M, dq, with_q=True):
    nx, nu = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32)
    keep, ptrs = _ptrs((dq.Q, dq.E, dq.C))
    if not with_q:
        ptrs[0] = ptrs[1] = None
    return M._L.hqpkkt_analyze_staged(M._h, dq.K, C.c_void_p(nx.ctypes.data), C.c_void_p(nu.ctypes.data), dq.n, dq.me_rest, dq.m, *ptrs)


def test_setter_return_codes_and_call_order():
    L = _lib.lib()
    assert L.hqpkkt_set_hessian_form(None, 1) == _lib.E_NULL
    T = ipmatrix.IpSpBKP()  # (not in STAGED mode)
    assert L.hqpkkt_set_hessian_form(T._h, 1) == _lib.E_INTERN
    M = ipmatrix.IpLQDOCP()
    for bad in (-1, 2, 3):
        assert L.hqpkkt_set_hessian_form(M._h, bad) == _lib.E_RANGE
    assert L.hqpkkt_set_hessian_form(M._h, _lib.HESS_DENSE) == 0 and L.hqpkkt_set_hessian_form(M._h, _lib.HESS_CSR) == 0
    # before the analysis; it holds over analyses until it is set again
    prog = CASES["nx70"]()
    M = ipmatrix.IpLQDOCP()
    M.set_hessian_form("dense")
    assert _analyze(M, prog) == 0
    lay = M.hessian_layout()
    assert lay[:, 0].tolist() == [73, 73, 73, 70] and lay[:, 1].tolist() == [80, 80, 80, 72]
    assert _analyze(M, prog) == 0 and np.array_equal(M.hessian_layout(), lay)
    M.set_hessian_form("csr")
    assert np.array_equal(M.hessian_layout(), lay)  # (the plan of the last analysis)
    assert _analyze(M, prog) == 0
    assert len(M.hessian_layout()) == 0 and M.debug(45).size == 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_bytes_and_terms_against_numpy(case):
    """Order and leading dimension of every block, the arena in bytes_panels and the terms of C'(Z/W)C that stay in the
    lists; the dense hand-over of the dynamics - with and without a pattern of Q - gives the identical layout."""
    prog = CASES[case]()
    opts = OPTIONS[case]
    csr, dense = ipmatrix.IpLQDOCP(**opts), ipmatrix.IpLQDOCP(q_dense=True, **opts)
    assert _analyze(csr, prog) == 0 and _analyze(dense, prog) == 0
    nz = orders(prog)
    left = terms_left(prog, opts.get("dense_rows", 0))
    lay = dense.hessian_layout()
    assert lay[:, 0].tolist() == nz and lay[:, 1].tolist() == [up8(v) for v in nz] and np.array_equal(lay[:, 2], left)
    assert csr.debug(45).size == 0
    assert dense.stats()["bytes_panels"] == csr.stats()["bytes_panels"] + arena_bytes(prog)
    assert dense.stats()["bytes_updates"] == csr.stats()["bytes_updates"] and dense.stats()["flops_factor"] == csr.stats()["flops_factor"]
    for item in PLAN_ITEMS[:-1]:  # (the dynamics' side of the plan does not depend on the form of the Hessians)
        assert np.array_equal(dense.debug(item), csr.debug(item)), item
    if opts.get("dense_rows"):  # the wide rows are the same rows; the terms kept are those of C alone
        kept_c, cut_c = csr.h_terms()
        kept_d, cut_d = dense.h_terms()
        assert dense.dense_rows() == csr.dense_rows() and np.array_equal(cut_c, cut_d) and np.array_equal(kept_d, left)
        assert (kept_c > kept_d).all()
    if case in DENSE_HANDOVER:
        dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=True)
        d0 = ipmatrix.IpLQDOCP(**opts)
        assert _analyze_staged(d0, dq) == 0
        for with_q in (True, False):
            D = ipmatrix.IpLQDOCP(q_dense=True, **opts)
            assert _analyze_staged(D, dq, with_q) == 0
            assert np.array_equal(D.hessian_layout(), lay)
            assert D.stats()["bytes_panels"] == d0.stats()["bytes_panels"] + arena_bytes(prog)
            assert D.stats()["nnz_kkt"] == d0.stats()["nnz_kkt"] - len(prog.Q[1])  # (Qp / Qi are not read)


def test_a_sharded_handle_is_refused_at_the_analysis():
    prog = CASES["with_carried_rows"]()
    M = ipmatrix.IpLQDOCP(q_dense=True)
    M.set_shard(0, 2, lambda *a: 0)
    assert _analyze(M, prog) == _lib.E_RANGE
    dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=True)
    assert _analyze_staged(M, dq, False) == _lib.E_RANGE
    M.set_hessian_form("csr")
    assert _analyze(M, prog) == 0


@pytest.mark.parametrize("case", ["nx150", "with_carried_rows", "wide_rows", "banded_sparse_form", "banded_profile_form", "banded_packed_panels"])
def test_form_0_is_a_handle_that_never_asked(case):
    prog = CASES[case]()
    never = ipmatrix.IpLQDOCP(**OPTIONS[case])
    zero = ipmatrix.IpLQDOCP(**OPTIONS[case])
    assert zero._L.hqpkkt_set_hessian_form(zero._h, _lib.HESS_CSR) == 0
    back = ipmatrix.IpLQDOCP(q_dense=True, **OPTIONS[case])  # (set and taken back before the analysis)
    back.set_hessian_form("csr")
    assert _analyze(never, prog) == 0 and _analyze(zero, prog) == 0 and _analyze(back, prog) == 0
    for M in (zero, back):
        for item in PLAN_ITEMS:
            assert np.array_equal(M.debug(item), never.debug(item)), item
        assert M.debug(45).size == 0 and never.debug(45).size == 0
        a, b = M.stats(), never.stats()
        assert all(a[key] == b[key] for key in ("bytes_panels", "bytes_updates", "flops_factor", "nnz_factor", "nnz_kkt"))


def test_hand_over_rules_without_a_device():
    """hqpkkt_set_stage_hessian is the dense hand-over's: HQPKKT_E_INTERN on a handle analysed by hqpkkt_analyze, with either
    form, and on a dense hand-over in form 0.  hqpkkt_set_values_staged refuses to end a hand-over to which no Hessian
    block has come - before anything is uploaded."""
    prog = CASES["nx70"]()
    L = _lib.lib()
    blk = np.eye(73)
    for kw in (dict(q_dense=True), dict()):
        M = ipmatrix.IpLQDOCP(**kw)
        assert _analyze(M, prog) == 0
        assert L.hqpkkt_set_stage_hessian(M._h, 0, C.c_void_p(blk.ctypes.data), 73) == _lib.E_INTERN
    assert L.hqpkkt_set_stage_hessian(None, 0, C.c_void_p(blk.ctypes.data), 73) == _lib.E_NULL
    dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=True)
    M = ipmatrix.IpLQDOCP()
    assert _analyze_staged(M, dq) == 0
    assert L.hqpkkt_set_stage_hessian(M._h, 0, C.c_void_p(blk.ctypes.data), 73) == _lib.E_INTERN
    M = ipmatrix.IpLQDOCP(q_dense=True)
    assert L.hqpkkt_set_stage_hessian(M._h, 0, C.c_void_p(blk.ctypes.data), 73) == _lib.E_INTERN  # (not analysed)
    assert _analyze_staged(M, dq, False) == 0
    assert L.hqpkkt_set_stage_hessian(M._h, 0, None, 73) == _lib.E_NULL
    F = [np.ascontiguousarray(b) for b in dq.F]
    fp = (C.c_void_p * dq.K)(*[b.ctypes.data for b in F])
    ld = (C.c_longlong * dq.K)(*[b.shape[1] for b in F])
    ex, cx = (np.ascontiguousarray(t[2], dtype=np.float64) for t in (dq.E, dq.C))
    vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None
    assert L.hqpkkt_set_values_staged(M._h, None, fp, ld, vp(ex), vp(cx)) == _lib.E_INTERN
    assert L.hqpkkt_set_values_staged(M._h, None, None, None, vp(ex), vp(cx)) == _lib.E_INTERN


def test_the_headline_sizes_without_a_pattern_of_q():
    """K = 200 stages of 5000 states and 50 controls, box bounds on the controls: 2.55e9 upper entries of Q, which no
    int32 CSR holds - hqpkkt_analyze_staged with Qp = NULL returns 0 without a device, and bytes_panels is the
    arithmetic: F, V and 200 blocks of 5050 x 5056 and one of 5000 x 5000 doubles."""
    K, nx, nu = 200, 5000, 50
    n = K * (nx + nu) + nx
    ucols = (np.arange(K)[:, None] * (nx + nu) + nx + np.arange(nu)[None, :]).ravel()
    Cp = np.arange(2 * ucols.size + 1, dtype=np.int32)
    Ci = np.concatenate([ucols, ucols]).astype(np.int32)
    Ep = np.arange(nx + 1, dtype=np.int32)  # (the rows that fix x_0)
    Ei = np.arange(nx, dtype=np.int32)
    nxs, nus = np.full(K + 1, nx, dtype=np.int32), np.full(K, nu, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)

    def analyze(M, Qp, Qi):
        return M._L.hqpkkt_analyze_staged(M._h, K, vp(nxs), vp(nus), n, nx, Cp.size - 1, Qp, Qi, vp(Ep), vp(Ei), vp(Cp), vp(Ci))

    t0 = time.perf_counter()
    M = ipmatrix.IpLQDOCP(q_dense=True)
    assert analyze(M, None, None) == 0
    took = time.perf_counter() - t0
    print(f"analysis of K = {K}, {nx} states, {nu} controls with dense Hessians: {took:.2f} s")  # (0.04 s when the test was written)
    D = ipmatrix.IpLQDOCP()  # (form 0 with a diagonal Q: the arenas of F and V)
    qp, qi = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    assert analyze(D, vp(qp), vp(qi)) == 0
    arena = 8 * (K * (nx + nu) * up8(nx + nu) + nx * up8(nx))
    assert arena == 40_852_480_000 + 200_000_000  # (200 blocks of 5050 x 5056 doubles, one of 5000 x 5000)
    assert M.stats()["bytes_panels"] == D.stats()["bytes_panels"] + arena
    lay = M.hessian_layout()
    assert lay.shape == (K + 1, 3) and lay[0].tolist() == [nx + nu, up8(nx + nu), 2 * nu] and lay[K].tolist() == [nx, nx, 0]
    assert M._L.hqpkkt_analyze_staged(ipmatrix.IpLQDOCP()._h, K, vp(nxs), vp(nus), n, nx, Cp.size - 1, None, None, vp(Ep), vp(Ei), vp(Cp), vp(Ci)) == _lib.E_NULL
