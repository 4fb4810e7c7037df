"""CPU tests of the dense stage Hessians stored as packed lower tiles (hqpkkt_set_packed_hessians): the setter's return
codes and call order, the layout (hqpkkt_debug_get 47) against the rule in numpy after both analyses, bytes_panels, the
hand-over count and the scratch of the product at the headline's sizes, and the refusal on a sharded handle.  The analysis
is host-only: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

import packed_hessian_cases as P
from dense_hessian_cases import CASES, OPTIONS, arena_bytes, orders, up8
from hqp_amd import _lib, ipmatrix, problems

PLAN_ITEMS = (20, 21, 22, 23, 24, 25, 26, 36, 37, 39, 41, 42, 43, 45, 46)
STATS = ("bytes_panels", "bytes_updates", "flops_factor", "nnz_factor", "nnz_kkt")
vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None


def _analyze(M, prog):
    arrs = []
    for (p, i, _x) in (prog.Q, prog.A, prog.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    sbw = C.c_int()
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *[vp(a) for a in arrs], C.byref(sbw))


def _analyze_sizes(M, nx, nu):
    """hqpkkt_analyze_staged without a pattern of Q: the rows that fix x_0, bounds on the controls."""
    nx, nu = np.asarray(nx, dtype=np.int32), np.asarray(nu, dtype=np.int32)
    K = len(nu)
    off = np.concatenate([[0], np.cumsum(nx[:K] + nu)])
    n = int(off[K] + nx[K])
    ucols = np.concatenate([off[k] + nx[k] + np.arange(nu[k]) for k in range(K)])
    Cp = np.arange(2 * ucols.size + 1, dtype=np.int32)
    Ci = np.concatenate([ucols, ucols]).astype(np.int32)
    Ep, Ei = np.arange(nx[0] + 1, dtype=np.int32), np.arange(nx[0], dtype=np.int32)
    return M._L.hqpkkt_analyze_staged(M._h, K, vp(nx), vp(nu), n, int(nx[0]), Cp.size - 1, None, None, vp(Ep), vp(Ei), vp(Cp), vp(Ci))


def _same_plan(A, B):
    for item in PLAN_ITEMS:
        assert np.array_equal(A.debug(item), B.debug(item)), item
    a, b = A.stats(), B.stats()
    assert all(a[key] == b[key] for key in STATS)


def test_the_rule_in_numpy():
    """What the header says of the rule: the orders 220 .. 256 pack (three tiles against 220 x 224 doubles and more), 257 ..
    312 do not, 313 is the first order of three tile rows that packs; 384 packs, 385 does not, 402 does."""
    assert [nz for nz in range(1, 385) if P.packs(nz)] == list(range(220, 257)) + list(range(313, 385))
    assert [P.packs(nz) for nz in P.ORDERS] == [False, True, True, False, False, True, True]
    assert all(P.arena(nz) <= nz * up8(nz) for nz in range(1, 3000))


def test_setter_return_codes_and_call_order():
    L = _lib.lib()
    assert L.hqpkkt_set_packed_hessians(None, 1) == _lib.E_NULL
    T = ipmatrix.IpSpBKP()  # (not in STAGED mode)
    assert L.hqpkkt_set_packed_hessians(T._h, 1) == _lib.E_INTERN
    M = ipmatrix.IpLQDOCP()
    for bad in (-1, 2, 3):
        assert L.hqpkkt_set_packed_hessians(M._h, bad) == _lib.E_RANGE
        assert L.hqpkkt_set_hessian_form(M._h, bad) == _lib.E_RANGE  # (its codes stay)
    assert L.hqpkkt_set_packed_hessians(M._h, 1) == 0 and L.hqpkkt_set_packed_hessians(M._h, 0) == 0
    # before the analysis; it holds over analyses until it is set again
    nx, nu = P.one_stage(384)
    M = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True)
    assert _analyze_sizes(M, nx, nu) == 0
    lay = M.hessian_packing()
    assert np.array_equal(lay, P.rows_of([384, 5]))
    assert _analyze_sizes(M, nx, nu) == 0 and np.array_equal(M.hessian_packing(), lay)
    M.set_packed_hessians(False)
    assert np.array_equal(M.hessian_packing(), lay)  # (the plan of the last analysis)
    assert _analyze_sizes(M, nx, nu) == 0
    assert len(M.hessian_packing()) == 0 and M.debug(47).size == 0 and M.debug(45).size == 8


@pytest.mark.parametrize("case", ["nx150", "wide_rows", "banded_profile_form"])
def test_ignored_with_the_csr_form_and_taken_back(case):
    """With HQPKKT_HESS_CSR the call is accepted and ignored: the plan of a handle that never asked, item for item.  on = 0
    after on = 1 before the analysis: the unpacked dense plan, item for item (item 45 among them)."""
    prog = CASES[case]()
    opts = OPTIONS[case]
    never, asked = ipmatrix.IpLQDOCP(**opts), ipmatrix.IpLQDOCP(q_packed=True, **opts)
    assert _analyze(never, prog) == 0 and _analyze(asked, prog) == 0
    _same_plan(asked, never)
    assert asked.debug(47).size == 0 and never.debug(47).size == 0
    dense, back, zero = (ipmatrix.IpLQDOCP(q_dense=True, **opts) for _ in range(3))
    back.set_packed_hessians(True), back.set_packed_hessians(False)
    zero.set_packed_hessians(False)
    for M in (dense, back, zero):
        assert _analyze(M, prog) == 0
    for M in (back, zero):
        _same_plan(M, dense)
        assert M.debug(47).size == 0 and dense.debug(47).size == 0


def _check_layout(packed, dense, nz):
    """47 against the rule; 45 unchanged; bytes_panels = the dense form's minus the saving, never above it."""
    lay = packed.hessian_packing()
    assert np.array_equal(lay, P.rows_of(nz))
    assert [bool(t) for t in lay[:, 0]] == [P.packs(v) for v in nz]
    assert np.array_equal(packed.debug(45), dense.debug(45))
    saving = 8 * sum(v * up8(v) - P.arena(v) for v in nz)
    assert saving >= 0 and (saving > 0) == any(P.packs(v) for v in nz)
    assert packed.stats()["bytes_panels"] == dense.stats()["bytes_panels"] - saving
    for key in STATS[1:]:
        assert packed.stats()[key] == dense.stats()[key]
    for item in PLAN_ITEMS:  # (the term lists, the wide rows and the dynamics' side of the plan are untouched)
        assert np.array_equal(packed.debug(item), dense.debug(item)), item


@pytest.mark.parametrize("nz", P.ORDERS + (219, 220, 256, 257))
def test_layout_of_one_order_after_both_analyses(nz):
    """A first stage of the given order (2 controls) and a terminal stage of 5 states, which never packs."""
    nx, nu = P.one_stage(nz)
    packed, dense = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True), ipmatrix.IpLQDOCP(q_dense=True)
    assert _analyze_sizes(packed, nx, nu) == 0 and _analyze_sizes(dense, nx, nu) == 0
    _check_layout(packed, dense, [nz, 5])
    # hqpkkt_analyze: the CSR hand-over of a program with this order (nx[0] = nx[1]: two stages of it and the terminal stage)
    prog = problems.with_dense_hessian(problems.sparse_docp(2, nz - 2, 2, band=3, seed=1, low_rank=False))
    packed, dense = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True), ipmatrix.IpLQDOCP(q_dense=True)
    assert _analyze(packed, prog) == 0 and _analyze(dense, prog) == 0
    assert orders(prog) == [nz, nz, nz - 2]
    _check_layout(packed, dense, orders(prog))
    assert dense.stats()["bytes_panels"] - packed.stats()["bytes_panels"] == arena_bytes(prog) - 8 * sum(P.arena(v) for v in orders(prog))


@pytest.mark.parametrize("opts", [dict(), dict(dense_rows=32), dict(a_profile=True, a_packed=True)])
def test_layout_of_mixed_stages_with_controls(opts):
    """Three stages of orders 313 (packs), 311 (does not), 403 = 386 + 17 controls (packs) and a terminal stage of 320
    (packs): the offsets run back to back - the arena elements of 47 sum to the arena -, under other options of the handle too."""
    nxs, nus = [310, 310, 386, 320], [3, 1, 17]
    prog = problems.with_dense_hessian(problems.sparse_docp(3, nxs, nus, band=4, seed=2, low_rank=False))
    if opts.get("dense_rows"):
        prog = problems.with_dense_hessian(problems.with_wide_rows(prog, [(2, 200, True), (0, 40, False)], seed=5))
    nz = orders(prog)
    assert nz == [313, 311, 403, 320] and [P.packs(v) for v in nz] == [True, False, True, True]
    packed, dense, csr = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True, **opts), ipmatrix.IpLQDOCP(q_dense=True, **opts), ipmatrix.IpLQDOCP(**opts)
    for M in (packed, dense, csr):
        assert _analyze(M, prog) == 0
    _check_layout(packed, dense, nz)
    lay = packed.hessian_packing()
    assert packed.stats()["bytes_panels"] == csr.stats()["bytes_panels"] + 8 * int(lay[:, 2].sum())  # (back to back: nothing between the stages)
    if not opts.get("a_profile"):  # (the dense hand-over of the dynamics gives the identical layout)
        D = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True, **opts)
        dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=True)
        nx, nu = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32)
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for t in (dq.E, dq.C) for a in t[:2]]
        assert D._L.hqpkkt_analyze_staged(D._h, dq.K, vp(nx), vp(nu), dq.n, dq.me_rest, dq.m, None, None, *[vp(a) for a in arrs]) == 0
        assert np.array_equal(D.hessian_packing(), lay)


def test_hand_over_count_and_scratch_at_the_headline_sizes():
    """An analysis only - nothing is allocated without a device.  The doubles one dense hand-over moves from a host block
    are at most 0.55 nz^2 at nz = 1024 and at nz = 5050: the rows go in groups of 64, every group from its first column on,
    nz (nz + 64) / 2 doubles for a multiple of 64 - 0.53125 nz^2 at 1024 (whole tile rows of 128 would move 0.5625 nz^2
    there).  K = 200 stages of 5000 states and 50 controls: the scratch of the product is at most 1 % of what packing saves."""
    for nz in (1024, 5050):
        nx, nu = P.one_stage(nz)
        M = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True)
        assert _analyze_sizes(M, nx, nu) == 0
        row = M.hessian_packing()[0]
        assert row[0] == P.T and row[3] == P.handover(nz)
        print(f"order {nz}: one hand-over moves {row[3]} doubles, {row[3] / nz ** 2:.4f} nz^2")
        assert row[3] <= 0.55 * nz * nz
    assert P.handover(1024) == 1024 * (1024 + 64) // 2
    K, nx, nu = 200, 5000, 50
    packed, dense = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True), ipmatrix.IpLQDOCP(q_dense=True)
    assert _analyze_sizes(packed, [nx] * (K + 1), [nu] * K) == 0 and _analyze_sizes(dense, [nx] * (K + 1), [nu] * K) == 0
    lay = packed.hessian_packing()
    assert lay.shape == (K + 1, 5) and (lay[:, 0] == P.T).all()
    assert lay[0].tolist() == [128, 40 * 41 // 2, 820 * 128 * 128, P.handover(5050), (120 + 780) * 128]  # (slots: 120 of the rows' chunks, 780 of the tiles below the diagonal)
    saving = dense.stats()["bytes_panels"] - packed.stats()["bytes_panels"]
    assert saving == 8 * int((K * 5050 * 5056 + 5000 * 5000) - lay[:, 2].sum()) and saving > 19e9
    scratch = 8 * int(lay[:, 4].sum())
    print(f"K = {K}: packing saves {saving / 1e9:.2f} GB, the product's scratch is {scratch / 1e6:.1f} MB")
    assert scratch <= 0.01 * saving


def test_a_sharded_handle_is_refused_at_the_analysis():
    prog = CASES["with_carried_rows"]()
    M = ipmatrix.IpLQDOCP(q_dense=True, q_packed=True)
    M.set_shard(0, 2, lambda *a: 0)
    assert _analyze(M, prog) == _lib.E_RANGE
    assert _analyze_sizes(M, prog.nx, prog.nu) == _lib.E_RANGE
    M.set_hessian_form("csr")  # (packing alone asks for nothing)
    assert _analyze(M, prog) == 0 and M.debug(47).size == 0
