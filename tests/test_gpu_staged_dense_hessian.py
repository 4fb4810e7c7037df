"""GPU tests of the dense stage Hessians of the STAGED engine (hqpkkt_set_hessian_form; hqp_amd/csrc/staged_hess.hip.h): the
blocks Q_k stored by copy + mirror or by the scatter of the CSR values, added into the stage's work block ahead of the
term lists, and multiplied by one launch over all stages for the residual and the interior-point loops.

The bars are the sibling tests' own (test_gpu_staged_wide_rows.py): the solution within 1e-8, relative to the vectors'
norms, of the comparison partner's, and the residuum() of our solution <= the partner's + 1e-10.  Partners: the CPU oracle
of the full system, the reference's own Hqp_IpLQDOCP (live, oracle/_ref), the same library in form 0 (term lists)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import new_d, rel_err
from dense_hessian_cases import CASES, DENSE_HANDOVER, OPTIONS, kkt_row_bound, padded, up8
from hqp_amd import ipmatrix, problems

import dense_hessian_worker as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RES_TOL = 1e-10
SOL_TOL = 1e-8
HANDOVERS = [(c, "csr") for c in sorted(CASES)] + [(c, "dense") for c in sorted(DENSE_HANDOVER)]


def _handle(case, q_dense=True):
    return ipmatrix.IpLQDOCP(q_dense=q_dense, **OPTIONS[case])


def _init(M, prog, how, q_dense=True):
    if how == "csr":
        M.init(prog)
    else:
        M.init_dense(problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=q_dense))
    return M


def _solve(M, prog, st, how="csr", q_dense=True):
    _init(M, prog, how, q_dense)
    M.factor(prog, st[0], st[1])
    d = new_d(prog)
    res = M.solve(prog, *st, *d)
    return d, res


def _step(M, prog, st):
    M.factor(prog, st[0], st[1])
    d = new_d(prog)
    M.step(prog, *st, *d)
    return d + [M.stage_block(k) for k in range(len(prog.nx))]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))


@pytest.mark.parametrize("case,how", HANDOVERS)
def test_dense_hessians_against_the_partners(case, how):
    """G1: factor + solve on ip_state vectors (z and w each over two decades), both hand-overs."""
    from oracle import oracleapi, refapi
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M = _handle(case)
    d, res = _solve(M, prog, st, how)
    assert len(M.hessian_layout()) == len(prog.nx)
    O = oracleapi.OracleIpMatrix("SpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    partners = {"oracle": O.solve(*st), "form 0": _solve(_handle(case, False), prog, st, how, False)}
    if refapi.available():
        L = refapi.RefIpMatrix("LQDOCP")
        L.init(prog)
        L.factor(st[0], st[1])
        partners["reference"] = L.solve(*st)
    for name, (psol, pres) in partners.items():
        err = rel_err(d, psol)
        print(f"{case} ({how}): res {res:.3e} ({name} {pres:.3e}) rel.err {err:.3e}")
        assert res <= pres + RES_TOL, (name, res, pres)
        assert err <= SOL_TOL, (name, err)


@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_blocks_are_symmetric_and_those_of_form_0(case):
    """G2: V_k bit-for-bit equal to its transpose for every k; equal to V_k of form 0 to 1e-10 of its largest entry."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    S, D = _handle(case), _handle(case, False)
    _solve(S, prog, st), _solve(D, prog, st, q_dense=False)
    for k in range(len(prog.nx)):
        vs, vd = S.stage_block(k), D.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vd).max() <= 1e-10 * np.abs(vd).max(), (k, np.abs(vs - vd).max(), np.abs(vd).max())


@pytest.mark.parametrize("case,how", [("nx150", "csr"), ("nx150", "dense"), ("banded_sparse_form", "csr"), ("wide_rows", "dense")])
def test_reproducible_and_takes_new_values(case, how):
    """G3: two factor + step rounds give the same bits.  New values of Q on the same pattern (another seed: every entry
    changes): the bits of a fresh handle, the step and every V_k - the scatter (CSR) or copy and mirror (dense) refill the
    blocks."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M = _init(_handle(case), prog, how)
    first, again = _step(M, prog, st), _step(M, prog, st)
    assert _same_bits(first, again)
    other = problems.with_dense_hessian(prog, seed=56)
    assert np.array_equal(other.Q[1], prog.Q[1]) and not np.array_equal(other.Q[2], prog.Q[2])
    if how == "csr":
        M.update(other)
    else:
        M.update_dense(problems.dense_docp_from_program(other, other.nx, other.nu, dense_hessian=True))
    moved = _step(M, other, st)
    fresh = _step(_init(_handle(case), other, how), other, st)
    assert _same_bits(moved, fresh)
    assert not np.array_equal(moved[0], first[0])


@pytest.mark.parametrize("case", ["nx150", "banded_profile_form", "wide_rows"])
def test_form_0_leaves_no_trace(case):
    """G4: form 0 set explicitly against a handle that never asked: the same launches, so the same bits - the step, every
    V_k and the residuum."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    A, B = ipmatrix.IpLQDOCP(**OPTIONS[case]), ipmatrix.IpLQDOCP(**OPTIONS[case])
    B.set_hessian_form("dense"), B.set_hessian_form("csr")
    outs, res = [], []
    for M in (A, B):
        M.init(prog)
        outs.append(_step(M, prog, st))
        res.append(M.residuum(prog, *st, *outs[-1][:4]))
    assert B.debug(45).size == 0
    assert _same_bits(*outs) and res[0] == res[1]


# block orders of the store and the product: 1, 7, the edges of a 64- and a 128-wide tile, 73, 154, and both sides of
# every edge of the mirror kernel's 32 x 32 tiles up to 160; three blocks per handle (stage 0, stage 1, stage K)
ORDERS = [(7, 31, 1), (32, 33, 63), (64, 65, 73), (95, 96, 97), (127, 128, 129), (154, 159, 160), (161, 8, 2)]


def _block_handle(orders, blocks, ld_extra=3):
    """A dense hand-over of K = 2 stages with Q_k of the given orders: stage k < 2 has order - 1 states and one control.
    The blocks go over with NaN in their strict lower triangle and in ld_extra columns behind the block."""
    nx, nu = [orders[0] - 1, orders[1] - 1, orders[2]], [1, 1]
    rng = np.random.default_rng(sum(orders))
    n = sum(orders)
    empty = lambda rows: (np.zeros(rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0))
    F = [0.1 * rng.uniform(-1, 1, (nx[k + 1], nx[k] + nu[k])) for k in range(2)]
    given = []
    for B in blocks:
        G = np.full((B.shape[0], B.shape[0] + ld_extra), np.nan)
        iu = np.triu_indices(B.shape[0])
        G[iu] = B[iu]
        given.append(G)
    dq = problems.DenseDocp(nx, nu, empty(n), empty(0), empty(0), F, 0, 0, Qd=given)
    M = ipmatrix.IpLQDOCP(q_dense=True)
    M.init_dense(dq)
    return M, dq


def _sym(rng, nz, integers):
    U = rng.integers(-8, 9, (nz, nz)).astype(float) if integers else rng.standard_normal((nz, nz)) * 10.0 ** rng.uniform(-3, 3, (nz, nz))
    return np.triu(U) + np.triu(U, 1).T


@pytest.mark.parametrize("orders", ORDERS)
def test_store_and_product(orders):
    """G5, G6: hqpkkt_set_stage_hessian reads the upper triangle alone - NaN in the caller's strict lower triangle and
    behind column nz_k - and the arena holds the symmetrised block exactly, with zero padding.  y = Q x by the kernel of
    the residual: bit for bit numpy's on integer-valued operands (every sum is exact in any order), within
    1e-14 sum_j |q_ij| |x_j| per entry on full-mantissa operands (the bar of test_gpu_dgemm_full.py); then new blocks on the
    same handle."""
    rng = np.random.default_rng(7)
    off = np.concatenate([[0], np.cumsum(orders)])
    M = None
    for integers in (True, False):
        blocks = [_sym(rng, nz, integers) for nz in orders]
        if M is None:
            M, dq = _block_handle(orders, blocks)
        else:  # (new values through the same hand-over)
            dq.Qd = [np.triu(B) for B in blocks]  # (zeros below the diagonal this time: not read either)
            M.update_dense(dq)
        lay = M.hessian_layout()
        assert lay[:, 0].tolist() == list(orders) and lay[:, 1].tolist() == [up8(v) for v in orders]
        for k, want in enumerate(padded(blocks)):
            got = M.stage_hessian(k)
            assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), (k, orders[k])
        x = rng.integers(-8, 9, dq.n).astype(float) if integers else rng.standard_normal(dq.n)
        y = M.hess_symv(x)
        assert np.array_equal(M.hess_symv(x), y)  # (a fixed order of the sums)
        for k, B in enumerate(blocks):
            xk, yk = x[off[k]: off[k + 1]], y[off[k]: off[k + 1]]
            if integers:
                assert np.array_equal(yk, B @ xk), (k, orders[k])
            else:
                bound = 1e-14 * (np.abs(B) @ np.abs(xk))
                worst = (np.abs(yk - B @ xk) / bound).max()
                print(f"order {orders[k]}: largest error {worst * 1e-14:.2e} of sum |q||x|")
                assert worst <= 1.0, (k, orders[k], worst)


def test_a_missing_hessian_block_is_refused():
    """hqpkkt_set_values_staged ends the hand-over only when every Hessian block has come since the analysis; on the CSR
    hand-over hqpkkt_set_stage_hessian is refused (on an uploaded handle too)."""
    import ctypes as C
    from hqp_amd import _lib
    orders = (7, 31, 1)
    blocks = [_sym(np.random.default_rng(1), nz, True) for nz in orders]
    M, dq = _block_handle(orders, blocks)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    F = [np.ascontiguousarray(b) for b in dq.F]
    fp = (C.c_void_p * dq.K)(*[b.ctypes.data for b in F])
    ld = (C.c_longlong * dq.K)(*[b.shape[1] for b in F])
    nx, nu, eye = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32), np.eye(73)
    L = M._L
    # a new analysis: nothing has come yet
    assert L.hqpkkt_analyze_staged(M._h, 2, vp(nx), vp(nu), dq.n, 0, 0, None, None, None, None, None, None) == 0
    for k in (0, 2):
        M.set_stage_hessian(k, blocks[k])
    assert L.hqpkkt_set_values_staged(M._h, None, fp, ld, None, None) == _lib.E_INTERN
    M.set_stage_hessian(1, blocks[1])
    assert L.hqpkkt_set_values_staged(M._h, None, fp, ld, None, None) == 0
    assert L.hqpkkt_set_stage_hessian(M._h, 3, vp(blocks[0]), 7) == _lib.E_RANGE
    assert L.hqpkkt_set_stage_hessian(M._h, 0, vp(blocks[0]), 6) == _lib.E_SIZES
    prog = CASES["nx70"]()
    N = _init(_handle("nx70"), prog, "csr")
    assert L.hqpkkt_set_stage_hessian(N._h, 0, vp(eye), 73) == _lib.E_INTERN


def test_blocks_out_of_the_staging_buffers():
    """A host block may come out of the hqpkkt_stage_staging buffers: with dense Hessians they hold the largest Q_k - here
    65 x 65 doubles, more than the largest block of the dynamics (64 x 33) - and a buffer is handed out again only when the
    copy that read it is over.  Three blocks through the two buffers in turn, NaN below the diagonal: the arena holds the
    symmetrised blocks bit for bit.  In form 0 the buffers keep the size of the largest block of the dynamics."""
    import ctypes as C
    orders = (65, 33, 64)
    rng = np.random.default_rng(11)
    blocks = [_sym(rng, nz, False) for nz in orders]
    M, dq = _block_handle(orders, blocks)
    L = M._L
    vp = lambda a: C.c_void_p(a.ctypes.data)
    nx, nu = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32)
    F = [np.ascontiguousarray(b) for b in dq.F]
    fp = (C.c_void_p * dq.K)(*[b.ctypes.data for b in F])
    ld = (C.c_longlong * dq.K)(*[b.shape[1] for b in F])

    def staging(H, which):
        buf, elems = C.c_void_p(), C.c_longlong()
        assert L.hqpkkt_stage_staging(H._h, which, C.byref(buf), C.byref(elems)) == 0
        return buf.value, elems.value

    plain = ipmatrix.IpLQDOCP()
    assert L.hqpkkt_analyze_staged(plain._h, 2, vp(nx), vp(nu), dq.n, 0, 0, vp(dq.Q[0]), None, None, None, None, None) == 0
    assert staging(plain, 0)[1] == 64 * 33
    # a new analysis: nothing has come yet
    assert L.hqpkkt_analyze_staged(M._h, 2, vp(nx), vp(nu), dq.n, 0, 0, None, None, None, None, None, None) == 0
    other = [_sym(rng, nz, False) for nz in orders]
    for k, B in enumerate(other):
        addr, elems = staging(M, k & 1)
        assert elems == 65 * 65
        buf = np.ctypeslib.as_array((C.c_double * elems).from_address(addr))
        buf[:] = np.nan
        view = buf[: B.size].reshape(B.shape)
        iu = np.triu_indices(B.shape[0])
        view[iu] = B[iu]
        assert L.hqpkkt_set_stage_hessian(M._h, k, C.c_void_p(addr), B.shape[0]) == 0
    assert L.hqpkkt_set_values_staged(M._h, None, fp, ld, None, None) == 0
    for k, want in enumerate(padded(other)):
        got = M.stage_hessian(k)
        assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), k


@pytest.mark.parametrize("case,how", [("nx150", "csr"), ("order_129", "dense"), ("with_carried_rows", "dense"), ("banded_packed_panels", "csr")])
def test_residuum_on_unsolved_vectors(case, how):
    """G7: residuum() on random vectors that solve nothing: form 1 against form 0 within 1e-14 of the largest row sum
    sum_j |K_ij| |d_j| of the Newton system - one rounding per product and per partial sum of a row of at most 304 entries
    in either order of summation."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    rng = np.random.default_rng(3)
    d = [rng.uniform(-1, 1, k) for k in (prog.n, prog.me, prog.m, prog.m)]
    res = []
    for q_dense in (True, False):
        M = _init(_handle(case, q_dense), prog, how, q_dense)
        res.append(M.residuum(prog, *st, *d))
    bound = kkt_row_bound(prog, st, d)
    print(f"{case} ({how}): residuum form 1 {res[0]!r} form 0 {res[1]!r}; difference {abs(res[0] - res[1]):.2e}, row sum {bound:.3e}")
    assert res[0] > 1.0 and abs(res[0] - res[1]) <= 1e-14 * bound


def _child(what, case, tmp_path, **env):
    out = str(tmp_path / f"{what}_{case}.npz")
    subprocess.run([sys.executable, os.path.join(HERE, "dense_hessian_worker.py"), what, case, out], env=dict(os.environ, **env), check=True, timeout=600)
    return np.load(out)


@pytest.mark.parametrize("case,iters", [("nx150", 3), ("x_bounds", 4)])
def test_interior_point_loops(case, iters, tmp_path):
    """G8: hqpkkt_mehrotra and hqpkkt_franke: result and iteration count of form 0 and of the reference's loops on its own
    Hqp_IpLQDOCP (Mehrotra: 3 and 4 iterations, result 0, measured on the CPU when the cases were written), the same point
    to 1e-8; a child process with HQPKKT_NO_IP_SEGMENTS=1 gives the same bits."""
    from oracle import refapi
    prog = CASES[case]()
    S, D = _handle(case), _handle(case, False)
    S.init(prog), D.init(prog)
    child = _child("ip", case, tmp_path, HQPKKT_NO_IP_SEGMENTS="1")
    for name, solver in (("mehrotra", "Mehrotra"), ("franke", "Franke")):
        xs, ys, zs, ws, infs = getattr(S, name)(prog)
        xd, yd, zd, wd, infd = getattr(D, name)(prog)
        print(f"{case} {name}: iterations dense blocks / term lists: {infs['iters']} / {infd['iters']}, result {infs['result']} / {infd['result']}")
        assert infs["result"] == infd["result"] and infs["iters"] == infd["iters"], (infs, infd)
        assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()
        if name == "mehrotra":
            assert infs["result"] == 0 and infs["iters"] == iters, infs
        if refapi.host_available("ref"):
            ref = refapi.ip_solve(prog, solver, "LQDOCP")
            print(f"{case} {name}: iterations of the reference: {ref['iters']}, result {ref['result']}")
            assert infs["result"] == ref["result"] and infs["iters"] == ref["iters"], (infs, ref["iters"], ref["result"])
            assert np.abs(xs - ref["x"]).max() <= 1e-8 * max(1.0, np.abs(ref["x"]).max()), np.abs(xs - ref["x"]).max()
        assert child[f"{name}_info"].tolist() == [infs["result"], infs["iters"]]
        assert _same_bits([xs, ys, zs, ws], [child[f"{name}_{v}"] for v in "xyzw"])


def test_interior_point_loops_on_the_dense_hand_over():
    """G8 on hqpkkt_analyze_staged with DenseDocp.Qd: the library holds no CSR form of Q there, so Q x of the right-hand
    sides comes from the blocks alone.  Both loops against the dense hand-over in form 0 (Q as CSR) and the iteration counts
    measured for the case: the same result, iterations and point."""
    prog = CASES["x_bounds"]()
    S = _init(_handle("x_bounds"), prog, "dense")
    D = _init(_handle("x_bounds", False), prog, "dense", False)
    dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu, dense_hessian=True)
    for name, iters in (("mehrotra", 4), ("franke", 10)):
        xs, ys, zs, ws, infs = getattr(S, name)(dq)
        xd, yd, zd, wd, infd = getattr(D, name)(dq)
        print(f"x_bounds {name} (dense hand-over): iterations dense blocks / term lists: {infs['iters']} / {infd['iters']}, result {infs['result']} / {infd['result']}")
        assert infs["result"] == infd["result"] == 0 and infs["iters"] == infd["iters"] == iters, (infs, infd)
        assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()


def test_the_fused_width_takes_the_128_tile_form():
    """(host code) The launch that forms V_k of a stage of FUSED_NX states gets 128 x 128 tiles from the rule - so
    HQPKKT_FUSED_V=1 fuses it - and a stage of 150 states does not and keeps the separate update."""
    nslab = (W.FUSED_NX + 15) // 16 + 1
    assert ipmatrix.gemm_form(W.FUSED_NX, W.FUSED_NX, 16 * nslab, lower=True, mirror=True)[0] in ("cut", "plain", "frac")
    assert ipmatrix.gemm_form(150, 150, 16 * 11, lower=True, mirror=True)[0] == "6464"


@pytest.mark.parametrize("case,fused", [("nx150", 0), ("fused_width", 1)])
def test_sequences_under_fused_v(case, fused, tmp_path):
    """G9: HQPKKT_FUSED_V=1 in a child process, form 1 against form 0: the 150-state case (whose stages are too narrow to
    form V_k in the G_xx launch: the switch changes nothing) and a stage of 2304 states and 8 controls that does - Q's
    control rows go into G ahead of the chain, Q_xx into V_k, which stays bit-for-bit symmetric."""
    g = _child("step", case, tmp_path, HQPKKT_FUSED_V="1")
    K = len(g["fused1"]) - 1
    assert g["fused1"][:K].tolist() == [fused] * K and g["fused0"][:K].tolist() == [fused] * K
    assert g["asym1"].max() == 0.0 and g["asym0"].max() == 0.0
    assert (g["vdiff"] <= 1e-10 * g["vmax0"]).all(), (g["vdiff"], g["vmax0"])
    err = rel_err([g[f"{v}1"] for v in ("dx", "dy", "dz", "dw")], [g[f"{v}0"] for v in ("dx", "dy", "dz", "dw")])
    print(f"{case} under HQPKKT_FUSED_V=1: step of form 1 against form 0 {err:.3e}")
    assert err <= SOL_TOL, err


def test_the_chain_on_the_second_stream():
    """G9: a stage of 1280 states runs its control-sized chain beside the large product G_xx: the state part of Q_k goes
    into G on the first stream, its control rows on the second."""
    prog = problems.with_dense_hessian(problems.sparse_docp(2, 1280, 8, band=5, seed=11, low_rank=False))
    st = problems.ip_state(prog, 3, 1.0)
    S, D = ipmatrix.IpLQDOCP(q_dense=True), ipmatrix.IpLQDOCP()
    (d, res), (dd, rd) = _solve(S, prog, st), _solve(D, prog, st, q_dense=False)
    err = rel_err(d, dd)
    print(f"1280 states: res form 1 {res:.3e} form 0 {rd:.3e} rel.err {err:.3e}")
    assert res <= rd + RES_TOL and err <= SOL_TOL, (res, rd, err)
    for k in range(3):
        vs, vd = S.stage_block(k), D.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vd).max() <= 1e-10 * np.abs(vd).max(), (k, np.abs(vs - vd).max(), np.abs(vd).max())


def test_dense_hessians_at_2000_states_are_not_slower():
    """G10: 2000 states, 8 controls, K = 4, a band of 5 in the dynamics, dense Hessians, form 1 against form 0 - the parent's
    code path, unchanged: the yardstick.  hqpkkt_stats.ms_factor of replayed factorisations, the handles taking turns, best
    of three each: form 1 is not above form 0.  No further margin: per entry of Q_k the blocks move 24 bytes where the
    lists move at least 40.  Measured on one MI355X (profiles/r17_dense_hessian.txt): blocks 2.394 ms, lists 2.522 ms, ratio 0.949;
    one residual 0.062 ms against 0.089 ms."""
    prog = problems.with_dense_hessian(problems.sparse_docp(4, 2000, 8, band=5, seed=2, low_rank=False))
    st = problems.ip_state(prog, 3, 1.0)
    H = {"blocks": ipmatrix.IpLQDOCP(q_dense=True), "lists": ipmatrix.IpLQDOCP()}
    sol = {name: _solve(M, prog, st, q_dense=name == "blocks") for name, M in H.items()}
    (d, res), (dd, rd) = sol["blocks"], sol["lists"]
    err = rel_err(d, dd)
    print(f"res blocks {res:.3e} lists {rd:.3e} rel.err {err:.3e}")
    assert res <= rd + RES_TOL, (res, rd)
    assert err <= SOL_TOL, err
    ms = {name: [] for name in H}
    for _ in range(3):
        for name, M in H.items():
            M.factor(prog, st[0], st[1])
            ms[name].append(M.stats()["ms_factor"])
    best = {name: min(t for t in v if t > 0) for name, v in ms.items()}  # (-1: the events gave no time)
    msr = {}
    for name, M in H.items():
        M.residuum(prog, *st, *d)
        msr[name] = M.stats()["ms_residual"]
    print("ms_factor (best of three): " + " ".join(f"{name} {v:.3f}" for name, v in best.items()) +
          f"; blocks / lists {best['blocks'] / best['lists']:.3f}; all: {ms}; one residual: " + " ".join(f"{name} {v:.3f} ms" for name, v in msr.items()))
    assert best["blocks"] <= best["lists"], best
