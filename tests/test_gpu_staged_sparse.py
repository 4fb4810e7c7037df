"""GPU tests of the sparse form of the STAGED engine's stage products (hqpkkt_set_dynamics_form, the reference's
mat_a_sparse; hqp_amd/csrc/staged_sparse.hip.h) on multistage QPs with banded dynamics (problems.sparse_docp).

The bar is the project's own: the solution within 1e-8, relative to the
vectors' norms, of the comparison partner's, and the residuum() of our solution <= the partner's + 1e-10.  Partners:
the reference's own Hqp_IpLQDOCP (live, oracle/_ref), the dense form of the same library, the full-system engine.
"""
import numpy as np
import pytest
import torch

from common import new_d, rel_err
from hqp_amd import ipmatrix, problems

pytestmark = pytest.mark.gpu

RES_TOL = 1e-10
SOL_TOL = 1e-8

# every case is factored by the reference's Hqp_IpLQDOCP without E_SING (checked on the CPU when the cases were written)
CASES = {
    "band1_nx40": lambda: problems.sparse_docp(6, 40, 3, band=1),
    "band5_nx40": lambda: problems.sparse_docp(6, 40, 3, band=5),
    "band1_nx130": lambda: problems.sparse_docp(4, 130, 4, band=1, seed=4),
    "band5_nx130": lambda: problems.sparse_docp(4, 130, 4, band=5, seed=5),
    "stages_differ": lambda: problems.sparse_docp(5, [40, 40, 37, 52, 45, 31], [3, 2, 4, 1, 3], band=4, seed=6),
    "odd_nx": lambda: problems.sparse_docp(5, 43, 3, band=3, seed=7),
    "final_eq_carried": lambda: problems.sparse_docp(7, 40, 3, band=4, final_eq=7, seed=8),
    "path_eq_xb_free_x0": lambda: problems.sparse_docp(6, 40, 4, band=3, path_eq=2, x_bounds=5, x0_fixed=False, seed=9),
    "path_eq_final_xb": lambda: problems.sparse_docp(6, 48, 4, band=5, path_eq=1, path_eq_every=2, final_eq=3, x_bounds=4, seed=10),
    "dense_F": lambda: problems.sparse_docp(4, 40, 3, dense=True, seed=11),
    "empty_col_row": lambda: problems.sparse_docp(5, 40, 3, band=2, empty_col=(2, 7), empty_row=(3, 11), seed=12),
}


def _solve(M, prog, st):
    M.init(prog)
    M.factor(prog, st[0], st[1])
    d = new_d(prog)
    res = M.solve(prog, *st, *d)
    return d, res


def _sparse():
    return ipmatrix.IpLQDOCP(a_sparse=True)


@pytest.mark.parametrize("case", sorted(CASES))
def test_sparse_form_against_the_reference(case, spread=1.0):
    """factor + solve on ip_state vectors (z and w each over two decades) against the reference's Hqp_IpLQDOCP (live,
    where oracle/_ref travelled, as in test_gpu_staged.py) and against the CPU oracle of the full system."""
    from oracle import oracleapi, refapi
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, spread)
    M = _sparse()
    d, res = _solve(M, prog, st)
    assert (M.dynamics_entries()[:, 1] == 1).all()
    O = oracleapi.OracleIpMatrix("SpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    osol, ores = O.solve(*st)
    err = rel_err(d, osol)
    print(f"{case}: res {res:.3e} (oracle {ores:.3e}) rel.err {err:.3e}")
    assert res <= ores + RES_TOL, (res, ores)
    assert err <= SOL_TOL, err
    if refapi.available():
        L = refapi.RefIpMatrix("LQDOCP")
        L.init(prog)
        L.factor(st[0], st[1])
        lsol, lres = L.solve(*st)
        err = rel_err(d, lsol)
        print(f"{case}: res {res:.3e} (reference {lres:.3e}) rel.err {err:.3e}")
        assert res <= lres + RES_TOL, (res, lres)
        assert err <= SOL_TOL, err


@pytest.mark.parametrize("nx", [1000, 2000])
def test_sparse_form_against_the_dense_form(nx):
    prog = problems.sparse_docp(6, nx, 20, band=5, seed=2)
    st = problems.ip_state(prog, 5, 1.0)
    S, D = _sparse(), ipmatrix.IpLQDOCP()
    ds, rs = _solve(S, prog, st)
    dd, rd = _solve(D, prog, st)
    err = rel_err(ds, dd)
    print(f"nx {nx}: res sparse {rs:.3e} dense {rd:.3e} rel.err {err:.3e}")
    assert rs <= rd + RES_TOL, (rs, rd)
    assert err <= SOL_TOL, err


def test_sparse_form_against_the_full_system_engine():
    prog = problems.sparse_docp(6, 300, 8, band=5, final_eq=4, seed=3)
    st = problems.ip_state(prog, 5, 1.0)
    S, F = _sparse(), ipmatrix.IpLQDOCPFull()
    ds, rs = _solve(S, prog, st)
    df, rf = _solve(F, prog, st)
    err = rel_err(ds, df)
    print(f"res sparse {rs:.3e} full {rf:.3e} rel.err {err:.3e}")
    assert rs <= rf + RES_TOL, (rs, rf)
    assert err <= SOL_TOL, err


@pytest.mark.parametrize("case", ["band5_nx130", "stages_differ", "odd_nx", "final_eq_carried", "dense_F", "empty_col_row"])
def test_stage_blocks_are_symmetric_and_the_dense_form_s(case):
    """V_k bit-for-bit equal to its transpose for every k; equal to the dense form's V_k to 1e-10 of its largest entry."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 4, 1.0)
    S, D = _sparse(), ipmatrix.IpLQDOCP()
    _solve(S, prog, st), _solve(D, prog, st)
    for k in range(len(S.debug(20))):
        vs, vd = S.stage_block(k), D.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vd).max() <= 1e-10 * np.abs(vd).max(), (k, np.abs(vs - vd).max(), np.abs(vd).max())


def test_sparse_form_is_reproducible_and_takes_new_values():
    """Two factorisations and solves in a row: the same bits.  set_values with new values on the same pattern: the result
    of a fresh handle, bit for bit."""
    prog = problems.sparse_docp(6, 260, 6, band=5, final_eq=3, seed=21)
    st = problems.ip_state(prog, 8, 1.0)
    M = _sparse()
    M.init(prog)
    outs = []
    for _ in range(2):
        M.factor(prog, st[0], st[1])
        d = new_d(prog)
        M.step(prog, *st, *d)
        outs.append(d)
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    p, i, x = prog.A
    rng = np.random.default_rng(5)
    x2 = np.where(x == -1.0, x, x * rng.uniform(0.8, 1.2, x.size))
    prog2 = problems.Program(prog.n, prog.me, prog.m, prog.Q, (p, i, x2), prog.C, c=prog.c, b=prog.b, d=prog.d)
    M.update(prog2)
    M.factor(prog2, st[0], st[1])
    d1 = new_d(prog)
    M.step(prog2, *st, *d1)
    N = _sparse()
    N.init(prog2)
    N.factor(prog2, st[0], st[1])
    d2 = new_d(prog)
    N.step(prog2, *st, *d2)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))
    assert not np.array_equal(d1[0], outs[0][0])


def test_mehrotra_on_the_sparse_form():
    """The device-resident interior-point loop: the iteration count of the dense form and of the reference's
    Hqp_IpsMehrotra on its own Hqp_IpLQDOCP, the same point to 1e-8."""
    from oracle import refapi
    prog = problems.sparse_docp(8, 60, 4, band=5, x_bounds=6, seed=13)
    S, D = _sparse(), ipmatrix.IpLQDOCP()
    S.init(prog), D.init(prog)
    xs, ys, zs, ws, infs = S.mehrotra(prog)
    xd, yd, zd, wd, infd = D.mehrotra(prog)
    print("iterations sparse / dense:", infs["iters"], infd["iters"])
    assert infs["result"] == infd["result"] == 0 and infs["iters"] == infd["iters"], (infs, infd)
    assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()
    if refapi.host_available("ref"):
        ref = refapi.ip_solve(prog, "Mehrotra", "LQDOCP")
        print("iterations of the reference:", ref["iters"])
        assert ref["result"] == 0 and infs["iters"] == ref["iters"], (infs["iters"], ref["iters"])
        assert np.abs(xs - ref["x"]).max() <= 1e-8 * max(1.0, np.abs(ref["x"]).max()), np.abs(xs - ref["x"]).max()


def test_sparse_form_is_at_least_twice_as_fast_at_2000_states():
    """hqpkkt_stats.ms_factor of the second factorisation of each form at nx = 2000, nu = 20, K = 8, band 5: the dense
    stage is about 2.4e10 flop at the measured 40 TFLOP/s (0.6 ms) plus the control-sized chain, the sparse stage the
    same chain plus the rank-q update plus two passes over about 130 MB - under 0.3 ms even at 1 TB/s.  Expected ratio
    3 or more; 2 leaves room for the chain."""
    prog = problems.sparse_docp(8, 2000, 20, band=5, seed=2)
    st = problems.ip_state(prog, 5, 1.0)
    ms = {}
    for form, M in (("sparse", _sparse()), ("dense", ipmatrix.IpLQDOCP())):
        M.init(prog)
        M.factor(prog, st[0], st[1])
        M.factor(prog, st[0], st[1])
        ms[form] = M.stats()["ms_factor"]
        d = new_d(prog)
        assert M.solve(prog, *st, *d) <= RES_TOL
    print(f"ms_factor: sparse {ms['sparse']:.3f} dense {ms['dense']:.3f} ratio {ms['dense'] / ms['sparse']:.2f}")
    assert 2.0 * ms["sparse"] <= ms["dense"], ms


def test_the_widest_shape_through_the_sparse_form():
    """nx = 5000, K = 4, band 5 on a device of >= 250 GB: the residual contract and symmetric V_k."""
    if torch.cuda.get_device_properties(0).total_memory < 250e9:
        pytest.skip("needs a device of >= 250 GB")
    prog = problems.sparse_docp(4, 5000, 20, band=5, seed=2, low_rank=False)  # (diagonal Q: 12.5e6 entries per stage otherwise)
    st = problems.ip_state(prog, 5, 1.0)
    M = _sparse()
    d, res = _solve(M, prog, st)
    print(f"nx 5000: res {res:.3e} ms_factor {M.stats()['ms_factor']:.3f}")
    assert res <= RES_TOL, res
    for k in range(5):
        v = M.stage_block(k)
        assert np.array_equal(v, v.T), k
