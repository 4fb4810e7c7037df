"""GPU tests of the heavy columns of the STAGED engine's sparse form (hqpkkt_set_dense_columns;
hqp_amd/csrc/staged_sparse.hip.h, staged_stage_sparse): the columns of F_k with many entries go through the fp64 MFMA
product as a small dense block D_k, all others stay on the column walks.

The bar is the sparse form's own (test_gpu_staged_sparse.py): the solution within 1e-8, relative to the vectors' norms,
of the comparison partner's, and the residuum() of our solution <= the partner's + 1e-10.  Partners: the reference's own
Hqp_IpLQDOCP (live, oracle/_ref), the CPU oracle of the full system, the dense form of the same library.
"""
import numpy as np
import pytest

from common import new_d, rel_err
from dense_columns_cases import BIG, CASES, MIN_ENTRIES, expected_heavy
from hqp_amd import ipmatrix, problems

pytestmark = pytest.mark.gpu

RES_TOL = 1e-10
SOL_TOL = 1e-8


def _solve(M, prog, st):
    M.init(prog)
    M.factor(prog, st[0], st[1])
    d = new_d(prog)
    res = M.solve(prog, *st, *d)
    return d, res


def _split(min_entries=8):
    return ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=min_entries)


@pytest.mark.parametrize("case", sorted(CASES))
def test_heavy_columns_against_the_partners(case):
    """factor + solve on ip_state vectors (z and w each over two decades) against the CPU oracle of the full system, the
    reference's Hqp_IpLQDOCP (live, where oracle/_ref travelled) and the dense form; the plan's heavy columns are what
    numpy counts."""
    from oracle import oracleapi, refapi
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M = _split(MIN_ENTRIES[case])
    d, res = _solve(M, prog, st)
    heavy = expected_heavy(prog, MIN_ENTRIES[case])
    assert M.dense_columns() == heavy and any(heavy)
    assert (M.dynamics_entries()[:, 1] == 1).all()
    O = oracleapi.OracleIpMatrix("SpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    partners = {"oracle": O.solve(*st), "dense form": _solve(ipmatrix.IpLQDOCP(), prog, st)}
    if refapi.available():
        L = refapi.RefIpMatrix("LQDOCP")
        L.init(prog)
        L.factor(st[0], st[1])
        partners["reference"] = L.solve(*st)
    for name, (psol, pres) in partners.items():
        err = rel_err(d, psol)
        print(f"{case}: res {res:.3e} ({name} {pres:.3e}) rel.err {err:.3e}")
        assert res <= pres + RES_TOL, (name, res, pres)
        assert err <= SOL_TOL, (name, err)


@pytest.mark.parametrize("case", ["dense_fu_nx130", "dense_fu_odd_nx", "dense_fu_stages_differ", "dense_fu_final_eq",
                                  "state_cols_some_stages", "nine_cols_nx130"])
def test_stage_blocks_are_symmetric_and_the_dense_form_s(case):
    """V_k bit-for-bit equal to its transpose for every k; equal to the dense form's V_k to 1e-10 of its largest entry."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    S, D = _split(MIN_ENTRIES[case]), ipmatrix.IpLQDOCP()
    _solve(S, prog, st), _solve(D, prog, st)
    for k in range(len(S.debug(20))):
        vs, vd = S.stage_block(k), D.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vd).max() <= 1e-10 * np.abs(vd).max(), (k, np.abs(vs - vd).max(), np.abs(vd).max())


def test_heavy_columns_are_reproducible_and_take_new_values():
    """Two factor + step rounds: the same bits.  update() with new values on the same pattern: the bits of a fresh handle
    (the scatter refills D_k; what it does not write stays zero)."""
    prog = CASES["state_cols_some_stages"]()
    st = problems.ip_state(prog, 3, 1.0)
    M = _split()
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
    N = _split()
    N.init(prog2)
    N.factor(prog2, st[0], st[1])
    d2 = new_d(prog)
    N.step(prog2, *st, *d2)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))
    assert not np.array_equal(d1[0], outs[0][0])


def test_a_threshold_nothing_reaches_changes_no_bit():
    """A threshold above every column's count: the launches of min_entries = 0, so its bits - the step and every V_k."""
    prog = CASES["state_cols_first_mid_last"]()
    st = problems.ip_state(prog, 3, 1.0)
    A, B = _split(0), _split(41)  # (a full column has 40 entries)
    outs = []
    for M in (A, B):
        M.init(prog)
        M.factor(prog, st[0], st[1])
        d = new_d(prog)
        M.step(prog, *st, *d)
        outs.append(d)
    assert B.dense_columns() == [[] for _ in prog.nu]
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert all(np.array_equal(A.stage_block(k), B.stage_block(k)) for k in range(len(prog.nx)))


def test_mehrotra_with_heavy_columns():
    """The device-resident interior-point loop: the iteration count of the dense form and of the reference's
    Hqp_IpsMehrotra on its own Hqp_IpLQDOCP (4, result 0, checked on the CPU when the case was written), the same point
    to 1e-8."""
    from oracle import refapi
    prog = problems.sparse_docp(8, 60, 4, band=5, x_bounds=6, fu_nnz=BIG, seed=13)
    S, D = _split(), ipmatrix.IpLQDOCP()
    S.init(prog), D.init(prog)
    assert all(set(range(60, 64)) <= set(h) for h in S.dense_columns())
    xs, ys, zs, ws, infs = S.mehrotra(prog)
    xd, yd, zd, wd, infd = D.mehrotra(prog)
    print("iterations split / dense:", infs["iters"], infd["iters"])
    assert infs["result"] == infd["result"] == 0 and infs["iters"] == infd["iters"], (infs, infd)
    assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()
    if refapi.host_available("ref"):
        ref = refapi.ip_solve(prog, "Mehrotra", "LQDOCP")
        print("iterations of the reference:", ref["iters"])
        assert ref["result"] == 0 and infs["iters"] == ref["iters"], (infs["iters"], ref["iters"])
        assert np.abs(xs - ref["x"]).max() <= 1e-8 * max(1.0, np.abs(ref["x"]).max()), np.abs(xs - ref["x"]).max()


def test_heavy_columns_at_2000_states_beat_both_forms():
    """nx = 2000, nu = 20 dense control columns, K = 8, band 5 on three handles - dense, sparse as it was (min_entries = 0)
    and sparse with the library's threshold (-1: the 20 control columns are D_k, the thin products take their cut-in-k
    form).  The split handle meets the bar against the dense one, and its hqpkkt_stats.ms_factor of a replayed
    factorisation - the three handles alternating, best of three each - is below both others, with no further margin:
    both partners are code paths that exist, and a form that beats neither has no reason to.  Measured on one MI355X
    (profiles/r12_dense_columns.txt): split 2.03 ms, dense 5.17, sparse 17.5 - ratios 0.39 and 0.12."""
    prog = problems.sparse_docp(8, 2000, 20, band=5, fu_nnz=BIG, seed=2)
    st = problems.ip_state(prog, 3, 1.0)
    H = {"dense": ipmatrix.IpLQDOCP(), "sparse": _split(0), "split": _split(-1)}
    sol = {name: _solve(M, prog, st) for name, M in H.items()}
    assert H["split"].dense_columns() == [list(range(2000, 2020))] * 8 and H["sparse"].dense_columns() == [[]] * 8
    (d, res), (dd, rd) = sol["split"], sol["dense"]
    err = rel_err(d, dd)
    print(f"res split {res:.3e} dense {rd:.3e} sparse {sol['sparse'][1]:.3e} rel.err {err:.3e}")
    assert res <= rd + RES_TOL, (res, rd)
    assert err <= SOL_TOL, err
    ms = {name: [] for name in H}
    for _ in range(3):
        for name, M in H.items():
            M.factor(prog, st[0], st[1])
            ms[name].append(M.stats()["ms_factor"])
    best = {name: min(t for t in v if t > 0) for name, v in ms.items()}  # (-1: the events gave no time)
    print("ms_factor (best of three): " + " ".join(f"{name} {v:.3f}" for name, v in best.items()) +
          f"; split / dense {best['split'] / best['dense']:.3f} split / sparse {best['split'] / best['sparse']:.3f}; all: {ms}")
    assert best["split"] < best["dense"] and best["split"] < best["sparse"], best
