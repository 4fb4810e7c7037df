"""GPU tests of the wide rows of C in the STAGED engine (hqpkkt_set_dense_rows; hqp_amd/csrc/staged_rows.hip.h,
st_add_h_wide): the rows of the inequality block with many entries leave the H term lists and add their share of
C'(Z/W)C as one thin-K fp64 MFMA product per stage.

The bars are the sibling tests' own (test_gpu_staged_dense_columns.py): the solution within 1e-8, relative to the vectors'
norms, of the comparison partner's, and the residuum() of our solution <= the partner's + 1e-10.  Partners: the CPU oracle
of the full system, the reference's own Hqp_IpLQDOCP (live, oracle/_ref), the same library with dense_rows = 0."""
import numpy as np
import pytest

from common import new_d, rel_err
from wide_rows_cases import CASES, MIN_ENTRIES, OPTIONS, expected_wide
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


def _split(case, min_entries=None):
    return ipmatrix.IpLQDOCP(dense_rows=MIN_ENTRIES[case] if min_entries is None else min_entries, **OPTIONS[case])


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_rows_against_the_partners(case):
    """G1: factor + solve on ip_state vectors (z and w each over two decades); the plan's wide rows are what numpy counts."""
    from oracle import oracleapi, refapi
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M = _split(case)
    d, res = _solve(M, prog, st)
    wide = expected_wide(prog, MIN_ENTRIES[case])
    assert M.dense_rows() == wide and any(wide)
    O = oracleapi.OracleIpMatrix("SpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    partners = {"oracle": O.solve(*st), "dense_rows = 0": _solve(_split(case, 0), prog, st)}
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


@pytest.mark.parametrize("case", ["one_row_nx70", "slab_edges", "terminal_set", "every_row_wide", "stages_differ", "with_carried_rows",
                                  "banded_sparse_form", "banded_packed_panels"])
def test_stage_blocks_are_symmetric_and_the_term_lists(case):
    """G2: V_k bit-for-bit equal to its transpose for every k; equal to V_k of the handle with dense_rows = 0 to 1e-10 of
    its largest entry."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    S, D = _split(case), _split(case, 0)
    _solve(S, prog, st), _solve(D, prog, st)
    for k in range(len(S.debug(20))):
        vs, vd = S.stage_block(k), D.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vd).max() <= 1e-10 * np.abs(vd).max(), (k, np.abs(vs - vd).max(), np.abs(vd).max())


@pytest.mark.parametrize("case", ["slab_edges", "banded_sparse_form"])
def test_wide_rows_are_reproducible_and_take_new_values(case):
    """G3: two factor + step rounds give the same bits.  update() with other values in the wide rows on the same pattern:
    the bits of a fresh handle (the scatter refills E_k; what it does not write stays zero)."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M = _split(case)
    M.init(prog)
    outs = []
    for _ in range(2):
        M.factor(prog, st[0], st[1])
        d = new_d(prog)
        M.step(prog, *st, *d)
        outs.append(d + [M.stage_block(k) for k in range(len(prog.nx))])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    p, i, x = prog.C
    rng = np.random.default_rng(5)
    wide = np.repeat(np.diff(p) >= MIN_ENTRIES[case], np.diff(p))
    x2 = np.where(wide, x * rng.uniform(0.5, 1.5, x.size), x)
    prog2 = problems.Program(prog.n, prog.me, prog.m, prog.Q, prog.A, (p, i, x2), c=prog.c, b=prog.b, d=prog.d)
    M.update(prog2)
    M.factor(prog2, st[0], st[1])
    d1 = new_d(prog)
    M.step(prog2, *st, *d1)
    N = _split(case)
    N.init(prog2)
    N.factor(prog2, st[0], st[1])
    d2 = new_d(prog)
    N.step(prog2, *st, *d2)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))
    assert all(np.array_equal(M.stage_block(k), N.stage_block(k)) for k in range(len(prog.nx)))
    assert not np.array_equal(d1[0], outs[0][0])


@pytest.mark.parametrize("case", ["slab_edges", "banded_profile_form"])
def test_a_threshold_nothing_reaches_changes_no_bit(case):
    """G4: a threshold above every row's count against a handle that never asked: the same launches, so the same bits -
    the step and every V_k."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    A, B = ipmatrix.IpLQDOCP(**OPTIONS[case]), _split(case, 10**6)
    outs = []
    for M in (A, B):
        M.init(prog)
        M.factor(prog, st[0], st[1])
        d = new_d(prog)
        M.step(prog, *st, *d)
        outs.append(d)
    assert B.dense_rows() == [[] for _ in prog.nx]
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    assert all(np.array_equal(A.stage_block(k), B.stage_block(k)) for k in range(len(prog.nx)))


@pytest.mark.parametrize("case", ["slab_edges", "terminal_set"])
def test_mehrotra_with_wide_rows(case):
    """G5: the device-resident interior-point loop: the iteration count of the handle with dense_rows = 0 and of the
    reference's Hqp_IpsMehrotra on its own Hqp_IpLQDOCP (3, result 0, on the CPU when the cases were written), the same
    point to 1e-8."""
    from oracle import refapi
    prog = CASES[case]()
    S, D = _split(case), _split(case, 0)
    S.init(prog), D.init(prog)
    assert any(S.dense_rows())
    xs, ys, zs, ws, infs = S.mehrotra(prog)
    xd, yd, zd, wd, infd = D.mehrotra(prog)
    print("iterations split / term lists:", infs["iters"], infd["iters"])
    assert infs["result"] == infd["result"] == 0 and infs["iters"] == infd["iters"], (infs, infd)
    assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()
    if refapi.host_available("ref"):
        ref = refapi.ip_solve(prog, "Mehrotra", "LQDOCP")
        print("iterations of the reference:", ref["iters"])
        assert ref["result"] == 0 and infs["iters"] == ref["iters"], (infs["iters"], ref["iters"])
        assert np.abs(xs - ref["x"]).max() <= 1e-8 * max(1.0, np.abs(ref["x"]).max()), np.abs(xs - ref["x"]).max()


def test_wide_rows_at_2000_states_are_not_slower():
    """G7: 2000 states, 8 controls, K = 4, a band of 5, diagonal Q, 16 inequality rows over all states in each of the
    stages 0 .. 3 on two handles, dense_rows = 32 and 0 (64e6 terms per stage in the lists).  The split handle meets the
    bar against the other, and its hqpkkt_stats.ms_factor of a replayed factorisation - the handles taking turns, best of
    three each - is not above the other's.  No ratio is fixed in advance; the ratio itself is not measured yet."""
    prog = problems.with_wide_rows(problems.sparse_docp(4, 2000, 8, band=5, seed=2, low_rank=False), [(k, 2000, False) for k in range(4) for _ in range(16)])
    st = problems.ip_state(prog, 3, 1.0)
    H = {"split": ipmatrix.IpLQDOCP(dense_rows=32), "lists": ipmatrix.IpLQDOCP()}
    sol = {name: _solve(M, prog, st) for name, M in H.items()}
    assert [len(r) for r in H["split"].dense_rows()] == [16, 16, 16, 16, 0]
    (d, res), (dd, rd) = sol["split"], sol["lists"]
    err = rel_err(d, dd)
    print(f"res split {res:.3e} lists {rd:.3e} rel.err {err:.3e}")
    assert res <= rd + RES_TOL, (res, rd)
    assert err <= SOL_TOL, err
    ms = {name: [] for name in H}
    for _ in range(3):
        for name, M in H.items():
            M.factor(prog, st[0], st[1])
            ms[name].append(M.stats()["ms_factor"])
    best = {name: min(t for t in v if t > 0) for name, v in ms.items()}  # (-1: the events gave no time)
    print("ms_factor (best of three): " + " ".join(f"{name} {v:.3f}" for name, v in best.items()) + f"; split / lists {best['split'] / best['lists']:.3f}; all: {ms}")
    assert best["split"] <= best["lists"], best
