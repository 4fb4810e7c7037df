"""GPU tests of the wide rows' vector products in the STAGED engine (hqp_amd/csrc/staged_rows.hip.h: k_st_rows_gemv, a
wavefront per wide row of a block E_k, and k_st_rows_gemv_t, a thread per pair of its columns): through the test hook
hqpkkt_debug_rows_gemv entry by entry, and through step / solve / residuum of a handle with dense_rows.

The hook's bars: on integer-valued operands (|values| <= 7) every order of summation is exact, so the result is numpy's
bit for bit; on full-mantissa operands |y - exact| <= 1e-14 sum |e||x| per entry, the project's criterion for the product
hooks, with `exact` summed in numpy.longdouble.  The step's epilogue adds two operations to cdx -
dz = tz - zw cdx, dw = -r3 + cdx -, each rounded once, so the same criterion reads 1e-14 (|tz| + |zw| sum |e||x|) and
1e-14 (|r3| + sum |e||x|) there.  The engine's bars are those of test_gpu_staged_wide_rows.py."""
import numpy as np
import pytest

from common import new_d, rel_err
from model_staged import kkt_residual
from wide_rows_cases import CASES, MIN_ENTRIES, OPTIONS, SMALL
from hqp_amd import ipmatrix, problems

pytestmark = pytest.mark.gpu

COLS = (1, 7, 8, 9, 63, 64, 65, 129, 257, 513)  # a partial 16-byte pair .. one lane trip of 128 doubles .. the unrolled trips
ROWS = (1, 0, 2, 17, 65)                        # (a block without rows between two with rows)
RES_TOL = 1e-10
SOL_TOL = 1e-8
LD = np.longdouble


def _case(first, odd, integer):
    """Five blocks, block i with ROWS[i] rows and COLS[(first + i) % 10] columns, side by side in x like the stages of a
    plan: the first starts at x[odd], every other where the one before ends, the last ends with x.  E: the blocks back to
    back (ld = the columns rounded up to 8) with NaN in every padding column; the rows are a random choice among m."""
    rng = np.random.default_rng(1000 * first + 10 * odd + integer)
    blocks, at, col0 = [], 0, odd
    for i, r in enumerate(ROWS):
        c = COLS[(first + i) % len(COLS)]
        ld = (c + 7) // 8 * 8
        blocks.append((r, c, ld, at, col0))
        at, col0 = at + r * ld + 2 * (i % 2), col0 + c  # (an even gap behind every other block)
    n, R = col0, sum(ROWS)
    m = R + 3

    def draw(k):
        return rng.integers(-7, 8, k).astype(np.float64) if integer else rng.uniform(-1.0, 1.0, k) * 2.0 ** rng.integers(-3, 4, k)

    E = np.full(at + 8, np.nan)
    mats = []
    for (r, c, ld, off, _c0) in blocks:
        A = draw(r * c).reshape(r, c)
        E[off: off + r * ld].reshape(r, ld)[:, :c] = A
        mats.append(A)
    return dict(blocks=blocks, E=E, mats=mats, n=n, m=m, rows=rng.permutation(m)[:R].astype(np.int32), x=draw(n), t=draw(m), tz=draw(m), zw=draw(m), r3=draw(m))


def _expected(k):
    """Per owned entry (exact value, sum of |terms|) of the three products, in longdouble; and numpy's own float64 sums."""
    rows, at = k["rows"], 0
    cdx, cdx_abs, cdx_np = {}, {}, {}
    xc, xc_abs, xc_np = np.zeros(k["n"], LD), np.zeros(k["n"], LD), np.zeros(k["n"])
    owned = np.zeros(k["n"], bool)
    for (r, c, _ld, _off, c0), A in zip(k["blocks"], k["mats"]):
        xs, ri = k["x"][c0: c0 + c], rows[at: at + r]
        for i in range(r):
            cdx[ri[i]] = (A[i].astype(LD) * xs.astype(LD)).sum()
            cdx_abs[ri[i]] = np.abs(A[i].astype(LD) * xs.astype(LD)).sum()
            cdx_np[ri[i]] = float(A[i] @ xs)
        tt = k["t"][ri]
        xc[c0: c0 + c] = (A.astype(LD) * tt.astype(LD)[:, None]).sum(axis=0)
        xc_abs[c0: c0 + c] = np.abs(A.astype(LD) * tt.astype(LD)[:, None]).sum(axis=0)
        xc_np[c0: c0 + c] = A.T @ tt if r else 0.0
        owned[c0: c0 + c] = True
        at += r
    return cdx, cdx_abs, cdx_np, xc, xc_abs, xc_np, owned


@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("first", range(len(COLS)))
@pytest.mark.parametrize("integer", [1, 0])
def test_hook_entry_by_entry(integer, first, odd):
    k = _case(first, odd, integer)
    cdx, cdx_abs, cdx_np, xc, xc_abs, xc_np, owned = _expected(k)
    n, m, rows = k["n"], k["m"], k["rows"]
    mark_m, mark_n = 777.25 + np.arange(m), -333.5 - np.arange(n)
    args = (k["blocks"], k["E"], rows, n, m)

    def twice(form, **kw):
        a, b = ipmatrix.rows_gemv(form, *args, **kw), ipmatrix.rows_gemv(form, *args, **kw)
        for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert np.array_equal(u, v, equal_nan=True), form  # two launches, the same bits
        return a

    # rows form, the residual's epilogue
    y = twice("rows", x=k["x"], y=mark_m)
    rest = np.setdiff1d(np.arange(m), rows)
    assert np.array_equal(y[rest], mark_m[rest])
    for j in rows:
        if integer:
            assert y[j] == cdx_np[j] == float(cdx[j]), (j, y[j], cdx_np[j])
        else:
            assert abs(LD(y[j]) - cdx[j]) <= 1e-14 * cdx_abs[j], (j, y[j], cdx[j], cdx_abs[j])
    # rows form, the step's epilogue
    dz, dw = twice("rows_step", x=k["x"], tz=k["tz"], zw=k["zw"], r3=k["r3"], dz=mark_m, dw=mark_m + 0.5)
    assert np.array_equal(dz[rest], mark_m[rest]) and np.array_equal(dw[rest], mark_m[rest] + 0.5)
    for j in rows:
        tz, zw, r3 = k["tz"][j], k["zw"][j], k["r3"][j]
        if integer:
            assert dz[j] == tz - zw * cdx_np[j] and dw[j] == -1.0 * r3 + cdx_np[j], (j, dz[j], dw[j])
        else:
            assert abs(LD(dz[j]) - (LD(tz) - LD(zw) * cdx[j])) <= 1e-14 * (abs(tz) + abs(zw) * cdx_abs[j]), (j, dz[j])
            assert abs(LD(dw[j]) - (cdx[j] - LD(r3))) <= 1e-14 * (abs(r3) + cdx_abs[j]), (j, dw[j])
    # columns form
    got = twice("cols", t=k["t"], xc=mark_n)
    assert np.array_equal(got[~owned], mark_n[~owned]) and (~owned).sum() == odd
    if integer:
        assert np.array_equal(got[owned], xc_np[owned]) and np.array_equal(xc_np[owned], xc[owned].astype(np.float64))
    else:
        assert (np.abs(got.astype(LD) - xc)[owned] <= 1e-14 * xc_abs[owned]).all(), np.abs(got.astype(LD) - xc)[owned].max()
    # (a block without rows: zeros)
    (_r, c, _ld, _off, c0) = k["blocks"][1]
    assert np.array_equal(got[c0: c0 + c], np.zeros(c))


def _split(case, min_entries=None, **kw):
    return ipmatrix.IpLQDOCP(dense_rows=MIN_ENTRIES[case] if min_entries is None else min_entries, **OPTIONS[case], **kw)


@pytest.mark.parametrize("case", SMALL)
def test_step_solve_and_residual_through_the_blocks(case):
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    H = {"wide": _split(case), "walks": _split(case, 0)}
    sol = {}
    for name, M in H.items():
        M.init(prog)
        M.factor(prog, st[0], st[1])
        d = new_d(prog)
        res = M.solve(prog, *st, *d)
        print(f"{case} {name}: res {res:.3e}")
        assert res <= RES_TOL, (name, res)
        d2 = new_d(prog)
        res2 = M.solve(prog, *st, *d2)
        assert res2 == res and all(np.array_equal(a, b) for a, b in zip(d, d2)), name  # a second solve: the same bits
        sol[name] = d
    assert H["wide"].dense_row_products()["on"] and H["walks"].dense_row_products() == {}
    err = rel_err(sol["wide"], sol["walks"])
    print(f"{case}: rel.err wide / walks {err:.3e}")
    assert err <= SOL_TOL, err
    # the residual of a vector that is not the solution, against the program's own blocks
    rng = np.random.default_rng(17)
    dp = [v + 1e-3 * rng.uniform(-1.0, 1.0, v.size) for v in sol["wide"]]
    model = kkt_residual(prog, st[0], st[1], st[2:], dp)
    for name, M in H.items():
        got = M.residuum(prog, *st, *dp)
        print(f"{case} {name}: residuum {got:.6e} model {model:.6e} rel.diff {abs(got - model) / model:.3e}")
        assert abs(got - model) <= 1e-10 * model, (name, got, model)
    # the launches of the new class: on the wide handle alone
    for name, M in H.items():
        M.set_profile(True)
        d = new_d(prog)
        M.step(prog, *st, *d)
        M.residuum(prog, *st, *d)
        launches = M.profile()["staged_rows_gemv"][1]
        M.set_profile(False)
        print(f"{case} {name}: launches of staged_rows_gemv {launches}")
        assert (launches > 0) if name == "wide" else (launches == 0), (name, launches)
        assert all(np.array_equal(a, b) for a, b in zip(d[2:], _step(M, prog, st)[2:])), name  # (profiled and replayed: the same bits)


def _step(M, prog, st):
    d = new_d(prog)
    M.step(prog, *st, *d)
    return d


@pytest.mark.parametrize("case", ["slab_edges", "banded_profile_form"])
def test_a_threshold_nothing_reaches_solves_with_the_same_bits(case):
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    outs = []
    for M in (ipmatrix.IpLQDOCP(**OPTIONS[case]), _split(case, 10**6)):
        M.init(prog)
        M.factor(prog, st[0], st[1])
        d = new_d(prog)
        res = M.solve(prog, *st, *d)
        assert M.dense_row_products() == {}
        outs.append(d + [np.float64(res), np.float64(M.residuum(prog, *st, *d))])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
