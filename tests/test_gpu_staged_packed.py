"""GPU tests of the packed panels of the profile form (hqpkkt_set_packed_panels): a stage that runs the profile sequence
stores F_k as the rows of every 128-column panel's k-slab range alone, its two large products and the solve's two
products take the panels through a table, and its carried rows come from k_pk_carried.

The bar is the project's own: the solution within 1e-8, relative to the vectors' norms, of the
comparison partner's, and the residuum() of our solution <= the partner's + 1e-10.  Partners: the CPU oracle of the full
system, the dense form and the unpacked profile form of the same library, the reference's own Hqp_IpLQDOCP (live, where
oracle/_ref travelled).  Where no stage carries rows the packed handle runs the unpacked one's launches by the same
lists in the same orders, only from other addresses: its solution is the unpacked one's bit for bit.

The kernels on their own (hqpkkt_debug_dgemm_packed, _gemv_packed, _carried_packed): this file packs, in numpy, by the
layout of include/hqpkkt.h - a hook that packed would index as the kernels do and see nothing.  The packed buffer is NaN
in front of, between and behind the panels and in their padding columns."""
import numpy as np
import pytest

from common import new_d, rel_err
from hqp_amd import ipmatrix, problems
from test_gpu_staged_profile import (BIG, CANARY, CASES, GUARD_COLS, GUARD_ROWS, RANGED, RES_TOL, SOL_TOL, _even, _ints, _operand, _ranges,
                                     _solve, _uniform)

pytestmark = pytest.mark.gpu

ENV = ("HQPKKT_NO_LDSDMA", "HQPKKT_DGEMM_WAVES", "HQPKKT_SK_TABLE", "HQPKKT_DGEMM_FORCE_SPLIT")


def _packed():
    return ipmatrix.IpLQDOCP(a_profile=True, a_packed=True)


def _unpacked():
    return ipmatrix.IpLQDOCP(a_profile=True)


def _bar(res, d, pres, pd, who):
    err = rel_err(d, pd)
    print(f"res {res:.3e} ({who} {pres:.3e}) rel.err {err:.3e}")
    assert res <= pres + RES_TOL, (who, res, pres)
    assert err <= SOL_TOL, (who, err)


# ---- the engine

@pytest.mark.parametrize("case", sorted(CASES))
def test_packed_against_the_partners(case):
    from oracle import oracleapi, refapi
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M, D = _packed(), ipmatrix.IpLQDOCP()
    d, res = _solve(M, prog, st)
    dd, rd = _solve(D, prog, st)
    assert (M.dynamics_entries()[:, 1] == 2).all()
    assert all((p[:, 0] >= 0).all() for p in M.packed_panels())
    assert M.stats()["bytes_panels"] < D.stats()["bytes_panels"]
    O = oracleapi.OracleIpMatrix("SpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    osol, ores = O.solve(*st)
    _bar(res, d, ores, osol, "oracle")
    _bar(res, d, rd, dd, "dense form")
    if refapi.available():
        L = refapi.RefIpMatrix("LQDOCP")
        L.init(prog)
        L.factor(st[0], st[1])
        lsol, lres = L.solve(*st)
        _bar(res, d, lres, lsol, "reference")


def test_packed_is_the_unpacked_profile_form_bit_for_bit_without_carried_rows():
    prog = CASES["band5_nx300"]()
    st = problems.ip_state(prog, 3, 1.0)
    M, U = _packed(), _unpacked()
    dm, rm = _solve(M, prog, st)
    du, ru = _solve(U, prog, st)
    assert (M.dynamics_entries()[:, 1] == 2).all() and (U.dynamics_entries()[:, 1] == 2).all()
    assert (M.stage_ranks()[:, 1] == 0).all() and (U.stage_ranks()[:, 1] == 0).all()
    assert M.stats()["bytes_panels"] < U.stats()["bytes_panels"]
    assert all(np.array_equal(a, b) for a, b in zip(dm, du)) and rm == ru
    for k in range(len(M.debug(20))):
        assert np.array_equal(M.stage_block(k), U.stage_block(k)), k


@pytest.mark.parametrize("case", ["final_eq_carried", "path_eq_final_xb"])
def test_packed_with_carried_rows_against_the_unpacked_profile_form(case):
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M, U = _packed(), _unpacked()
    dm, rm = _solve(M, prog, st)
    du, ru = _solve(U, prog, st)
    assert (M.stage_ranks()[:, 1] > 0).any()  # (k_pk_carried ran)
    assert np.array_equal(M.stage_ranks(), U.stage_ranks())
    _bar(rm, dm, ru, du, "unpacked profile form")


@pytest.mark.parametrize("case", ["final_eq_carried", "dense_control_panel"])
def test_stage_blocks_are_symmetric_and_the_unpacked_profile_form_s(case):
    prog = CASES[case]()
    st = problems.ip_state(prog, 4, 1.0)
    M, U = _packed(), _unpacked()
    _solve(M, prog, st), _solve(U, prog, st)
    for k in range(len(M.debug(20))):
        vs, vu = M.stage_block(k), U.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vu).max() <= 1e-10 * np.abs(vu).max(), (k, np.abs(vs - vu).max(), np.abs(vu).max())


def test_packed_is_reproducible_and_takes_new_values():
    prog = problems.sparse_docp(5, 300, 6, band=5, final_eq=3, seed=21)
    st = problems.ip_state(prog, 8, 1.0)
    M = _packed()
    M.init(prog)
    assert (M.dynamics_entries()[:, 1] == 2).all() and all((p[:, 0] >= 0).all() for p in M.packed_panels())
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
    N = _packed()
    N.init(prog2)
    N.factor(prog2, st[0], st[1])
    d2 = new_d(prog)
    N.step(prog2, *st, *d2)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))
    assert not np.array_equal(d1[0], outs[0][0])


@pytest.mark.parametrize("case", ["dense_F", "two_panels_no_saving", "one_panel"])
def test_stages_without_a_saving_give_the_dense_form_s_bits(case):
    prog = {"dense_F": lambda: problems.sparse_docp(3, 300, 4, dense=True, seed=37),
            "two_panels_no_saving": lambda: problems.sparse_docp(4, 200, 3, band=128, seed=38),
            "one_panel": lambda: problems.sparse_docp(4, 120, 3, band=5, seed=38)}[case]()
    st = problems.ip_state(prog, 4, 1.0)
    M, D = _packed(), ipmatrix.IpLQDOCP()
    dm, rm = _solve(M, prog, st)
    dd, rd = _solve(D, prog, st)
    assert (M.dynamics_entries()[:, 1] == 0).all() and all((p == (-1, 0)).all() for p in M.packed_panels())
    assert M.stats()["bytes_panels"] == D.stats()["bytes_panels"]
    assert all(np.array_equal(a, b) for a, b in zip(dm, dd)) and rm == rd


def test_mehrotra_on_packed_panels():
    prog = problems.sparse_docp(5, 300, 4, band=5, x_bounds=6, seed=13)
    S, D = _packed(), ipmatrix.IpLQDOCP()
    S.init(prog), D.init(prog)
    assert (S.dynamics_entries()[:, 1] == 2).all()
    xs, ys, zs, ws, infs = S.mehrotra(prog)
    xd, yd, zd, wd, infd = D.mehrotra(prog)
    print("iterations packed / dense:", infs["iters"], infd["iters"])
    assert infs["result"] == infd["result"] == 0 and infs["iters"] == infd["iters"], (infs, infd)
    assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()


# ---- the kernels on their own

GAP = 10  # doubles of NaN in front of every panel and behind the last (even: a panel starts on a 16-byte boundary)


def _pack(blk, kr):
    """The K x W block `blk` as packed panels: panel p holds the rows [16 lo, min(16 hi, K)) of its columns, row-major
    with leading dimension 128, the last panel up8 of its columns; NaN between the panels and in the padding columns.  An
    empty panel takes no room.  Returns the flat buffer and (offset, ld) per panel."""
    K, W = blk.shape
    np_ = (W + 127) // 128
    parts, pan, off = [], [], 0
    for p, (lo, hi) in enumerate(kr):
        w = min(128, W - 128 * p)
        ld = 128 if p + 1 < np_ else (w + 7) // 8 * 8
        rows = min(16 * hi, K) - 16 * lo
        parts.append(np.full(GAP, np.nan))
        off += GAP
        pan.append((off, ld))
        body = np.full((rows, ld), np.nan)
        body[:, :w] = blk[16 * lo: 16 * lo + rows, 128 * p: 128 * p + w]
        parts.append(body.ravel())
        off += rows * ld
    parts.append(np.full(GAP, np.nan))
    return np.concatenate(parts), np.array(pan, dtype=np.int64)


def _ranged_block(rng, K, W, kr, values):
    """values inside the panels' ranges, zeros outside (what no result may depend on)"""
    blk = values(rng, (K, W))
    inside = np.zeros((K, W), bool)
    for p, (lo, hi) in enumerate(kr):
        inside[16 * lo: 16 * hi, 128 * p: 128 * p + 128] = True
    return np.where(inside, blk, 0.0)


def _launch_packed(M, N, K, by, lower, odd, values, seed):
    rng = np.random.default_rng([seed, M, N, K, by, lower, odd])
    kr = _ranges(rng, ((M if by == 2 else N) + 127) // 128, (K + 15) // 16)
    a_col0, b_col0 = (3, 5) if odd else (2, 4)
    if by == 2:
        a = _ranged_block(rng, K, M, kr, values)
        B, b = _operand(rng, K, N, b_col0, odd, values)
        pk, pan = _pack(a, kr)
        other = dict(B=B, b_col0=b_col0)
    else:
        A, a = _operand(rng, K, M, a_col0, odd, values)
        b = _ranged_block(rng, K, N, kr, values)
        pk, pan = _pack(b, kr)
        other = dict(A=A, a_col0=a_col0)
    r0, c0 = GUARD_ROWS + 1, 5 if odd else 4
    ldc = _even(c0 + N + GUARD_COLS + 1) + (1 if odd else 0)
    Cb = np.empty((r0 + M + GUARD_ROWS, ldc))
    Cb.view(np.uint64)[...] = CANARY
    rows, cols = slice(r0, r0 + M), slice(c0, c0 + N)
    want = Cb.copy()
    ref = a.T @ b
    if lower:
        ii, jj = np.indices((M, N), sparse=True)
        low = np.broadcast_to(ii >= jj, (M, N))
        want[rows, cols][low] = ref[low]
    else:
        want[rows, cols] = ref
    ran = ipmatrix.dgemm_packed(M, N, K, Cb, r0, c0, pk, pan, kr, by, lower=bool(lower), **other)
    print("%d x %d x %d by %d lower %d odd %d: form %s, %d tiles, LDS-DMA %d; ranges %s panels %s" % (
        M, N, K, by, lower, odd, ran[0], ran[1], ran[3], kr.tolist(), pan.tolist()))
    assert ran[0] == "profile"
    return Cb, want, (rows, cols), (a, b), ran


def _exact(got, want, rows, cols):
    g, w = got.view(np.uint64), want.view(np.uint64)
    touched = np.argwhere((w == CANARY) & (g != CANARY))
    assert touched.size == 0, "%d elements that must not be written were, the first at buffer row, column %s" % (len(touched), touched[:8].tolist())
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%d wrong entries, the first at block row, column %s (got %r, exact %r)" % (
        len(bad), (bad[:8] - [rows.start, cols.start]).tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("M,N,K,by,lower,odd", RANGED)
def test_packed_product_every_entry_exact_and_nothing_else_written(M, N, K, by, lower, odd, monkeypatch):
    """Integer operands: C equals numpy's product bit for bit and no canary is touched.  The last panel is ragged (49 and
    11 columns: ld 56 and 16), the last slab partial (12 and 5 rows); one panel runs to it, one is empty, one holds one
    slab.  odd: the other operand at an odd column with an odd leading dimension - the launch stages through registers."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    got, want, (rows, cols), _, ran = _launch_packed(M, N, K, by, lower, odd, _ints, 0)
    assert ran[3] == (not odd)
    _exact(got, want, rows, cols)


def test_packed_product_staged_through_registers(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("HQPKKT_NO_LDSDMA", "1")
    for (M, N, K, by, lower) in [(517, 523, 517, 1, 0), (523, 523, 517, 2, 1)]:
        got, want, (rows, cols), _, ran = _launch_packed(M, N, K, by, lower, 0, _ints, 2)
        assert not ran[3]
        _exact(got, want, rows, cols)


def test_packed_product_within_the_rounding_bound(monkeypatch):
    """Full-mantissa operands: |C - ref| <= 1e-14 sum |a||b| for every entry, the reference a longdouble product."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    got, want, (rows, cols), (a, b), _ = _launch_packed(517, 523, 517, 1, 0, 0, _uniform, 1)
    guard = want.view(np.uint64) == CANARY
    guard[rows, cols] = False
    assert np.array_equal(got.view(np.uint64)[guard], want.view(np.uint64)[guard])
    ref = a.astype(np.longdouble).T @ b.astype(np.longdouble)
    bound = 1e-14 * (np.abs(a).T @ np.abs(b))
    err = np.abs(got[rows, cols].astype(np.longdouble) - ref)
    assert not np.isnan(got[rows, cols]).any()
    assert (err <= bound).all(), float((err - bound).max())


def test_packed_hooks_refuse_panels_outside_the_buffer():
    rng = np.random.default_rng(3)
    K, N = 300, 305
    kr = _ranges(rng, 3, 19)
    pk, pan = _pack(_ranged_block(rng, K, N, kr, _uniform), kr)
    x = np.zeros(K)
    for bad in ((0, 0, pk.size), (2, 1, 8), (0, 0, 11)):  # behind the buffer; an ld below the panel's columns; an odd offset
        q = pan.copy()
        q[bad[0], bad[1]] = bad[2]
        with pytest.raises(ipmatrix.KktError) as err:
            ipmatrix.gemv_packed(pk, q, kr, x, K, N)
        assert err.value.code == ipmatrix._lib.E_RANGE


@pytest.mark.parametrize("K,N", [(300, 305), (517, 523)])
@pytest.mark.parametrize("rows_form", [False, True])
def test_gemv_packed(K, N, rows_form):
    """Both products of the solve on packed panels: |y - ref| <= 1e-14 sum |a||x| against a longdouble product, no NaN in
    y, run-to-run identical, and the bits of hqpkkt_debug_gemv_profile on the same data unpacked.  The hook reports a
    write behind y."""
    rng = np.random.default_rng([7, K, N, rows_form])
    kr = _ranges(rng, (N + 127) // 128, (K + 15) // 16)
    a = _ranged_block(rng, K, N, kr, _uniform)
    pk, pan = _pack(a, kr)
    x = rng.uniform(-1.0, 1.0, N if rows_form else K)
    add = rng.uniform(-1.0, 1.0, K if rows_form else N)
    alpha = -1.0 if rows_form else 1.0
    y = ipmatrix.gemv_packed(pk, pan, kr, x, K, N, add=add, alpha=alpha, rows_form=rows_form)
    al = a.astype(np.longdouble)
    prod = al @ x if rows_form else al.T @ x
    bound = 1e-14 * (np.abs(a) @ np.abs(x) if rows_form else np.abs(a).T @ np.abs(x))
    err = np.abs(y.astype(np.longdouble) - (add + alpha * prod))
    print("rows_form %d %d x %d ranges %s: max err %.3e (bound at it %.3e)" % (rows_form, K, N, kr.tolist(), float(err.max()), float(bound[np.argmax(err)])))
    assert not np.isnan(y).any()
    assert (err <= bound).all(), float((err - bound).max())
    assert np.array_equal(y, ipmatrix.gemv_packed(pk, pan, kr, x, K, N, add=add, alpha=alpha, rows_form=rows_form))  # run-to-run
    A = np.full((K + 1, (N + 7) // 8 * 8), np.nan)  # the same data as a dense block, NaN outside the ranges
    for p, (lo, hi) in enumerate(kr):
        A[16 * lo: min(16 * hi, K), 128 * p: min(128 * p + 128, N)] = a[16 * lo: 16 * hi, 128 * p: 128 * p + 128]
    assert np.array_equal(y, ipmatrix.gemv_profile(A, kr, x, add=add, alpha=alpha, rows_form=rows_form, K=K, N=N))


def _launch_carried(K, N, R, values, seed):
    rng = np.random.default_rng([seed, K, N, R])
    kr = _ranges(rng, (N + 127) // 128, (K + 15) // 16)
    f = _ranged_block(rng, K, N, kr, values)
    pk, pan = _pack(f, kr)
    BT = np.full((K, (R + 7) // 8 * 8 + 8), np.nan)
    bt = values(rng, (K, R))
    BT[:, :R] = bt
    r0, c0 = GUARD_ROWS, 3
    Cb = np.empty((r0 + R + GUARD_ROWS, c0 + N + GUARD_COLS))
    Cb.view(np.uint64)[...] = CANARY
    want = Cb.copy()
    rows, cols = slice(r0, r0 + R), slice(c0, c0 + N)
    want[rows, cols] = bt.T @ f
    got = ipmatrix.carried_packed(BT, R, pk, pan, kr, K, N, Cb.copy(), r0, c0)
    again = ipmatrix.carried_packed(BT, R, pk, pan, kr, K, N, Cb.copy(), r0, c0)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))  # run-to-run
    return got, want, (rows, cols), (bt, f)


@pytest.mark.parametrize("K,N", [(300, 305), (517, 523)])
@pytest.mark.parametrize("R", [1, 5, 256])
def test_carried_packed(K, N, R):
    """k_pk_carried: exact on integer operands with every canary intact; full-mantissa operands within 1e-14 sum |b||f|
    of a longdouble product."""
    got, want, (rows, cols), _ = _launch_carried(K, N, R, _ints, 0)
    _exact(got, want, rows, cols)
    got, want, (rows, cols), (bt, f) = _launch_carried(K, N, R, _uniform, 1)
    guard = want.view(np.uint64) == CANARY
    assert np.array_equal(got.view(np.uint64)[guard], want.view(np.uint64)[guard])
    ref = bt.astype(np.longdouble).T @ f.astype(np.longdouble)
    bound = 1e-14 * (np.abs(bt).T @ np.abs(f))
    err = np.abs(got[rows, cols].astype(np.longdouble) - ref)
    assert not np.isnan(got[rows, cols]).any()
    assert (err <= bound).all(), float((err - bound).max())


# ---- the wide case

def test_packed_at_2000_states_against_the_unpacked_profile_form():
    """nx = 2000, nu = 20 dense control columns, K = 8, band 50.  The bar against the unpacked profile handle - the parent
    code path; the F arena smaller by exactly 8 x (32 384 000 - 5 530 624) bytes; hqpkkt_stats.ms_factor of a replayed
    factorisation, best of three, the two handles taking turns: packed <= 1.05 x unpacked (a little over twice the
    0.3 - 2 % spread of repeated readings of these sweeps)."""
    prog = problems.sparse_docp(8, 2000, 20, band=50, fu_nnz=BIG, low_rank=False, seed=2)
    st = problems.ip_state(prog, 5, 1.0)
    hs = {"packed": _packed(), "unpacked": _unpacked()}
    sol = {}
    for form, M in hs.items():
        sol[form] = _solve(M, prog, st)
        M.factor(prog, st[0], st[1])  # (warm-up of the replayed sequence)
    assert all((h.dynamics_entries()[:, 1] == 2).all() for h in hs.values())
    _bar(sol["packed"][1], sol["packed"][0], sol["unpacked"][1], sol["unpacked"][0], "unpacked profile form")
    assert hs["unpacked"].stats()["bytes_panels"] - hs["packed"].stats()["bytes_panels"] == 8 * (32384000 - 5530624)
    ms, ms_solve = {form: [] for form in hs}, {}
    for _ in range(3):
        for form, M in hs.items():
            M.factor(prog, st[0], st[1])
            ms[form].append(M.stats()["ms_factor"])
    for form, M in hs.items():
        M.solve(prog, *st, *new_d(prog))
        ms_solve[form] = M.stats()["ms_solve"]
    best = {form: min(t for t in v if t > 0) for form, v in ms.items()}  # (a reading without an event time is -1)
    print("ms_factor, best of three: packed %.3f unpacked %.3f; ms_solve: packed %.3f unpacked %.3f" % (
        best["packed"], best["unpacked"], ms_solve["packed"], ms_solve["unpacked"]))
    assert best["packed"] <= 1.05 * best["unpacked"], best
