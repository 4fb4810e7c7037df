"""GPU tests of the profile form of the STAGED engine's stage products (hqpkkt_set_dynamics_form(HQPKKT_DYN_PROFILE)): the
two large MFMA products and the solve's two products with F_k over the k-slabs that hold each 128-column panel's stored
entries (staged_stage_profile, staged_profile.hip.h), on multistage QPs with banded dynamics (problems.sparse_docp).

The bar is the project's own: the solution within 1e-8, relative to the vectors' norms, of the
comparison partner's, and the residuum() of our solution <= the partner's + 1e-10.  Partners: the CPU oracle of the full
system, the dense form of the same library, the reference's own Hqp_IpLQDOCP (live, where oracle/_ref travelled).

The kernels on their own: hqpkkt_debug_dgemm_full with krange (the product by a profile list, entry by entry and bit
for bit on integer operands that are NaN outside their panels' ranges) and hqpkkt_debug_gemv_profile (both kernels of the
solve against a longdouble product)."""
import numpy as np
import pytest

from common import new_d, rel_err
from hqp_amd import ipmatrix, problems

pytestmark = pytest.mark.gpu

RES_TOL = 1e-10
SOL_TOL = 1e-8
BIG = 10**6

# (every case is factored by the CPU oracle with a residual of 1e-11 or less: checked on the CPU when the cases were written)
CASES = {
    "band5_nx300": lambda: problems.sparse_docp(5, 300, 5, band=5, seed=31),
    "band20_odd_nx517": lambda: problems.sparse_docp(4, 517, 6, band=20, seed=32),
    "stages_differ": lambda: problems.sparse_docp(4, [400, 400, 330, 520, 460], [4, 2, 6, 3], band=8, seed=33),
    "final_eq_carried": lambda: problems.sparse_docp(6, 300, 8, band=5, final_eq=4, seed=3),
    "path_eq_xb_free_x0": lambda: problems.sparse_docp(4, 300, 4, band=4, path_eq=2, x_bounds=5, x0_fixed=False, seed=35),
    "path_eq_final_xb": lambda: problems.sparse_docp(5, 320, 6, band=5, path_eq=1, path_eq_every=2, final_eq=3, x_bounds=4, seed=39),
    "dense_control_panel": lambda: problems.sparse_docp(5, 320, 12, band=5, fu_nnz=BIG, seed=36),
}


def _solve(M, prog, st):
    M.init(prog)
    M.factor(prog, st[0], st[1])
    d = new_d(prog)
    res = M.solve(prog, *st, *d)
    return d, res


def _profile():
    return ipmatrix.IpLQDOCP(a_profile=True)


@pytest.mark.parametrize("case", sorted(CASES))
def test_profile_form_against_the_partners(case):
    from oracle import oracleapi, refapi
    prog = CASES[case]()
    st = problems.ip_state(prog, 3, 1.0)
    M, D = _profile(), ipmatrix.IpLQDOCP()
    d, res = _solve(M, prog, st)
    D.init(prog)
    assert (M.dynamics_entries()[:, 1] == 2).all()
    rng = np.concatenate(M.profile_ranges())
    share = (rng[:, 1] - rng[:, 0]).sum() / sum(len(r) * ((n + 15) // 16) for r, n in zip(M.profile_ranges(), prog.nx[1:]))
    assert 0.2 < share < 0.8, share  # (the lists differ from whole tiles)
    assert M.stats()["bytes_panels"] == D.stats()["bytes_panels"]
    O = oracleapi.OracleIpMatrix("SpBKP")
    O.init(prog)
    O.factor(st[0], st[1])
    osol, ores = O.solve(*st)
    err = rel_err(d, osol)
    print(f"{case}: slab share {share:.2f} res {res:.3e} (oracle {ores:.3e}) rel.err {err:.3e}")
    assert res <= ores + RES_TOL, (res, ores)
    assert err <= SOL_TOL, err
    D.factor(prog, st[0], st[1])
    dd = new_d(prog)
    rd = D.solve(prog, *st, *dd)
    err = rel_err(d, dd)
    print(f"{case}: res {res:.3e} (dense form {rd:.3e}) rel.err {err:.3e}")
    assert res <= rd + RES_TOL, (res, rd)
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


@pytest.mark.parametrize("case", ["dense_F", "two_panels_no_saving", "one_panel"])
def test_stages_without_a_saving_give_the_dense_form_s_bits(case):
    """Every range full (dense F_k; two panels under a band as wide as a panel), or one panel: no stage runs the profile
    sequence, and factor + solve give the dense form's solution bit for bit."""
    prog = {"dense_F": lambda: problems.sparse_docp(3, 300, 4, dense=True, seed=37),
            "two_panels_no_saving": lambda: problems.sparse_docp(4, 200, 3, band=128, seed=38),
            "one_panel": lambda: problems.sparse_docp(4, 120, 3, band=5, seed=38)}[case]()
    st = problems.ip_state(prog, 4, 1.0)
    M, D = _profile(), ipmatrix.IpLQDOCP()
    dm, rm = _solve(M, prog, st)
    dd, rd = _solve(D, prog, st)
    assert (M.dynamics_entries()[:, 1] == 0).all() and len(M.profile_ranges()) == len(prog.nu)
    assert all(np.array_equal(a, b) for a, b in zip(dm, dd)) and rm == rd


def test_two_narrow_panels_with_a_saving():
    """200 states under a band of 5: two panels whose ranges (9 and 6 of 13 slabs) are shorter than all slabs, so every
    stage runs the profile sequence; its tiles are cut where the dense form's are not, so the bar is the project's, not
    bit identity."""
    prog = problems.sparse_docp(4, 200, 3, band=5, seed=38)
    st = problems.ip_state(prog, 4, 1.0)
    M, D = _profile(), ipmatrix.IpLQDOCP()
    dm, rm = _solve(M, prog, st)
    dd, rd = _solve(D, prog, st)
    assert (M.dynamics_entries()[:, 1] == 2).all()
    assert rm <= rd + RES_TOL and rel_err(dm, dd) <= SOL_TOL, (rm, rd, rel_err(dm, dd))


@pytest.mark.parametrize("case", ["band5_nx300", "stages_differ", "final_eq_carried", "dense_control_panel"])
def test_stage_blocks_are_symmetric_and_the_dense_form_s(case):
    """V_k bit-for-bit equal to its transpose for every k; equal to the dense form's V_k to 1e-10 of its largest entry."""
    prog = CASES[case]()
    st = problems.ip_state(prog, 4, 1.0)
    M, D = _profile(), ipmatrix.IpLQDOCP()
    _solve(M, prog, st), _solve(D, prog, st)
    for k in range(len(M.debug(20))):
        vs, vd = M.stage_block(k), D.stage_block(k)
        assert np.array_equal(vs, vs.T), k
        assert np.abs(vs - vd).max() <= 1e-10 * np.abs(vd).max(), (k, np.abs(vs - vd).max(), np.abs(vd).max())


def test_profile_form_is_reproducible_and_takes_new_values():
    """Two factorisations and solves in a row: the same bits.  set_values with new values on the same pattern: the result
    of a fresh handle, bit for bit."""
    prog = problems.sparse_docp(5, 300, 6, band=5, final_eq=3, seed=21)
    st = problems.ip_state(prog, 8, 1.0)
    M = _profile()
    M.init(prog)
    assert (M.dynamics_entries()[:, 1] == 2).all()
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
    N = _profile()
    N.init(prog2)
    N.factor(prog2, st[0], st[1])
    d2 = new_d(prog)
    N.step(prog2, *st, *d2)
    assert all(np.array_equal(a, b) for a, b in zip(d1, d2))
    assert not np.array_equal(d1[0], outs[0][0])


def test_mehrotra_on_the_profile_form():
    """The device-resident interior-point loop: the iteration count and the point of the dense form."""
    prog = problems.sparse_docp(5, 300, 4, band=5, x_bounds=6, seed=13)
    S, D = _profile(), ipmatrix.IpLQDOCP()
    S.init(prog), D.init(prog)
    assert (S.dynamics_entries()[:, 1] == 2).all()
    xs, ys, zs, ws, infs = S.mehrotra(prog)
    xd, yd, zd, wd, infd = D.mehrotra(prog)
    print("iterations profile / dense:", infs["iters"], infd["iters"])
    assert infs["result"] == infd["result"] == 0 and infs["iters"] == infd["iters"], (infs, infd)
    assert np.abs(xs - xd).max() <= 1e-8 * max(1.0, np.abs(xd).max()), np.abs(xs - xd).max()


# ---- the product by a profile list, entry by entry (hqpkkt_debug_dgemm_full with krange)

CANARY = np.uint64(0x7FF8C0DE5EEDBEEF)  # a quiet NaN no arithmetic produces
GUARD_ROWS, GUARD_COLS, POISON_ROWS = 2, 3, 16


def _even(x):
    return x + (x & 1)


def _ranges(rng, panels, nslab):
    """One range to the last (partial) slab, one empty panel, one of one slab, the others random."""
    r = np.zeros((panels, 2), dtype=np.int32)
    for p in range(panels):
        lo = int(rng.integers(0, nslab - 2))
        r[p] = lo, int(rng.integers(lo + 2, nslab + 1))
    r[0] = int(rng.integers(1, nslab // 2)), nslab
    r[1] = 5, 5
    r[panels - 1] = nslab // 2, nslab // 2 + 1
    return r


def _operand(rng, k, w, col0, odd_ld, values, ranges=None):
    """k x w values at column col0 of a buffer of k + 16 poison rows + 1 spare row; NaN everywhere else - with `ranges`
    also in the block, outside the k-slabs [lo, hi) of every 128-wide panel.  Returns the buffer and the block with zeros
    for what no result may depend on."""
    ld = _even(col0 + w + 3) + (1 if odd_ld else 0)
    buf = np.full((k + POISON_ROWS + 1, ld), np.nan)
    blk = values(rng, (k, w))
    if ranges is not None:
        inside = np.zeros((k, w), bool)
        for p, (lo, hi) in enumerate(ranges):
            inside[16 * lo: 16 * hi, 128 * p: 128 * p + 128] = True
        buf[:k, col0:col0 + w] = np.where(inside, blk, np.nan)
        blk = np.where(inside, blk, 0.0)
    else:
        buf[:k, col0:col0 + w] = blk
    return buf, blk


def _ints(rng, shape):
    v = rng.integers(1, 2 ** 15, size=shape, endpoint=True) * rng.choice([-1, 1], size=shape)  # (nonzero)
    return v.astype(np.float64)


def _uniform(rng, shape):
    return rng.uniform(-1.0, 1.0, size=shape)


def _launch_ranged(M, N, K, by, lower, odd, values, seed):
    rng = np.random.default_rng([seed, M, N, K, by, lower, odd])
    nslab = (K + 15) // 16
    kr = _ranges(rng, ((M if by == 2 else N) + 127) // 128, nslab)
    a_col0, b_col0 = (3, 5) if odd else (2, 4)
    A, a = _operand(rng, K, M, a_col0, odd, values, kr if by == 2 else None)
    B, b = _operand(rng, K, N, b_col0, odd, values, kr if by == 1 else None)
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
    ran = ipmatrix.dgemm_full(M, N, K, Cb, r0, c0, A=A, a_col0=a_col0, B=B, b_col0=b_col0, lower=bool(lower), krange=kr, krange_by=by)
    print("%d x %d x %d by %d lower %d odd %d: form %s, %d tiles, LDS-DMA %d; ranges %s" % (M, N, K, by, lower, odd, ran[0], ran[1], ran[3], kr.tolist()))
    assert ran[0] == "profile" and ran[3] == (not odd)
    return Cb, want, (rows, cols), (a, b)


RANGED = [(M, N, K, by, lower, odd) for (M, N, K, by, lower) in
          [(300, 305, 300, 1, 0), (300, 305, 300, 2, 0), (305, 305, 300, 2, 1), (517, 523, 517, 1, 0), (517, 523, 517, 2, 0), (523, 523, 517, 2, 1)]
          for odd in (0, 1)]


@pytest.mark.parametrize("M,N,K,by,lower,odd", RANGED)
def test_ranged_product_every_entry_exact_and_nothing_else_written(M, N, K, by, lower, odd, monkeypatch):
    """Integer operands (every sum exact in fp64, whatever its order or cut), the ranged operand NaN outside its ranges
    and nonzero inside, one empty panel and one of one slab: C equals numpy's product with the outside zeroed bit for
    bit, and no canary around C - nor above the diagonal of a lower product - is touched."""
    for name in ("HQPKKT_NO_LDSDMA", "HQPKKT_DGEMM_WAVES", "HQPKKT_SK_TABLE", "HQPKKT_DGEMM_FORCE_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    got, want, (rows, cols), _ = _launch_ranged(M, N, K, by, lower, odd, _ints, 0)
    g, w = got.view(np.uint64), want.view(np.uint64)
    guard = w == CANARY
    touched = np.argwhere(guard & (g != CANARY))
    assert touched.size == 0, "%d elements that must not be written were, the first at buffer row, column %s" % (len(touched), touched[:8].tolist())
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%d wrong entries, the first at block row, column %s (got %r, exact %r)" % (
        len(bad), (bad[:8] - [rows.start, cols.start]).tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def test_ranged_product_within_the_rounding_bound(monkeypatch):
    """Full-mantissa operands: |C - ref| <= 1e-14 sum |a||b| for every entry, the reference a longdouble product."""
    for name in ("HQPKKT_NO_LDSDMA", "HQPKKT_DGEMM_WAVES", "HQPKKT_SK_TABLE", "HQPKKT_DGEMM_FORCE_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    got, want, (rows, cols), (a, b) = _launch_ranged(517, 523, 517, 1, 0, 0, _uniform, 1)
    guard = want.view(np.uint64) == CANARY
    guard[rows, cols] = False
    assert np.array_equal(got.view(np.uint64)[guard], want.view(np.uint64)[guard])
    ref = a.astype(np.longdouble).T @ b.astype(np.longdouble)
    bound = 1e-14 * (np.abs(a).T @ np.abs(b))
    err = np.abs(got[rows, cols].astype(np.longdouble) - ref)
    assert not np.isnan(got[rows, cols]).any()
    assert (err <= bound).all(), float((err - bound).max())


# ---- the solve's two products (hqpkkt_debug_gemv_profile)

@pytest.mark.parametrize("K,N", [(300, 305), (517, 523)])
@pytest.mark.parametrize("rows_form", [False, True])
def test_gemv_profile(K, N, rows_form):
    """A is NaN outside its panels' ranges and in the columns behind N; one panel is empty, one holds one slab, one runs
    to the last (partial) slab - several chunks of the columns form.  |y - ref| <= 1e-14 sum |a||x| against a longdouble
    product with the outside zeroed, no NaN in y; the hook reports a write behind y."""
    rng = np.random.default_rng([7, K, N, rows_form])
    kr = _ranges(rng, (N + 127) // 128, (K + 15) // 16)
    ld = (N + 7) // 8 * 8
    A = np.full((K + 1, ld), np.nan)
    a = np.zeros((K, N))
    for p, (lo, hi) in enumerate(kr):
        blk = rng.uniform(-1.0, 1.0, (K, N))[16 * lo: 16 * hi, 128 * p: 128 * p + 128]
        a[16 * lo: 16 * hi, 128 * p: 128 * p + 128] = blk
        A[16 * lo: min(16 * hi, K), 128 * p: min(128 * p + 128, N)] = blk
    x = rng.uniform(-1.0, 1.0, N if rows_form else K)
    add = rng.uniform(-1.0, 1.0, K if rows_form else N)
    alpha = -1.0 if rows_form else 1.0
    y = ipmatrix.gemv_profile(A, kr, x, add=add, alpha=alpha, rows_form=rows_form, K=K, N=N)
    al = a.astype(np.longdouble)
    prod = al @ x if rows_form else al.T @ x
    ref = add + alpha * prod
    bound = 1e-14 * (np.abs(a) @ np.abs(x) if rows_form else np.abs(a).T @ np.abs(x))
    err = np.abs(y.astype(np.longdouble) - ref)
    print("rows_form %d %d x %d ranges %s: max err %.3e (bound at it %.3e)" % (rows_form, K, N, kr.tolist(), float(err.max()), float(bound[np.argmax(err)])))
    assert not np.isnan(y).any()
    assert (err <= bound).all(), float((err - bound).max())
    y0 = ipmatrix.gemv_profile(A, kr, x, add=None, alpha=alpha, rows_form=rows_form, K=K, N=N)  # (without add: the bound alone)
    assert (np.abs(y0.astype(np.longdouble) - alpha * prod) <= bound).all()
    assert np.array_equal(y, ipmatrix.gemv_profile(A, kr, x, add=add, alpha=alpha, rows_form=rows_form, K=K, N=N))  # run-to-run


def test_profile_form_at_2000_states_beats_both_forms():
    """nx = 2000, nu = 20 dense control columns, K = 8, band 50: the bar against the dense form, and hqpkkt_stats.ms_factor
    of a replayed factorisation - best of three, the handles taking turns - below the dense form's and below the sparse
    form's with the library's heavy-column threshold.  Both partners are existing code paths: a form that beats neither
    has no reason to exist.  Measured on one MI355X: see profiles/r13_profile_form.txt."""
    prog = problems.sparse_docp(8, 2000, 20, band=50, fu_nnz=BIG, low_rank=False, seed=2)
    st = problems.ip_state(prog, 5, 1.0)
    hs = {"profile": _profile(), "dense": ipmatrix.IpLQDOCP(), "sparse": ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=-1)}
    sol = {}
    for form, M in hs.items():
        sol[form] = _solve(M, prog, st)
        M.factor(prog, st[0], st[1])  # (warm-up of the replayed sequence)
    assert (hs["profile"].dynamics_entries()[:, 1] == 2).all()
    err = rel_err(sol["profile"][0], sol["dense"][0])
    print(f"res profile {sol['profile'][1]:.3e} dense {sol['dense'][1]:.3e} rel.err {err:.3e}")
    assert sol["profile"][1] <= sol["dense"][1] + RES_TOL
    assert err <= SOL_TOL, err
    ms = {form: [] for form in hs}
    for _ in range(3):
        for form, M in hs.items():
            M.factor(prog, st[0], st[1])
            ms[form].append(M.stats()["ms_factor"])
    best = {form: min(v) for form, v in ms.items()}
    print("ms_factor, best of three: profile %.3f dense %.3f sparse + dense columns %.3f" % (best["profile"], best["dense"], best["sparse"]))
    assert best["profile"] < best["dense"] and best["profile"] < best["sparse"], best
