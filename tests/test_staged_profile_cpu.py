"""CPU tests of the profile form of the STAGED engine's stage products (hqpkkt_set_dynamics_form(HQPKKT_DYN_PROFILE)): the
k-slab ranges of the 128-column panels of F_k that the analysis records (hqpkkt_debug_get 41) against numpy, which stages
run the profile sequence (item 36), the return codes and the call order, and the work list of tiles of unequal length
(hqpkkt_debug_sk_profile, sk_table.hpp).  hqpkkt_analyze and the list are host-only: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix, problems

BIG = 10**6

CASES = {
    "band1": lambda: problems.sparse_docp(3, 300, 5, band=1, seed=41),
    "band5": lambda: problems.sparse_docp(3, 300, 5, band=5, seed=42),
    "band20_odd": lambda: problems.sparse_docp(3, 517, 6, band=20, seed=43),
    "stages_differ": lambda: problems.sparse_docp(4, [400, 400, 330, 520, 460], [4, 2, 6, 3], band=8, seed=44),
    "empty_col": lambda: problems.sparse_docp(3, 300, 3, band=2, empty_col=(1, 7), seed=45),
    "empty_panel": lambda: _without_columns(problems.sparse_docp(3, 256, 3, band=2, seed=46), 1, range(256, 259)),  # (F_1 without control entries)
    "dense_controls": lambda: problems.sparse_docp(3, 320, 12, band=5, fu_nnz=BIG, seed=47),
    "one_panel": lambda: problems.sparse_docp(3, 100, 4, band=3, seed=48),
    "dense": lambda: problems.sparse_docp(3, 300, 4, dense=True, seed=49),
}


def _without_columns(prog, k, cols):
    """prog without the entries of the state columns `cols` of F_k (its pattern: the values do not matter here)."""
    p, i, x = (np.asarray(a) for a in prog.A)
    c0 = int(sum(prog.nx[s] + prog.nu[s] for s in range(k)))
    r0, r1 = int(sum(prog.nx[1: k + 1])), int(sum(prog.nx[1: k + 2]))
    rows = np.repeat(np.arange(len(p) - 1), np.diff(p))
    drop = (rows >= r0) & (rows < r1) & np.isin(i, c0 + np.asarray(list(cols)))
    keep = ~drop
    p2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=len(p) - 1))]).astype(p.dtype)
    out = problems.Program(prog.n, prog.me, prog.m, prog.Q, (p2, i[keep], x[keep]), prog.C, c=prog.c, b=prog.b, d=prog.d)
    out.nx, out.nu = prog.nx, prog.nu
    return out


def _analyze(M, prog):
    arrs = []
    for (p, i, _x) in (prog.Q, prog.A, prog.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    sbw = C.c_int()
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *ptrs, C.byref(sbw))


def expected_ranges(prog):
    """Per stage k < K the (lo, hi) pairs of the panels of F_k = [fx_k fu_k], from the pattern of A with numpy."""
    p, i, _x = (np.asarray(a) for a in prog.A)
    nx, nu = list(prog.nx), list(prog.nu)
    out, c0, r0 = [], 0, 0
    for k in range(len(nu)):
        nz, np1 = nx[k] + nu[k], nx[k + 1]
        first, last = np.full(nz, -1), np.full(nz, -1)
        for li in range(np1):
            cols = i[p[r0 + li]: p[r0 + li + 1] - 1] - c0  # (the row without its trailing -1)
            assert ((cols >= 0) & (cols < nz)).all()
            first[cols] = np.where(first[cols] < 0, li, first[cols])
            last[cols] = li
        rng = []
        for q in range((nz + 127) // 128):
            f, l = first[128 * q: 128 * q + 128], last[128 * q: 128 * q + 128]
            rng.append((0, 0) if (f < 0).all() else (int(f[f >= 0].min()) // 16, int(l.max()) // 16 + 1))
        out.append(np.array(rng, dtype=np.int32).reshape(-1, 2))
        c0, r0 = c0 + nz, r0 + np1
    return out


def test_symbols_and_constants():
    L = _lib.lib()
    assert _lib.DYN_PROFILE == 3
    for sym in ("hqpkkt_debug_sk_profile", "hqpkkt_debug_gemv_profile"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
    assert [f[0] for f in _lib.DgemmCase._fields_][-2:] == ["krange", "krange_by"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_ranges_against_numpy(case):
    prog = CASES[case]()
    M = ipmatrix.IpLQDOCP(a_profile=True)
    assert _analyze(M, prog) == 0
    want, got = expected_ranges(prog), M.profile_ranges()
    K = len(prog.nu)
    assert len(got) == K
    for k in range(K):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    d = M.debug(41)
    assert d[0] == 0 and list(np.diff(d[: K + 1])) == [(prog.nx[k] + prog.nu[k] + 127) // 128 for k in range(K)]
    # which stages run the profile sequence: at least two panels, a range shorter than all slabs of n_{k+1}
    runs = [int(len(want[k]) >= 2 and bool(((want[k][:, 1] - want[k][:, 0]) < (prog.nx[k + 1] + 15) // 16).any())) for k in range(K)]
    assert list(M.dynamics_entries()[:, 1]) == [2 * r for r in runs]
    nnz = [int(np.diff(np.asarray(prog.A[0]))[sum(prog.nx[1: k + 1]): sum(prog.nx[1: k + 2])].sum()) - prog.nx[k + 1] for k in range(K)]
    assert list(M.dynamics_entries()[:, 0]) == nnz
    if case == "dense":
        assert all((want[k] == (0, (prog.nx[k + 1] + 15) // 16)).all() for k in range(K)) and not any(runs)
    if case == "one_panel":
        assert not any(runs)
    if case in ("band5", "dense_controls", "stages_differ", "empty_panel"):
        assert all(runs)
    if case == "empty_panel":
        assert tuple(want[1][2]) == (0, 0)
    if case == "dense_controls":  # (the control panel holds every row)
        assert all(tuple(want[k][-1]) == (0, 20) for k in range(K))


def test_ranges_are_the_pattern_s_and_other_forms_have_none():
    prog = CASES["band5"]()
    M = ipmatrix.IpLQDOCP(a_profile=True)
    assert _analyze(M, prog) == 0
    first = [r.copy() for r in M.profile_ranges()]
    assert _analyze(M, prog) == 0  # (the form holds over analyses)
    assert all(np.array_equal(a, b) for a, b in zip(first, M.profile_ranges()))
    for form in ("dense", "sparse"):
        M.set_dynamics_form(form)
        assert _analyze(M, prog) == 0
        assert M.profile_ranges() == [] and M.debug(41).size == 0
        assert (M.dynamics_entries()[:, 1] == (1 if form == "sparse" else 0)).all()
    # same arena as the dense form
    D, P = ipmatrix.IpLQDOCP(), ipmatrix.IpLQDOCP(a_profile=True)
    assert _analyze(D, prog) == 0 and _analyze(P, prog) == 0
    assert P.stats()["bytes_panels"] == D.stats()["bytes_panels"]


def test_return_codes_and_call_order():
    L = _lib.lib()
    prog = problems.sparse_docp(3, 300, 2, band=1)
    assert L.hqpkkt_set_dynamics_form(None, _lib.DYN_PROFILE) == _lib.E_NULL
    M = ipmatrix.IpLQDOCP()
    for unknown in (2, 4):  # (2 stays no form: the value the sparse form's tests probe)
        assert L.hqpkkt_set_dynamics_form(M._h, unknown) == _lib.E_RANGE
    assert L.hqpkkt_set_dynamics_form(M._h, -1) == _lib.E_RANGE
    for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):  # not a STAGED handle
        assert L.hqpkkt_set_dynamics_form(cls()._h, _lib.DYN_PROFILE) == _lib.E_INTERN
    assert L.hqpkkt_set_dynamics_form(M._h, _lib.DYN_PROFILE) == 0
    assert L.hqpkkt_set_dense_columns(M._h, 8) == 0  # accepted and ignored
    assert _analyze(M, prog) == 0
    assert (M.dynamics_entries()[:, 1] == 2).all() and M.dense_columns() == []
    # the dense hand-over is not available with it
    dq = problems.dense_docp_from_program(prog, list(prog.nx), list(prog.nu))
    with pytest.raises(ipmatrix.KktError) as err:
        M.init_dense(dq)
    assert err.value.code == _lib.E_INTERN
    nx, nu = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32)
    arrs = []
    for (p, i, _x) in (dq.Q, dq.E, dq.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    assert L.hqpkkt_analyze_staged(M._h, dq.K, C.c_void_p(nx.ctypes.data), C.c_void_p(nu.ctypes.data), dq.n, dq.me_rest, dq.m, *ptrs) == _lib.E_INTERN
    # one system over several ranks stays dense
    R = ipmatrix.IpLQDOCP(a_profile=True, shard=(0, 2, lambda *a: None))
    assert _analyze(R, prog) == _lib.E_RANGE
    R.set_dynamics_form("dense")
    assert _analyze(R, prog) == 0


# ---- the work list of tiles of unequal length

def _random_ranges(rng, tiles, nslab, kind):
    lo = rng.integers(0, nslab, tiles)
    ln = rng.integers(0, 12, tiles)
    if kind == "empty_and_one":
        ln = rng.choice([0, 1, 1, 3, 9], tiles)
    if kind == "one_long":
        ln = rng.integers(1, 6, tiles)
        lo[tiles // 2], ln[tiles // 2] = 0, nslab
    if kind == "all_empty":
        ln[:] = 0
    return np.stack([lo, np.minimum(lo + ln, nslab)], 1).astype(np.int32)


LISTS = [(kind, tiles, nslab, grid, seed)
         for seed, (kind, tiles, nslab) in enumerate([("random", 700, 40), ("empty_and_one", 333, 19), ("one_long", 257, 313), ("random", 5, 64),
                                                      ("one_long", 3, 313), ("all_empty", 41, 8), ("random", 1600, 313)])
         for grid in (8, 64, 512)]


@pytest.mark.parametrize("kind,tiles,nslab,grid,seed", LISTS)
def test_profile_list(kind, tiles, nslab, grid, seed):
    rng = np.random.default_rng(100 + seed)
    r = _random_ranges(rng, tiles, nslab, kind)
    got = ipmatrix.sk_profile(r, grid)
    assert got is not None
    units, pieces = got
    assert units.shape[0] == grid and (units[:, -1, 0] == -1).all()  # (an end mark behind every workgroup's list)
    total = int((r[:, 1] - r[:, 0]).sum())
    longest = 0
    seen = [[] for _ in range(tiles)]
    for b in range(grid):
        mine, parked, ended = 0, 0, False
        for u in units[b]:
            t, s0, s1, slot0, np_, j = (int(v) for v in u)
            if t < 0:
                ended = True
                continue
            assert not ended and 0 <= t < tiles
            assert r[t, 0] <= s0 <= s1 <= r[t, 1]  # (no slab outside the tile's range)
            assert s1 > s0 or (np_ == 1 and r[t, 0] == r[t, 1])  # (only an empty tile gives an empty unit)
            seen[t].append((j, s0, s1, slot0, np_))
            mine += s1 - s0
            parked += np_ > 1
            longest = max(longest, s1 - s0)
        assert parked <= 2, (b, parked)
        units_b = [int(u[2] - u[1]) for u in units[b] if u[0] >= 0]
        assert mine <= -(-total // grid) + max(units_b, default=0), (b, mine, total)
    slots = []
    for t in range(tiles):
        ps = sorted(seen[t])
        assert ps, t  # (every tile is written, an empty one too)
        n = ps[0][4]
        assert [q[0] for q in ps] == list(range(n)) and all(q[4] == n and q[3] == ps[0][3] for q in ps)  # pieces numbered 0 .. n - 1
        # in the order of k, and every slab of the range exactly once
        assert ps[0][1] == r[t, 0] and ps[-1][2] == r[t, 1] and all(a[2] == b_[1] for a, b_ in zip(ps, ps[1:]))
        if n > 1:
            slots.append((ps[0][3], ps[0][3] + n))
    slots.sort()
    assert all(a[1] <= b_[0] for a, b_ in zip(slots, slots[1:])) and (not slots or (slots[0][0] >= 0 and slots[-1][1] <= pieces))
    assert pieces <= 2 * grid
    if tiles < grid and kind != "all_empty":
        assert sum(len(s) for s in seen) > tiles or total < tiles  # (fewer tiles than workgroups: tiles are shared)


def test_profile_list_refuses_bad_ranges():
    assert ipmatrix.sk_profile(np.array([[3, 2]]), 8) is None
    assert ipmatrix.sk_profile(np.array([[-1, 2]]), 8) is None
    assert ipmatrix.sk_profile(np.array([[0, 70000]]), 8) is None


def test_equal_ranges_give_the_fractional_list():
    """Tiles of one length: the list of gemm_frac_table, unit for unit."""
    for tiles, nslab, grid in [(272, 125, 512), (37, 40, 13), (300, 188, 512)]:
        u, pieces = ipmatrix.sk_profile(np.tile([0, nslab], (tiles, 1)), grid)
        f, fpieces, _, _ = ipmatrix.sk_table(tiles, nslab, grid, "frac")
        assert pieces == fpieces and np.array_equal(u, f)
