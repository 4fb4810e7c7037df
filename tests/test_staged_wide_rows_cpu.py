"""CPU tests of the wide rows of C in the STAGED engine (hqpkkt_set_dense_rows): the setter's return codes and call
order, the plan's wide rows and term counts (hqpkkt_debug_get 43) against numpy, what the blocks E_k add to
hqpkkt_stats.bytes_panels, a setting of 0 against a handle that never asked, and the guard on the number of H terms.
The analysis is host-only: no GPU needed."""
import ctypes as C
import time

import numpy as np
import pytest

from wide_rows_cases import CASES, MIN_ENTRIES, OPTIONS, expected_terms, expected_wide
from hqp_amd import _lib, ipmatrix, problems

PLAN_ITEMS = (20, 21, 22, 23, 24, 25, 26, 36, 37, 39, 41, 42)


def _analyze(M, prog):
    arrs = []
    for (p, i, _x) in (prog.Q, prog.A, prog.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    sbw = C.c_int()
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *ptrs, C.byref(sbw))


def test_setter_return_codes_and_call_order():
    L = _lib.lib()
    assert L.hqpkkt_set_dense_rows(None, 8) == _lib.E_NULL
    T = ipmatrix.IpSpBKP()  # (not in STAGED mode)
    assert L.hqpkkt_set_dense_rows(T._h, 8) == _lib.E_INTERN
    M = ipmatrix.IpLQDOCP()
    assert L.hqpkkt_set_dense_rows(M._h, -2) == _lib.E_RANGE
    for v in (0, 1, 32, 10**6):
        assert L.hqpkkt_set_dense_rows(M._h, v) == 0
    # before the analysis; it holds over analyses until it is set again
    prog = CASES["slab_edges"]()
    M = ipmatrix.IpLQDOCP()
    M.set_dense_rows(32)
    assert _analyze(M, prog) == 0
    assert M.dense_rows() == expected_wide(prog, 32) and [len(r) for r in M.dense_rows()] == [1, 15, 16, 17, 0]
    assert _analyze(M, prog) == 0
    assert M.dense_rows() == expected_wide(prog, 32)
    M.set_dense_rows(0)
    assert M.dense_rows() == expected_wide(prog, 32)  # (the plan of the last analysis)
    assert _analyze(M, prog) == 0
    assert M.dense_rows() == [] and M.debug(43).size == 0 and M.h_terms() == ([], [])


def test_the_library_threshold_is_not_set_yet():
    """-1 asks for the library's own threshold, the result of tools/wide_rows_sweep.py on one MI355X.  That sweep has not
    been run: the setter refuses -1 and the handle keeps the setting it had."""
    prog = CASES["at_the_threshold"]()
    M = ipmatrix.IpLQDOCP(dense_rows=32)
    assert M._L.hqpkkt_set_dense_rows(M._h, -1) == _lib.E_RANGE
    assert _analyze(M, prog) == 0
    assert M.dense_rows() == expected_wide(prog, 32)


def test_both_hand_overs():
    """hqpkkt_analyze_staged (the dynamics as dense blocks): C is CSR there too."""
    prog = CASES["stages_differ"]()
    dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu)
    M = ipmatrix.IpLQDOCP(dense_rows=32)
    nx, nu = np.asarray(dq.nx, dtype=np.int32), np.asarray(dq.nu, dtype=np.int32)
    arrs = []
    for (p, i, _x) in (dq.Q, dq.E, dq.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    assert M._L.hqpkkt_analyze_staged(M._h, dq.K, C.c_void_p(nx.ctypes.data), C.c_void_p(nu.ctypes.data), dq.n, dq.me_rest, dq.m, *ptrs) == 0
    assert M.dense_rows() == expected_wide(prog, 32) and any(M.dense_rows())


def test_accepted_and_ignored_on_a_sharded_handle():
    prog = CASES["at_the_threshold"]()
    plain = ipmatrix.IpLQDOCP()
    plain.set_shard(0, 2, lambda *a: 0)
    M = ipmatrix.IpLQDOCP(dense_rows=32)
    M.set_shard(0, 2, lambda *a: 0)
    assert _analyze(plain, prog) == 0 and _analyze(M, prog) == 0
    assert M.debug(43).size == 0 and M.dense_rows() == []
    assert M.stats()["bytes_panels"] == plain.stats()["bytes_panels"] and M.stats()["flops_factor"] == plain.stats()["flops_factor"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_wide_rows_and_term_counts_against_numpy(case):
    prog = CASES[case]()
    for min_entries in (MIN_ENTRIES[case], 10**6):
        M = ipmatrix.IpLQDOCP(dense_rows=min_entries, **OPTIONS[case])
        assert _analyze(M, prog) == 0
        want = expected_wide(prog, min_entries)
        assert M.dense_rows() == want and any(want) == (min_entries < 10**6)
        K = len(prog.nu)
        d = M.debug(43)
        assert d.size == K + 2 + sum(len(w) for w in want) + 4 * (K + 1)
        assert d[0] == 0 and list(np.diff(d[: K + 2])) == [len(w) for w in want]
        kept, removed = M.h_terms()
        ekept, eremoved = expected_terms(prog, min_entries)
        assert np.array_equal(kept, ekept) and np.array_equal(removed, eremoved)
        assert (removed > 0).tolist() == [len(w) > 0 for w in want]


def test_what_the_cases_make_wide():
    """The generators give what the GPU tests count on."""
    count = lambda name: [len(w) for w in expected_wide(CASES[name](), MIN_ENTRIES[name])]
    assert count("one_row_nx70") == [0, 1, 0, 0]
    assert count("slab_edges") == [1, 15, 16, 17, 0]
    assert count("terminal_set") == [0, 0, 0, 17]
    assert count("every_row_wide") == [6, 7, 7, 6, 0]  # (the bounds of the controls, one and one wide row; none at stage K)
    assert count("at_the_threshold") == [0, 1, 1, 0]   # (of a row of 32 and one of 31 entries each)
    assert count("overlap_width") == [0, 20, 0]
    prog = CASES["with_carried_rows"]()
    p, i, _x = prog.C
    wide = expected_wide(prog, 32)
    for k in range(4):  # (every wide row of a stage k < K touches its controls)
        assert all(i[p[r + 1] - 1] >= sum(prog.nx[:k]) + sum(prog.nu[:k]) + prog.nx[k] for r in wide[k])


def test_with_wide_rows_keeps_what_is_there():
    base = problems.lq_docp(3, 20, 2, seed=4)
    rows = [(0, 5, True), (3, 20, False), (1, 7, False)]
    prog, again = problems.with_wide_rows(base, rows), problems.with_wide_rows(base, rows)
    assert all(np.array_equal(a, b) for a, b in zip(prog.C, again.C))
    (p0, i0, x0), (p1, i1, x1) = base.C, prog.C
    assert prog.m == base.m + 3 and np.array_equal(p1[: base.m + 1], p0) and np.array_equal(i1[: i0.size], i0) and np.array_equal(x1[: x0.size], x0)
    assert np.diff(p1)[base.m:].tolist() == [5, 20, 7] and np.abs(x1[x0.size:]).max() <= 0.05
    assert (prog.d > 0).all() and prog.d.size == prog.m  # (x = 0 is strictly inside)
    assert prog.Q is base.Q and prog.A is base.A
    row0 = i1[p1[base.m]: p1[base.m + 1]]
    assert (np.diff(row0) > 0).all() and row0.max() >= 20 and row0.max() < 22  # (stage 0: states 0 .. 19, controls 20, 21)
    rowK = i1[p1[base.m + 1]: p1[base.m + 2]]
    assert rowK.tolist() == list(range(66, 86))


@pytest.mark.parametrize("case", ["one_row_nx70", "slab_edges", "terminal_set", "stages_differ", "banded_sparse_form", "banded_packed_panels"])
def test_bytes_panels(case):
    prog = CASES[case]()

    def panels(**kw):
        M = ipmatrix.IpLQDOCP(**kw, **OPTIONS[case])
        assert _analyze(M, prog) == 0
        return M.stats(), M

    zero, _ = panels(dense_rows=0)
    none, _ = panels(dense_rows=10**6)
    split, M = panels(dense_rows=MIN_ENTRIES[case])
    assert none["bytes_panels"] == zero["bytes_panels"] and none["flops_factor"] == zero["flops_factor"]
    up8 = lambda v: (v + 7) // 8 * 8
    width = [prog.nx[k] + prog.nu[k] for k in range(len(prog.nu))] + [prog.nx[-1]]
    blocks = sum(len(r) * up8(width[k]) for k, r in enumerate(M.dense_rows()))
    assert blocks > 0 and split["bytes_panels"] == zero["bytes_panels"] + 8 * blocks
    # the products S'S over the lower half: r_k (n_k + m_k)^2 flops per stage
    assert split["flops_factor"] == zero["flops_factor"] + sum(len(r) * width[k] ** 2 for k, r in enumerate(M.dense_rows()))


@pytest.mark.parametrize("case", ["slab_edges", "with_carried_rows", "banded_sparse_form", "banded_profile_form", "banded_packed_panels"])
def test_zero_is_a_handle_that_never_asked(case):
    prog = CASES[case]()
    never = ipmatrix.IpLQDOCP(**OPTIONS[case])
    zero = ipmatrix.IpLQDOCP(**OPTIONS[case])
    assert zero._L.hqpkkt_set_dense_rows(zero._h, 0) == 0
    back = ipmatrix.IpLQDOCP(dense_rows=32, **OPTIONS[case])  # (set and taken back before the analysis)
    back.set_dense_rows(0)
    assert _analyze(never, prog) == 0 and _analyze(zero, prog) == 0 and _analyze(back, prog) == 0
    for M in (zero, back):
        for item in PLAN_ITEMS:
            assert np.array_equal(M.debug(item), never.debug(item)), item
        assert M.debug(43).size == 0 and never.debug(43).size == 0
        a, b = M.stats(), never.stats()
        assert all(a[key] == b[key] for key in ("bytes_panels", "bytes_updates", "flops_factor", "nnz_factor", "nnz_kkt"))


def _one_long_row(L):
    """One stage (K = 1) of L states, fixed, and one control, one state behind it; a diagonal Q, the bounds of the
    control and one inequality row over all L states."""
    n = L + 2
    Q = (np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    # (the dynamics row, then the rows that fix x_0: a free initial state of more than 4096 components is refused)
    A = (np.concatenate([[0], 3 + np.arange(L + 1)]).astype(np.int32), np.concatenate([[0, L, L + 1], np.arange(L)]).astype(np.int32),
         np.concatenate([[0.5, 1.0, -1.0], np.ones(L)]))
    Cp = np.array([0, 1, 2, 2 + L], dtype=np.int32)
    Ci = np.concatenate([[L, L], np.arange(L)]).astype(np.int32)
    Cx = np.concatenate([[1.0, -1.0], np.full(L, 1.0 / L)])
    prog = problems.Program(n, 1 + L, 3, Q, A, (Cp, Ci, Cx), d=np.ones(3))
    prog.nx, prog.nu = [L, 1], [1]
    return prog


def test_the_guard_on_the_number_of_terms():
    """One row of 46 400 entries is 2.15e9 terms, more than the int offsets of the term lists hold: without the split
    the analysis says HQPKKT_E_SIZES - at once, by counting before anything is reserved - and with it the plan keeps the
    terms of Q and of the two bounds."""
    prog = _one_long_row(46400)
    t0 = time.perf_counter()
    M = ipmatrix.IpLQDOCP()
    M.set_stages(prog.nx, prog.nu)
    assert _analyze(M, prog) == _lib.E_SIZES
    N = ipmatrix.IpLQDOCP(dense_rows=32)
    N.set_stages(prog.nx, prog.nu)
    assert _analyze(N, prog) == 0
    assert time.perf_counter() - t0 < 10.0
    assert N.dense_rows() == [[2], []]
    kept, removed = N.h_terms()
    assert kept.sum() == prog.n + 2 < 10**6 and removed.tolist() == [46400 ** 2, 0]
    # a row just below the limit of the lists is not refused for its size
    small = _one_long_row(300)
    S = ipmatrix.IpLQDOCP()
    S.set_stages(small.nx, small.nu)
    assert _analyze(S, small) == 0
