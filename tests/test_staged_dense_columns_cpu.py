"""CPU tests of the heavy columns of the STAGED engine's sparse form (hqpkkt_set_dense_columns): the setter's return
codes and call order, the plan's list of heavy columns (hqpkkt_debug_get 39) against numpy, and what the dense blocks
D_k add to hqpkkt_stats.bytes_panels.  hqpkkt_analyze is host-only: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

from dense_columns_cases import BIG, CASES, MIN_ENTRIES, expected_heavy
from hqp_amd import _lib, ipmatrix, problems

def _analyze(M, prog):
    arrs = []
    for (p, i, _x) in (prog.Q, prog.A, prog.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    sbw = C.c_int()
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *ptrs, C.byref(sbw))


def test_setter_return_codes_and_call_order():
    L = _lib.lib()
    assert L.hqpkkt_set_dense_columns(None, 8) == _lib.E_NULL
    T = ipmatrix.IpSpBKP()  # (not in STAGED mode)
    assert L.hqpkkt_set_dense_columns(T._h, 8) == _lib.E_INTERN
    M = ipmatrix.IpLQDOCP()
    assert L.hqpkkt_set_dense_columns(M._h, -2) == _lib.E_RANGE
    for v in (-1, 0, 1, 10**6):
        assert L.hqpkkt_set_dense_columns(M._h, v) == 0
    # the dynamics form keeps its two values
    assert L.hqpkkt_set_dynamics_form(M._h, 2) == _lib.E_RANGE
    # before the analysis, in either order with the form; it holds over analyses until it is set again
    prog = CASES["dense_fu_nx40"]()
    M = ipmatrix.IpLQDOCP()
    M.set_dense_columns(8)
    M.set_dynamics_form("sparse")
    assert _analyze(M, prog) == 0
    assert M.dense_columns() == expected_heavy(prog, 8)
    assert _analyze(M, prog) == 0
    assert M.dense_columns() == expected_heavy(prog, 8)
    M.set_dense_columns(0)
    assert M.dense_columns() == expected_heavy(prog, 8)  # (the plan of the last analysis)
    assert _analyze(M, prog) == 0
    assert M.dense_columns() == [[] for _ in prog.nu]


@pytest.mark.parametrize("case", ["dense_fu_nx40", "dense_fu_stages_differ", "state_cols_some_stages", "nine_cols_nx130", "all_dense"])
@pytest.mark.parametrize("min_entries", [1, 8, 10**6])
def test_heavy_columns_against_numpy(case, min_entries):
    prog = CASES[case]()
    M = ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=min_entries)
    assert _analyze(M, prog) == 0
    want = expected_heavy(prog, min_entries)
    assert M.dense_columns() == want
    d = M.debug(39)
    K = len(prog.nu)
    assert d.size == K + 1 + sum(len(w) for w in want) and d[0] == 0 and list(np.diff(d[: K + 1])) == [len(w) for w in want]
    assert (M.dynamics_entries()[:, 1] == 1).all()  # (item 36 is unchanged)


def test_what_the_cases_make_heavy():
    """The generators give what the GPU tests count on: dense fu = every control column (a band of 4 either side has 9
    entries per inner column: at a threshold of 8 those are heavy too, columns at the band's ends are not),
    with_dense_columns = its list."""
    prog = CASES["dense_fu_stages_differ"]()
    for k, h in enumerate(expected_heavy(prog, 8)):
        assert set(range(prog.nx[k], prog.nx[k] + prog.nu[k])) <= set(h) and len(h) < prog.nx[k] + prog.nu[k]
    assert expected_heavy(prog, 30) == [list(range(prog.nx[k], prog.nx[k] + prog.nu[k])) for k in range(5)]
    assert expected_heavy(CASES["state_cols_some_stages"](), 20) == [[], [5, 6], [], [], [47, 50], []]  # (band 5: 11 entries)
    assert expected_heavy(CASES["nine_cols_nx130"](), 8) == [[3, 4, 5, 64, 65, 129, 130, 131, 133]] * 4
    assert expected_heavy(CASES["all_dense"](), 1) == [list(range(43))] * 4


def test_with_dense_columns_keeps_what_is_there():
    base = problems.sparse_docp(6, 40, 3, band=2, seed=14)
    cols = [(k, j) for k in range(6) for j in (0, 17, 39)]
    prog = problems.with_dense_columns(base, cols)
    again = problems.with_dense_columns(base, cols)
    assert all(np.array_equal(a, b) for a, b in zip(prog.A, again.A))
    (p0, i0, x0), (p1, i1, x1) = base.A, prog.A
    r0, r1 = np.repeat(np.arange(base.me), np.diff(p0)), np.repeat(np.arange(prog.me), np.diff(p1))
    old = dict(zip(zip(r0.tolist(), i0.tolist()), x0.tolist()))
    new = dict(zip(zip(r1.tolist(), i1.tolist()), x1.tolist()))
    assert all(new[key] == v for key, v in old.items())
    added = [v for key, v in new.items() if key not in old]
    assert len(added) == len(new) - len(old) > 0 and max(abs(v) for v in added) <= 0.05
    assert expected_heavy(prog, 40) == [[0, 17, 39]] * 6
    assert (prog.Q is base.Q) and (prog.C is base.C)


def test_empty_without_the_feature_and_on_a_dense_form_handle():
    prog = CASES["dense_fu_nx40"]()
    M = ipmatrix.IpLQDOCP(a_sparse=True)  # min_entries = 0
    assert _analyze(M, prog) == 0
    assert M.dense_columns() == [[] for _ in prog.nu] and M.debug(39).size == len(prog.nu) + 1
    D = ipmatrix.IpLQDOCP(dense_columns=8)  # accepted and ignored
    assert _analyze(D, prog) == 0
    assert D.debug(39).size == 0 and D.dense_columns() == []
    assert (D.dynamics_entries()[:, 1] == 0).all()


def test_the_library_threshold():
    """-1 is the library's own threshold, one of the entry counts of its sweep (16 .. 2000: tools/dense_columns_sweep.py):
    it leaves the columns of a band alone (11 entries) and takes the full columns of a stage of 2100 states."""
    prog = problems.sparse_docp(2, 2100, 2, band=5, fu_nnz=BIG, seed=2, low_rank=False)
    M = ipmatrix.IpLQDOCP(a_sparse=True, dense_columns=-1)
    assert _analyze(M, prog) == 0
    assert M.dense_columns() == [[2100, 2101]] * 2


@pytest.mark.parametrize("case", ["dense_fu_nx40", "dense_fu_stages_differ", "state_cols_some_stages", "nine_cols_nx130", "all_dense"])
def test_bytes_panels(case):
    prog = CASES[case]()

    def panels(**kw):
        M = ipmatrix.IpLQDOCP(**kw)
        assert _analyze(M, prog) == 0
        return M.stats()["bytes_panels"], M

    sparse, _ = panels(a_sparse=True)
    dense, _ = panels()
    none, _ = panels(a_sparse=True, dense_columns=10**6)
    assert none == sparse
    split, M = panels(a_sparse=True, dense_columns=MIN_ENTRIES[case])
    assert sparse < split <= dense, (sparse, split, dense)
    # the V arena and the blocks D_k: n_{k+1} rows of up8(heavy columns) doubles, each block rounded up to 16 doubles
    up = lambda v, q: (v + q - 1) // q * q
    blocks = sum(up(prog.nx[k + 1] * up(len(h), 8), 16) for k, h in enumerate(M.dense_columns()) if h)
    assert split == sparse + 8 * blocks
