"""CPU tests of the sparse form of the STAGED engine's stage products (hqpkkt_set_dynamics_form): the ABI's call-order
and argument errors, the plan's sizes and work counts against the dense form's, and the per-stage row ranges into the
CSR arrays of A and A' against numpy.  hqpkkt_analyze is host-only: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix, problems


def _analyze(M, prog):
    arrs = []
    for (p, i, _x) in (prog.Q, prog.A, prog.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    M._keep = arrs
    sbw = C.c_int()
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *ptrs, C.byref(sbw))


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_symbol_and_constants():
    L = _lib.lib()
    assert "hqpkkt_set_dynamics_form" in _lib.SYMBOLS and hasattr(L, "hqpkkt_set_dynamics_form")
    assert (_lib.DYN_DENSE, _lib.DYN_SPARSE) == (0, 1)


def test_call_order_and_argument_errors():
    L = _lib.lib()
    prog = problems.sparse_docp(3, 12, 2, band=1)
    assert L.hqpkkt_set_dynamics_form(None, 1) == _lib.E_NULL
    M = ipmatrix.IpLQDOCP()
    assert L.hqpkkt_set_dynamics_form(M._h, 2) == _lib.E_RANGE
    assert L.hqpkkt_set_dynamics_form(M._h, -1) == _lib.E_RANGE
    for cls in (ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP):  # not a STAGED handle
        assert L.hqpkkt_set_dynamics_form(cls()._h, 1) == _lib.E_INTERN
    # the form holds until it is set again: every later analysis picks it up
    assert L.hqpkkt_set_dynamics_form(M._h, _lib.DYN_SPARSE) == 0
    assert _analyze(M, prog) == 0 and (M.dynamics_entries()[:, 1] == 1).all()
    assert _analyze(M, prog) == 0 and (M.dynamics_entries()[:, 1] == 1).all()
    assert L.hqpkkt_set_dynamics_form(M._h, _lib.DYN_DENSE) == 0
    assert (M.dynamics_entries()[:, 1] == 1).all()  # (the analysis that was made stays what it is)
    assert _analyze(M, prog) == 0 and (M.dynamics_entries()[:, 1] == 0).all() and len(M.debug(37)) == 0
    # the dense hand-over is refused on a sparse-form handle ...
    S = ipmatrix.IpLQDOCP(a_sparse=True)
    dq = problems.dense_docp_from_program(prog, prog.nx, prog.nu)
    with pytest.raises(ipmatrix.KktError) as e:
        S.init_dense(dq)
    assert e.value.code == _lib.E_INTERN
    # ... and so is one system over several ranks (it stays dense)
    R = ipmatrix.IpLQDOCP(a_sparse=True, shard=(0, 2, lambda *a: None))
    assert _analyze(R, prog) == _lib.E_RANGE
    R.set_dynamics_form("dense")
    assert _analyze(R, prog) == 0


def test_numeric_entries_need_the_device():
    prog = problems.sparse_docp(3, 12, 2, band=1)
    M = ipmatrix.IpLQDOCP(a_sparse=True)
    if _has_gpu():
        M.init(prog)
        return
    with pytest.raises(ipmatrix.KktError) as e:
        M.init(prog)  # (the analysis passes; update() needs the device)
    assert e.value.code == _lib.E_DEVICE
    st = problems.ip_state(prog, 1)
    with pytest.raises(ipmatrix.KktError) as e:
        M.factor(prog, st[0], st[1])
    assert e.value.code in (_lib.E_DEVICE, _lib.E_INTERN)


def _stage_entries(prog, nx, nu):
    """Per stage the (row, column, position in A's arrays) of every entry of F_k, from A's CSR in numpy."""
    p, i, _x = prog.A
    K = len(nu)
    nmk = np.concatenate([[0], np.cumsum([nx[k] + nu[k] for k in range(K)])])
    nks = np.concatenate([[0], np.cumsum(nx[1:])])
    rows = np.repeat(np.arange(prog.me), np.diff(p))
    pos = np.arange(i.size)
    out = []
    for k in range(K):
        sel = (rows >= nks[k]) & (rows < nks[k + 1]) & (i >= nmk[k]) & (i < nmk[k + 1])
        out.append((rows[sel], i[sel], pos[sel]))
    return out, nmk, nks


def test_sizes_and_work_counts_against_the_dense_form():
    K, nx, nu = 6, 300, 4
    prog = problems.sparse_docp(K, nx, nu, band=5, final_eq=2)
    D, S = ipmatrix.IpLQDOCP(), ipmatrix.IpLQDOCP(a_sparse=True)
    assert _analyze(D, prog) == 0 and _analyze(S, prog) == 0
    sd, ss = D.stats(), S.stats()
    f_arena = 8 * sum(prog.nx[k + 1] * (prog.nx[k] + prog.nu[k]) for k in range(K))
    # (the allocation keeps 8192 doubles of slack behind the arena in either form: not part of bytes_panels)
    assert sd["bytes_panels"] - ss["bytes_panels"] >= f_arena, (sd["bytes_panels"], ss["bytes_panels"], f_arena)
    assert ss["flops_factor"] < sd["flops_factor"]
    ent, _nmk, _nks = _stage_entries(prog, prog.nx, prog.nu)
    counts = [len(e[0]) for e in ent]
    assert [list(r) for r in S.dynamics_entries()] == [[c, 1] for c in counts]
    assert [list(r) for r in D.dynamics_entries()] == [[c, 0] for c in counts]


@pytest.mark.parametrize("case", ["band", "stages_differ", "empty_col_row", "eq_rows", "dense"])
def test_row_ranges_cover_every_entry_of_every_block_once(case):
    prog = {"band": lambda: problems.sparse_docp(5, 30, 3, band=2),
            "stages_differ": lambda: problems.sparse_docp(4, [20, 20, 17, 26, 9], [3, 1, 2, 4], band=3),
            "empty_col_row": lambda: problems.sparse_docp(4, 25, 2, band=2, empty_col=(1, 6), empty_row=(2, 9)),
            "eq_rows": lambda: problems.sparse_docp(5, 20, 3, band=1, path_eq=2, final_eq=4, x0_fixed=False),
            "dense": lambda: problems.sparse_docp(3, 15, 2, dense=True)}[case]()
    S = ipmatrix.IpLQDOCP(a_sparse=True)
    assert _analyze(S, prog) == 0
    p, i, _x = prog.A
    nx, nu = prog.nx, prog.nu
    K = len(nu)
    assert list(S.debug(20)) == nx and list(S.debug(21)) == nu
    ent, nmk, nks = _stage_entries(prog, nx, nu)
    ndyn, ncol = int(nks[K]), int(nmk[K])
    rng = S.debug(37).astype(np.int64)
    assert rng.size == 2 * ndyn + 2 * ncol
    arow, tcol = rng[:2 * ndyn].reshape(-1, 2), rng[2 * ndyn:].reshape(-1, 2)
    # A' as the library builds it: a stable counting sort of A's entries by column (rows ascending inside a column)
    order = np.argsort(i, kind="stable")
    t_rows = np.repeat(np.arange(prog.me), np.diff(p))[order]
    if case == "empty_col_row":
        c = nmk[1] + 6
        assert tcol[c, 0] == tcol[c, 1]  # the empty state column of F_1
        r = nks[2] + 9
        assert (i[arow[r, 0]:arow[r, 1]] >= nmk[2] + nx[2]).all() and arow[r, 1] > arow[r, 0]  # row 9 of fx_2 is empty: fu alone
    for k in range(K):
        rows, cols, pos = ent[k]
        # by rows: positions in A's arrays
        got = np.concatenate([np.arange(arow[r, 0], arow[r, 1]) for r in range(nks[k], nks[k + 1])] or [np.zeros(0, np.int64)])
        assert np.array_equal(np.sort(got), np.sort(pos)) and got.size == np.unique(got).size
        for r in range(nks[k], nks[k + 1]):  # the trailing -1 of the row is left out
            assert arow[r, 1] == p[r + 1] - 1 and i[p[r + 1] - 1] == nmk[k + 1] + (r - nks[k])
        # by columns: positions in the arrays of A', mapped back to A's
        got = np.concatenate([np.arange(tcol[c, 0], tcol[c, 1]) for c in range(nmk[k], nmk[k + 1])] or [np.zeros(0, np.int64)])
        assert got.size == np.unique(got).size
        assert np.array_equal(np.sort(order[got]), np.sort(pos))
        assert ((t_rows[got] >= nks[k]) & (t_rows[got] < nks[k + 1])).all()
        for c in range(nmk[k], nmk[k + 1]):  # inside a column the entries come in the order of the rows
            assert (np.diff(t_rows[tcol[c, 0]:tcol[c, 1]]) > 0).all()
