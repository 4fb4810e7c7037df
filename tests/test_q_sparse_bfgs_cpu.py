"""CPU tests of hqpkkt_q_components (host code) against hessian_update.q_components_model - plain union-find - on all three
plugins, with `full` and the cap / NULL conventions of hqpkkt_q_blocks, and of the three new symbols.  Hqp_IpLQDOCP accepts no
entry of Q across two stages: there a pattern keeps the entries inside the stages of lq_docp."""
import ctypes as C

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu

PLUGINS = [ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP, ipmatrix.IpLQDOCP]


def program(cls, kind, drop=None):
    """lq_docp with Q's pattern replaced: `evenodd` (n = 12: i ~ j where j - i is even, both classes dense), `cute` (n = 310,
    rows of cute_like_qp), `diag`, `denserow` (row 0 full); `drop`: one pair left out"""
    K, nx, nu = (20, 10, 5) if kind == "cute" else (1, 4, 4)
    base = problems.lq_docp(K, nx, nu)
    n = base.n
    if kind == "cute":
        q = problems.cute_like_qp(n, nnz_lo=1, nnz_hi=4, far=0.0).Q
        i, j = np.repeat(np.arange(n), np.diff(q[0])), np.asarray(q[1])
    else:
        i, j = np.triu_indices(n)
        k = {"evenodd": (j - i) % 2 == 0, "diag": i == j, "denserow": (i == j) | (i == 0)}[kind]
        i, j = i[k], j[k]
    stage = np.minimum(np.arange(n) // (nx + nu), K)
    k = (stage[i] == stage[j]) | (cls is not ipmatrix.IpLQDOCP)
    if drop is not None:
        k &= ~((i == drop[0]) & (j == drop[1]))
    Q = problems._csr(i[k], j[k], np.ones(int(k.sum())), n)
    return problems.Program(n, base.me, base.m, Q, base.A, base.C, base.c, base.b, base.d)


def test_symbols():
    L = _lib.lib()
    for nm in ("q_components", "q_sparse_bfgs_update", "q_sparse_bfgs_report"):
        assert "hqpkkt_" + nm in _lib.SYMBOLS and getattr(L, "hqpkkt_" + nm) is not None and callable(getattr(ipmatrix.Hqp_IpMatrix, nm))


@pytest.mark.parametrize("cls", PLUGINS)
@pytest.mark.parametrize("kind", ["evenodd", "cute", "diag", "denserow"])
def test_components_against_model(cls, kind):
    prog = program(cls, kind)
    n, staged = prog.n, cls is ipmatrix.IpLQDOCP
    M = cls()
    M.analyze(prog)
    first, member, full = M.q_components()
    want = hu.q_components_model(prog.Q[0], prog.Q[1], n)
    assert first.tolist() == want[0].tolist() and member.tolist() == want[1].tolist() and full.tolist() == want[2].tolist()
    assert (np.diff(member[first[:-1]]) > 0).all() and all((np.diff(member[a:e]) > 0).all() for a, e in zip(first, first[1:]))
    if kind == "evenodd":
        assert member.tolist() == ([0, 2, 4, 6, 1, 3, 5, 7, 8, 10, 9, 11] if staged else [0, 2, 4, 6, 8, 10, 1, 3, 5, 7, 9, 11]) and full.all()
    elif kind == "cute":
        assert 1 < len(full) < n and (staged or (not full.all() and np.diff(first).max() > 8))
    elif kind == "diag":
        assert member.tolist() == list(range(n)) and len(full) == n and full.all()
    else:
        assert np.diff(first).tolist() == ([8, 1, 1, 1, 1] if staged else [n]) and full.tolist() == [0] + [1] * (len(full) - 1)


@pytest.mark.parametrize("cls", PLUGINS)
def test_full_caps_and_nulls(cls):
    L = _lib.lib()
    M = cls()
    k = C.c_longlong(-1)
    assert L.hqpkkt_q_components(M._h, None, None, None, 0, C.byref(k)) == _lib.E_INTERN  # (before the analysis)
    assert L.hqpkkt_q_components(None, None, None, None, 0, C.byref(k)) == L.hqpkkt_q_components(M._h, None, None, None, 0, None) == _lib.E_NULL
    prog = program(cls, "evenodd", drop=(0, 2))  # 0 - 4 - 2 still holds the evens together
    M.analyze(prog)
    first, member, full = M.q_components()
    assert member.tolist() == hu.q_components_model(prog.Q[0], prog.Q[1], 12)[1].tolist() and full.tolist() == [0] + [1] * (len(full) - 1)
    nb = len(full)
    assert L.hqpkkt_q_components(M._h, None, None, None, 0, C.byref(k)) == _lib.OK and k.value == nb
    f, m, vp = np.full(nb + 1, -7, dtype=np.int32), np.full(12, -7, dtype=np.int32), lambda a: C.c_void_p(a.ctypes.data)
    assert L.hqpkkt_q_components(M._h, vp(f), vp(m), None, nb - 1, C.byref(k)) == _lib.E_RANGE and k.value == nb and (f == -7).all() and (m == -7).all()
    assert L.hqpkkt_q_components(M._h, vp(f), None, None, nb, C.byref(k)) == _lib.E_NULL
    assert L.hqpkkt_q_components(M._h, vp(f), vp(m), None, nb, C.byref(k)) == _lib.OK and f.tolist() == first.tolist() and m.tolist() == member.tolist()
    assert all(a.size == 0 for a in hu.q_components_model(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), 0))  # n = 0: no blocks
