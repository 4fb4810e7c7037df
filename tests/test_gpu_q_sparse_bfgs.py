"""GPU tests of hqpkkt_q_sparse_bfgs_update / _report (hqp_amd/csrc/q_sparse_bfgs.hip.h).  Shapes: components i mod 3 of length 70
(past a wavefront) and 257 (past a workgroup), fully stored; n = 8300 whose even variables 0 .. 8198 are a chain of 4100 (past
a chunk of 4096) among singletons, the stored entries alone.  Real-valued programs hold a NaN below the diagonal wherever the
pattern allows one.  (A stored entry with col >= row joins its ends in one component: no entry ACROSS components exists.)
Bounds, U = 2^-53: integers exact against int64; (Q s)_i within (r_i + 1) U sum |q_ij s_j| of longdouble, r_i the row's entries;
a reported sum within (L + 2) U sum |terms|, L the block's length (L fused multiply-adds in any order); the rest bit for bit
hessian_update.q_sparse_bfgs_replay."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hqp_amd import _lib, ipmatrix, problems  # noqa: E402
from hqp_amd import hessian_update as hu  # noqa: E402
from q_values_worker import _state_bits, band_qp, bits, handle, rows_of, sym_terms, with_lower_nan, with_q  # noqa: E402

pytestmark = pytest.mark.gpu
U, ld = 2.0 ** -53, np.longdouble
SP, RED = ipmatrix.IpSpBKP, ipmatrix.IpRedSpBKP
MOD3 = [np.arange(b, 210, 3) for b in range(3)]


def with_pattern(n, r, c, v, nan_below):
    b = band_qp(n)
    prog = problems.Program(n, b.me, b.m, problems._csr(r, c, v, n), b.A, b.C, b.c, b.b, b.d)
    return with_lower_nan(prog)[0] if nan_below else prog


def dense_blocks(members, integer=False, nan_below=True):
    """every pair of a component (`members`: one ascending list each) stored; its values come from its number and length alone"""
    r, c, v = [], [], []
    for b, m in enumerate(members):
        rng, k = np.random.default_rng(5 + b), len(m)
        M = rng.uniform(-1, 1, (k, k))
        B = rng.integers(-8, 9, (k, k)).astype(float) if integer else M @ M.T / k + np.diag(rng.uniform(.5, 1.5, k))
        i, j = np.triu_indices(k)
        r.append(np.asarray(m)[i]), c.append(np.asarray(m)[j]), v.append(B[i, j])
    return with_pattern(sum(map(len, members)), np.concatenate(r), np.concatenate(c), np.concatenate(v), nan_below and not integer)


def chain(integer):
    n, ev, rng = 8300, np.arange(0, 8200, 2), np.random.default_rng(3)
    v = np.concatenate([rng.integers(1, 9, n), rng.integers(-8, 9, 4099)] if integer else [rng.uniform(4, 6, n), rng.uniform(-1, 1, 4099)])
    return with_pattern(n, np.concatenate([np.arange(n), ev[:-1]]), np.concatenate([np.arange(n), ev[1:]]), v.astype(float), not integer)


def run(M, prog, s, y, pattern=False):
    before = M.q_values().copy()
    v, Qs = M.q_sparse_bfgs_update(s, y, pattern=pattern, want_v=True, want_Qs=True)
    first, member, _full = hu.q_components_model(prog.Q[0], prog.Q[1], prog.n)
    rep = M.q_sparse_bfgs_report()
    assert rep.shape == (len(first) - 1, 8) and bits(rep[:, 5], member[first[:-1]]) and bits(rep[:, 6], np.diff(first)) and (rep[:, 2] == 0.2).all()
    return rep, v, Qs, before, M.q_values(), first, member


def block_sums(terms, first, member):
    of = np.repeat(np.arange(len(first) - 1), np.diff(first))
    out, mag = np.zeros(len(first) - 1, dtype=terms.dtype), np.zeros(len(first) - 1, dtype=terms.dtype)
    np.add.at(out, of, terms[member]), np.add.at(mag, of, np.abs(terms[member]))
    return out, mag


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("name,cls", [("wave", SP), ("group", RED), ("chain", SP), ("chain", RED)])
def test_shapes(name, cls, integer):
    L = {"wave": 70, "group": 257, "chain": 0}[name]
    prog = dense_blocks([np.arange(b, 3 * L, 3) for b in range(3)], integer) if L else chain(integer)
    rng, n, low = np.random.default_rng(2), prog.n, np.isnan(np.asarray(prog.Q[2]))
    M = handle(cls, prog)
    if integer:
        s, y = rng.integers(-8, 9, (2, n)).astype(float)
        rep, v, Qs, before, after, first, member = run(M, prog, s, y, not L)
        want = sym_terms(prog.Q, s, np.int64)[0]
        sums = [block_sums(t.astype(np.int64), first, member)[0] for t in (s * y, s * want)]
        assert bits(Qs, want) and bits(rep[:, 0], sums[0]) and bits(rep[:, 1], sums[1])
        return
    s = rng.normal(size=n) * rng.choice([1e-2, 1.0, 1e2], n)
    first, member, _f = hu.q_components_model(prog.Q[0], prog.Q[1], n)
    of = np.repeat(np.arange(len(first) - 1), np.diff(first))[np.argsort(member)]
    y = sym_terms(prog.Q, s, np.float64)[0] * np.where(of % 3 == 0, -0.5, 1.1) * rng.uniform(0.9, 1.1, n)  # every third block damped
    y[member[first[2]]] = np.nan  # block 2: a NaN that reaches no other block
    if not L:
        s[member[first[1]]] = 0.0  # block 1, a singleton: left alone, zero
    rep, v, Qs, before, after, first, member = run(M, prog, s, y, not L)
    assert low.any() and np.isnan(after[low]).all() and np.isfinite(after[~low]).all() and np.isfinite(Qs).all()
    q, mag, _off, cnt = sym_terms(prog.Q, s, ld)
    assert (np.abs(Qs - q) <= (cnt + 1) * U * mag).all()
    for col, terms in ((0, s * y), (1, s * Qs), (4, s * v)):
        t, m = block_sums(terms.astype(ld), first, member)
        use = np.isfinite(m) & ((rep[:, 7] == 1) | (col != 4))  # (sv is a sum of its own on a damped block alone)
        assert (np.abs(rep[use, col] - t[use]) <= (np.diff(first)[use] + 2) * U * m[use]).all(), col
    v2, x2, out, theta = hu.q_sparse_bfgs_replay(rep, (prog.Q[0], prog.Q[1], before), y, Qs, first, member)
    assert bits(v, v2) and bits(after, x2) and bits(rep[:, 7], out) and bits(rep[:, 3], theta) and bits(rep[out == 0, 4], rep[out == 0, 0])
    assert rep[:3, 7].tolist() == [1, 0 if L else 2, 3] and not bits(after[~low], before[~low])
    M.update(prog)  # the same bits from call to call
    assert bits(run(M, prog, s, y, not L)[4], after)


def test_clamp_and_partition_against_q_bfgs_update():
    """Q = -I on three components of 5 (stored zeros join them), so sQs = -s's; a fourth with a zero diagonal.  sy = 2 sQs: theta
    would be -0.8 and is 0, v = Q s; sy = 0.5 sQs: 1.6 and is 1, v = y, reported damped; sy = 0.1 sQs: not damped; sQs = sy = 0:
    theta 1, outcome 2.  The same reported sums without the clamp give -0.8 and 1.6 - the clamp; hqpkkt_q_bfgs_update with
    bsize 0 on the same data has one block and other values - the partition."""
    prog = dense_blocks([np.arange(b, 20, 4) for b in range(4)])
    r, ix, x = rows_of(prog.Q), np.asarray(prog.Q[1]), np.asarray(prog.Q[2])
    prog = with_q(prog, np.where(np.isnan(x), x, np.where((r == ix) & (r % 4 != 3), -1.0, 0.0)))
    s = np.random.default_rng(4).normal(size=20)
    y = -s * np.array([2.0, 0.5, 0.1, 0.0])[np.arange(20) % 4]
    rep, v, Qs, before, after, first, member = run(handle(SP, prog, zd_policy=-1), prog, s, y)
    assert bits(Qs, np.where(np.arange(20) % 4 != 3, -s, 0.0)) and rep[:, 3].tolist() == [0.0, 1.0, 1.0, 1.0] and rep[:, 7].tolist() == [1, 1, 0, 2]
    assert bits(v[member[:5]], Qs[member[:5]]) and bits(v[member[5:]], y[member[5:]])
    with np.errstate(all="ignore"):
        assert np.abs(hu._damped(rep, np.arange(20) % 4, y, Qs)[5] - [-0.8, 1.6, 1.0, 1.0]).max() < 1e-15
    G = handle(SP, prog, zd_policy=-1)
    G.q_bfgs_update(s, y, gamma=0.2, bsize=0, pattern=True)
    assert G.q_bfgs_report().shape == (1, 8) and not bits(G.q_values()[~np.isnan(x)], after[~np.isnan(x)])


def test_bits_do_not_depend_on_where_the_variables_lie():
    """three components of 70 at i mod 3, and the same values with the components' places exchanged (b -> 2 - b)"""
    res = []
    for members in (MOD3, MOD3[::-1]):
        prog, rng = dense_blocks(members), np.random.default_rng(6)
        sb, fb = rng.normal(size=(3, 70)), rng.uniform(0.9, 1.1, (3, 70)) * np.array([[-0.5], [1.1], [1.1]])
        s, f = np.zeros(210), np.zeros(210)
        for b, m in enumerate(members):
            s[m], f[m] = sb[b], fb[b]
        rep, v, Qs, before, after, first, member = run(handle(SP, prog), prog, s, f * sym_terms(prog.Q, s, np.float64)[0])
        D = np.zeros((210, 210))
        D[rows_of(prog.Q), np.asarray(prog.Q[1])] = after
        rep = rep[::-1] if res else rep  # (blocks are numbered by their smallest variable: reversed in the second layout)
        res.append([rep[:, :5]] + [D[np.ix_(m, m)][np.triu_indices(70)] for m in members] + [v[m] for m in members])
    assert all(bits(a, b) for a, b in zip(*res)) and (res[0][0][:, 3] != 1.0).any()


def test_refusals_and_the_handle_afterwards():
    from common import new_d
    prog, clean = dense_blocks(MOD3), dense_blocks(MOD3, nan_below=False)
    r, ix = rows_of(prog.Q), np.asarray(prog.Q[1])
    keep = ~((r == 0) & (ix == 3))
    holed = with_pattern(210, r[keep], ix[keep], np.asarray(prog.Q[2])[keep], False)
    s = np.random.default_rng(8).normal(size=210)
    y = 1.1 * sym_terms(prog.Q, s, np.float64)[0]
    H, u = handle(SP, holed), _lib.QBfgsUpdate()
    u.s, u.y, u.gamma, u.alpha = s.ctypes.data, y.ctypes.data, 0.2, 1.0
    call = lambda: _lib.lib().hqpkkt_q_sparse_bfgs_update(H._h, u)
    assert call() == _lib.E_FORMAT and bits(H.q_values(), holed.Q[2])  # FULL with one pair missing: Q unchanged
    u.fill, u.bsize = _lib.HQPKKT_QBFGS_PATTERN, 5
    assert call() == _lib.E_RANGE
    u.bsize, u.gamma = 0, -0.2
    assert call() == _lib.E_RANGE
    docp = problems.with_dense_hessian(problems.lq_docp(4, 3, 2))
    D = ipmatrix.IpLQDOCP(q_dense=True)
    D.init(docp)
    for refused in (H.q_sparse_bfgs_report, lambda: D.q_sparse_bfgs_update(np.ones(docp.n), np.ones(docp.n))):  # (no update yet; dense Q_k)
        with pytest.raises(ipmatrix.KktError) as e:
            refused()
        assert e.value.code == _lib.E_INTERN
    u.gamma = 0.2
    assert call() == _lib.OK and H.q_sparse_bfgs_report().shape == (3, 8)
    # afterwards: as a fresh handle given q_values(); on a DOCP's stage blocks the bits of hqpkkt_q_bfgs_update, detected blocks
    sd = np.random.default_rng(9).normal(size=docp.n)
    for cls, p, s, y in ((SP, clean, s, y), (RED, clean, s, y), (ipmatrix.IpLQDOCP, docp, sd, 1.1 * sym_terms(docp.Q, sd, np.float64)[0])):
        st = problems.ip_state(p, seed=12, spread=1.0)
        M = handle(cls, p)
        M.factor(p, st[0], st[1])
        M.q_sparse_bfgs_update(s, y)
        with pytest.raises(ipmatrix.KktError) as e:
            M.solve(p, *st, *new_d(p))
        assert e.value.code == _lib.E_INTERN
        p2 = with_q(p, M.q_values())
        a, b = _state_bits(M, p2, st), _state_bits(handle(cls, p2), p2, st)
        assert len(a) == len(b) and all(bits(g, h) for g, h in zip(a, b)) and a[0] == 0.0 and not bits(p2.Q[2], p.Q[2])
        if p is docp:
            B = handle(cls, p)
            B.q_bfgs_update(s, y, gamma=0.2, bsize=-1)
            assert bits(B.q_values(), p2.Q[2]) and bits(B.q_bfgs_report()[:, :5], M.q_sparse_bfgs_report()[:, :5])
