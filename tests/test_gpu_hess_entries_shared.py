"""GPU tests of what the entries on the dense stage Hessians and on the sparse Q share: one pair of buffers for a host
caller's vectors (CallerVecs, hqpkkt_handle.hpp), one set of work vectors and one update launch (HessCall,
staged_hess_host.hip.h).  Entries of different kinds run back to back on ONE handle with nothing synchronised in
between; every vector, report and block must be bit for bit what the same call gives alone on a fresh handle that was
handed the state before it.  A host caller's inputs are overwritten with NaN the moment a call returns, so a vector the
stream still reads shows.

Shapes.  K = 2, so three blocks.  (5, T - 1, T + 3) lies around the edge of the T = 128 tile; no order below 220 packs
(packed_hessian_cases.packs), so (220, T + 3, 2 T) adds the smallest order that packs, a block that stays dense beside it,
and two whole tile rows.  A stage of order 0 has no case: the analysis refuses a stage without a state (asserted below).
The sparse Q: problems.banded_qp(300, 8, 5) on Hqp_IpRedSpBKP.

Models.  The rank-4 update on integers is exact in int64.  The BFGS update follows it on integers: s'y and s'Qs are the
int64 sums, no stage damps, v = y, the coefficients are bfgs_terms'.  The blocks are no integers from there on: the row
maxima are still numpy's bit for bit (a maximum rounds nothing), the off-diagonal sums lie within nz 2^-53 sum_j |q_ij|
of longdouble (nz - 1 additions in any order)."""
import numpy as np
import pytest

import hessian_guard_cases as G
import hessian_update_cases as H
import packed_hessian_cases as P
from hqp_amd import _lib, ipmatrix, problems
from hqp_amd import hessian_update as hu

pytestmark = pytest.mark.gpu

T = P.T
ORDERS = [(5, T - 1, T + 3), (220, T + 3, 2 * T)]
SY, SQS, GAMMA, THETA, SV, C0, C1, OUTCOME = range(8)


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _np(a):
    return None if a is None else (a.cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a))


class Caller:
    """A caller's vectors: numpy arrays that are poisoned after the call (host), or CUDA tensors that stay as they are."""

    def __init__(self, device):
        self.device = device
        self.given = []

    def vec(self, a):
        a = np.array(a, dtype=np.float64)
        if self.device:
            import torch
            return torch.as_tensor(a).cuda()
        self.given.append(a)
        return a

    def poison(self):
        for a in self.given:
            a[:] = np.nan
        self.given = []


def test_a_stage_of_order_zero_is_refused():
    assert H.analyze_only(H.handle(True), (0, 5, T - 1)) == _lib.E_RANGE


# ---- the dense stage Hessians ---------------------------------------------------------------------------------------

def _dense_handle(nz, blocks, packed, device):
    M = H.handle(packed, device_vectors=device)
    dq = H.block_docp(nz, [np.array(Q, dtype=np.float64) for Q in blocks])
    if device:
        import torch
        dq.Qd = [torch.as_tensor(Q).cuda() for Q in dq.Qd]
        dq.F = [torch.as_tensor(f).cuda() for f in dq.F]
    M.init_dense(dq)
    return M


def _blocks_of(M, nz):
    """The blocks as they lie in the handle (waits for its stream): (arena views, the blocks themselves)."""
    views = [M.stage_hessian(k) for k in range(len(nz))]
    return views, [a[:, :v].copy() for a, v in zip(views, nz)]


def _dense_operands(nz, seed):
    """Integers throughout: positive-definite blocks, a rank-4 update with positive coefficients and diagonal (the blocks
    stay positive definite), and behind it s and y = 2 Q s + e for the UPDATED blocks; every sum below 2^53 (asserted)."""
    rng = np.random.default_rng(seed)
    off = H.offsets(nz)
    n = int(off[-1])
    blocks = H.int_blocks(rng, nz, spd=True)
    U = [rng.integers(-2 ** 6, 2 ** 6 + 1, n) for _ in range(4)]
    coef = rng.integers(1, 4, (3, 4))
    beta = np.array([1, 2, 1])
    diag = rng.integers(0, 2 ** 10, n)
    updated, _scales = H.apply(blocks, nz, U, coef, beta, diag, np.int64)
    s = rng.integers(1, 2 ** 6 + 1, n) * rng.choice([-1, 1], n)
    Qs = np.concatenate([B @ s[off[k]: off[k + 1]] for k, B in enumerate(updated)])
    y = 2 * Qs + rng.integers(-2, 3, n)
    for k, B in enumerate(updated):
        b = slice(int(off[k]), int(off[k + 1]))
        assert int((np.abs(B) @ np.abs(s[b])).max()) < 2 ** 53
        assert int(np.abs(s[b]) @ np.abs(y[b])) < 2 ** 53 and int(np.abs(s[b]) @ np.abs(Qs[b])) < 2 ** 53
    x = rng.integers(-8, 9, n)
    return dict(blocks=blocks, U=U, coef=coef, beta=beta, diag=diag, updated=updated, s=s, y=y, Qs=Qs, x=x)


RESTART = (0, 1, 0)
RESTART_EPS = 2.0 ** -12


def _dense_calls(op):
    """The six calls, each (name, call(M, caller) -> what it returns)."""
    return [
        ("update", lambda M, c: M.update_stage_hessians([c.vec(u) for u in op["U"]], _f(op["coef"]), beta=_f(op["beta"]), diag=c.vec(op["diag"]))),
        ("bfgs", lambda M, c: M.bfgs_update_device(c.vec(op["s"]), c.vec(op["y"]), want_v=True)),
        ("row_stats", lambda M, c: M.hessian_row_stats()),
        ("eigen_control", lambda M, c: M.eigen_control(G.EPS, from_bfgs=True)),
        ("restart", lambda M, c: M.restart_hessians(RESTART_EPS, stages=RESTART)),
        ("product", lambda M, c: M.hessian_product(c.vec(op["x"]))),
    ]


def _flat(out):
    """What a call returned as a list of numpy arrays (after the handle's stream has been waited for)."""
    if out is None:
        return []
    return [_np(a) for a in (out if isinstance(out, tuple) else (out,))]


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("nz", ORDERS)
def test_dense_entries_back_to_back(nz, packed, device):
    op = _dense_operands(nz, 7 + sum(nz))
    calls = _dense_calls(op)
    off = H.offsets(nz)
    # the shared handle: the six calls, nothing in between; the last one waits for the stream, the reports do too
    A = _dense_handle(nz, op["blocks"], packed, device)
    caller = Caller(device)
    raw = []
    for _name, call in calls:
        raw.append(call(A, caller))
        caller.poison()
    got_views, _got_blocks = _blocks_of(A, nz)
    got = [_flat(r) for r in raw]
    got_brep, (got_erep, got_T) = A.bfgs_report(), A.eigen_report(with_T=True)
    # every call alone on a fresh handle that was handed the blocks before it
    state = [_f(B) for B in op["blocks"]]
    before = {}
    for i, (name, call) in enumerate(calls):
        before[name] = state
        F = _dense_handle(nz, before["bfgs"] if name == "eigen_control" else state, packed, device)
        c = Caller(device)
        if name == "eigen_control":  # (its floors come from the words of the update before it: the handle needs that update)
            calls[1][1](F, c)
            _v, blocks = _blocks_of(F, nz)
            assert all(H.bits(a, b) for a, b in zip(blocks, state))
        out = call(F, c)
        views, state = _blocks_of(F, nz)
        want = _flat(out)
        assert len(want) == len(got[i]) and all(H.bits(a, b) for a, b in zip(got[i], want)), name
        if name == "bfgs":
            assert H.bits(got_brep, F.bfgs_report()), name
        if name == "eigen_control":
            rep, Tm = F.eigen_report(with_T=True)
            assert H.bits(got_erep, rep) and H.bits(got_T, Tm), name
    for k, (a, w) in enumerate(zip(got_views, views)):
        assert np.isfinite(a).all() and H.bits(a, w), k
    # ... and the models of the first three
    assert all(H.bits(B, _f(W)) for B, W in zip(before["bfgs"], op["updated"]))
    for k in range(3):
        b = slice(int(off[k]), int(off[k + 1]))
        sy, sQs = int(op["s"][b] @ op["y"][b]), int(op["s"][b] @ op["Qs"][b])
        assert got_brep[k, SY] == float(sy) and got_brep[k, SQS] == float(sQs) and got_brep[k, OUTCOME] == 0.0, (k, got_brep[k])
    _U, coef = hu.bfgs_terms(_f(op["s"]), _f(op["y"]), _f(op["Qs"]), off, 0.1, 1.0)
    assert H.bits(got_brep[:, C0: C1 + 1], coef) and H.bits(got[1][0], _f(op["y"]))
    Ab = [np.abs(B).astype(np.longdouble) for B in before["row_stats"]]
    assert H.bits(got[2][0], np.concatenate([np.abs(B).max(axis=1) for B in before["row_stats"]]))
    want_sum = np.concatenate([a.sum(axis=1) - np.diag(a) for a in Ab])
    bound = np.concatenate([a.shape[0] * np.longdouble(2.0) ** -53 * a.sum(axis=1) for a in Ab])
    assert (np.abs(got[2][1].astype(np.longdouble) - want_sum) <= bound).all()
    # the restart has made stage 1 a diagonal block, and the product is of the blocks as they are now
    assert H.bits(state[1], hu.restart_model(before["restart"][1], RESTART_EPS))
    assert np.isfinite(got[5][0]).all() and np.abs(got[5][0]).max() > 0.0


# ---- the sparse Q ---------------------------------------------------------------------------------------------------

def _with_q(prog, x):
    return problems.Program(prog.n, prog.me, prog.m, (prog.Q[0], prog.Q[1], _f(x)), prog.A, prog.C, prog.c, prog.b, prog.d)


@pytest.mark.parametrize("device", [False, True])
def test_sparse_q_entries_back_to_back(device):
    prog = problems.banded_qp(300, 8, 5)
    n, me, m = prog.dims
    rng = np.random.default_rng(3)
    p, ix = np.asarray(prog.Q[0]), np.asarray(prog.Q[1])
    di = np.flatnonzero(ix == np.repeat(np.arange(n), np.diff(p)))
    q = _f(prog.Q[2])[di]
    s = rng.normal(size=n)
    y = np.where(np.arange(n) < n // 2, 1.1, -0.5) * q * s  # (the second half damps)
    x, cc, mi, yy, zz = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n), rng.normal(size=me), rng.normal(size=m)
    calls = [
        ("dscale", lambda M, c: M.q_dscale_update(c.vec(s), c.vec(y), gamma=0.2, bsize=64, want_v=True)),
        ("product", lambda M, c: M.q_product(c.vec(x))),
        ("gradient", lambda M, c: M.lagrangian_gradient(c.vec(cc), c.vec(yy), c.vec(zz), minus=c.vec(mi))),
        ("row_stats", lambda M, c: M.q_row_stats()),
    ]

    def handle(pr):
        M = ipmatrix.IpRedSpBKP(device_vectors=device)
        M.init(pr)
        return M

    A = handle(prog)
    caller = Caller(device)
    raw = []
    for _name, call in calls:
        raw.append(call(A, caller))
        caller.poison()
    got_rep = A.q_dscale_report()  # (waits for the stream)
    got = [_flat(r) for r in raw]
    got_q = _np(A.q_values())
    values = _f(prog.Q[2])
    for i, (name, call) in enumerate(calls):
        F = handle(_with_q(prog, values))
        out = call(F, Caller(device))
        values = _np(F.q_values()).copy()  # (waits for the stream)
        want = _flat(out)
        assert len(want) == len(got[i]) and all(H.bits(a, b) for a, b in zip(got[i], want)), name
        if name == "dscale":
            rep = F.q_dscale_report()
            assert H.bits(got_rep, rep), name
            v_r, q_r, out_r = hu.dscale_replay(rep, s, y, q, bsize=64)
            assert H.bits(got[0][0], v_r) and H.bits(values[di], q_r) and H.bits(rep[:, 7], out_r)
            assert set(rep[:, 7].astype(int).tolist()) == {0, 1}
    assert H.bits(got_q, values)
    assert all(np.isfinite(a).all() for g in got for a in g)
