"""GPU tests of the in-place update of the dense stage Hessians (hqpkkt_update_stage_hessians, hqpkkt_hessian_product;
hqp_amd/csrc/staged_hess_update.hip.h): exact on integer operands against int64 numpy, within (3 r + 4) 2^-53 of the longdouble
value on real ones, packed against unpacked bit for bit, the skips, the hand-over rule, factor / step / residuum / mehrotra
against a fresh handle that was handed the updated blocks, the public product, and the BFGS update end to end.

Shapes: hessian_update_cases.ORDERS, every case on a packed and on an unpacked handle."""
import numpy as np
import pytest

import hessian_update_cases as H
from common import new_d
from hqp_amd import _lib, ipmatrix, problems
from hqp_amd.hessian_update import bfgs_terms

pytestmark = pytest.mark.gpu

LAYOUTS = [True, False]  # packed, unpacked
BIG = (313, 384, 220)


def _floats(blocks):
    return [np.asarray(B, dtype=np.float64) for B in blocks]


def _handle(nz, blocks, packed, device=False, bounds=False):
    M = H.handle(packed, device_vectors=device)
    dq = H.block_docp(nz, _floats(blocks), bounds=bounds)
    if device:
        import torch
        dq.Qd = [torch.as_tensor(B).cuda() for B in dq.Qd]
        dq.F = [torch.as_tensor(f).cuda() for f in dq.F]
    M.init_dense(dq)
    return M, dq


def _sym(rng, nz):
    U = rng.standard_normal((nz, nz)) * 10.0 ** rng.uniform(-3, 3, (nz, nz))
    return np.triu(U) + np.triu(U, 1).T


def _spread(rng, k):
    return rng.standard_normal(k) * 10.0 ** rng.uniform(-3, 3, k)


def _views(M, nz):
    return [M.stage_hessian(k) for k in range(len(nz))]


def _assert_exact(M, nz, want, label):
    """stage_hessian(k) is the int64 result exactly, the padding columns +0.0, compared as bits."""
    for k, W in enumerate(want):
        got = M.stage_hessian(k)
        assert np.isfinite(got).all(), (label, k)
        assert H.bits(got, H.padded(np.asarray(W, dtype=np.float64))), (label, k, nz[k])


# (r, beta per stage, with diag): beta in {1, 0, 2, -1} in every stage once, r in {0, 1, 2, 4}, with and without diag
INT_STEPS = [(0, (1, 0, 2), True), (1, (0, 2, -1), False), (2, (-1, 1, 0), True), (4, (2, -1, 1), False), (4, (1, 1, 1), True)]


@pytest.mark.parametrize("nz", H.ORDERS)
def test_exact_on_integers(nz):
    """Q_k symmetric integers |q| <= 2^20, u integers |u| <= 2^10, c in -3 .. 3, d integers: five updates one after the
    other, each against the int64 result, on a packed and an unpacked handle; their views are bit-identical."""
    rng = np.random.default_rng(sum(nz))
    blocks = H.int_blocks(rng, nz)
    Ms = [_handle(nz, blocks, p)[0] for p in LAYOUTS]
    want = blocks
    for step, (r, beta, with_diag) in enumerate(INT_STEPS):
        U, coef, beta, diag = H.int_update(rng, nz, r, beta, with_diag)
        want, _ = H.apply(want, nz, U, coef, beta, diag, np.int64)
        assert max(int(np.abs(W).max()) for W in want) < 2 ** 50
        for M in Ms:
            M.update_stage_hessians(U, coef, beta=beta, diag=diag)
            _assert_exact(M, nz, want, (step, r))
        for a, b in zip(_views(Ms[0], nz), _views(Ms[1], nz)):
            assert H.bits(a, b), step


@pytest.mark.parametrize("nz", H.ORDERS)
@pytest.mark.parametrize("r", [1, 4])
def test_bound_on_reals(nz, r):
    """Operands with full mantissas, magnitudes over 10^+-3: every entry within (3 r + 4) 2^-53 S of the longdouble value, S =
    |beta||Q_ij| + |d_i| [i = j] + sum |c_j||u_i||u_j| - one rounding for the scale, one for the diagonal, three per term if
    nothing is fused, with slack for compounding.  Every block symmetric bit for bit, packed and unpacked bit-identical, a
    second run from the same start bit-identical."""
    rng = np.random.default_rng(sum(nz) + r)
    blocks = [_sym(rng, v) for v in nz]
    n = sum(nz)
    U = [_spread(rng, n) for _ in range(r)]
    coef = _spread(rng, len(nz) * r).reshape(len(nz), r)
    beta, diag = _spread(rng, len(nz)), _spread(rng, n)
    want, scale = H.apply(blocks, nz, U, coef, beta, diag, np.longdouble)
    runs = []
    for packed in LAYOUTS:
        M, dq = _handle(nz, blocks, packed)
        for again in range(2):
            if again:
                M.update_dense(dq)  # (the same start: the blocks handed over anew)
            M.update_stage_hessians(U, coef, beta=beta, diag=diag)
            runs.append(_views(M, nz))
    for k, v in enumerate(nz):
        got = runs[0][k]
        assert (got[:, v:] == 0.0).all() and not np.signbit(got[:, v:]).any()
        G = got[:, :v]
        assert H.bits(G, G.T), k
        err = np.abs(G.astype(np.longdouble) - want[k])
        bound = (3 * r + 4) * 2.0 ** -53 * scale[k]
        worst = float((err / np.where(bound > 0, bound, 1)).max())
        print(f"order {v}, r = {r}: largest error {worst:.3f} of the bound")
        assert (err <= bound).all(), (k, v, worst)
        for other in runs[1:]:
            assert H.bits(got, other[k]), k


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("nz", [BIG, (402, 311, 320)])
def test_skips(nz, packed):
    rng = np.random.default_rng(11)
    off = H.offsets(nz)
    blocks = H.int_blocks(rng, nz)
    M, dq = _handle(nz, blocks, packed)
    # a stage with beta = 1, c = 0 and no diag is not touched, whatever its slices hold; the others change
    U, coef, beta, _ = H.int_update(rng, nz, 2, (2, 1, -1), False)
    coef[1] = 0.0
    for u in U:
        u[off[1]: off[2]] = np.nan
    before = M.stage_hessian(1)
    M.update_stage_hessians(U, coef, beta=beta)
    want, _ = H.apply(blocks, nz, U, coef, beta, None, np.int64)
    _assert_exact(M, nz, want, "untouched stage")
    assert H.bits(M.stage_hessian(1), before)
    assert not np.array_equal(want[0], blocks[0]) and not np.array_equal(want[2], blocks[2])
    # a term with c = 0 in every stage whose vector is all NaN and Inf leaves finite, correct values
    U, coef, beta, diag = H.int_update(rng, nz, 3, (1, 2, 1), True)
    coef[:, 1] = 0.0
    U[1][:] = np.nan
    U[1][::3] = np.inf
    coef[2, 0] = 0.0
    U[0][off[2]:] = -np.inf  # (and a term skipped in one stage alone)
    M.update_stage_hessians(U, coef, beta=beta, diag=diag)
    want, _ = H.apply(want, nz, U, coef, beta, diag, np.int64)
    _assert_exact(M, nz, want, "zero coefficient")
    # beta = 0: blocks full of NaN are not read
    dq.Qd = [np.full((v, v), np.nan) for v in nz]
    M.update_dense(dq)
    assert all(np.isnan(M.stage_hessian(k)[:, :v]).all() for k, v in enumerate(nz))
    U, coef, beta, diag = H.int_update(rng, nz, 2, (0, 0, 0), True)
    M.update_stage_hessians(U, coef, beta=beta, diag=diag)
    want, _ = H.apply(dq.Qd, nz, U, coef, beta, diag, np.int64)
    _assert_exact(M, nz, want, "beta = 0")


def _assert_product(M, nz, blocks, x, stages, label):
    """hessian_product against numpy on the given blocks within (nz + 1) 2^-52 sum |q x| per row (any order of the sums)."""
    off = H.offsets(nz)
    y = M.hessian_product(x)
    for k in stages:
        B = np.asarray(blocks[k], dtype=np.float64)
        xk = x[off[k]: off[k + 1]]
        ref = B.astype(np.longdouble) @ xk.astype(np.longdouble)
        bound = (nz[k] + 1) * 2.0 ** -52 * (np.abs(B) @ np.abs(xk))
        yk = y[off[k]: off[k + 1]]
        assert np.isfinite(yk).all(), (label, k)
        assert (np.abs(yk.astype(np.longdouble) - ref) <= bound).all(), (label, k)


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("nz", [BIG, (402, 311, 320), (256, 129, 640)])
def test_neighbouring_slices_do_not_enter(nz, packed):
    """Stage 1 updated, stages 0 and 2 skipped, NaN in the neighbours' slices of U: nothing of it reaches stage 1, its tile
    padding included - a NaN there would show in the product.  Then with a diagonal, whose neighbouring slices hold NaN as
    well: the neighbours are no longer skipped (they receive their NaN), stage 1 is exact and its product finite."""
    rng = np.random.default_rng(13)
    off = H.offsets(nz)
    blocks = H.int_blocks(rng, nz)
    M, _dq = _handle(nz, blocks, packed)
    x = rng.integers(-8, 9, sum(nz)).astype(np.float64)
    U, coef, beta, diag = H.int_update(rng, nz, 2, (1, -1, 1), True)
    coef[0] = coef[2] = 0.0
    coef[1] = [2.0, -3.0]
    for v in U + [diag]:
        v[: off[1]] = np.nan
        v[off[2]:] = np.nan
    M.update_stage_hessians(U, coef, beta=beta)
    want, _ = H.apply(blocks, nz, U, coef, beta, None, np.int64)
    _assert_exact(M, nz, want, "neighbours skipped")
    _assert_product(M, nz, want, x, (0, 1, 2), "neighbours skipped")
    M.update_stage_hessians(U, coef, beta=beta, diag=diag)
    want1, _ = H.apply(want, nz, U, coef, beta, diag, np.float64)
    assert H.bits(M.stage_hessian(1), H.padded(want1[1]))
    for k in (0, 2):  # (the neighbours: their own NaN on the diagonal, nothing else)
        got, off_diag = M.stage_hessian(k)[:, : nz[k]], ~np.eye(nz[k], dtype=bool)
        assert np.isnan(np.diag(got)).all() and H.bits(got[off_diag], want[k][off_diag])
    _assert_product(M, nz, want1, x, (1,), "neighbours with NaN")


@pytest.mark.parametrize("packed", LAYOUTS)
def test_hand_over_rule(packed):
    nz = BIG
    n = sum(nz)
    M = H.handle(packed)
    assert H.analyze_only(M, nz) == 0
    d = np.arange(1.0, n + 1.0)
    with pytest.raises(ipmatrix.KktError) as e:  # no block has arrived: beta = 1 on a stage the call touches
        M.update_stage_hessians([], np.zeros((3, 0)), diag=d)
    assert e.value.code == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as e:  # ... and nothing was launched: the handle is not even on the device
        M.stage_hessian(0)
    assert e.value.code == _lib.E_INTERN
    M.update_stage_hessians([], np.zeros((3, 0)), beta=[0.0, 0.0, 1.0])  # (stage 2 is left alone)
    dq = H.block_docp(nz, None)
    with pytest.raises(ipmatrix.KktError) as e:
        M.update_dense(dq)  # hqpkkt_set_values_staged(Qx = NULL, F, ..): block 2 is missing
    assert e.value.code == _lib.E_INTERN
    M.update_stage_hessians([], np.zeros((3, 0)), beta=[1.0, 1.0, 0.0], diag=d)
    M.update_dense(dq)
    off = H.offsets(nz)
    for k in range(3):
        assert H.bits(M.stage_hessian(k), H.padded(np.diag(d[off[k]: off[k + 1]])))
    x = np.random.default_rng(3).standard_normal(n)
    assert H.bits(M.hessian_product(x), d * x)


def _code(call):
    try:
        call()
    except ipmatrix.KktError as e:
        return e.code
    return 0


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("nz", H.ORDERS)
def test_nothing_stale(nz, packed):
    """Handle A: positive-definite integer blocks, then an integer update on the device.  Handle B: a fresh handle that is
    handed the numpy-updated blocks.  factor + step and residuum are bit-identical, with bounds on the controls as rows of C so
    that z and w are not empty.  A step between the change and the next factor answers on A what it answers on a handle
    whose block came through set_stage_hessian."""
    rng = np.random.default_rng(17)
    blocks = H.int_blocks(rng, nz, spd=True)
    U, coef, beta, diag = H.int_update(rng, nz, 2, (1, 2, 1), True, positive=True)
    updated, _ = H.apply(blocks, nz, U, coef, beta, diag, np.int64)
    A, dq = _handle(nz, blocks, packed, bounds=True)
    C_, _ = _handle(nz, blocks, packed, bounds=True)
    st = problems.ip_state(dq, 3, 1.0)
    for M in (A, C_):
        M.factor(dq, st[0], st[1])
        M.step(dq, *st, *new_d(dq))
    A.update_stage_hessians(U, coef, beta=beta, diag=diag)
    for k, W in enumerate(updated):
        C_.set_stage_hessian(k, np.asarray(W, dtype=np.float64))
    codes = [_code(lambda M=M: M.step(dq, *st, *new_d(dq))) for M in (A, C_)]
    assert codes[0] == codes[1], codes
    B, dqb = _handle(nz, updated, packed, bounds=True)
    for k in range(3):
        assert H.bits(A.stage_hessian(k), B.stage_hessian(k))
    outs = []
    for M in (A, B):
        M.factor(dq, st[0], st[1])
        d = new_d(dq)
        M.step(dq, *st, *d)
        outs.append(d + [np.array([M.residuum(dq, *st, *d)])])
    for q, (a, b) in enumerate(zip(*outs)):
        assert np.isfinite(a).all() and H.bits(a, b), q
    assert np.abs(outs[0][0]).max() > 0.0
    if nz != BIG:
        return
    xa, _y, _z, _w, ia = A.mehrotra(dq)
    xb, _y, _z, _w, ib = B.mehrotra(dqb)
    print(f"mehrotra: iterations {ia['iters']} / {ib['iters']}, result {ia['result']} / {ib['result']}")
    assert ia["result"] == ib["result"] and ia["iters"] == ib["iters"] and ia["iters"] > 1
    assert H.bits(xa, xb)


@pytest.mark.parametrize("packed", LAYOUTS)
def test_hessian_product(packed):
    nz = BIG
    rng = np.random.default_rng(19)
    blocks = [_sym(rng, v) for v in nz]
    M, _dq = _handle(nz, blocks, packed)
    x = _spread(rng, sum(nz))
    y = M.hessian_product(x)
    assert H.bits(y, M.hess_symv(x)) and np.abs(y).max() > 0
    import torch
    D, _dq = _handle(nz, blocks, packed, device=True)
    yd = D.hessian_product(torch.as_tensor(x).cuda())
    assert yd.is_cuda and H.bits(yd.cpu().numpy(), y)
    csr = ipmatrix.IpLQDOCP()  # HQPKKT_HESS_CSR
    csr.init_dense(H.block_docp(nz, None))
    assert _code(lambda: csr.hessian_product(x)) == _lib.E_INTERN


@pytest.mark.parametrize("packed", LAYOUTS)
def test_integers_with_device_vectors(packed):
    """The integer case with torch CUDA U and diag, host coef and beta: the same exact result."""
    import torch
    nz = BIG
    rng = np.random.default_rng(23)
    blocks = H.int_blocks(rng, nz)
    M, _dq = _handle(nz, blocks, packed, device=True)
    want = blocks
    for r, beta, with_diag in INT_STEPS[1:4]:
        U, coef, beta, diag = H.int_update(rng, nz, r, beta, with_diag)
        want, _ = H.apply(want, nz, U, coef, beta, diag, np.int64)
        M.update_stage_hessians([torch.as_tensor(u).cuda() for u in U], coef, beta=beta,
                                diag=None if diag is None else torch.as_tensor(diag).cuda())
        _assert_exact(M, nz, want, r)


def test_bfgs_update_end_to_end():
    """Orders (313, 384, 220), s and y integer-valued; the middle block is large against y, so it takes the damped branch.
    The blocks after bfgs_update against the numpy application, in longdouble, of the terms bfgs_terms returns for the
    device's own hessian_product - the real-operand bound with r = 2 -, and the secant property along s: s'Q+s against s'v
    within (nz + 8) 2^-52 sum_ij |s_i| S_ij |s_j|, S the per-entry scale of that bound (the sum runs over the update's terms:
    the subtracted and the added rank-one term cancel)."""
    nz = BIG
    rng = np.random.default_rng(29)
    off = H.offsets(nz)
    blocks = []
    for k, v in enumerate(nz):
        A = rng.standard_normal((v, v))
        blocks.append((A @ A.T + v * np.eye(v)) * (1000.0 if k == 1 else 1.0))
        blocks[-1] = np.triu(blocks[-1]) + np.triu(blocks[-1], 1).T
    s = rng.integers(-8, 9, sum(nz)).astype(np.float64)
    y = 300.0 * s + rng.integers(-2, 3, sum(nz))
    for packed in LAYOUTS:
        M, _dq = _handle(nz, blocks, packed)
        Qs = M.hessian_product(s)
        U, coef = bfgs_terms(s, y, Qs, off)
        Ua, ca = M.bfgs_update(s, y)
        assert H.bits(ca, coef) and all(H.bits(a, b) for a, b in zip(Ua, U))
        assert not np.array_equal(U[0][off[1]: off[2]], y[off[1]: off[2]]) and np.array_equal(U[0][: off[1]], y[: off[1]])  # (damped: the middle block alone)
        assert (coef[:, 0] > 0).all() and (coef[:, 1] < 0).all()
        want, scale = H.apply(blocks, nz, U, coef, None, None, np.longdouble)
        for k, v in enumerate(nz):
            got = M.stage_hessian(k)[:, :v].astype(np.longdouble)
            err = np.abs(got - want[k])
            bound = 10 * 2.0 ** -53 * scale[k]
            assert (err <= bound).all(), (k, float((err / bound).max()))
            sk = s[off[k]: off[k + 1]].astype(np.longdouble)
            vk = U[0][off[k]: off[k + 1]].astype(np.longdouble)
            sQs, sv = sk @ got @ sk, sk @ vk
            sbound = (v + 8) * 2.0 ** -52 * (np.abs(sk) @ scale[k] @ np.abs(sk))
            print(f"order {v}: s'Q+s - s'v = {float(sQs - sv):.3e}, bound {float(sbound):.3e}")
            assert sv > 0 and abs(sQs - sv) <= sbound, (k, float(sQs - sv), float(sbound))
