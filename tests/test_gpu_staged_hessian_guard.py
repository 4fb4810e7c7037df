"""GPU tests of the safeguards of the dense stage Hessians (hqpkkt_hessian_row_stats, hqpkkt_restart_stage_hessians,
hqpkkt_gerschgorin_stage_hessians, hqpkkt_eigen_control_stage_hessians, hqpkkt_eigen_report;
hqp_amd/csrc/staged_hess_guard.hip.h): the row statistics against numpy, restart_Q and Gerschgorin against their models and
against the update entry, and the eigenvalue control against an exact Sturm count of the reported T, against
hessian_update.eigen_replay, against numpy.linalg.eigvalsh and against the update entry.

Shapes: hessian_guard_cases.ORDERS, every case on a packed and on an unpacked handle.  Outcome 5 of the control (a stage of
order 0) has no case here: hqpkkt_analyze_staged refuses a stage without a state, so no handle has such a stage; the model
covers it (test_staged_hessian_guard_cpu.py)."""
import numpy as np
import pytest

import hessian_guard_cases as G
import hessian_update_cases as H
from common import new_d
from hqp_amd import problems
from hqp_amd import hessian_update as hu

pytestmark = pytest.mark.gpu

LAYOUTS = [True, False]  # packed, unpacked
BIG = (313, 384, 220)
GK, THETA, STEPS, LO, HI, RHO, LAM, DK, NORMT, OUTCOME = range(10)


def _handle(nz, blocks, packed, device=False, bounds=False):
    M = H.handle(packed, device_vectors=device)
    dq = H.block_docp(nz, [np.asarray(Q, dtype=np.float64) for Q in blocks], bounds=bounds)
    if device:
        import torch
        dq.Qd = [torch.as_tensor(Q).cuda() for Q in dq.Qd]
        dq.F = [torch.as_tensor(f).cuda() for f in dq.F]
    M.init_dense(dq)
    return M, dq


def _views(M, nz):
    return [M.stage_hessian(k) for k in range(len(nz))]


def _f(a):
    return np.asarray(a, dtype=np.float64)


def _cat(parts):
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])


# ---- row statistics -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz", G.ORDERS)
def test_row_stats_on_reals(nz):
    """Full-mantissa operands: the maxima bit for bit numpy's on both layouts (so packed = unpacked), the sums within
    nz 2^-53 sum_j |q_ij| of longdouble; either output may be left out."""
    blocks = G.real_blocks(np.random.default_rng(11), nz)
    want_max = _cat([np.abs(Q).max(axis=1) for Q in blocks])
    A = [np.abs(Q).astype(np.longdouble) for Q in blocks]
    want_sum = np.concatenate([a.sum(axis=1) - np.diag(a) for a in A])
    bound = np.concatenate([a.shape[0] * np.longdouble(2.0) ** -53 * a.sum(axis=1) for a in A])
    for packed in LAYOUTS:
        M, _dq = _handle(nz, blocks, packed)
        rm, os = M.hessian_row_stats()
        assert H.bits(rm, want_max), packed
        err = np.abs(os.astype(np.longdouble) - want_sum)
        print(f"packed {packed}: offsum error / bound {float((err / bound).max()):.3g}")
        assert (err <= bound).all(), packed
        rm1, none = M.hessian_row_stats(want_sum=False)
        assert none is None and H.bits(rm1, rm)
        none, os1 = M.hessian_row_stats(want_max=False)
        assert none is None and H.bits(os1, os)  # (the same bits from run to run)


@pytest.mark.parametrize("nz", G.ORDERS)
def test_row_stats_exact_on_integers(nz):
    blocks = H.int_blocks(np.random.default_rng(12), nz)
    want_max = _cat([np.abs(Q).max(axis=1) for Q in blocks])
    want_sum = _cat([np.abs(Q).sum(axis=1) - np.abs(np.diag(Q)) for Q in blocks])
    for packed in LAYOUTS:
        M, _dq = _handle(nz, blocks, packed)
        rm, os = M.hessian_row_stats()
        assert H.bits(rm, want_max) and H.bits(os, want_sum), packed


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("nz", [BIG, (402, 311, 320), (513, 1, 2)])
def test_row_stats_nan_stays_in_its_row(nz, packed):
    """NaNs in the middle stage, handed over with three padding columns of NaN: one on the diagonal of its last row - that
    row's maximum is NaN, its off-diagonal sum is a number, the diagonal is no part of it - and, from order 3 on, one at
    (0, 1), which the symmetric block holds at (1, 0) as well: rows 0 and 1 report NaN in both statistics.  Every other
    row of the stage and the stages beside it report their numbers: the padding is never read as a value."""
    blocks = [_f(Q) for Q in H.int_blocks(np.random.default_rng(13), nz)]
    M, _dq = _handle(nz, blocks, packed)
    v = nz[1]
    wide = np.full((v, v + 3), np.nan)
    wide[:, :v] = blocks[1]
    wide[v - 1, v - 1] = np.nan
    if v >= 3:
        wide[0, 1] = np.nan
    M.set_stage_hessian(1, wide)
    rm, os = M.hessian_row_stats()
    o = int(H.offsets(nz)[1])
    nan_max = {o + v - 1} | ({o, o + 1} if v >= 3 else set())
    nan_sum = {o, o + 1} if v >= 3 else set()
    assert set(np.flatnonzero(np.isnan(rm)).tolist()) == nan_max
    assert set(np.flatnonzero(np.isnan(os)).tolist()) == nan_sum
    want_max = _cat([np.abs(Q).max(axis=1) for Q in blocks])
    want_sum = _cat([np.abs(Q).sum(axis=1) - np.abs(np.diag(Q)) for Q in blocks])
    keep_max, keep_sum = (np.array([i not in bad for i in range(sum(nz))]) for bad in (nan_max, nan_sum))
    assert H.bits(rm[keep_max], want_max[keep_max]) and H.bits(os[keep_sum], want_sum[keep_sum])


def test_row_stats_device_vectors():
    nz = (255, 257, 512)
    blocks = G.real_blocks(np.random.default_rng(14), nz)
    for packed in LAYOUTS:
        Mh, _dq = _handle(nz, blocks, packed)
        rm, os = Mh.hessian_row_stats()
        D, _dq = _handle(nz, blocks, packed, device=True)
        trm, tos = D.hessian_row_stats()
        assert trm.is_cuda and tos.is_cuda
        assert H.bits(trm.cpu().numpy(), rm) and H.bits(tos.cpu().numpy(), os)


# ---- restart_Q ------------------------------------------------------------------------------------------------------

def _restart_blocks(nz, seed):
    """Integer blocks, eps = 2^-3: in every block of order > 2 a row (and column) of zeros, which is raised to eps, and an
    entry 2^20 > 1 / eps, which is cut; entries 1 .. 7 elsewhere keep their row maximum between the clips."""
    rng = np.random.default_rng(seed)
    out = []
    for v in nz:
        U = np.triu(rng.integers(-7, 8, (v, v)))
        B = (U + np.triu(U, 1).T).astype(np.float64)
        if v > 2:
            B[1, :] = B[:, 1] = 0.0
            B[0, v - 1] = B[v - 1, 0] = 2.0 ** 20
        out.append(B)
    return out


@pytest.mark.parametrize("stages", [None, (1, 0, 1), (0, 1, 0)])
@pytest.mark.parametrize("nz", G.ORDERS)
def test_restart(nz, stages):
    eps = 0.125
    blocks = _restart_blocks(nz, 21)
    chosen = [True] * 3 if stages is None else [bool(s) for s in stages]
    want = [H.padded(hu.restart_model(Q, eps) if c else Q) for Q, c in zip(blocks, chosen)]
    if nz[0] > 2 and chosen[0]:
        dg = np.diag(want[0])
        assert dg[1] == eps and dg[0] == 8.0 and eps < dg[2] < 8.0  # (both clips act)
    diag = _cat([np.diag(hu.restart_model(Q, eps)) if c else np.zeros(Q.shape[0]) for Q, c in zip(blocks, chosen)])
    views = []
    for packed in LAYOUTS:
        M, _dq = _handle(nz, blocks, packed)
        M.restart_hessians(eps, stages)
        views.append(_views(M, nz))
        R, _dq = _handle(nz, blocks, packed)  # the twin: the update entry with beta = 0 and that diagonal
        R.update_stage_hessians([], np.zeros((3, 0)), beta=[0.0 if c else 1.0 for c in chosen], diag=diag)
        for k, (a, w, r) in enumerate(zip(views[-1], want, _views(R, nz))):
            assert H.bits(a, w), (packed, k)
            assert H.bits(a, r), (packed, k)
    for k, (a, u) in enumerate(zip(*views)):
        assert H.bits(a, u), k


@pytest.mark.parametrize("packed", LAYOUTS)
def test_restart_nothing_stale(packed):
    """factor + step and residuum after a restart are bit-identical to a fresh handle that was handed the restarted blocks."""
    nz = BIG
    blocks = H.int_blocks(np.random.default_rng(22), nz, spd=True)
    A, dq = _handle(nz, blocks, packed, bounds=True)
    st = problems.ip_state(dq, 3, 1.0)
    A.factor(dq, st[0], st[1])
    A.step(dq, *st, *new_d(dq))
    A.restart_hessians(2.0 ** -12)
    restarted = [A.stage_hessian(k)[:, :v].copy() for k, v in enumerate(nz)]
    assert all(H.bits(U, hu.restart_model(_f(Q), 2.0 ** -12)) for U, Q in zip(restarted, blocks))
    Bh, _dqb = _handle(nz, restarted, packed, bounds=True)
    outs = []
    for M in (A, Bh):
        M.factor(dq, st[0], st[1])
        d = new_d(dq)
        M.step(dq, *st, *d)
        outs.append(d + [np.array([M.residuum(dq, *st, *d)])])
    for q, (a, b) in enumerate(zip(*outs)):
        assert np.isfinite(a).all() and H.bits(a, b), q
    assert np.abs(outs[0][0]).max() > 0.0


# ---- Gerschgorin ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nz", G.ORDERS)
def test_gerschgorin_exact_on_integers(nz):
    """|q| <= 2^20 and eps = 3: every sum is an integer far below 2^53.  The blocks are bit for bit the model's - the
    off-diagonal entries and the padding with them -, the last block, dominant already, keeps its bits."""
    rng = np.random.default_rng(31)
    blocks = [_f(Q) for Q in H.int_blocks(rng, nz[:2])] + [_f(H.int_blocks(rng, nz[2:], spd=True)[0]) + 2.0 * np.eye(nz[2])]
    want = [H.padded(hu.gerschgorin_model(Q, 3.0)) for Q in blocks]
    assert H.bits(want[2], H.padded(blocks[2]))
    assert nz[0] < 2 or not H.bits(want[0], H.padded(blocks[0]))
    views = []
    for packed in LAYOUTS:
        M, _dq = _handle(nz, blocks, packed)
        M.gerschgorin_hessians(3.0)
        views.append(_views(M, nz))
        for k, (a, w) in enumerate(zip(views[-1], want)):
            assert H.bits(a, w), (packed, k)
    for k, (a, u) in enumerate(zip(*views)):
        assert H.bits(a, u), k


@pytest.mark.parametrize("packed", LAYOUTS)
def test_restart_and_gerschgorin_on_a_device_vectors_handle(packed):
    """Blocks handed over from device memory on a device_vectors handle; Gerschgorin, then a restart of two stages, nothing
    synchronised in between: the bits of a host-vector handle given the same two calls."""
    nz = (255, 257, 512)
    blocks = [_f(Q) for Q in H.int_blocks(np.random.default_rng(32), nz)]
    views = []
    for device in (False, True):
        M, _dq = _handle(nz, blocks, packed, device=device)
        M.gerschgorin_hessians(3.0)
        M.restart_hessians(2.0 ** -30, stages=[1, 0, 1])
        views.append(_views(M, nz))
    want = [hu.restart_model(hu.gerschgorin_model(Q, 3.0), 2.0 ** -30) if k != 1 else hu.gerschgorin_model(Q, 3.0) for k, Q in enumerate(blocks)]
    for k, (a, b) in enumerate(zip(*views)):
        assert H.bits(a, b) and H.bits(a, H.padded(want[k])), k


# ---- the eigenvalue control -----------------------------------------------------------------------------------------

def _check_stage(nz, k, Q0, after, rep, T, twin_after, want_outcomes=None):
    """The checks (i) - (v) of one stage: the block before the call, after it, its report and T, the twin's block."""
    v = nz[k]
    r = rep[k]
    outcome = int(r[OUTCOME])
    unit = 2.0 ** -53 * v * G.norm_inf(Q0)
    lam = float(np.linalg.eigvalsh(Q0)[0])
    print(f"stage {k} order {v}: outcome {outcome} g {r[GK]:.6g} theta {r[THETA]:.3g} steps {int(r[STEPS])} lo {r[LO]!r} rho {r[RHO]:.3g} "
          f"lambda_est {r[LAM]!r} eigvalsh {lam!r} d {r[DK]:.6g} |T| {r[NORMT]:.6g}")
    if want_outcomes is not None:
        assert outcome in want_outcomes, (k, outcome)
    # (ii) the replay of the reported T
    m = hu.eigen_replay(v, r[GK], r[THETA], int(r[STEPS]) if outcome not in (0, 5) else 0, T[k])
    assert m["outcome"] == outcome, (k, m["outcome"], outcome)
    if outcome in (1, 2, 3):
        for word, key in ((LO, "lo"), (HI, "hi"), (RHO, "rho"), (LAM, "lam"), (DK, "d"), (NORMT, "normT")):
            assert H.bits(r[word], m[key]), (k, key, r[word], m[key])
        steps = int(r[STEPS])
        assert 1 <= steps <= min(v, 128)
        # (i) the bracket is honest for the reported T
        al, be, gg = T[k][0][:steps], T[k][1][:steps], 8 * 2.0 ** -53 * r[NORMT]
        assert G.sturm_count(al, be, r[LO] - gg) == 0 and G.sturm_count(al, be, r[HI] + gg) >= 1, k
        assert r[HI] - r[LO] <= 2.0 ** -50 * r[NORMT]
        # (iii) the estimate against the block as it was read back before the call
        assert abs(r[LAM] - lam) <= r[RHO] + 8 * G.ALLOWANCE * unit, (k, r[LAM], lam, r[RHO])
    if outcome == 0:
        assert r[GK] >= r[THETA] and lam >= r[GK] - 8 * G.ALLOWANCE * unit
    # (iv) the block after the call: the twin's, given update_stage_hessians(r = 0, beta = 1, diag = d); d = 0: unchanged
    assert H.bits(after, twin_after), k
    if r[DK] == 0.0:
        assert H.bits(after, H.padded(Q0)), k
    else:
        # (v) after a shift the block is not below its floor
        assert outcome in (2, 3) and r[DK] > 0.0
        lam_new = float(np.linalg.eigvalsh(after[:, :v])[0])
        assert lam_new >= r[THETA] - 8 * G.ALLOWANCE * unit, (k, lam_new)
    return outcome


def _run_control(nz, blocks, packed, want=None, **ctl):
    M, _dq = _handle(nz, blocks, packed)
    before = [a[:, :v].copy() for a, v in zip(_views(M, nz), nz)]
    M.eigen_control(G.EPS, **ctl)
    rep, T = M.eigen_report(with_T=True)
    assert rep.shape == (3, 10) and T.shape == (3, 2, 128)
    R, _dq = _handle(nz, blocks, packed)
    diag = _cat([np.full(v, rep[k, DK]) for k, v in enumerate(nz)])
    touched = [rep[k, DK] != 0.0 for k in range(3)]
    if any(touched):  # (a stage with d = 0 gets + 0.0 on its diagonal, which keeps the bits of every entry but a -0.0: none here)
        R.update_stage_hessians([], np.zeros((3, 0)), diag=diag)
    after, twin = _views(M, nz), _views(R, nz)
    outs = [_check_stage(nz, k, before[k], after[k], rep, T, twin[k], None if want is None else want[k]) for k in range(3)]
    return M, rep, T, outs


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("case", range(len(G.ORDERS)))
def test_eigen_control(case, packed):
    nz, kinds, blocks = G.eigen_cases()[case]
    want = []
    for kind, v in zip(kinds, nz):
        want.append((0,) if kind == "dominant" or (kind == "definite" and v < 4) else (1,) if kind == "definite" else (2,))
    _M, rep, _T, outs = _run_control(nz, blocks, packed, want)
    assert (rep[:, THETA] == G.EPS ** 2).all()
    for k, kind in enumerate(kinds):  # orders 1, 2, 3 end by j = order; the rank-2 blocks by their invariant subspace
        if outs[k] != 0:
            assert rep[k, STEPS] == min(nz[k], 64 if kind == "indefinite" else 3 if kind == "rank2" else 2), (k, rep[k, STEPS])


@pytest.mark.parametrize("packed", LAYOUTS)
def test_eigen_control_floors_steps_and_every_outcome(packed):
    """Floors per stage, max_steps = 1 (not converged, on blocks whose smallest eigenvector is nearly the start vector), the
    largest cap, and a block with a NaN (left alone): with test_eigen_control's cases the outcomes 0 .. 4."""
    nz = (313, 65, 220)
    rng = np.random.default_rng(41)
    seen = set()
    # one step: outcome 3 on the aligned blocks; the dominant block leaves by Gerschgorin
    blocks = [G.aligned_block(rng, nz[0]), G.dominant_block(rng, nz[1]), G.aligned_block(rng, nz[2])]
    _M, rep, _T, outs = _run_control(nz, blocks, packed, [(3,), (0,), (3,)], max_steps=1)
    assert rep[0, STEPS] == 1 and rep[0, RHO] > 2.0 ** -40 * rep[0, NORMT]
    seen |= set(outs)
    # floors: stage 0 below its spectrum, whose end is near -47, but above its Gerschgorin bound (no shift, by Lanczos), stage 1 above its Gerschgorin bound (the dominant block
    # is shifted up to it), stage 2 at 1.0; the cap of 128 steps
    lam1 = float(np.linalg.eigvalsh(blocks[1])[0])
    floors = [-55.0, 2.0 * lam1, 1.0]
    _M, rep, _T, outs = _run_control(nz, blocks, packed, [(1,), (2,), (2,)], floor=floors, max_steps=128)
    assert rep[:, THETA].tolist() == floors
    seen |= set(outs)
    # a NaN on the diagonal: the stage is left alone, bit for bit, and its neighbours are not touched by it
    blocks[1] = blocks[1].copy()
    blocks[1][7, 7] = np.nan
    M, _dq = _handle(nz, blocks, packed)
    before = _views(M, nz)
    M.eigen_control(G.EPS)
    rep = M.eigen_report()
    assert rep[1, OUTCOME] == 4.0 and rep[1, DK] == 0.0 and rep[0, OUTCOME] == 2.0 and rep[2, OUTCOME] == 2.0
    after = _views(M, nz)
    assert H.bits(after[1], before[1])
    assert all(np.isfinite(after[k]).all() and not H.bits(after[k], before[k]) for k in (0, 2))
    seen.add(4)
    assert seen >= {0, 1, 2, 3, 4}, seen


@pytest.mark.parametrize("packed", LAYOUTS)
def test_eigen_control_floor_from_bfgs(packed):
    """bfgs_update_device(eigen_control=eps): the floors are those the reference's rule gives from the s'Qs that
    bfgs_report shows - eps^2, lowered to s'Qs where 0 <= s'Qs < eps^2 (stage 1: a tiny step) - and the blocks are those of
    the update followed by eigen_control(from_bfgs=True)."""
    nz = (255, 257, 512)
    rng = np.random.default_rng(51)
    blocks = [G.rank2_block(rng, v, 0.0) for v in nz]
    off = H.offsets(nz)
    s, y = rng.uniform(-1, 1, sum(nz)), rng.uniform(-1, 1, sum(nz))
    s[off[1]: off[2]] *= 2.0 ** -16  # s'Qs of stage 1 about 3 |s|^2 2^-32, some 2^-24: below eps^2 = 2^-20
    y[off[2]:] = -y[off[2]:] - 3.0 * s[off[2]:]  # (an indefinite pair on stage 2)
    M, _dq = _handle(nz, blocks, packed)
    M.bfgs_update_device(s, y, eigen_control=G.EPS)
    brep, rep = M.bfgs_report(), M.eigen_report()
    want = [b[1] if 0.0 <= b[1] < G.EPS ** 2 else G.EPS ** 2 for b in brep]
    assert rep[:, THETA].tolist() == want and want[1] < G.EPS ** 2 == want[0]
    R, _dq = _handle(nz, blocks, packed)
    R.bfgs_update_device(s, y)
    R.eigen_control(G.EPS, from_bfgs=True)
    assert H.bits(R.eigen_report(), rep)
    for k, (a, r) in enumerate(zip(_views(M, nz), _views(R, nz))):
        assert H.bits(a, r), k


@pytest.mark.parametrize("packed", LAYOUTS)
def test_eigen_control_device_vectors(packed):
    """A device_vectors handle: two controls right behind each other - no report, no synchronisation between them; the
    second call reuses the pinned floors - leave the bits of a host-vector handle given the same two calls."""
    nz, _kinds, blocks = G.eigen_cases()[0]
    Mh, _dq = _handle(nz, blocks, packed)
    Mh.eigen_control(G.EPS, floor=[1.0, 2.0, 3.0])
    Mh.eigen_control(G.EPS, floor=[5.0, 1.0, 4.0])
    rh, Th = Mh.eigen_report(with_T=True)
    D, _dq = _handle(nz, blocks, packed, device=True)
    D.eigen_control(G.EPS, floor=[1.0, 2.0, 3.0])
    D.eigen_control(G.EPS, floor=[5.0, 1.0, 4.0])
    rd, Td = D.eigen_report(with_T=True)
    assert H.bits(rd, rh) and H.bits(Td, Th)
    assert rh[:, THETA].tolist() == [5.0, 1.0, 4.0]
    for k, (a, w) in enumerate(zip(_views(D, nz), _views(Mh, nz))):
        assert H.bits(a, w), k


@pytest.mark.parametrize("packed", LAYOUTS)
def test_bfgs_steps_stay_above_the_floor(packed):
    """Five damped BFGS updates with pairs (s, y) of negative curvature s'y.  Powell's damping (gamma = 0.1) leaves
    s'Q+ s = 0.1 s'Q s: from blocks whose smallest eigenvalue is 3 the curvature along s falls to about 0.3.  With the
    control behind every update (eps = 1: theta = 1, and s'Q s, some tens, never lowers it) every block keeps its smallest
    eigenvalue at the floor; the twin without the control ends below it."""
    nz = (63, 64, 65)
    rng = np.random.default_rng(61)
    blocks = [G.rank2_block(rng, v, 0.0) for v in nz]
    M, _dq = _handle(nz, blocks, packed)
    R, _dq = _handle(nz, blocks, packed)
    n = sum(nz)
    for it in range(5):
        s = rng.uniform(-1, 1, n)
        y = -3.0 * s + 0.1 * rng.uniform(-1, 1, n)
        M.bfgs_update_device(s, y, eigen_control=1.0)
        R.bfgs_update_device(s, y)
        rep = M.eigen_report()
        assert (rep[:, THETA] == 1.0).all() and set(rep[:, OUTCOME].tolist()) <= {0.0, 1.0, 2.0}, (it, rep[:, OUTCOME])
        for k, v in enumerate(nz):
            Q = M.stage_hessian(k)[:, :v]
            lam = float(np.linalg.eigvalsh(Q)[0])
            print(f"update {it} stage {k}: outcome {int(rep[k, OUTCOME])} smallest eigenvalue {lam!r}")
            assert lam >= 1.0 - 8 * G.ALLOWANCE * 2.0 ** -53 * v * G.norm_inf(Q), (it, k, lam)
    low = [float(np.linalg.eigvalsh(R.stage_hessian(k)[:, :v])[0]) for k, v in enumerate(nz)]
    print("without the control:", low)
    assert max(low) < 1.0
