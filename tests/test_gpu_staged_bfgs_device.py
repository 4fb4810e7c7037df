"""GPU tests of the damped BFGS update of the dense stage Hessians on the device (hqpkkt_bfgs_update_stage_hessians,
hqpkkt_bfgs_report; hqp_amd/csrc/staged_hess_bfgs.hip.h): exact on integer operands against int64 numpy and against the
host-terms path (bfgs_update), the chain product - sums - decision - v - coefficients - update on real operands against
hessian_update.bfgs_replay and the update entry, the skips, the damping adapted to the step, device vectors, and factor /
step / residuum against a fresh handle that was handed the updated blocks.

Shapes: hessian_update_cases.ORDERS and bfgs_device_cases.ORDERS, every case on a packed and on an unpacked handle."""
import numpy as np
import pytest

import bfgs_device_cases as B
import hessian_update_cases as H
from common import new_d
from hqp_amd import problems
from hqp_amd.hessian_update import bfgs_replay

pytestmark = pytest.mark.gpu

LAYOUTS = [True, False]  # packed, unpacked
BIG = (313, 384, 220)
SY, SQS, GAMMA, THETA, SV, C0, C1, OUTCOME = range(8)


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


@pytest.mark.parametrize("nz", B.ALL_ORDERS)
def test_exact_on_integers(nz):
    """Q_k positive-definite integers, s integers |s| <= 2^6, y = 2 Q s + e: every sum is an integer below 2^53 (asserted in
    int64 by int_operands), so the reported s'y and s'Qs are the int64 values, no stage damps, the coefficients are the
    correctly rounded reciprocals, and the blocks are bit for bit those of a handle updated by the host-terms path,
    packed and unpacked alike."""
    blocks, s, y, Qs = B.int_operands(nz, sum(nz))
    off = H.offsets(nz)
    views = []
    for packed in LAYOUTS:
        M, _dq = _handle(nz, blocks, packed)
        assert H.bits(M.hessian_product(_f(s)), _f(Qs))
        v = M.bfgs_update_device(_f(s), _f(y), want_v=True)
        rep = M.bfgs_report()
        assert rep.shape == (3, 8)
        for k in range(3):
            b = slice(int(off[k]), int(off[k + 1]))
            sy, sQs = int(s[b] @ y[b]), int(s[b] @ Qs[b])
            assert sy > 0 and sQs > 0
            assert rep[k, SY] == float(sy) and rep[k, SQS] == float(sQs), (k, rep[k])
            assert rep[k, GAMMA] == 0.1 and rep[k, THETA] == 1.0 and rep[k, SV] == float(sy) and rep[k, OUTCOME] == 0.0, (k, rep[k])
            assert rep[k, C0] == 1.0 / np.float64(sy) and rep[k, C1] == -1.0 / np.float64(sQs), (k, rep[k])
        assert H.bits(v, _f(y))
        R, _dq = _handle(nz, blocks, packed)
        _U, coef = R.bfgs_update(_f(s), _f(y))
        assert H.bits(coef, rep[:, C0: C1 + 1])
        views.append(_views(M, nz))
        for k, (a, r) in enumerate(zip(views[-1], _views(R, nz))):
            assert np.isfinite(a).all() and H.bits(a, r), (packed, k)
            assert not H.bits(a, H.padded(_f(blocks[k]))), (packed, k)  # (the block has changed)
    for k, (a, u) in enumerate(zip(*views)):
        assert H.bits(a, u), k


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("case", range(len(B.ALL_ORDERS)))
def test_chain_on_reals(case, packed):
    """Operands with full mantissas, magnitudes over 10^+-2, Q_k positive definite; one stage not damped (y = 2 Qs + noise),
    one damped with s'y < 0 (y = -Qs + noise), one damped with y = 0 (s'v = gamma s'Qs), the kinds rotated over the cases.
    Condition on the inputs, in numpy before the device is asked: |s'y - gamma s'Qs| > 8 x the sum of the two dot bounds on
    every stage, so the branch cannot depend on the order of the sums.
    1. Q s of hessian_product on the same handle are the bits the update used: on the damped stages v, which holds them,
       is bfgs_replay's for that Q s bit for bit; on the stage that is not damped v is y (want_v) and Q s enters through
       the rank-one term of 5.
    2. The reported s'y and s'Qs within n 2^-53 sum |s_i||y_i| (sum |s_i||Qs_i|) of the longdouble sums.
    3. The reported theta, c0, c1 and the returned v are bfgs_replay's from the REPORTED sums, bit for bit.
    4. The reported s'v of a damped stage within the same bound of the longdouble s'v.
    5. The blocks are bit for bit those of a fresh handle given update_stage_hessians([v, Qs], the reported coefficients)."""
    nz = B.ALL_ORDERS[case]
    off = H.offsets(nz)
    blocks, s, y, kinds = B.chain_operands(nz, 100 + case, shift=case)
    L = np.longdouble
    for k, Q in enumerate(blocks):
        b = slice(int(off[k]), int(off[k + 1]))
        Qs = Q @ s[b]
        sy, sQs = s[b].astype(L) @ y[b].astype(L), s[b].astype(L) @ Qs.astype(L)
        assert abs(sy - L(0.1) * sQs) > 8 * (B.dot_bound(s[b], y[b]) + B.dot_bound(s[b], Qs)), (k, kinds[k])
    M, _dq = _handle(nz, blocks, packed)
    Qs = M.hessian_product(s)
    v = M.bfgs_update_device(s, y, want_v=True)
    rep = M.bfgs_report()
    vr, cr = bfgs_replay(rep, s, y, Qs, off)
    assert H.bits(v, vr)  # 1, 3
    assert H.bits(rep[:, C0: C1 + 1], cr)  # 3
    one = np.float64(1.0)
    for k in range(3):
        b = slice(int(off[k]), int(off[k + 1]))
        sl, yl, ql, vl = (a[b].astype(L) for a in (s, y, Qs, v))
        e_sy, e_sqs = abs(L(rep[k, SY]) - sl @ yl), abs(L(rep[k, SQS]) - sl @ ql)
        b_sy, b_sqs = B.dot_bound(s[b], y[b]), B.dot_bound(s[b], Qs[b])
        print(f"stage {k} (order {nz[k]}, {kinds[k]}): s'y error {float(e_sy):.3e} (bound {float(b_sy):.3e}), s'Qs error {float(e_sqs):.3e} (bound {float(b_sqs):.3e})")
        assert e_sy <= b_sy and e_sqs <= b_sqs, k  # 2
        assert rep[k, GAMMA] == 0.1
        damped = kinds[k] != "undamped"
        assert rep[k, OUTCOME] == (1.0 if damped else 0.0), (k, rep[k])
        if damped:
            g, sy, sQs = (np.float64(rep[k, j]) for j in (GAMMA, SY, SQS))
            assert H.bits(rep[k, THETA], ((one - g) * sQs) / (sQs - sy))  # 3
            e_sv, b_sv = abs(L(rep[k, SV]) - sl @ vl), B.dot_bound(s[b], v[b])
            print(f"    s'v error {float(e_sv):.3e} (bound {float(b_sv):.3e})")
            assert e_sv <= b_sv, k  # 4
            assert not np.array_equal(v[b], y[b])
            if kinds[k] == "zero":
                # s'v = gamma s'Qs: v_i = fl(omt Qs_i) with omt within 4 * 2^-53 of gamma (the roundings of 1 - gamma, its
                # product, the quotient and 1 - theta), one rounding per v_i, and the two sums' own bounds
                tol = b_sv + b_sqs + 8 * L(2.0) ** -53 * (np.abs(sl) @ np.abs(ql))
                assert abs(L(rep[k, SV]) - L(0.1) * L(rep[k, SQS])) <= tol, (k, rep[k])
        else:
            assert rep[k, THETA] == 1.0 and H.bits(rep[k, SV], rep[k, SY]) and H.bits(v[b], y[b])
        assert rep[k, C0] > 0.0 > rep[k, C1]
    R, _dq = _handle(nz, blocks, packed)
    R.update_stage_hessians([v, Qs], rep[:, C0: C1 + 1])
    for k, (a, r) in enumerate(zip(_views(M, nz), _views(R, nz))):
        assert np.isfinite(a).all() and H.bits(a, r), k  # 5
        assert not H.bits(a, H.padded(blocks[k])), k


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("nz", [(513, 1, 2), (255, 257, 512)])
def test_skips(nz, packed):
    """For every stage in turn, from the same start: s = 0 on the stage alone - outcome 2 -, then NaN in y of the stage alone -
    outcome 3.  The stage's block keeps its bits, the neighbouring stages are updated (outcome 0), finite and bit for bit
    those of the host-terms path, which skips the same stage.  (513, 1, 2) has the stage of order 1."""
    blocks, s, y, _Qs = B.int_operands(nz, 31)
    off = H.offsets(nz)
    M, dq = _handle(nz, blocks, packed)
    R, dqr = _handle(nz, blocks, packed)
    start = _views(M, nz)
    for stage in range(3):
        b = slice(int(off[stage]), int(off[stage + 1]))
        for outcome in (2.0, 3.0):
            sk, yk = _f(s), _f(y)
            if outcome == 2.0:
                sk[b] = 0.0
            else:
                yk[b] = np.nan
            if stage or outcome == 3.0:
                M.update_dense(dq)
                R.update_dense(dqr)
            M.bfgs_update_device(sk, yk)
            R.bfgs_update(sk, yk)
            rep = M.bfgs_report()
            want = [0.0] * 3
            want[stage] = outcome
            assert rep[:, OUTCOME].tolist() == want, (stage, rep[:, OUTCOME])
            assert (rep[stage, C0: C1 + 1] == 0.0).all()
            assert np.isnan(rep[stage, SY]) == (outcome == 3.0)
            for k, (a, r) in enumerate(zip(_views(M, nz), _views(R, nz))):
                assert np.isfinite(a).all() and H.bits(a, r), (stage, outcome, k)
                assert H.bits(a, start[k]) == (k == stage), (stage, outcome, k)


@pytest.mark.parametrize("gamma,alpha", [(-0.2, 0.5), (-0.45, 0.7)])
def test_damping_adapted_to_the_step(gamma, alpha):
    """gamma < 0: the reported damping factor is the value bfgs_terms forms, g + (1 - g)(1 - alpha) in its operations, bit
    for bit ((-0.45, 0.7): 0.615, where the product and the sum fused into one operation give 0.6150000000000001), and
    the decision follows it."""
    nz = (2, 1, 3)
    blocks, s, y, kinds = B.chain_operands(nz, 41)
    M, _dq = _handle(nz, blocks, False)
    Qs = M.hessian_product(s)
    v = M.bfgs_update_device(s, y, gamma=gamma, alpha=alpha, want_v=True)
    rep = M.bfgs_report()
    want = B.gamma_eff(gamma, alpha)
    assert 0.0 < want < 1.0 and all(H.bits(g, want) for g in rep[:, GAMMA]), (rep[:, GAMMA], want)
    vr, cr = bfgs_replay(rep, s, y, Qs, H.offsets(nz))
    assert H.bits(v, vr) and H.bits(rep[:, C0: C1 + 1], cr)
    assert rep[:, OUTCOME].tolist() == [0.0 if kind == "undamped" else 1.0 for kind in kinds]


@pytest.mark.parametrize("packed", LAYOUTS)
def test_device_vectors(packed):
    """torch CUDA s, y and v on a device_vectors handle: two updates right behind each other - no report, no
    synchronisation between them: the second call reuses the descriptor buffer - leave the bits of a host-vector handle
    given the same two updates, v and the report of the second included; again from the same start, the same bits."""
    import torch
    nz = (255, 257, 512)
    blocks, s1, y1, _kinds = B.chain_operands(nz, 51)
    _b, s2, y2, _kinds = B.chain_operands(nz, 52, shift=1)
    Mh, _dq = _handle(nz, blocks, packed)
    Mh.bfgs_update_device(s1, y1)
    vh = Mh.bfgs_update_device(s2, y2, want_v=True)
    rh, want = Mh.bfgs_report(), _views(Mh, nz)
    assert set(rh[:, OUTCOME].tolist()) <= {0.0, 1.0} and all(np.isfinite(a).all() for a in want)
    D, dq = _handle(nz, blocks, packed, device=True)
    t = [torch.as_tensor(a).cuda() for a in (s1, y1, s2, y2)]
    for again in range(2):
        if again:
            D.update_dense(dq)
        assert D.bfgs_update_device(t[0], t[1]) is None
        vd = D.bfgs_update_device(t[2], t[3], want_v=True)
        assert vd.is_cuda and H.bits(D.bfgs_report(), rh), again
        assert H.bits(vd.cpu().numpy(), vh), again
        for k, (a, w) in enumerate(zip(_views(D, nz), want)):
            assert H.bits(a, w), (again, k)


@pytest.mark.parametrize("packed", LAYOUTS)
@pytest.mark.parametrize("nz", [BIG, (255, 257, 512), (513, 1, 2)])
def test_nothing_stale(nz, packed):
    """Handle A: positive-definite integer blocks, factor + step, then the BFGS update on the device.  Handle B: a fresh
    handle that is handed the updated blocks as stage_hessian reads them.  factor + step and residuum are bit-identical
    (the comparison of test_gpu_staged_hessian_update.py's test_nothing_stale: the same stored bits, the same launches),
    with bounds on the controls as rows of C so that z and w are not empty."""
    blocks, s, y, _Qs = B.int_operands(nz, 61)
    A, dq = _handle(nz, blocks, packed, bounds=True)
    st = problems.ip_state(dq, 3, 1.0)
    A.factor(dq, st[0], st[1])
    A.step(dq, *st, *new_d(dq))
    A.bfgs_update_device(_f(s), _f(y))
    assert (A.bfgs_report()[:, OUTCOME] == 0.0).all()
    updated = [A.stage_hessian(k)[:, :v].copy() for k, v in enumerate(nz)]
    assert all(not np.array_equal(U, _f(Q)) for U, Q in zip(updated, blocks))
    Bh, _dqb = _handle(nz, updated, packed, bounds=True)
    outs = []
    for M in (A, Bh):
        M.factor(dq, st[0], st[1])
        d = new_d(dq)
        M.step(dq, *st, *d)
        outs.append(d + [np.array([M.residuum(dq, *st, *d)])])
    for q, (a, b) in enumerate(zip(*outs)):
        assert np.isfinite(a).all() and H.bits(a, b), q
    assert np.abs(outs[0][0]).max() > 0.0
