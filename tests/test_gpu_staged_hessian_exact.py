"""GPU tests of the exact eigenvalue control of the dense stage Hessians (hqpkkt_eigen_control_stage_hessians_exact,
hqpkkt_eigen_report_exact; hqp_amd/csrc/staged_hess_exact.hip.h) on packed and unpacked handles of three stages.

Operands: q_eigen_short_worker.block.  Orders: (1, 2, 3) no reflector; (16, 17, 33) the panel's edge, a ragged tile and panel;
(128, 129, 257) the packed tile's edge, a ragged tile row, a transposed tile; (527, 1025, 64) a thread's second index; (2048, 8,
513) the cap.  The eigenvalues of the reported T against eigvalsh of the block: A_SHORT v 2^-53 |Q_k|_inf + 2^-50 |T|, A_SHORT = 2.1
of q_eigen_short_worker, the project's measured bound of the same reduction on the sparse Q.

Between the layouts T, the blocks and the report's words 1 .. 9 are compared bit for bit; word 0, g_k, is the row pass's, whose
sums the layouts take in different orders ((527, 1025, 64) `full`, stage 0: -13.189030883733802 packed, ..805 unpacked): it is
held to the two passes' rounding, (2 v + 2) 2^-53 |Q_k|_inf - v 2^-53 sum_j |q_ij| per pass and one rounding of q_ii - offsum_i each."""
import functools

import numpy as np
import pytest

import hessian_guard_cases as G
import hessian_update_cases as H
import q_eigen_short_worker as W
from hqp_amd import _lib, ipmatrix
from hqp_amd import hessian_update as hu

pytestmark = pytest.mark.gpu

ORDERS = [(1, 2, 3), (16, 17, 33), (128, 129, 257), (527, 1025, 64), (2048, 8, 513)]
CASES = [(nz, kind) for nz in ORDERS[:4] for kind in W.KINDS] + [(ORDERS[4], "full")]
GK, THETA, STEPS, LO, HI, RHO, LAM, DK, NORMT, OUTCOME = range(10)


def _handle(nz, blocks, packed):
    M = H.handle(packed)
    M.init_dense(H.block_docp(nz, [np.asarray(Q, dtype=np.float64) for Q in blocks]))
    return M


def _control(nz, blocks, packed, **kw):
    """one exact control on a fresh handle: (report, T, blocks after)"""
    M = _handle(nz, blocks, packed)
    M.eigen_control_exact(G.EPS, **kw)
    rep, T = M.eigen_report_exact(with_T=True)
    assert rep.shape == (3, 10) and T.shape == (3, 2, max(nz))
    return rep, T, [M.stage_hessian(k) for k in range(3)]


def _blocks(ci):
    return [W.block(CASES[ci][1], v) for v in CASES[ci][0]]


@functools.lru_cache(maxsize=None)
def _run(ci, packed):
    return _control(CASES[ci][0], _blocks(ci), packed)


def _same(a, b):
    return H.bits(a[0], b[0]) and H.bits(a[1], b[1]) and all(H.bits(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_exact_control(ci, packed):
    (nz, kind), blocks = CASES[ci], _blocks(ci)
    rep, T, after = _run(ci, packed)
    lanczos = _handle(nz, blocks, packed)
    lanczos.eigen_control(G.EPS)
    twin = _handle(nz, blocks, packed)
    if rep[:, DK].any():
        twin.update_stage_hessians([], np.zeros((3, 0)), diag=np.concatenate([np.full(v, rep[k, DK]) for k, v in enumerate(nz)]))
    for k, (v, Q0, r) in enumerate(zip(nz, blocks, rep)):
        tag = (nz, kind, k)
        assert H.bits(r[:2], lanczos.eigen_report()[k, :2]) and r[OUTCOME] in (0.0, 1.0, 2.0), (tag, r)  # 3
        assert H.bits(after[k], twin.stage_hessian(k)), tag  # 4
        assert r[DK] != 0.0 or H.bits(after[k], H.padded(Q0)), tag
        assert r[OUTCOME] == {"full": 2.0, "dominant": 0.0}.get(kind, r[OUTCOME]), (tag, r)
        if r[OUTCOME] == 0.0:
            assert (r[2:9] == 0.0).all() and (T[k] == 0.0).all(), tag
            continue
        m = hu.eigen_replay(v, r[GK], r[THETA], v, T[k])
        assert r[STEPS] == v and H.bits(r[3:], [m[w] for w in ("lo", "hi", "rho", "lam", "d", "normT", "outcome")]), (tag, r, m)  # 2
        assert r[RHO] == 0.0 and H.bits(r[LAM], r[LO]) and (T[k][:, v:] == 0.0).all() and T[k][1, v - 1] == 0.0, tag
        bound = W.A_SHORT * v * W.E.U * G.norm_inf(Q0) + 2.0 ** -50 * r[NORMT]
        err = np.abs(W.tri_eigs(T[k][0, :v], T[k][1, :v]) - np.linalg.eigvalsh(Q0)).max()
        print(f"{tag}: outcome {r[OUTCOME]} d {r[DK]!r} eigenvalue error {err:.3g} bound {bound:.3g}")
        assert err <= bound, (tag, err, bound)  # 1
        assert r[DK] == 0.0 or np.linalg.eigvalsh(after[k][:, :v])[0] >= r[THETA] - bound, tag
        assert kind != "integers" or H.bits(T[k][0, :v], np.diag(Q0)), tag
    assert _same((rep, T, after), _control(nz, blocks, packed))  # 5: a fresh handle, and the other layout
    orep, oT, oafter = _run(ci, not packed)
    assert _same((rep[:, 1:], T, after), (orep[:, 1:], oT, oafter))
    for k, (v, Q0) in enumerate(zip(nz, blocks)):
        assert abs(rep[k, GK] - orep[k, GK]) <= (2 * v + 2) * W.E.U * G.norm_inf(Q0), (nz, kind, k, rep[k, GK], orep[k, GK])


def test_nan_stage_is_left_alone():
    ci = CASES.index(((128, 129, 257), "full"))
    nz, blocks = CASES[ci][0], _blocks(ci)
    blocks[1][7, 7] = np.nan
    rep, T, after = _control(nz, blocks, True)
    clean = _run(ci, True)
    assert rep[1, OUTCOME] == 4.0 and rep[1, DK] == 0.0 and H.bits(after[1], H.padded(blocks[1]))
    for k in (0, 2):
        assert H.bits(rep[k], clean[0][k]) and H.bits(T[k], clean[1][k]) and H.bits(after[k], clean[2][k]), k


def test_host_floors_and_floor_from_bfgs():
    ci = CASES.index(((16, 17, 33), "full"))
    floors = [50.0, -50.0, 40.0]
    rep, _T, _after = _control(CASES[ci][0], _blocks(ci), False, floor=floors)
    assert rep[:, THETA].tolist() == floors and rep[1, DK] == 0.0
    assert all(rep[k, OUTCOME] == 2.0 and H.bits(rep[k, DK], rep[k, THETA] - rep[k, LO]) for k in (0, 2))
    nz, rng = (255, 257, 512), np.random.default_rng(51)
    blocks = [G.rank2_block(rng, v, 0.0) for v in nz]
    off = H.offsets(nz)
    s, y = rng.uniform(-1, 1, sum(nz)), rng.uniform(-1, 1, sum(nz))
    s[off[1]: off[2]] *= 2.0 ** -16
    y[off[2]:] = -y[off[2]:] - 3.0 * s[off[2]:]
    M = _handle(nz, blocks, True)
    M.bfgs_update_device(s, y)
    M.eigen_control_exact(G.EPS, from_bfgs=True)
    want = [b[1] if 0.0 <= b[1] < G.EPS ** 2 else G.EPS ** 2 for b in M.bfgs_report()]
    assert M.eigen_report_exact()[:, THETA].tolist() == want and want[1] < G.EPS ** 2 == want[0]


@pytest.mark.parametrize("hook", [("HQPKKT_HX_SLOTS", "1"), ("HQPKKT_HX_ROWS", "4"), ("HQPKKT_HX_ROWS", "8")])
def test_hooks_keep_the_bits(hook, monkeypatch):
    ci = CASES.index(((527, 1025, 64), "full"))
    monkeypatch.setenv(*hook)
    assert _same(_control(CASES[ci][0], _blocks(ci), True), _run(ci, True))


def test_sizes_the_old_report_and_one_lanczos_step():
    nz = (2049, 1, 2)
    blocks = [3.0 * np.eye(v) - 4.0 * np.eye(v, k=1) - 4.0 * np.eye(v, k=-1) for v in nz]
    M = _handle(nz, blocks, False)
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_control_exact(G.EPS)
    assert e.value.code == _lib.E_SIZES and all(H.bits(a, H.padded(Q)) for a, Q in zip([M.stage_hessian(k) for k in range(3)], blocks))
    ci = CASES.index(((16, 17, 33), "full"))
    M = _handle(CASES[ci][0], _blocks(ci), False)
    M.eigen_control_exact(G.EPS)
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_report(with_T=True)
    assert e.value.code == _lib.E_SIZES and H.bits(M.eigen_report(), M.eigen_report_exact())
    # converged where one Lanczos step is not
    nz, rng = (313, 65, 220), np.random.default_rng(41)
    blocks = [G.aligned_block(rng, nz[0]), G.dominant_block(rng, nz[1]), G.aligned_block(rng, nz[2])]
    M = _handle(nz, blocks, True)
    M.eigen_control(G.EPS, max_steps=1)
    one, (rep, _T, _after) = M.eigen_report(), _control(nz, blocks, True)
    for k in (0, 2):
        assert one[k, OUTCOME] == 3.0 and rep[k, OUTCOME] == 2.0 and rep[k, DK] < one[k, DK], (k, one[k], rep[k])
