"""GPU tests of the wide exact eigenvalue control of the dense stage Hessians (hqpkkt_eigen_control_stage_hessians_wide;
hqp_amd/csrc/staged_hess_wide.hip.h) on packed and unpacked handles of three stages.

Operands: q_eigen_short_worker.block.  With HQPKKT_HW_FROM=1, so that every stage takes the k_hw_* kernels: (1, 2, 3) no
reflector; (16, 17, 33) the panel's edge and a ragged panel; (64, 65, 129) a row group's and a macro-tile's edge, a transposed
tile; (257, 130, 8) mixed lengths in one lockstep batch; (527, 220, 8) `full`, stages a packed handle stores as tiles (a stage
packs from order 220 on: none of the others does).  Without the hook (2049, 8, 2176) `full`, the short stage through k_hx_block.
The eigenvalues of the reported T against eigvalsh of the block: A_SHORT v 2^-53 |Q_k|_inf + 2^-50 |T|, A_SHORT = 2.1 of
q_eigen_short_worker, the project's measured bound of this reduction.  Largest err / bound seen: 0.194 ((1, 2, 3) `full`, stage 2); 0.0053 at order 2049.

Between the layouts T, the blocks and the report's words 1 .. 9 are compared bit for bit; word 0, g_k, is the row pass's and is
held to the two passes' rounding, (2 v + 2) 2^-53 |Q_k|_inf, as in test_gpu_staged_hessian_exact.py."""
import functools
import os
from unittest import mock

import numpy as np
import pytest

import hessian_guard_cases as G
import hessian_update_cases as H
import q_eigen_short_worker as W
from hqp_amd import _lib, ipmatrix
from hqp_amd import hessian_update as hu

pytestmark = pytest.mark.gpu

FROM1 = {"HQPKKT_HW_FROM": "1"}
ORDERS = [(1, 2, 3), (16, 17, 33), (64, 65, 129), (257, 130, 8)]
CASES = [(nz, kind, FROM1) for nz in ORDERS for kind in W.KINDS] + [((527, 220, 8), "full", FROM1), ((2049, 8, 2176), "full", {})]
MIXED = CASES.index(((257, 130, 8), "full", FROM1))
GK, THETA, STEPS, LO, HI, RHO, LAM, DK, NORMT, OUTCOME = range(10)


def _handle(nz, blocks, packed):
    M = H.handle(packed)
    M.init_dense(H.block_docp(nz, [np.asarray(Q, dtype=np.float64) for Q in blocks]))
    return M


def _control(nz, blocks, packed, env, entry="eigen_control_wide"):
    """one control on a fresh handle under the hooks `env`: (report, T, blocks after)"""
    with mock.patch.dict(os.environ, env):
        M = _handle(nz, blocks, packed)
        getattr(M, entry)(G.EPS)
        rep, T = M.eigen_report_exact(with_T=True)
    assert rep.shape == (3, 10) and T.shape == (3, 2, max(nz))
    return rep, T, [M.stage_hessian(k) for k in range(3)]


@functools.lru_cache(maxsize=None)
def _blocks(ci):
    return [W.block(CASES[ci][1], v) for v in CASES[ci][0]]


@functools.lru_cache(maxsize=None)
def _run(ci, packed):
    return _control(CASES[ci][0], _blocks(ci), packed, CASES[ci][2])


@functools.lru_cache(maxsize=None)
def _eigs(ci, k):
    """(eigenvalues of the packed run's T, eigvalsh of the block): T is the same bits in both layouts"""
    v, T = CASES[ci][0][k], _run(ci, True)[1][k]
    return W.tri_eigs(T[0, :v], T[1, :v]), np.linalg.eigvalsh(_blocks(ci)[k])


def _same(a, b):
    return H.bits(a[0], b[0]) and H.bits(a[1], b[1]) and all(H.bits(x, y) for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_wide_control(ci, packed):
    (nz, kind, env), blocks = CASES[ci], _blocks(ci)
    rep, T, after = _run(ci, packed)
    lanczos = _handle(nz, blocks, packed)
    lanczos.eigen_control(G.EPS)
    twin = _handle(nz, blocks, packed)
    if rep[:, DK].any():
        twin.update_stage_hessians([], np.zeros((3, 0)), diag=np.concatenate([np.full(v, rep[k, DK]) for k, v in enumerate(nz)]))
    for k, (v, Q0, r) in enumerate(zip(nz, blocks, rep)):
        tag = (nz, kind, k)
        assert H.bits(r[:2], lanczos.eigen_report()[k, :2]) and r[OUTCOME] in (0.0, 1.0, 2.0), (tag, r)  # 2
        assert H.bits(after[k], twin.stage_hessian(k)), tag  # 3
        assert r[DK] != 0.0 or H.bits(after[k], H.padded(Q0)), tag
        assert r[OUTCOME] == {"full": 2.0, "dominant": 0.0}.get(kind, r[OUTCOME]), (tag, r)
        if r[OUTCOME] == 0.0:
            assert (r[2:9] == 0.0).all() and (T[k] == 0.0).all(), tag
            continue
        m = hu.eigen_replay(v, r[GK], r[THETA], v, T[k])
        assert r[STEPS] == v and H.bits(r[3:], [m[w] for w in ("lo", "hi", "rho", "lam", "d", "normT", "outcome")]), (tag, r, m)  # 2
        assert r[RHO] == 0.0 and H.bits(r[LAM], r[LO]) and (T[k][:, v:] == 0.0).all() and T[k][1, v - 1] == 0.0, tag
        assert kind != "integers" or H.bits(T[k][0, :v], np.diag(Q0)), tag
    assert _same((rep, T, after), _control(nz, blocks, packed, env))  # 4: a fresh handle, and the other layout
    orep, oT, oafter = _run(ci, not packed)
    assert _same((rep[:, 1:], T, after), (orep[:, 1:], oT, oafter))
    for k, (v, Q0) in enumerate(zip(nz, blocks)):
        assert abs(rep[k, GK] - orep[k, GK]) <= (2 * v + 2) * W.E.U * G.norm_inf(Q0), (nz, kind, k, rep[k, GK], orep[k, GK])
        if rep[k, OUTCOME] != 0.0:  # 1
            bound = W.A_SHORT * v * W.E.U * G.norm_inf(Q0) + 2.0 ** -50 * rep[k, NORMT]
            err = np.abs(np.subtract(*_eigs(ci, k))).max()
            print(f"{(nz, kind, k)}: outcome {rep[k, OUTCOME]} d {rep[k, DK]!r} eigenvalue error {err:.3g} bound {bound:.3g} err / bound {err / bound:.3g}")
            assert err <= bound, (nz, kind, k, err, bound)


@pytest.mark.parametrize("hook", [("HQPKKT_HW_SLOTS", "1"), ("HQPKKT_HW_GROUPS", "1")])
def test_hooks_keep_the_bits(hook):
    nz, _kind, env = CASES[MIXED]
    assert _same(_control(nz, _blocks(MIXED), True, dict(env, **dict([hook]))), _run(MIXED, True))  # 5


@pytest.mark.parametrize("packed", [True, False])
def test_short_stages_are_the_exact_entrys(packed):
    nz = (527, 1025, 64)
    blocks = [W.block("full", v) for v in nz]
    assert _same(_control(nz, blocks, packed, {}), _control(nz, blocks, packed, {}, entry="eigen_control_exact"))  # 6


def test_nan_stage_is_left_alone():
    nz, blocks = CASES[MIXED][0], [B.copy() for B in _blocks(MIXED)]
    blocks[1][7, 7] = np.nan
    rep, T, after = _control(nz, blocks, True, FROM1)
    clean = _run(MIXED, True)
    assert rep[1, OUTCOME] == 4.0 and rep[1, DK] == 0.0 and H.bits(after[1], H.padded(blocks[1]))  # 7
    for k in (0, 2):
        assert H.bits(rep[k], clean[0][k]) and H.bits(T[k], clean[1][k]) and H.bits(after[k], clean[2][k]), k


def test_sizes_and_the_old_report():
    nz = (2, 1, 8193)  # (the long stage last: the analysis holds a free initial state to 4096 components)
    blocks = [np.diag(np.full(v, 3.0)) for v in nz]
    for Q in blocks:
        Q[np.arange(Q.shape[0] - 1), np.arange(1, Q.shape[0])] = Q[np.arange(1, Q.shape[0]), np.arange(Q.shape[0] - 1)] = -4.0
    M = _handle(nz, blocks, False)
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_control_wide(G.EPS)
    assert e.value.code == _lib.E_SIZES and all(H.bits(M.stage_hessian(k), H.padded(Q)) for k, Q in enumerate(blocks))  # 8
    ci = CASES.index(((16, 17, 33), "full", FROM1))
    M = _handle(CASES[ci][0], _blocks(ci), False)
    M.eigen_control_wide(G.EPS)
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_report(with_T=True)
    assert e.value.code == _lib.E_SIZES and H.bits(M.eigen_report(), M.eigen_report_exact())  # 9
