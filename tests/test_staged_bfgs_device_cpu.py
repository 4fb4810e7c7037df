"""CPU tests of the damped BFGS update of the dense stage Hessians on the device (hqpkkt_bfgs_update_stage_hessians,
hqpkkt_bfgs_report): the exported symbols, the return codes that are reachable without a device - the arguments are checked
before the device is asked for -, and hessian_update.bfgs_replay, the numpy model of k_hb_terms, against bfgs_terms.

HQPKKT_E_DEVICE of the update is the one code of its list that no host-only run reaches: it stands behind the hand-over
rule, and a block arrives through the device alone, so a handle whose blocks have all arrived already holds a device."""
import ctypes as C
import os

import numpy as np
import pytest

import bfgs_device_cases as B
import hessian_update_cases as H
from dense_hessian_cases import CASES
from hqp_amd import _lib, ipmatrix
from hqp_amd.hessian_update import bfgs_replay, bfgs_terms

NZ = (5, 4, 6)
N = sum(NZ)


def _args(n=N, s=True, y=True, gamma=0.1, alpha=1.0, v=False):
    """(hqpkkt_bfgs_update, what keeps its arrays alive) over n variables."""
    keep = [np.arange(1.0, n + 1.0), np.ones(n), np.zeros(n)]
    b = _lib.BfgsUpdate()
    b.s = keep[0].ctypes.data if s else None
    b.y = keep[1].ctypes.data if y else None
    b.gamma, b.alpha = gamma, alpha
    b.v = keep[2].ctypes.data if v else None
    return b, keep


def _call(M, b):
    return _lib.lib().hqpkkt_bfgs_update_stage_hessians(M._h if M is not None else None, C.byref(b) if b is not None else None)


def _report(M, n_out=3 * 8):
    out = np.zeros(n_out)
    return _lib.lib().hqpkkt_bfgs_report(M._h if M is not None else None, C.c_void_p(out.ctypes.data))


def _dense_handle():
    M = H.handle(False)
    assert H.analyze_only(M, NZ) == 0
    return M


def test_symbols_and_constant():
    L = _lib.lib()
    assert L.hqpkkt_bfgs_update_stage_hessians is not None and L.hqpkkt_bfgs_report is not None
    assert {"hqpkkt_bfgs_update_stage_hessians", "hqpkkt_bfgs_report"} <= set(_lib.SYMBOLS)
    assert _lib.HQPKKT_BFGS_REPORT == 8
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), "include", "hqpkkt.h")).read()
    assert "#define HQPKKT_BFGS_REPORT 8" in hdr


def test_argument_checks_come_before_the_device():
    M = _dense_handle()
    b, keep = _args()
    assert _call(None, b) == _lib.E_NULL
    assert _call(M, None) == _lib.E_NULL
    b, keep = _args(s=False)
    assert _call(M, b) == _lib.E_NULL
    b, keep = _args(y=False)
    assert _call(M, b) == _lib.E_NULL
    for gamma in (np.nan, np.inf, -np.inf):
        b, keep = _args(gamma=gamma)
        assert _call(M, b) == _lib.E_RANGE, gamma
    for alpha in (np.nan, np.inf, -np.inf):
        b, keep = _args(gamma=-0.2, alpha=alpha)
        assert _call(M, b) == _lib.E_RANGE, alpha
        b, keep = _args(gamma=0.2, alpha=alpha)  # (alpha is read only when gamma < 0: the next check answers)
        assert _call(M, b) == _lib.E_INTERN, alpha


def test_handles_that_are_refused():
    b, keep = _args()
    assert _call(ipmatrix.IpSpBKP(), b) == _lib.E_INTERN  # (the tree engine)
    M = H.handle(False)
    assert _call(M, b) == _lib.E_INTERN  # (not analysed)
    prog = CASES["nx70"]()

    def analyzed(M):
        arrs = []
        for (p, i, _x) in (prog.Q, prog.A, prog.C):
            arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
        sbw = C.c_int()
        assert M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *[C.c_void_p(a.ctypes.data) if a.size else None for a in arrs], C.byref(sbw)) == 0
        return M, arrs

    b, keep = _args(n=prog.n)
    M, arrs = analyzed(ipmatrix.IpLQDOCP())  # STAGED with HQPKKT_HESS_CSR
    assert _call(M, b) == _lib.E_INTERN
    M, arrs = analyzed(ipmatrix.IpLQDOCP(q_dense=True))  # dense Hessians by the CSR hand-over
    assert len(M.hessian_layout()) == len(prog.nx)
    assert _call(M, b) == _lib.E_INTERN


def test_blocks_that_have_not_arrived():
    """An analysed handle of the dense hand-over and a valid call: every block is kept (beta = 1 on every stage), none has
    arrived, so the hand-over rule answers - through the wrapper as well - and nothing has asked for a device."""
    M = _dense_handle()
    b, keep = _args(v=True)
    assert _call(M, b) == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as e:
        M.bfgs_update_device(keep[0], keep[1], want_v=True)
    assert e.value.code == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as e:  # (... the handle is not even on the device)
        M.stage_hessian(0)
    assert e.value.code == _lib.E_INTERN


def test_report_before_an_update():
    M = _dense_handle()
    assert _report(None) == _lib.E_NULL
    assert _lib.lib().hqpkkt_bfgs_report(M._h, None) == _lib.E_NULL
    assert _report(M) == _lib.E_INTERN
    assert _report(ipmatrix.IpSpBKP()) == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as e:
        M.bfgs_report()
    assert e.value.code == _lib.E_INTERN


@pytest.mark.parametrize("gamma,alpha", [(0.1, 1.0), (-0.2, 0.6)])
def test_bfgs_replay_against_bfgs_terms(gamma, alpha):
    """Blocks of orders 5, 17, 40 and 300: plain, damped (s'y far below gamma s'Qs), a zero step (left alone, coefficients
    exactly 0), damped with s'y < 0.  The report is made of the scalars numpy computes itself, as bfgs_terms computes
    them.  Not damped: bfgs_replay returns bfgs_terms's v and coefficients bit for bit.  Damped: every entry of v within
    4 * 2^-53 |v_i| - bfgs_replay rounds theta y_i, (1 - theta) (Qs)_i and their sum once each from one theta and one 1 - theta, three
    roundings per entry, and bfgs_terms may order or fuse its own otherwise: one more for that -, -1 / s'Qs bit for bit, and
    1 / s'v within the dot product's bound on s'v over the two v."""
    rng = np.random.default_rng(7)
    nz = [5, 17, 40, 300]
    off = H.offsets(nz)
    Q = B.spd_blocks(rng, nz)
    s = rng.standard_normal(int(off[-1]))
    s[22:62] = 0.0
    Qs = np.concatenate([Q[k] @ s[off[k]: off[k + 1]] for k in range(4)])
    y = np.concatenate([Qs[:5] + 0.3 * rng.standard_normal(5), 1e-3 * s[5:22], rng.standard_normal(40), -Qs[62:] + 0.1 * rng.standard_normal(300)])
    U, coef = bfgs_terms(s, y, Qs, off, gamma=gamma, alpha=alpha)
    report = np.zeros((4, 8))
    for k in range(4):
        b = slice(int(off[k]), int(off[k + 1]))
        report[k, :3] = float(s[b] @ y[b]), float(s[b] @ Qs[b]), B.gamma_eff(gamma, alpha)
    report[:, 4] = report[:, 0]
    v, _c = bfgs_replay(report, s, y, Qs, off)  # (v does not depend on the reported s'v)
    damped = [not np.array_equal(v[off[k]: off[k + 1]], y[off[k]: off[k + 1]]) for k in range(4)]
    assert damped == [False, True, False, True]
    for k in range(4):
        b = slice(int(off[k]), int(off[k + 1]))
        if damped[k]:
            report[k, 4] = float(s[b] @ v[b])
    v, c = bfgs_replay(report, s, y, Qs, off)
    for k in range(4):
        b = slice(int(off[k]), int(off[k + 1]))
        if not damped[k]:
            assert H.bits(v[b], U[0][b]) and H.bits(c[k], coef[k]), k
            continue
        err = np.abs(v[b] - U[0][b])
        print(f"block {k}: largest difference of v {float((err / np.abs(v[b])).max() * 2.0 ** 53):.3f} * 2^-53 relative")
        assert (err <= 4 * 2.0 ** -53 * np.abs(v[b])).all(), k
        assert H.bits(c[k, 1], coef[k, 1]) and c[k, 1] < 0.0, k
        sv = np.longdouble(1.0) / np.array([c[k, 0], coef[k, 0]], dtype=np.longdouble)
        slack = B.dot_bound(s[b], v[b]) + B.dot_bound(s[b], U[0][b]) + 4 * np.longdouble(2.0) ** -53 * (np.abs(s[b]) @ np.abs(v[b])) + 4 * np.longdouble(2.0) ** -53 * np.abs(sv).max()
        assert abs(sv[0] - sv[1]) <= slack and c[k, 0] > 0.0, k
    assert (c[2] == 0.0).all() and (coef[2] == 0.0).all()
