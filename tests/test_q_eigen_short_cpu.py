"""CPU tests of hqpkkt_q_eigen_control_short: the symbol, the return codes a host-only run reaches in the header's order, and
hessian_update.q_tridiag_model against eigvalsh on the blocks of the GPU test, which measures A_SHORT.  A handle gets its values
through the device alone, so on a host without one "no values yet" (HQPKKT_E_INTERN) answers before HQPKKT_E_SIZES can, as in
test_q_eigen_cpu.py; tests/test_gpu_q_eigen_short.py reaches the rest."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hqp_amd import _lib, ipmatrix  # noqa: E402
from hqp_amd import hessian_update as hu  # noqa: E402
import q_eigen_cases as E  # noqa: E402
import q_eigen_short_worker as W  # noqa: E402
from test_q_eigen_cpu import _ctl, _give_values  # noqa: E402


@pytest.mark.parametrize("cls", E.SP)
def test_symbol_and_refusals_in_order(cls):
    """NULL; RANGE (eps, max_steps != 0, floor_from_bfgs), also before the analysis; INTERN before the analysis and before values;
    where values arrive INTERN for floor_from_bfgs without an update, RANGE for a floor, then SIZES for the block of 65."""
    assert "hqpkkt_q_eigen_control_short" in _lib.SYMBOLS and callable(ipmatrix.Hqp_IpMatrix.q_eigen_control_short)
    short = _lib.lib().hqpkkt_q_eigen_control_short
    M = cls()
    assert short(None, C.byref(_ctl(eps=np.nan))) == short(M._h, None) == _lib.E_NULL
    prog = E.program_of([[W.block("full", 65)], [W.block("full", 8)]])[0]
    nan, inf, ones = np.full(2, np.nan), np.array([1.0, np.inf]), np.ones(2)
    for _analysed in (False, True):
        for bad in (_ctl(eps=np.nan), _ctl(eps=0.0), _ctl(max_steps=1), _ctl(max_steps=64), _ctl(max_steps=-1), _ctl(from_bfgs=2)):
            assert short(M._h, C.byref(bad)) == _lib.E_RANGE
        assert short(M._h, C.byref(_ctl())) == short(M._h, C.byref(_ctl(floor=nan))) == _lib.E_INTERN
        M.analyze(prog)
    if _give_values(M, prog):
        assert short(M._h, C.byref(_ctl(from_bfgs=1))) == _lib.E_INTERN and short(M._h, C.byref(_ctl(floor=inf))) == _lib.E_RANGE
        assert short(M._h, C.byref(_ctl())) == short(M._h, C.byref(_ctl(floor=ones))) == _lib.E_SIZES


def test_tridiag_model_and_the_allowance():
    """All L eigenvalues of q_tridiag_model's T against eigvalsh of the block, on every block of the GPU test's plans: the largest
    distance in units of L 2^-53 |B|_inf, doubled, is at most A_SHORT, itself not above ten times the Lanczos constant."""
    worst = 0.0
    for plan in W.plans():
        for b, (kind, L) in enumerate(plan["kinds"]):
            B = hu.q_block_dense(plan["prog"].Q, plan["first"], b)
            al, be = hu.q_tridiag_model(B)
            assert be[L - 1] == 0.0 and (kind != "integers" or (al == np.diag(B)).all()) and (kind != "zero_column" or be[0] == 0.0)
            worst = max(worst, np.abs(W.tri_eigs(al, be) - np.linalg.eigvalsh(B)).max() / (L * E.U * W.G.norm_inf(B)))
    print("largest distance %.3f units; A_SHORT %.2f" % (worst, W.A_SHORT))
    assert 2.0 * worst <= W.A_SHORT <= 10 * E.ALLOWANCE
