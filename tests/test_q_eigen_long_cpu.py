"""CPU tests of hqpkkt_q_eigen_control_long, after test_q_eigen_exact_cpu.py: symbol, macro and method, the return codes a host-only run
reaches in the header's order (HQPKKT_E_SIZES is a block of 513 here), q_tridiag_model against eigvalsh on the GPU test's long blocks."""
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
from q_eigen_long_worker import LENGTHS  # noqa: E402
from test_q_eigen_cpu import _ctl, _give_values  # noqa: E402


@pytest.mark.parametrize("cls", E.SP)
def test_symbol_macro_and_refusals_in_order(cls):
    assert "hqpkkt_q_eigen_control_long" in _lib.SYMBOLS and callable(ipmatrix.Hqp_IpMatrix.q_eigen_control_long)
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hqpkkt.h")).read()
    assert _lib.HQPKKT_QEIG_LONG_MAX == 512 and "#define HQPKKT_QEIG_LONG_MAX 512\n" in header
    long_ = _lib.lib().hqpkkt_q_eigen_control_long
    M = cls()
    assert long_(None, C.byref(_ctl(eps=np.nan))) == long_(M._h, None) == _lib.E_NULL
    prog = E.program_of([[W.block("full", 513)], [W.block("full", 8)]])[0]
    for _analysed in (False, True):
        for bad in (_ctl(eps=np.nan), _ctl(eps=0.0), _ctl(max_steps=1), _ctl(max_steps=128), _ctl(max_steps=-1), _ctl(from_bfgs=2)):
            assert long_(M._h, C.byref(bad)) == _lib.E_RANGE
        assert long_(M._h, C.byref(_ctl())) == long_(M._h, C.byref(_ctl(floor=np.full(2, np.nan)))) == _lib.E_INTERN
        M.analyze(prog)
    if _give_values(M, prog):
        assert long_(M._h, C.byref(_ctl(from_bfgs=1))) == _lib.E_INTERN and long_(M._h, C.byref(_ctl(floor=np.array([1.0, np.inf])))) == _lib.E_RANGE
        assert long_(M._h, C.byref(_ctl())) == long_(M._h, C.byref(_ctl(floor=np.ones(2)))) == _lib.E_SIZES


def test_tridiag_model_holds_the_allowance_at_these_lengths():
    """twice the largest distance of T's eigenvalues from eigvalsh, in units of L 2^-53 |B|_inf, is at most A_SHORT (0.089 seen); the
    blocks are what the GPU test takes them for: "full" and "zero_column" with an eigenvalue near -5, which eigen_replay shifts
    (outcome 2), "dominant" decided by g (g >= 8)"""
    worst = 0.0
    for kind, L in ((k, L) for L in LENGTHS[2:] for k in W.KINDS):
        B = W.block(kind, L)
        (al, be), lam = hu.q_tridiag_model(B), np.linalg.eigvalsh(B)
        assert be[L - 1] == 0.0 and (kind != "integers" or (al == np.diag(B)).all()) and (kind != "zero_column" or be[0] == 0.0)
        if kind in ("full", "zero_column"):
            T = np.zeros((2, L))
            T[0], T[1] = al, be
            assert -6.0 < lam[0] < -4.0 and hu.eigen_replay(L, -1.0, E.EPS ** 2, L, T)["outcome"] == 2.0
        assert kind != "dominant" or (B.diagonal() - (np.abs(B).sum(1) - np.abs(B.diagonal()))).min() >= 8.0
        worst = max(worst, np.abs(W.tri_eigs(al, be) - lam).max() / (L * E.U * W.G.norm_inf(B)))
    assert 2.0 * worst <= W.A_SHORT
