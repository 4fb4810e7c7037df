"""CPU tests of hqpkkt_q_eigen_control_blocked, after test_q_eigen_long_cpu.py: symbol, macro and method, the return codes a host-only
run reaches in the header's order (HQPKKT_E_SIZES is a block of 2049 here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hqp_amd import _lib, ipmatrix  # noqa: E402
import q_eigen_cases as E  # noqa: E402
import q_eigen_short_worker as W  # noqa: E402
from test_q_eigen_cpu import _ctl, _give_values  # noqa: E402


@pytest.mark.parametrize("cls", E.SP)
def test_symbol_macro_and_refusals_in_order(cls):
    assert "hqpkkt_q_eigen_control_blocked" in _lib.SYMBOLS and callable(ipmatrix.Hqp_IpMatrix.q_eigen_control_blocked)
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hqpkkt.h")).read()
    assert _lib.HQPKKT_QEIG_BLOCKED_MAX == 2048 and "#define HQPKKT_QEIG_BLOCKED_MAX 2048\n" in header
    blocked = _lib.lib().hqpkkt_q_eigen_control_blocked
    M = cls()
    assert blocked(None, C.byref(_ctl(eps=np.nan))) == blocked(M._h, None) == _lib.E_NULL
    prog = E.program_of([[W.block("full", 2049)], [W.block("full", 8)]])[0]
    for _analysed in (False, True):
        for bad in (_ctl(eps=np.nan), _ctl(eps=0.0), _ctl(max_steps=1), _ctl(max_steps=128), _ctl(max_steps=-1), _ctl(from_bfgs=2)):
            assert blocked(M._h, C.byref(bad)) == _lib.E_RANGE
        assert blocked(M._h, C.byref(_ctl())) == blocked(M._h, C.byref(_ctl(floor=np.full(2, np.nan)))) == _lib.E_INTERN
        M.analyze(prog)
    if _give_values(M, prog):
        assert blocked(M._h, C.byref(_ctl(from_bfgs=1))) == _lib.E_INTERN and blocked(M._h, C.byref(_ctl(floor=np.array([1.0, np.inf])))) == _lib.E_RANGE
        assert blocked(M._h, C.byref(_ctl())) == blocked(M._h, C.byref(_ctl(floor=np.ones(2)))) == _lib.E_SIZES
    long_ = _lib.lib().hqpkkt_q_eigen_control_long  # (the long entry has not moved: the same plan is over ITS limit)
    assert not _give_values(M, prog) or long_(M._h, C.byref(_ctl())) == _lib.E_SIZES
