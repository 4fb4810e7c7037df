"""CPU tests of hqpkkt_q_eigen_control_wide, after test_q_eigen_blocked_cpu.py: symbol, macro and method, the return codes a host-only
run reaches in the header's order (HQPKKT_E_SIZES is a block of 8193 here)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hqp_amd import _lib, ipmatrix  # noqa: E402
import q_eigen_cases as E  # noqa: E402
from test_q_eigen_cpu import _ctl, _give_values  # noqa: E402


@pytest.mark.parametrize("cls", E.SP)
def test_symbol_macro_and_refusals_in_order(cls):
    assert "hqpkkt_q_eigen_control_wide" in _lib.SYMBOLS and callable(ipmatrix.Hqp_IpMatrix.q_eigen_control_wide)
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "hqpkkt.h")).read()
    assert _lib.HQPKKT_QEIG_WIDE_MAX == 8192 and "#define HQPKKT_QEIG_WIDE_MAX 8192\n" in header
    wide = _lib.lib().hqpkkt_q_eigen_control_wide
    M = cls()
    assert wide(None, C.byref(_ctl(eps=np.nan))) == wide(M._h, None) == _lib.E_NULL
    from q_eigen_wide_worker import over_program
    prog = over_program()
    for _analysed in (False, True):
        for bad in (_ctl(eps=np.nan), _ctl(eps=0.0), _ctl(max_steps=1), _ctl(max_steps=128), _ctl(max_steps=-1), _ctl(from_bfgs=2)):
            assert wide(M._h, C.byref(bad)) == _lib.E_RANGE
        assert wide(M._h, C.byref(_ctl())) == wide(M._h, C.byref(_ctl(floor=np.full(2, np.nan)))) == _lib.E_INTERN
        M.analyze(prog)
    if _give_values(M, prog):
        assert wide(M._h, C.byref(_ctl(from_bfgs=1))) == _lib.E_INTERN and wide(M._h, C.byref(_ctl(floor=np.array([1.0, np.inf])))) == _lib.E_RANGE
        assert wide(M._h, C.byref(_ctl())) == wide(M._h, C.byref(_ctl(floor=np.ones(2)))) == _lib.E_SIZES
    blocked = _lib.lib().hqpkkt_q_eigen_control_blocked  # (the blocked entry has not moved: the same plan is over ITS limit)
    assert not _give_values(M, prog) or blocked(M._h, C.byref(_ctl())) == _lib.E_SIZES
