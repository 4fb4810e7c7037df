"""CPU tests of the wide exact eigenvalue control of the dense stage Hessians (hqpkkt_eigen_control_stage_hessians_wide):
the exported name, the constant, and the return codes a host-only run reaches - the exact entry's, in its order."""
import ctypes as C

import numpy as np
import pytest

import hessian_update_cases as H
from hqp_amd import _lib, ipmatrix

NZ = (5, 4, 6)


def _call(M, eps=1e-3, max_steps=0, floor=None, null_args=False):
    c, keep = _lib.EigenControl(), np.ascontiguousarray([0.0] * 3 if floor is None else floor, dtype=np.float64)
    c.eps, c.floor_from_bfgs, c.max_steps, c.floor = eps, 0, max_steps, keep.ctypes.data
    return _lib.lib().hqpkkt_eigen_control_stage_hessians_wide(None if M is None else M._h, None if null_args else C.byref(c))


def test_name_constant_and_refused_handles():
    assert "hqpkkt_eigen_control_stage_hessians_wide" in _lib.SYMBOLS and _lib.HQPKKT_EIG_WIDE_MAX == 8192
    assert callable(ipmatrix.IpLQDOCP.eigen_control_wide)
    for M in (ipmatrix.IpSpBKP(), H.handle(False), ipmatrix.IpLQDOCP()):  # the tree engine; not analysed; the CSR hand-over
        assert _call(M) == _lib.E_INTERN
    M = H.handle(True)
    assert H.analyze_only(M, NZ) == 0
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_control_wide(1e-3)
    assert e.value.code == _lib.E_INTERN


@pytest.mark.parametrize("kw, code", [(dict(eps=0.0), _lib.E_RANGE), (dict(eps=np.nan), _lib.E_RANGE), (dict(max_steps=1), _lib.E_RANGE),
                                      (dict(floor=[0.0, np.inf, 0.0]), _lib.E_RANGE), (dict(null_args=True), _lib.E_NULL),
                                      (dict(), _lib.E_INTERN)])  # (valid arguments: no block has arrived)
def test_codes_before_the_device(kw, code):
    M = H.handle(False)
    assert H.analyze_only(M, NZ) == 0 and _call(M, **kw) == code and _call(None) == _lib.E_NULL


def test_sizes_comes_behind_the_floors_and_before_the_arrival():
    M = H.handle(False)  # (the long stage last: the analysis holds a free initial state to 4096 components)
    assert H.analyze_only(M, (2, 1, 8193)) == 0
    assert _call(M, floor=[0.0, np.nan, 0.0]) == _lib.E_RANGE and _call(M) == _lib.E_SIZES
    M = H.handle(False)
    assert H.analyze_only(M, (2, 1, 8192)) == 0 and _call(M) == _lib.E_INTERN  # (served: no block has arrived)
