"""CPU tests of the exact eigenvalue control of the dense stage Hessians (hqpkkt_eigen_control_stage_hessians_exact,
hqpkkt_eigen_report_exact): the exported names and the return codes a host-only run reaches - the arguments are checked
before the device is asked for, in the order of hqpkkt_eigen_control_stage_hessians."""
import ctypes as C

import numpy as np
import pytest

import hessian_update_cases as H
from hqp_amd import _lib, ipmatrix

NZ = (5, 4, 6)


def _call(M, eps=1e-3, max_steps=0, floor=None, null_args=False):
    c, keep = _lib.EigenControl(), np.ascontiguousarray([0.0] * 3 if floor is None else floor, dtype=np.float64)
    c.eps, c.floor_from_bfgs, c.max_steps, c.floor = eps, 0, max_steps, keep.ctypes.data
    return _lib.lib().hqpkkt_eigen_control_stage_hessians_exact(None if M is None else M._h, None if null_args else C.byref(c))


def test_names_refused_handles_and_the_report_before_a_control():
    assert {"hqpkkt_eigen_control_stage_hessians_exact", "hqpkkt_eigen_report_exact"} <= set(_lib.SYMBOLS) and _lib.HQPKKT_EIG_EXACT_MAX == 2048
    assert callable(ipmatrix.IpLQDOCP.eigen_control_exact) and callable(ipmatrix.IpLQDOCP.eigen_report_exact)
    for M in (ipmatrix.IpSpBKP(), H.handle(False), ipmatrix.IpLQDOCP()):  # the tree engine; not analysed; the CSR hand-over
        assert _call(M) == _lib.E_INTERN
    M = H.handle(False)
    assert H.analyze_only(M, NZ) == 0
    out, ts = np.zeros((3, 10)), C.c_int(0)
    assert _lib.lib().hqpkkt_eigen_report_exact(M._h, C.c_void_p(out.ctypes.data), None, C.byref(ts)) == _lib.E_INTERN
    with pytest.raises(ipmatrix.KktError) as e:
        M.eigen_control_exact(1e-3)
    assert e.value.code == _lib.E_INTERN


@pytest.mark.parametrize("kw, code", [(dict(eps=0.0), _lib.E_RANGE), (dict(eps=np.nan), _lib.E_RANGE), (dict(max_steps=1), _lib.E_RANGE),
                                      (dict(floor=[0.0, np.inf, 0.0]), _lib.E_RANGE), (dict(null_args=True), _lib.E_NULL),
                                      (dict(), _lib.E_INTERN)])  # (valid arguments: no block has arrived)
def test_codes_before_the_device(kw, code):
    M = H.handle(False)
    assert H.analyze_only(M, NZ) == 0 and _call(M, **kw) == code and _call(None) == _lib.E_NULL
