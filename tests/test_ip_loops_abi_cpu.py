"""CPU: the argument and call-order checks that hqpkkt_mehrotra and hqpkkt_franke share (hqp_amd/csrc/ip_loops.hip,
IpRun::begin) - their codes and their order, the same for both loops.  No device is touched before these returns."""
import ctypes as C

import pytest

from hqp_amd import _lib, ipmatrix, problems

LOOPS = ["hqpkkt_mehrotra", "hqpkkt_franke"]


def _call(entry, h, opts=None, res=None, vecs=(None,) * 7):
    return getattr(_lib.lib(), entry)(h, C.byref(opts) if opts is not None else None, *vecs,
                                      C.byref(res) if res is not None else None)


def _analysed_only(prog):
    """hqpkkt_analyze alone (host-only): the handle has a pattern and no values."""
    M = ipmatrix.IpRedSpBKP()
    M.n, M.me, M.m = prog.dims
    M._keep = [ipmatrix._i32(a) for (p, i, _x) in (prog.Q, prog.A, prog.C) for a in (p, i)]
    sbw = C.c_int()
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in M._keep]
    assert M._L.hqpkkt_analyze(M._h, M.n, M.me, M.m, *ptrs, C.byref(sbw)) == _lib.OK
    return M


def _codes(entry):
    prog = problems.banded_qp(20, 3, 1)
    fresh, analysed = ipmatrix.IpRedSpBKP(), _analysed_only(prog)
    negative = _lib.IpOpts()
    _lib.lib().hqpkkt_default_ip_opts(C.byref(negative))
    negative.max_iters = -1
    res = lambda: _lib.IpResult()
    return {
        "null handle": _call(entry, None, res=res()),
        "null handle, null res": _call(entry, None),
        "null res": _call(entry, fresh._h),                      # before the state of the handle is looked at
        "null res, analysed": _call(entry, analysed._h),
        "not analysed": _call(entry, fresh._h, res=res()),
        "not analysed, max_iters < 0": _call(entry, fresh._h, opts=negative, res=res()),  # the state before the options
        "no values": _call(entry, analysed._h, res=res()),       # ... and before the caller's vectors (all null here)
        "no values, max_iters < 0": _call(entry, analysed._h, opts=negative, res=res()),
    }


@pytest.mark.parametrize("entry", LOOPS)
def test_shared_checks_and_their_order(entry):
    E_NULL, E_INTERN = _lib.E_NULL, _lib.E_INTERN
    assert _codes(entry) == {
        "null handle": E_NULL, "null handle, null res": E_NULL, "null res": E_NULL, "null res, analysed": E_NULL,
        "not analysed": E_INTERN, "not analysed, max_iters < 0": E_INTERN,
        "no values": E_INTERN, "no values, max_iters < 0": E_INTERN}


def test_both_loops_give_the_same_codes():
    assert _codes(LOOPS[0]) == _codes(LOOPS[1])
