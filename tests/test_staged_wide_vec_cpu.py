"""CPU tests of the wide rows' vector products in the STAGED engine (hqp_amd/csrc/staged_rows.hip.h): what the analysis
reports of the split between the dense blocks E_k and the narrow copies of C that the CSR walks of step and residual take
(hqpkkt_debug_get 46) against numpy, on every case of wide_rows_cases, and the new symbols.  The analysis is host-only:
no GPU needed."""
import ctypes as C

import numpy as np
import pytest

from wide_rows_cases import CASES, MIN_ENTRIES, OPTIONS, expected_wide
from hqp_amd import _lib, ipmatrix


def _analyze(M, prog):
    arrs = []
    for (p, i, _x) in (prog.Q, prog.A, prog.C):
        arrs += [np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(i, dtype=np.int32)]
    sbw = C.c_int()
    ptrs = [C.c_void_p(a.ctypes.data) if a.size else None for a in arrs]
    return M._L.hqpkkt_analyze(M._h, prog.n, prog.me, prog.m, *ptrs, C.byref(sbw))


@pytest.mark.parametrize("case", sorted(CASES))
def test_item_46_against_numpy(case):
    """The flag is on, the rows are the rows of expected_wide, and the two counts are the stored entries of C outside and
    inside those rows."""
    prog = CASES[case]()
    M = ipmatrix.IpLQDOCP(dense_rows=MIN_ENTRIES[case], **OPTIONS[case])
    assert _analyze(M, prog) == 0
    wide = np.concatenate([np.asarray(r, dtype=np.int64) for r in expected_wide(prog, MIN_ENTRIES[case])])
    cnt = np.diff(np.asarray(prog.C[0])).astype(np.int64)
    inside = int(cnt[wide].sum())
    d = M.debug(46)
    assert d.size == 6 and d[0] == 1 and d[1] == wide.size
    got = M.dense_row_products()
    assert got == {"on": True, "rows": int(wide.size), "kept": int(cnt.sum()) - inside, "removed": inside}
    assert wide.size > 0 and inside > 0


@pytest.mark.parametrize("min_entries", [0, 10**6])
def test_item_46_is_empty_without_wide_rows(min_entries):
    prog = CASES["slab_edges"]()
    M = ipmatrix.IpLQDOCP(dense_rows=min_entries)
    assert _analyze(M, prog) == 0
    assert M.debug(46).size == 0 and M.dense_row_products() == {}


def test_item_46_on_a_handle_that_never_asked():
    prog = CASES["one_row_nx70"]()
    M = ipmatrix.IpLQDOCP()
    assert _analyze(M, prog) == 0
    assert M.debug(46).size == 0 and M.dense_row_products() == {}


def test_item_46_on_a_sharded_handle():
    """set_shard(0, 2) before the analysis: the setting is accepted and ignored, the handle keeps its walks."""
    prog = CASES["at_the_threshold"]()
    M = ipmatrix.IpLQDOCP(dense_rows=32)
    M.set_shard(0, 2, lambda *a: 0)
    assert _analyze(M, prog) == 0
    d = M.debug(46)
    assert d.size == 0 or d[0] == 0
    assert not M.dense_row_products().get("on", False)


def test_the_new_symbols_exist():
    L = _lib.lib()
    assert "hqpkkt_debug_rows_gemv" in _lib.SYMBOLS
    assert getattr(L, "hqpkkt_debug_rows_gemv") is not None
    assert callable(ipmatrix.rows_gemv) and hasattr(ipmatrix.Hqp_IpLQDOCP, "dense_row_products")


def test_the_hook_refuses_what_the_kernels_do_not_take():
    """The checks that come before the device is touched (hqpkkt_debug_gemv_dense's conventions): NULL, then RANGE."""
    L = _lib.lib()
    assert L.hqpkkt_debug_rows_gemv(0, 0, None) == _lib.E_NULL
    E, x, y = np.ones(64), np.ones(10), np.zeros(4)

    def code(form, rows=2, cols=7, ld=8, off=0, col0=0, ri=(0, 1), n=10, m=4):
        a = [np.asarray([v], dtype=np.int32) for v in (rows, cols, ld, col0)]
        o, r = np.asarray([off], dtype=np.int64), np.asarray(ri, dtype=np.int32)
        c = _lib.RowsCase()
        c.nblocks, c.e_len, c.n, c.m = 1, E.size, n, m
        c.rows, c.cols, c.ld, c.col0 = (v.ctypes.data for v in a)
        c.off, c.E, c.row_index, c.x, c.y = o.ctypes.data, E.ctypes.data, r.ctypes.data, x.ctypes.data, y.ctypes.data
        return L.hqpkkt_debug_rows_gemv(0, form, C.byref(c))

    assert code(3) == _lib.E_RANGE and code(-1) == _lib.E_RANGE
    assert code(2) == _lib.E_NULL  # (the columns form's vectors are missing)
    assert code(0, ld=7) == _lib.E_RANGE and code(0, ld=12) == _lib.E_RANGE  # below the columns / no multiple of 8
    assert code(0, off=1) == _lib.E_RANGE  # an odd offset: no 16-byte rows
    assert code(0, rows=9) == _lib.E_RANGE  # past the end of E
    assert code(0, col0=4) == _lib.E_RANGE  # past the end of x
    assert code(0, ri=(0, 4)) == _lib.E_RANGE and code(0, ri=(1, 1)) == _lib.E_RANGE  # a row outside m / twice
