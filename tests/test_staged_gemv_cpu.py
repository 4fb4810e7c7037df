"""CPU tests of the hooks of the STAGED solve's dense vector products (hqpkkt_debug_gemv_dense, hqpkkt_debug_symv,
hqpkkt_debug_symv_batch, hqpkkt_debug_symv_map): the symbols, the tile order of the triangle form as the kernel's own code
numbers it (evaluated on the host), and the argument checks, which answer before any device is touched.  The products
themselves: tests/test_gpu_staged_gemv.py."""
import ctypes as C

import numpy as np
import pytest

from hqp_amd import _lib, ipmatrix

NO_DEVICE = 1 << 20  # (a device number no machine has: the checks of the arguments come first)


def test_symbols():
    L = _lib.lib()
    for sym in ("hqpkkt_debug_gemv_dense", "hqpkkt_debug_symv", "hqpkkt_debug_symv_batch", "hqpkkt_debug_symv_map"):
        assert sym in _lib.SYMBOLS and hasattr(L, sym)
    assert [f[0] for f in _lib.GemvCase._fields_][-2:] == ["chunks", "vec16"]
    # (hqpkkt_gemv_case: 2 ints, 2 operands of 4 words, 2 ints, 6 words, a double, 4 words, 2 ints)
    assert C.sizeof(_lib.GemvCase) == 8 + 2 * 32 + 8 + 6 * 8 + 8 + 4 * 8 + 8


@pytest.mark.parametrize("N", [1, 64, 65, 512, 513, 5000, 8192, 40000])
def test_tile_map(N):
    """Row tile bi (64 rows) has the column tiles 0 .. bi // 8 (512 columns): every pair once, in tile order."""
    pairs = ipmatrix.symv_map(N)
    nrt = (N + 63) // 64
    want = [(bi, bj) for bi in range(nrt) for bj in range(bi // 8 + 1)]
    assert len(pairs) == sum(bi // 8 + 1 for bi in range(nrt)) == len(want)
    assert np.array_equal(pairs, np.array(want, dtype=np.int32).reshape(-1, 2))
    assert len({(int(a), int(b)) for a, b in pairs}) == len(want)


def test_tile_map_small_buffer_and_no_order():
    L = _lib.lib()
    assert L.hqpkkt_debug_symv_map(0, None, 0) == 0 and L.hqpkkt_debug_symv_map(-5, None, 0) == 0
    buf = np.full(8, -7, dtype=np.int32)
    assert L.hqpkkt_debug_symv_map(513, buf.ctypes.data_as(C.POINTER(C.c_int)), buf.size) == 10  # 8 row tiles of one tile, one of two
    assert (buf == -7).all()  # (too small: nothing written)


def _code(fn, *a, **kw):
    with pytest.raises(ipmatrix.KktError) as e:
        fn(*a, device=NO_DEVICE, **kw)
    return e.value.code


def test_gemv_dense_argument_checks():
    L = _lib.lib()
    A, x = np.ones((5, 8)), np.ones(8)
    assert L.hqpkkt_debug_gemv_dense(0, 0, None) == _lib.E_NULL
    c = _lib.GemvCase()
    assert L.hqpkkt_debug_gemv_dense(0, 0, C.byref(c)) == _lib.E_NULL  # (no A, x, y)
    g = ipmatrix.gemv_dense
    assert _code(g, "rows", A, 4, 6, x) == _lib.E_DEVICE  # (a case that is fine: the device is asked for last)
    assert _code(g, "wide", A, 4, 6, x) == _lib.E_DEVICE
    assert _code(g, "cols", A, 4, 6, x, part_chunks=64) == _lib.E_DEVICE
    c, _y, _y2, _k = ipmatrix._gemv_case(A, 4, 6, x, 4)
    assert L.hqpkkt_debug_gemv_dense(NO_DEVICE, 3, C.byref(c)) == _lib.E_RANGE and L.hqpkkt_debug_gemv_dense(NO_DEVICE, -1, C.byref(c)) == _lib.E_RANGE
    assert L.hqpkkt_debug_gemv_dense(-1, 0, C.byref(c)) == _lib.E_DEVICE
    for form in ("rows", "wide", "cols"):
        assert _code(g, form, A, 0, 6, x) == _lib.E_RANGE
        assert _code(g, form, A, 4, 0, x) == _lib.E_RANGE
        assert _code(g, form, A, 6, 6, x) == _lib.E_RANGE  # more rows than the buffer holds
        assert _code(g, form, A, 4, 9, np.ones(9)) == _lib.E_RANGE  # wider than ld
        assert _code(g, form, A, 4, 6, x, col0=3) == _lib.E_RANGE  # the block leaves its rows
        assert _code(g, form, A, 4, 6, x, col0=-1) == _lib.E_RANGE
    assert _code(g, "rows", A, 4, 6, x[:5]) == _lib.E_RANGE  # x too short
    assert _code(g, "cols", A, 4, 6, x[:3]) == _lib.E_RANGE
    assert _code(g, "cols", A, 4, 6, x, part_chunks=0) == _lib.E_RANGE
    # the second block: the rows form alone, inside its buffer, with its x2
    A2 = np.ones((4, 7))
    assert _code(g, "rows", A, 4, 6, x, A2=A2, n2=7, x2=np.ones(7)) == _lib.E_DEVICE
    assert _code(g, "rows", A, 4, 6, x, A2=A2, n2=0, x2=np.ones(0)) == _lib.E_DEVICE
    assert _code(g, "rows", A, 4, 6, x, A2=A2, n2=3) == _lib.E_NULL
    assert _code(g, "rows", A, 4, 6, x, A2=A2, n2=8, x2=np.ones(8)) == _lib.E_RANGE
    assert _code(g, "rows", A, 4, 6, x, A2=A2, n2=-1, x2=np.ones(8)) == _lib.E_RANGE
    assert _code(g, "rows", A, 4, 6, x, A2=A2, n2=5, x2=np.ones(4)) == _lib.E_RANGE
    assert _code(g, "rows", A, 4, 6, x, A2=A2[:3], n2=5, x2=np.ones(5)) == _lib.E_RANGE
    assert _code(g, "wide", A, 4, 6, x, A2=A2, n2=5, x2=np.ones(5)) == _lib.E_RANGE
    assert _code(g, "cols", A, 4, 6, x, A2=A2, n2=5, x2=np.ones(5)) == _lib.E_RANGE
    # add2 / y2: the columns form alone, both or neither
    assert _code(g, "cols", A, 4, 6, x, add2=np.ones(6)) == _lib.E_DEVICE
    assert _code(g, "cols", A, 4, 6, x, y2=np.ones(6)) == _lib.E_RANGE
    assert _code(g, "rows", A, 4, 6, x, add2=np.ones(4)) == _lib.E_RANGE


def test_symv_argument_checks():
    L = _lib.lib()
    assert L.hqpkkt_debug_symv(0, None) == _lib.E_NULL
    c = _lib.GemvCase()
    assert L.hqpkkt_debug_symv(0, C.byref(c)) == _lib.E_NULL
    s = ipmatrix.symv
    V, x = np.ones((7, 8)), np.ones(7)
    assert _code(s, V, 7, x) == _lib.E_DEVICE
    assert _code(s, V, 5, x, col0=2) == _lib.E_DEVICE
    assert _code(s, V, 0, x) == _lib.E_RANGE
    assert _code(s, V, 8, np.ones(8)) == _lib.E_RANGE  # rows
    assert _code(s, V, 7, x[:6]) == _lib.E_RANGE
    # what the engine gives to the rows form: an odd leading dimension, a start that is not 16-byte aligned
    assert _code(s, np.ones((7, 9)), 7, x) == _lib.E_RANGE
    assert _code(s, V, 5, x, col0=1) == _lib.E_RANGE
    assert _code(s, V, 7, x, A2=np.ones((7, 3)), n2=4, x2=np.ones(4)) == _lib.E_RANGE
    assert _code(s, V, 7, x, A2=np.ones((7, 3)), n2=2) == _lib.E_NULL


def test_symv_batch_argument_checks():
    L = _lib.lib()
    assert L.hqpkkt_debug_symv_batch(0, 1, None, None, 0, None, 0, 0, 0) == _lib.E_NULL
    b = ipmatrix.symv_batch
    V, x = np.ones((7, 8)), np.ones(7)
    item = dict(V=V, N=7, x=x)
    assert _code(b, [item, item]) == _lib.E_DEVICE
    assert _code(b, [item], grid_tiles=-1) == _lib.E_RANGE
    assert _code(b, [item], grid_fins=-1) == _lib.E_RANGE
    cs = (_lib.GemvCase * 1)()
    assert L.hqpkkt_debug_symv_batch(NO_DEVICE, 0, cs, None, 0, None, 0, 0, 0) == _lib.E_RANGE
    assert _code(b, [item, dict(V=np.ones((7, 9)), N=7, x=x)]) == _lib.E_RANGE  # the second item's odd ld
    assert _code(b, [item, dict(V=V, N=7)]) == _lib.E_NULL  # no x of its own and no base
    # vectors relative to a base: inside it
    xb, yb = np.ones(20), np.zeros(20)
    rel = dict(V=V, N=7, xoff=13, yoff=0)
    assert _code(b, [rel], xbase=xb) == _lib.E_DEVICE
    assert _code(b, [dict(rel, xoff=14)], xbase=xb) == _lib.E_RANGE
    assert _code(b, [dict(rel, xoff=-1)], xbase=xb) == _lib.E_RANGE
    assert _code(b, [dict(rel, x=x, yoff=13)], ybase=yb) == _lib.E_DEVICE
    assert _code(b, [dict(rel, x=x, yoff=14)], ybase=yb) == _lib.E_RANGE
