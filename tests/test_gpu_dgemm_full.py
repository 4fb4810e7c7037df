"""The fp64 product of the STAGED engine (k_dgemm_tn, k_dgemm_tn_sk, k_dgemm_tn_ks + k_dgemm_ks_finish) entry by entry:
one launch on operands of the test's own through hqpkkt_debug_dgemm_full - the engine's launch rule and launch code -
and the whole C buffer compared on the host.  Nothing here samples, and the reference is numpy on the host, not device
code that indexes as the kernel does.

Criterion (a), every case of dgemm_full_cases.CASES: operands are random integers of magnitude <= 2^15 stored as fp64
without symmetry, Cin integers below 2^40, alpha and beta +-1.  Every product, partial sum and result is an integer
below 2^53 (at most 4101 products of at most 2^30), so the fp64 result is exact whatever the order of summation, the cut
in k or the use of FMA, and so is numpy's float64 product.  The C buffer is compared with what it must hold bit for bit,
np.array_equal on the uint64 patterns of the WHOLE buffer:
  canaries  C is a block at a non-zero row and column of a larger buffer (2 guard rows above and below, >= 3 guard
            columns on each side).  One quiet-NaN pattern fills every element outside the M x N block, every element
            strictly above the diagonal of a `lower` product without `mirror`, and the block itself when beta == 0.
            Afterwards every guard still holds that pattern and no element that had to be written does.
  poison    every operand has 16 rows of NaN behind row K (K2), NaN in the columns between its block and its leading
            dimension, and one spare row.  Reads stay inside the buffers: the register-staged loop
            (GemmTile::accumulate) reads row K - 1 again for k >= K and its 16-byte loads reach column lda of that
            row at most - one element into the first poison row; the LDS-DMA loops (accumulate_dma) read rows < K and
            the zero row.  No result may depend on any of it.
Criterion (b), dgemm_full_cases.ROUNDING: full-mantissa random operands, one case per kernel body, against a
numpy.longdouble product: |C - ref| <= 1e-14 (|A|'|B| + |A2|'|B2|) for every entry (k_gemm_check's criterion).

Each case asserts the form that ran, the tile order and the LDS-DMA staging through the hook's return value, and skips
with the CU count where the device gives the shape another form (tests/test_dgemm_full_forms_cpu.py holds the forms
for 256 CUs)."""
import time

import numpy as np
import pytest
import torch

from dgemm_full_cases import CASES, ROUNDING, rule_kwargs
from hqp_amd import ipmatrix

pytestmark = pytest.mark.gpu

CANARY = np.uint64(0x7FF8C0DE5EEDBEEF)  # a quiet NaN no arithmetic produces
GUARD_ROWS, GUARD_COLS, POISON_ROWS = 2, 3, 16


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _even(x):
    return x + (x & 1)


def _operand(rng, k, w, col0, odd_ld, values):
    """k x w values at column col0 of a buffer of k + 16 poison rows + 1 spare row; NaN everywhere else."""
    ld = _even(col0 + w + 3) + (1 if odd_ld else 0)
    buf = np.full((k + POISON_ROWS + 1, ld), np.nan)
    blk = values(rng, (k, w))
    buf[:k, col0:col0 + w] = blk
    return buf, blk


def _ints(rng, shape):
    return rng.integers(-2 ** 15, 2 ** 15, size=shape, endpoint=True).astype(np.float64)


def _uniform(rng, shape):
    return rng.uniform(-1.0, 1.0, size=shape)


def _tile_hint(case, i, j):
    b = 64 if case.form in ("6464", "6432", "ks") else 128
    bn = 32 if case.form == "6432" else b
    return "tile (%d, %d), 16 x 16 block (%d, %d), row %d column %d of the block" % (i // b, j // bn, i % b // 16, j % bn // 16, i % 16, j % 16)


def _launch(case, option, values=_ints, seed=0, **over):
    """Builds the operands and the C buffer of a case, launches it, and returns (got buffer, expected buffer, block
    slices, operand blocks, what the hook reported)."""
    alpha, beta, cin_where = option
    M, N, K, K2, lay = case.M, case.N, case.K, case.K2, dict(case.layout, **over)
    rng = np.random.default_rng([seed, M, N, K, K2])
    A, a = _operand(rng, K, M, lay.get("a_col0", 2), False, values)
    B, b = _operand(rng, K, N, lay.get("b_col0", 4), lay.get("ldb_odd", False), values)
    A2 = B2 = None
    a2 = b2 = np.zeros((0, 0))
    if K2:
        A2, a2 = _operand(rng, K2, M, 6, False, values)
        B2, b2 = _operand(rng, K2, N, 2, False, values)
    r0, c0 = GUARD_ROWS + 1, lay.get("c_col0", 4)
    ldc = _even(c0 + N + GUARD_COLS + 1) + (1 if lay.get("ldc_odd") else 0)
    Cb = np.empty((r0 + M + GUARD_ROWS, ldc))
    Cb.view(np.uint64)[...] = CANARY
    rows, cols = slice(r0, r0 + M), slice(c0, c0 + N)
    ii, jj = np.indices((M, N), sparse=True)
    low = ii >= jj
    cin = None
    Cin, cin_col0 = None, 0
    if cin_where:
        cin = rng.integers(-2 ** 40 + 1, 2 ** 40, size=(M, N)).astype(np.float64) if values is _ints else values(rng, (M, N))
        if cin_where == "own":  # another leading dimension than C's, poison around the block
            cin_col0 = 5
            Cin = np.full((M + 1, _even(cin_col0 + N + 7)), np.nan)
            Cin[:M, cin_col0:cin_col0 + N] = cin
        elif case.lower:  # in place: what the product may not read stays a canary
            blk = Cb[rows, cols]
            blk[np.broadcast_to(low, blk.shape)] = cin[np.broadcast_to(low, blk.shape)]
        else:
            Cb[rows, cols] = cin
    want = Cb.copy()
    prod = a.T @ b if K else np.zeros((M, N))
    if K2:
        prod = prod + a2.T @ b2
    ref = alpha * prod
    if beta != 0.0:
        ref = ref + beta * cin
    wb = want[rows, cols]
    if case.lower:
        wb[np.broadcast_to(low, wb.shape)] = ref[np.broadcast_to(low, ref.shape)]
        if case.mirror:  # (M == N) the image of the lower triangle, not the product's own upper one
            up = np.broadcast_to(~low, wb.shape)
            wb[up] = ref.T[up]
    else:
        wb[...] = ref
    t0 = time.perf_counter()
    ran = ipmatrix.dgemm_full(M, N, K, Cb, r0, c0, A=A, a_col0=lay.get("a_col0", 2), B=B, b_col0=lay.get("b_col0", 4), alpha=alpha, beta=beta,
                              Cin=Cin, cin_col0=cin_col0, cin_is_c=cin_where == "inplace", lower=bool(case.lower), mirror=bool(case.mirror),
                              K2=K2, A2=A2, a2_col0=6, B2=B2, b2_col0=2, sharded=bool(lay.get("sharded")), force_split=bool(lay.get("force_split")),
                              no_tile_map=bool(lay.get("no_tile_map")))
    print("%s alpha %+g beta %g Cin %s: form %s, %d tiles, tile order %d, LDS-DMA %d, pieces of k %d; hook %.0f ms" %
          ((case.name, alpha, beta, cin_where) + ran + ((time.perf_counter() - t0) * 1e3,)))
    return Cb, want, (rows, cols), (a, b, a2, b2), ran


def _skip_unless_form(case):
    cus = _cus()
    form = ipmatrix.gemm_form(**rule_kwargs(case, cus=cus, grid=2 * cus))[0]
    if form != case.form:
        pytest.skip("a device of %d CUs gives %d x %d x %d the form %s, not %s" % (cus, case.M, case.N, case.K, form, case.form))


def _check_ran(case, ran, lay=None):
    lay = case.layout if lay is None else lay
    form, tiles, tile_map, dma, nsplit = ran
    assert form == case.form, (case.name, form)
    assert tile_map == (bool(lay.get("tile_map")) and not lay.get("no_tile_map")), case.name
    assert dma == lay.get("dma", True), case.name
    if form == "ks":
        assert nsplit > 1, (case.name, nsplit)


def _assert_exact(case, option, got, want, block):
    rows, cols = block
    g, w = got.view(np.uint64), want.view(np.uint64)
    guard = w == CANARY
    touched = np.argwhere(guard & (g != CANARY))
    assert touched.size == 0, "%s %s: %d elements that must not be written were, the first at buffer row, column %s (block at %d, %d)" % (
        case.name, option, len(touched), touched[:8].tolist(), rows.start, cols.start)
    left = np.argwhere(~guard & (g == CANARY))
    assert left.size == 0, "%s %s: %d elements of the result were not written, the first at block row, column %s: %s" % (
        case.name, option, len(left), (left[:8] - [rows.start, cols.start]).tolist(), _tile_hint(case, *(left[0] - [rows.start, cols.start])))
    bad = np.argwhere(g != w)
    assert bad.size == 0, "%s %s: %d wrong entries, the first at block row, column %s (got %r, exact %r): %s" % (
        case.name, option, len(bad), (bad[:8] - [rows.start, cols.start]).tolist(), got[tuple(bad[0])], want[tuple(bad[0])],
        _tile_hint(case, *(bad[0] - [rows.start, cols.start])))
    assert np.array_equal(g, w)


EXACT = [(c, o) for c in CASES for o in c.options]


@pytest.mark.parametrize("case,option", EXACT, ids=["%s-a%+d-b%d-%s" % (c.name, o[0], o[1], o[2]) for c, o in EXACT])
def test_every_entry_exact_and_nothing_else_written(case, option, monkeypatch):
    for name in ("HQPKKT_NO_LDSDMA", "HQPKKT_DGEMM_WAVES", "HQPKKT_SK_TABLE", "HQPKKT_DGEMM_FORCE_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    _skip_unless_form(case)
    got, want, block, _, ran = _launch(case, option)
    _check_ran(case, ran)
    _assert_exact(case, option, got, want, block)
    if case.layout.get("tile_map"):
        # the same product row by row: the order of the tiles changes no bit
        got2, _, _, _, ran2 = _launch(case, option, no_tile_map=True)
        _check_ran(case, ran2, dict(case.layout, no_tile_map=True))
        assert np.array_equal(got.view(np.uint64), got2.view(np.uint64)), case.name


@pytest.mark.parametrize("case", ROUNDING, ids=lambda c: c.name)
def test_every_entry_within_the_rounding_bound(case, monkeypatch):
    for name in ("HQPKKT_NO_LDSDMA", "HQPKKT_DGEMM_WAVES", "HQPKKT_SK_TABLE", "HQPKKT_DGEMM_FORCE_SPLIT"):
        monkeypatch.delenv(name, raising=False)
    _skip_unless_form(case)
    got, want, (rows, cols), (a, b, a2, b2), ran = _launch(case, (1.0, 0.0, None), values=_uniform, seed=1)
    _check_ran(case, ran)
    # the canaries as in (a); the block against the longdouble product
    guard = want.view(np.uint64) == CANARY
    guard[rows, cols] = False
    assert np.array_equal(got.view(np.uint64)[guard], want.view(np.uint64)[guard]), case.name
    ref = a.astype(np.longdouble).T @ b.astype(np.longdouble)
    bound = 1e-14 * (np.abs(a).T @ np.abs(b))
    err = np.abs(got[rows, cols].astype(np.longdouble) - ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("%s: max |C - ref| / (|A|'|B|) = %.3e" % (case.name, float((err / (bound * 1e14)).max())))
    assert not np.isnan(got[rows, cols]).any(), case.name
    assert (err <= bound).all(), (case.name, worst, float(err[worst]), float(bound[worst]), _tile_hint(case, *worst))
