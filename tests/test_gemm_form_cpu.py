"""The launch rule of the STAGED engine's fp64 product (hqp_amd/csrc/gemm_form.hpp, host code) through
hqpkkt_debug_gemm_form: which of the six forms a shape takes, with how many tiles, and whether it wants a work table and
a tile order.

The expected values in tests/golden/gemm_form_expected.json were produced by the rule functions of commit 865a106, the
last one before the rule became one function: cut out of its staged.hip.h into a host program that adds a transcription
of the conditions around them and prints one row per shape (gemm_big_tiles, gemm_use_split, gemm_use_frac, gemm_tiles_6432, gemm_tiles and the conditions
written out in st_gemm, StagedDev::sk_tab_prepare and hqpkkt_debug_dgemm), compiled as host code - never by
gemm_form itself.  A row: mode ("e": a launch of the engine, "s": of the self-test hqpkkt_debug_dgemm), M, N, K, lower,
mirror, CUs, split grid, counter capacity, workspace of the first / second stream, sharded, first stream (allow_sk);
then form, tiles, "a table is looked up at the launch", tile order, "the upload builds a table for the shape" (that
commit's sk_tab_prepare together with the capacity check tiles <= sk_tiles of the sk_tab it calls), and the pieces of
the k range of the thin-deep form.  Besides 256 CUs with a grid of 512 a few rows have a grid of one workgroup per CU and
a device of 304 CUs.

Which rows cover which form:
  frac  (fractional cut)       2000 x 2050 x 2000, the G of 3000 states, 5000 x 640 x 5000 (not sharded)
  cut   (planned / table cut)  the C4 products 5000 x 5050 x 5000 and 5050 x 5050 x 5000 (lower), self-test and engine
  plain (128 x 128 round)      5000 x 640 x 5000 sharded, the C4 products on the second stream, the shape with grid 0
  ks    (thin-deep cut in k)   50 x 5050 x 5000 (the control rows of G), both streams
  6432  (64 x 32 tiles)        1000 x 1050 x 1000, 1000 x 1050 x 256, 130 x 70 x 300
  6464  (64 x 64 tiles)        1500 x 1540 x 1500, 64 x 64 x 16, 1050 x 1050 x 1000 (lower)"""
import json
import os

import pytest

from hqp_amd import ipmatrix

ROWS = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_form_expected.json")))


def _decide(row, **over):
    mode, M, N, K, lower, mirror, cus, grid, skt, ws, ws2, sharded, first = row[:13]
    kw = dict(cus=cus, grid=grid, sk_tiles=skt, ws_elems=ws, ws2_elems=ws2, sharded=bool(sharded), first_stream=bool(first),
              no_ks=mode == "s", no_tile_map=mode == "s")  # (what the self-test sets)
    kw.update(over)
    return ipmatrix.gemm_form(M, N, K, bool(lower), bool(mirror), **kw)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "%s-%dx%dx%d-l%d%d-c%d-g%d-s%d-a%d-t%d-w%d-%d" % (r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[11], r[12], r[8], r[9], r[10]))
def test_form_tiles_table_and_tile_order(row):
    form, tiles, table, tile_map, prepared, nsplit = row[13], row[14], bool(row[15]), bool(row[16]), bool(row[17]), row[18]
    got = _decide(row)
    assert got == (form, tiles, table, tile_map, nsplit), (row, got)
    # the table the launch looks up is one that was prepared at upload time ...
    assert not table or prepared, row
    # ... and for a system on one GPU the upload prepares exactly the tables its first-stream launches want
    if row[0] == "e" and not row[11]:
        assert _decide(row, first_stream=True)[2] == prepared, row


def test_every_form_occurs():
    assert {r[13] for r in ROWS} == set(ipmatrix.GEMM_FORMS)
    assert {r[13] for r in ROWS if r[0] == "e"} == set(ipmatrix.GEMM_FORMS)


def test_shapes_without_a_launch():
    assert ipmatrix.gemm_form(0, 10, 10)[0] is None
    assert ipmatrix.gemm_form(100, 200, 50, lower=True)[0] is None  # lower: a triangle or the column strip of one
    # the self-test's switch: the cut form whatever the rule says
    assert ipmatrix.gemm_form(1000, 1050, 1000)[0] == "6432" and ipmatrix.gemm_form(1000, 1050, 1000, force_split=True)[0] == "cut"
