"""The schedule of a launch of the STAGED engine's fp64 product (hqp_amd/csrc/gemm_schedule.hpp, host code) through
hqpkkt_debug_gemm_schedule: form, variant, work list, tile order and whether the control-row segment is taken, for the
shapes the engine launches.  The expected values come from the hooks of the primitives the schedule combines -
hqpkkt_debug_gemm_form, _sk_table, _sk_ctrl_rows, _sk_profile - and from tile orders recomputed here; a device of 256 CUs
with a grid of 512 workgroups unless stated.  No GPU needed."""
import numpy as np
import pytest

from hqp_amd import ipmatrix
from hqp_amd.ipmatrix import gemm_caps, gemm_launch, gemm_schedule

SLOT = 128 * 128


def tri_order(T):
    """Tiles of a lower triangle with T tile rows in super-blocks of 8 x 8, row by row; inside a block column by column."""
    out = []
    for I in range((T + 7) // 8):
        for J in range(I + 1):
            for tn in range(J * 8, min(T, (J + 1) * 8)):
                for tm in range(max(I * 8, tn), min(T, (I + 1) * 8)):
                    out.append(tm << 16 | tn)
    return np.array(out, dtype=np.int32)


def rect_order(tiles_m, tiles_n):
    """The kernel's own order of a rectangular product: groups of eight tile rows, column by column."""
    out = []
    for t in range(tiles_m * tiles_n):
        grp = t // (8 * tiles_n)
        first = grp * 8
        rows = min(8, tiles_m - first)
        i = t - grp * 8 * tiles_n
        out.append((first + i % rows, i // rows))
    return out


def ok(caps, launch):
    st, s = gemm_schedule(caps, launch)
    assert st == 0, st
    return s


def check_rule(s, caps_kw=None, **shape):
    """form, tiles and nsplit are those of the launch rule for the shape"""
    form, tiles, _, tile_map, nsplit = ipmatrix.gemm_form(**shape, **(caps_kw or {}))
    assert (s["form"], s["tiles"], s["nsplit"], s["order"] is not None) == (form, tiles, nsplit, tile_map), (s["form"], s["tiles"], form, tiles)


def check_list(s, kind, tiles, nslab, grid=512):
    want = ipmatrix.sk_table(tiles, nslab, grid, kind)
    assert want is not None and s["list"] == kind and s["nslab"] == nslab
    assert s["stride"] == want[0].shape[1] and s["pieces"] == want[1] and np.array_equal(s["units"], want[0])


def test_headline_w_and_its_control_row_segment():
    caps = gemm_caps()
    s = ok(caps, gemm_launch(5000, 5050, 5000))
    check_rule(s, M=5000, N=5050, K=5000)
    assert (s["form"], s["tiles"], s["variant"], s["seg"]) == ("cut", 1600, 2, False)
    check_list(s, "unequal", 1600, 313)
    s = ok(caps, gemm_launch(5000, 5050, 5000, mu=50))
    units, order, pieces = ipmatrix.sk_ctrl_rows(40, 40, 313, 512)
    assert s["seg"] and (s["form"], s["tiles"], s["nslab"]) == ("cut", 1600, 313) and s["pieces"] == pieces
    assert np.array_equal(s["units"], units) and np.array_equal(s["order"], order)
    assert ok(gemm_caps(unequal=False), gemm_launch(5000, 5050, 5000))["list"] == "equal"  # (HQPKKT_SK_TABLE=0)


def test_headline_v_launch_with_the_second_k_segment():
    v = dict(K2=50, lower=True, mirror=True, a2=0x8000, lda2=5000, b2=0x9000, ldb2=5000)
    s = ok(gemm_caps(), gemm_launch(5000, 5000, 5000, **v))
    check_rule(s, M=5000, N=5000, K=317 * 16, lower=True, mirror=True)
    assert (s["tiles"], s["nslab"], s["variant"]) == (820, 317, 2) and s["form"] in ("frac", "cut", "plain")
    assert np.array_equal(s["order"], tri_order(40))
    if s["form"] != "plain":
        check_list(s, "frac" if s["form"] == "frac" else "unequal", 820, 317)
    # the second segment exists in the LDS-DMA kernels alone: an odd leading dimension, an operand at an odd column, or a
    # holder on the register-staged variant
    for bad in (dict(lda=5001), dict(b2=0x9008), dict(ldb2=5001)):
        assert gemm_schedule(gemm_caps(), gemm_launch(5000, 5000, 5000, **{**v, **bad}))[0] == 1, bad
    assert gemm_schedule(gemm_caps(variant=0), gemm_launch(5000, 5000, 5000, **v))[0] == 1
    s = ok(gemm_caps(), gemm_launch(5000, 5000, 5000, lower=True, mirror=True, lda=5001))  # (without it: register-staged)
    assert s["variant"] == 0 and s["tiles"] == 820


def test_stage_of_2304_states_and_16_controls():
    caps = gemm_caps()
    s = ok(caps, gemm_launch(2304, 2320, 2304))
    check_rule(s, M=2304, N=2320, K=2304)
    assert (s["form"], s["tiles"], s["order"]) == ("cut", 342, None)
    check_list(s, "unequal", 342, 144)
    s = ok(caps, gemm_launch(2304, 2304, 2304, lower=True))
    check_rule(s, M=2304, N=2304, K=2304, lower=True)
    assert (s["form"], s["tiles"]) == ("frac", 171) and np.array_equal(s["order"], tri_order(18))
    check_list(s, "frac", 171, 144)
    # the control rows on the second stream: cut in k, no list, as many pieces as the SECOND stream's workspace holds
    small = dict(ws2_elems=5 * 16 * 2320)
    s = ok(gemm_caps(**small), gemm_launch(16, 2320, 2304, second_stream=True))
    check_rule(s, small, M=16, N=2320, K=2304, first_stream=False)
    assert (s["form"], s["nsplit"], s["list"], s["units"], s["order"]) == ("ks", 5, None, None, None)
    assert ok(gemm_caps(**small), gemm_launch(16, 2320, 2304))["nsplit"] > 5  # (the first stream's is its own)


def test_stage_of_1600_states():
    caps = gemm_caps()
    s = ok(caps, gemm_launch(1600, 1616, 1600))
    check_rule(s, M=1600, N=1616, K=1600)
    assert (s["form"], s["tiles"]) == ("frac", 169)
    check_list(s, "frac", 169, 100)
    s = ok(caps, gemm_launch(1616, 1616, 1600, lower=True))
    check_rule(s, M=1616, N=1616, K=1600, lower=True)
    assert (s["form"], s["list"], s["units"], s["order"], s["stride"]) == ("6464", None, None, None, 0)


def test_capacity_of_the_cut_forms():
    one_slot = gemm_caps(ws_elems=SLOT)  # holds no list's pieces: a plain round of whole tiles
    s = ok(one_slot, gemm_launch(5000, 5050, 5000))
    assert (s["form"], s["tiles"], s["list"], s["units"]) == ("cut", 1600, None, None)
    s = ok(one_slot, gemm_launch(5000, 5050, 5000, mu=50))
    assert not s["seg"] and (s["form"], s["list"], s["order"]) == ("cut", None, None)
    s = ok(gemm_caps(cnt_elems=1600), gemm_launch(5000, 5050, 5000, mu=50))  # (the augmented tile has a counter of its own)
    assert not s["seg"] and s["order"] is None
    check_list(s, "unequal", 1600, 313)
    assert ok(gemm_caps(cnt_elems=1601), gemm_launch(5000, 5050, 5000, mu=50))["seg"]
    # what the segment asks of the launch: an even ragged last tile row with room for the rows, its columns inside C's last
    # tile column, the 2 x 4 LDS-DMA kernels
    for caps, kw in ((gemm_caps(), dict(M=4999)), (gemm_caps(), dict(M=5110)), (gemm_caps(), dict(c0=4900)), (gemm_caps(), dict(lda=5001)),
                     (gemm_caps(variant=1), {})):
        assert not ok(caps, gemm_launch(**{**dict(M=5000, N=5050, K=5000, mu=50), **kw}))["seg"], kw


PANELS = np.array([(0, 132), (3, 3), (0, 40), (10, 90)] + [(p, 100 + p) for p in range(13)], dtype=np.int32)  # full, empty, ...


@pytest.mark.parametrize("by", (2, 1))
def test_profile_form(by):
    if by == 2:  # G = F'W: lower, the tile order of a large triangle in force, a tile takes its tile ROW's panel
        M = N = 2100
        order = tri_order(17)
        tiles = [(int(t) >> 16, int(t) & 0xffff) for t in order]
    else:  # W = V+ F: the kernel's own order, a tile takes its tile COLUMN's panel
        M, N, order = 2048, 2100, None
        tiles = rect_order(16, 17)
    launch = gemm_launch(M, N, 2100, lower=by == 2, by=by, panel=PANELS)
    s = ok(gemm_caps(), launch)
    assert (s["form"], s["list"], s["tiles"], s["variant"]) == ("profile", "profile", len(tiles), 2)
    assert (s["order"] is None) if order is None else np.array_equal(s["order"], order)
    ranges = np.array([PANELS[tm if by == 2 else tn] for tm, tn in tiles])
    units, pieces = ipmatrix.sk_profile(ranges, 512)
    assert s["pieces"] == pieces and s["stride"] == units.shape[1] and np.array_equal(s["units"], units)
    # counters or workspace too small: an error, never a plain round (it would read what the ranges leave out)
    assert gemm_schedule(gemm_caps(cnt_elems=len(tiles) + 3), launch)[0] == 2
    assert gemm_schedule(gemm_caps(cnt_elems=len(tiles) + 4), launch)[0] == 0
    assert pieces > 1 and gemm_schedule(gemm_caps(ws_elems=(pieces - 1) * SLOT), launch)[0] == 2
    assert gemm_schedule(gemm_caps(ws_elems=pieces * SLOT), launch)[0] == 0


def test_one_system_over_several_ranks():
    sharded = gemm_caps(sharded=True, unequal=False)
    s = ok(sharded, gemm_launch(5000, 5050, 5000))
    check_rule(s, dict(sharded=True), M=5000, N=5050, K=5000)
    assert s["form"] == "cut"
    check_list(s, "equal", 1600, 313)
    s = ok(sharded, gemm_launch(1600, 1616, 1600))  # (never the fractional form)
    check_rule(s, dict(sharded=True), M=1600, N=1616, K=1600)
    assert s["form"] != "frac"
    # a rank's tile list: cut where the count does not fill the grid evenly, the product is deep enough and the counters
    # hold the tiles (gemm_form_tiles); the shape of the block does not count
    for ntiles, sk_tiles, form in ((300, 1 << 30, "cut"), (300, 299, "plain"), (512, 1 << 30, "plain"), (16 * 512 + 1, 1 << 30, "plain")):
        s = ok(gemm_caps(sharded=True, unequal=False, sk_tiles=sk_tiles), gemm_launch(640, 5000, 69 * 16, ntiles=ntiles))
        assert (s["form"], s["tiles"], s["order"]) == (form, ntiles, None), (ntiles, sk_tiles, s["form"])
        if form == "cut":
            check_list(s, "equal", ntiles, 69)
    assert ok(sharded, gemm_launch(640, 5000, 31 * 16, ntiles=300))["form"] == "plain"  # (too shallow to cut)


def test_keys():
    def same(l1, l2):
        return gemm_schedule(gemm_caps(), l1, l2)[1]["same_key"]

    w = dict(M=5000, N=5050, K=5000)
    assert same(gemm_launch(**w), gemm_launch(**w, a=0x7f0000, lda=6000, b=0x100, ldb=5052, c=0x55550, ldc=5060))
    assert not same(gemm_launch(**w), gemm_launch(**w, lda=5001))  # (another parity: another kernel)
    assert not same(gemm_launch(**w), gemm_launch(**w, a=0x1008))
    assert not same(gemm_launch(**w), gemm_launch(**w, mu=50))
    assert not same(gemm_launch(**w, mu=50), gemm_launch(**w, mu=48))
    assert not same(gemm_launch(**w), gemm_launch(**w, second_stream=True))
    assert not same(gemm_launch(**w), gemm_launch(**w, ntiles=300))
    v = dict(M=5000, N=5000, K=5000, lower=True, mirror=True)
    assert not same(gemm_launch(**v), gemm_launch(**v, K2=50, a2=0x8000, lda2=5000, b2=0x9000, ldb2=5000))
    assert not same(gemm_launch(**v), gemm_launch(**{**v, "mirror": False}))
    p = dict(M=2100, N=2100, K=2100, lower=True, by=2)
    other = PANELS.copy()
    other[5, 1] -= 1
    assert same(gemm_launch(**p, panel=PANELS), gemm_launch(**p, panel=PANELS.copy(), a=0x3000))
    assert not same(gemm_launch(**p, panel=PANELS), gemm_launch(**p, panel=other))
    assert not same(gemm_launch(**p, panel=PANELS), gemm_launch(**{**p, "lower": False, "by": 1}, panel=PANELS))
