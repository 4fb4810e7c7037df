"""The cases of tests/test_gpu_dgemm_full.py: one launch of the STAGED engine's fp64 product each, on operands of the
test's own, through hqpkkt_debug_dgemm_full (ipmatrix.dgemm_full).  tests/test_dgemm_full_forms_cpu.py checks without a
GPU that the launch rule (gemm_form.hpp) gives every shape the form named here on a device of 256 CUs with a grid of
512 workgroups, so a change of the rule that moves a case to another form is seen before the GPU test skips it.

The shapes are the smallest ones of their form, with ragged last tiles, by the thresholds of gemm_form.hpp:
  64 x 64 / 64 x 32 tiles   anything below 384 tiles of 128 x 128; 64 x 32: not lower, K >= 256, at most 512 tiles of 64 x 64
  ks    (thin, cut in k)    not lower, K >= 512, at most 128 tiles of 64 x 64
  plain (128 x 128 rounds)  from 384 tiles of 128 on: a triangle of 28 tile rows (406 tiles: 3457 .. 3584 rows), 19 x 21
                            or 20 x 20 tiles of a rectangle; shallower than 32 k-slabs (K <= 496), else it is cut
  plain, three LDS buffers  160 .. 256 tiles, not lower, K >= 4096, one system over several ranks (on one GPU the
                            fractional form takes these shapes): the rule's `sharded` flag
  cut   (work list)         more than 320 tiles, not a multiple of the grid, K > 496
  frac                      160 .. 320 tiles, K > 1008
  tile order                lower, M = N, 128 x 128 tiles, at least 16 tile rows"""
import collections

Case = collections.namedtuple("Case", "name M N K K2 lower mirror form options env layout")


def capacity(M, N, lower, grid=512):
    """What hqpkkt_debug_dgemm and hqpkkt_debug_dgemm_full tell the launch rule about their workspace: arrival counters for
    the product's own 128 x 128 tiles, 16 parked pieces per tile (staged_engine.hip, DebugGemm::prepare)."""
    tm, tn = -(-M // 128), -(-N // 128)
    t128 = tn * (tn + 1) // 2 + (tm - tn) * tn if lower else tm * tn
    return t128, max(16 * t128 + 8, 2 * grid + 2) * 128 * 128


# (alpha, beta, where Cin lies: None, "own" - another buffer with another leading dimension - or "inplace")
BETA0 = (1.0, 0.0, None)
UPDATE = (-1.0, 1.0, "own")
INPLACE = (-1.0, 1.0, "inplace")
ADD = (1.0, 1.0, "own")
THREE = (BETA0, UPDATE, INPLACE)


def _c(name, M, N, K, form, options=(BETA0,), lower=0, mirror=0, K2=0, env=None, **layout):
    return Case(name, M, N, K, K2, lower, mirror, form, tuple(options), dict(env or {}), layout)


# layout: a_col0 / b_col0 / c_col0 first columns, ldb_odd / ldc_odd leading dimensions made odd, sharded / force_split /
# no_tile_map the rule's flags, dma: operands staged by LDS-DMA (default True), tile_map: tile order used (default False)
ODD_OPERANDS = dict(a_col0=3, ldb_odd=True, dma=False)
CASES = [
    # 64 x 64 and 64 x 32 tiles
    _c("6464-100x37x53", 100, 37, 53, "6464", THREE),
    _c("6464-lower-130x130x70", 130, 130, 70, "6464", THREE, lower=1),
    _c("6464-mirror-130x130x70", 130, 130, 70, "6464", THREE, lower=1, mirror=1),
    _c("6464-333x777x65", 333, 777, 65, "6464", THREE),
    _c("6432-130x70x300", 130, 70, 300, "6432", THREE),
    # an empty k loop: the result is Cin, mirrored where asked (a stage without controls: V_k = G_xx)
    _c("6464-mirror-130x130x0", 130, 130, 0, "6464", (ADD,), lower=1, mirror=1),
    _c("6464-100x37x0", 100, 37, 0, "6464", (ADD,)),
    # the thin product cut in k and its finishing kernel
    _c("ks-50x130x523", 50, 130, 523, "ks", THREE),
    _c("ks-64x690x1000", 64, 690, 1000, "ks", THREE),
    # plain rounds of 128 x 128 tiles, the V_k update's own combination (2600 rows, 231 lower tiles, get 64 x 64 tiles)
    _c("plain-mirror-3461x3461x70", 3461, 3461, 70, "plain", (UPDATE,), lower=1, mirror=1, tile_map=True),
    # ... with three LDS buffers, one workgroup per CU: 10 x 16 tiles
    _c("plain3-1153x1921x4101", 1153, 1921, 4101, "plain", sharded=True),
    # cut by a work list, unequal and equal shares
    _c("cut-2432x2560x520", 2432, 2560, 520, "cut", env={"HQPKKT_SK_TABLE": "1"}),
    _c("cut-equal-2432x2560x520", 2432, 2560, 520, "cut", env={"HQPKKT_SK_TABLE": "0"}),
    _c("cut-mirror-3500x3500x528+40", 3500, 3500, 528, "cut", (ADD,), lower=1, mirror=1, K2=40, env={"HQPKKT_SK_TABLE": "1"}, tile_map=True),
    _c("cut-equal-mirror-3500x3500x528+40", 3500, 3500, 528, "cut", (ADD,), lower=1, mirror=1, K2=40, env={"HQPKKT_SK_TABLE": "0"}, tile_map=True),
    _c("frac-1664x1664x1024", 1664, 1664, 1024, "frac"),
    # the tile order of a large triangle: 28 tile rows, the last one of 5 rows (the GPU test repeats these without the order)
    _c("order-lower-3461x3461x40", 3461, 3461, 40, "plain", lower=1, tile_map=True),
    _c("order-mirror-3461x3461x40", 3461, 3461, 40, "plain", lower=1, mirror=1, tile_map=True),
    # operands that cannot be staged by LDS-DMA: A from an odd column, B with an odd leading dimension; and the switch
    _c("odd-6464-333x777x65", 333, 777, 65, "6464", **ODD_OPERANDS),
    _c("odd-plain-2433x2500x40", 2433, 2500, 40, "plain", **ODD_OPERANDS),
    _c("noldsdma-6464-333x777x65", 333, 777, 65, "6464", env={"HQPKKT_NO_LDSDMA": "1"}, dma=False),
    _c("noldsdma-plain-2433x2500x40", 2433, 2500, 40, "plain", env={"HQPKKT_NO_LDSDMA": "1"}, dma=False),
    # the mirrored write where its 16-byte stores are not possible: C from an odd column with an odd leading dimension, and
    # an odd M, so that i + 1 == M occurs in the last tile row - on 128 x 128 and on 64 x 64 tiles
    _c("oddc-mirror-3461x3461x20", 3461, 3461, 20, "plain", lower=1, mirror=1, c_col0=3, ldc_odd=True, tile_map=True),
    _c("oddc-mirror-2601x2601x20", 2601, 2601, 20, "6464", lower=1, mirror=1, c_col0=3, ldc_odd=True),
    # 2 x 2 wavefronts of 64 x 64 instead of 2 x 4 of 64 x 32
    _c("waves4-cut-2432x2560x520", 2432, 2560, 520, "cut", env={"HQPKKT_DGEMM_WAVES": "4"}),
    _c("waves4-plain-2433x2500x40", 2433, 2500, 40, "plain", env={"HQPKKT_DGEMM_WAVES": "4"}),
]

# Criterion (b), rounding: one case per kernel body, small enough for a longdouble product on the host.  The 128 x 128 body
# of the cut forms (k_dgemm_tn_sk) is reached at such a size only with the rule's force_split, and then every tile is
# whole: a list with parked pieces needs more than 320 tiles and K > 496 - 3 G multiplications, minutes in longdouble - so
# the sum over the parked pieces has criterion (a) alone (the cut and frac cases above)
ROUNDING = [
    _c("round-6464-333x777x65", 333, 777, 65, "6464"),
    _c("round-6432-130x70x300", 130, 70, 300, "6432"),
    _c("round-plain-2433x2500x24", 2433, 2500, 24, "plain"),
    _c("round-cut-380x290x200", 380, 290, 200, "cut", force_split=True),
    _c("round-ks-50x130x523", 50, 130, 523, "ks"),
]


def rule_kwargs(case, cus=256, grid=512):
    """Arguments of ipmatrix.gemm_form for the launch of a case as hqpkkt_debug_dgemm_full decides it."""
    t128, ws = capacity(case.M, case.N, case.lower, grid)
    K = case.K if not case.K2 else (-(-case.K // 16) + -(-case.K2 // 16)) * 16
    return dict(M=case.M, N=case.N, K=K, lower=bool(case.lower), mirror=bool(case.mirror), cus=cus, grid=grid, sk_tiles=t128,
                ws_elems=ws, ws2_elems=0, sharded=bool(case.layout.get("sharded")), force_split=bool(case.layout.get("force_split")),
                no_tile_map=bool(case.layout.get("no_tile_map")))
