// The launch rule of the STAGED engine's dense fp64 product C = A'B (staged_gemm.hip.h): which of its forms an
// M x N x K product takes, with how many tiles, and whether it wants a tile order.  Plain C++ (no device code, no HIP
// call, no allocation): the schedule of a launch (gemm_schedule.hpp) - asked by st_gemm at a launch and in upload's dry
// walk of the factor sequence, and by the hooks hqpkkt_debug_dgemm* - decides the form here, and the CPU tests see the
// decision through hqpkkt_debug_gemm_form.  The two cut forms (FRAC, CUT) walk a work list; which one is sk_table.hpp's
// decision (gemm_choose_list), made for the engine's shapes at upload.
#pragma once
#include <algorithm>

namespace stg {

static const int GEMM_BK = 16;

// number of b x b tiles of an M x N product; lower: only tiles with tile row >= tile column (M >= N: a triangle of
// ceil(N / b) tile columns on top of a rectangle - the column strip of a lower triangle that one rank computes)
static inline long long gemm_tiles(int M, int N, int b, int lower) {
  const long long tm = (M + b - 1) / b, tn = (N + b - 1) / b;
  return lower ? tn * (tn + 1) / 2 + (tm > tn ? (tm - tn) * tn : 0) : tm * tn;
}
static inline long long gemm_slabs(int K) { return (K + GEMM_BK - 1) / GEMM_BK; }

// 128 x 128 tiles from 384 tiles on (the grid of 2 x 256 workgroups three quarters full).  Below that the 64 x 64
// kernel with four times the tiles is faster (same-box comparisons of round 3: 2000 x 2050 x 2000
// 0.41 against 0.50 ms, 1500 x 1540 x 1500 0.19 against 0.21) with one exception: a deep rectangular product of 160 -
// 256 tiles - the column strip of W when a C4 system is sharded over 8 ranks, 5000 x 640 x 5000 - as ONE round of one
// workgroup per CU (gemm_launch_plain): 0.71 against 0.83 ms.
static inline bool gemm_big_tiles(int M, int N, int lower, int K = 0) {
  const long long t = gemm_tiles(M, N, 128, lower);
  return t >= 384 || (!lower && t >= 160 && t <= 256 && K >= 256 * GEMM_BK);
}

// The split form (k_dgemm_tn_sk) pays where whole rounds of 128 x 128 tiles would leave slots idle and the product is
// deep enough to be cut - for a given number of tiles of `nslab` k-slabs (the blocks of G_xx one rank owns) ...
static inline bool gemm_use_split_tiles(long long tiles, long long nslab, int grid) {
  if (grid <= 0 || nslab < 32) return false;                    // too shallow to cut
  return !(tiles % grid == 0 || tiles >= 16LL * grid);          // even, or the tail does not matter
}
// ... and for a whole product.  Returns true when the launch should use it with the whole
// `grid` (two workgroups per CU): more than one tile, not a multiple of the grid, and either more tiles
// than half the grid or a plan that puts at least a quarter of the grid to work (below that the 64 x 64
// tiles fill the chip better).
static inline bool gemm_use_split(int M, int N, int K, int lower, int grid) {
  if ((long long)M * N < 256LL * 256) return false;
  const long long tiles = gemm_tiles(M, N, 128, lower);
  if (!gemm_use_split_tiles(tiles, gemm_slabs(K), grid)) return false;
  // (a CU with one workgroup reaches 92 % of what it does with two: up to 5/8 of the grid one plain round of one
  // or two workgroups per CU is as fast as cut pieces, without their parked partial sums)
  // (few tiles - a stage of ~1000 states: 72 - run on 64 x 64 tiles; cut pieces for them were measured slower)
  return tiles > grid * 5 / 8;
}
// The fractional form pays for a few hundred tiles - between 5/16 and 5/8 of the grid, where neither whole rounds nor
// the 64 x 64 tiles fill the chip (measured, one MI355X, tools/dgemm_shapes.py: W of a stage of 2000 states, 272 tiles:
// 367 us against 413; G of 3000 states, 300 lower tiles: 532 against 609; a 640-column strip of the headline's W, 200
// tiles: 611 against 652).  Its workgroups are at different k at any moment, so they share less of the operands in L2
// than the rounds of the plan above: with more tiles (the headline's 1600: 4.13 against 3.90 ms) the plan stays.
static inline bool gemm_use_frac(int M, int N, int K, int lower, int grid) {
  if (grid <= 0) return false;
  const long long tiles = gemm_tiles(M, N, 128, lower), nslab = gemm_slabs(K);
  return nslab >= 64 && tiles * 16 >= grid * 5LL && tiles * 8 <= grid * 5LL;
}
// the rule for 64 x 32 tiles: a rectangular product of at most two 64 x 64 tiles per CU, deep
static inline bool gemm_tiles_6432(int M, int N, int K, int lower, int mirror, int cus) {
  return cus > 0 && !lower && !mirror && gemm_tiles(M, N, 64, 0) <= 2LL * cus && K >= 16 * GEMM_BK;
}

// NONE: nothing to launch, or lower with M < N (lower: a triangle, or the column strip of one).  FRAC: k_dgemm_tn_sk by the
// fractional list, the k-slabs of all tiles in one sequence, an equal share per workgroup; CUT: k_dgemm_tn_sk by a list of
// whole tiles and cut ones, unequal or equal shares; PLAIN: one 128 x 128 tile per workgroup (gemm_launch_plain); KS: a thin, deep product on
// 64 x 64 tiles, its k range cut over the chip (k_dgemm_tn_ks); 6432, 6464: 64 x 32 and 64 x 64 tiles; PROFILE: k_dgemm_tn_sk
// on 128 x 128 tiles by a list in which every tile takes a k range of its own (gemm_profile_table) - never the rule's
// answer: the profile form of the stage products asks for it (gemm_form_profile)
enum GemmFormKind { GEMM_FORM_NONE = -1, GEMM_FORM_FRAC, GEMM_FORM_CUT, GEMM_FORM_PLAIN, GEMM_FORM_KS, GEMM_FORM_6432, GEMM_FORM_6464, GEMM_FORM_PROFILE };
// What the rule depends on besides the shape and the device: one system over several ranks; a launch of the second stream
// (the split forms' workspace belongs to the first).  The last three are off in every launch of the engine; the self-test
// (hqpkkt_debug_dgemm) sets them so that it launches what it always has: never the thin product cut in k, never a tile
// order for large triangles, the cut form whatever the rule says (HQPKKT_DGEMM_FORCE_SPLIT)
enum { GEMM_SHARDED = 1, GEMM_SECOND_STREAM = 2, GEMM_NO_KS = 8, GEMM_NO_TILE_MAP = 16, GEMM_FORCE_SPLIT = 32 };
struct GemmForm {
  int kind = GEMM_FORM_NONE;
  long long tiles = 0;     // workgroups of the plain forms / tiles of the split ones
  int nsplit = 1;          // GEMM_FORM_KS: pieces of the k range
  bool tile_map = false;   // the tile order of a large triangle is wanted (GemmSchedule::order)
};
// cus: CUs of the device; grid: workgroups of the split forms (0: not used); sk_tiles: most tiles the arrival counters
// hold; ws_elems: workspace of the first stream (parked partial tiles; the pieces of a product cut in k), ws2_elems: of the
// second (products cut in k only)
static inline GemmForm gemm_form(int M, int N, int K, int lower, int mirror, int cus, int grid, long long sk_tiles, long long ws_elems,
                                 long long ws2_elems, int flags) {
  GemmForm f;
  if (M <= 0 || N <= 0 || (lower && M < N)) return f;
  const bool first = !(flags & GEMM_SECOND_STREAM), force = flags & GEMM_FORCE_SPLIT;
  // (not for one system over several ranks: there the strip product W_p = V+ F_p - 200 tiles at eight ranks - runs beside
  // the second stream's control-sized products, and a launch whose 512 workgroups hold every CU for its whole duration
  // starves them: 1.46 against 1.32 ms per stage, tools/shard_pieces.py 8 0)
  const bool may_split = first && grid > 0;
  const bool frac = may_split && !force && !(flags & GEMM_SHARDED) && gemm_use_frac(M, N, K, lower, grid) &&
                    2LL * grid * 128 * 128 <= ws_elems;
  const bool split = frac || (may_split && (force || gemm_use_split(M, N, K, lower, grid)));
  const bool big = split || gemm_big_tiles(M, N, lower, K);
  const int b = big ? 128 : 64;
  const long long tm = (M + b - 1) / b;
  f.tiles = gemm_tiles(M, N, b, lower);
  f.tile_map = !(flags & GEMM_NO_TILE_MAP) && lower && M == N && big && tm >= 16 && tm < 32768;
  if (split && f.tiles <= sk_tiles) {
    // tile count that does not fill the chip evenly: whole rounds, then the k ranges of the rest cut (k_dgemm_tn_sk)
    f.kind = frac ? GEMM_FORM_FRAC : GEMM_FORM_CUT;  // (both walk a work list of (tiles, k-slabs), GemmSchedule::tab)
  } else if (big)
    f.kind = GEMM_FORM_PLAIN;
  else if (!(flags & GEMM_NO_KS) && cus > 0 && !lower && !mirror && K >= 512 && f.tiles * 2 <= cus &&
           (long long)M * N * 4 <= (first ? ws_elems : ws2_elems)) {
    // a thin, deep product: its k range cut over the chip (k_dgemm_tn_ks), the pieces added in their order (the
    // launches of the second stream have a workspace of their own)
    const long long wse = first ? ws_elems : ws2_elems;
    f.kind = GEMM_FORM_KS;
    f.nsplit = (int)std::min<long long>(gemm_slabs(K) / 4, std::max<long long>(1, (2LL * cus) / f.tiles));
    f.nsplit = (int)std::max<long long>(1, std::min<long long>(f.nsplit, wse / std::max<long long>(1, (long long)M * N)));
  } else if (gemm_tiles_6432(M, N, K, lower, mirror, cus)) {
    // few tiles of a deep rectangular product (W of a stage of ~1000 states: 272): 64 x 32 tiles, so that a CU holds two
    // workgroups and one multiplies while the other waits at its barrier: 81 -> 73 us
    f.kind = GEMM_FORM_6432;
    f.tiles = ((M + 63) / 64) * (long long)((N + 31) / 32);
  } else
    f.kind = GEMM_FORM_6464;
  return f;
}
// ... and where the tiles of the launch are given (st_gemm with a tile count: 128 x 128 tiles out of a list)
static inline GemmForm gemm_form_tiles(long long ntiles, int K, int grid, long long sk_tiles) {
  GemmForm f;
  f.tiles = ntiles;
  f.kind = gemm_use_split_tiles(ntiles, gemm_slabs(K), grid) && ntiles <= sk_tiles ? GEMM_FORM_CUT : GEMM_FORM_PLAIN;
  return f;
}
// ... and a product whose tiles take k ranges of their own (the profile form): 128 x 128 tiles whatever their number,
// the tile order of a large triangle as the rule above wants it
static inline GemmForm gemm_form_profile(int M, int N, int lower, int flags = 0) {
  GemmForm f;
  if (M <= 0 || N <= 0 || (lower && M < N)) return f;
  const long long tm = (M + 127) / 128;
  f.kind = GEMM_FORM_PROFILE;
  f.tiles = gemm_tiles(M, N, 128, lower);
  f.tile_map = !(flags & GEMM_NO_TILE_MAP) && lower && M == N && tm >= 16 && tm < 32768;
  return f;
}
}  // namespace stg
