// The schedule of one launch of the STAGED engine's dense fp64 product (staged_gemm.hip.h): everything a launch looks up
// and runs - the form (gemm_form.hpp), the 128 x 128 variant, the work list (sk_table.hpp), the tile order and whether
// the control-row segment is taken - decided from what the holder of the launch offers (GemmCaps) and what the launch is
// (GemmRequest).  Decided HERE ALONE: the engine (GemmCache, staged_host.hip.h: st_gemm in upload's dry walk and at a
// launch, staged_upload for its stages) and the test hooks (hqpkkt_debug_dgemm*) ask gemm_schedule, and the CPU tests see
// its answer through hqpkkt_debug_gemm_schedule.  Plain C++ (no device code, no HIP call, no allocation on the device).
#pragma once
#include <algorithm>
#include <vector>

#include "gemm_form.hpp"
#include "sk_table.hpp"

namespace stg {

// The variants of the 128 x 128 product.  0: operands staged through registers, 4 waves (round 2's loop, kept
// for comparisons: HQPKKT_NO_LDSDMA); 1: LDS-DMA, 2 x 2 waves of 64 x 64; 2: LDS-DMA, 2 x 4 waves of 64 x 32 (default)
enum { GEMM_REG4 = 0, GEMM_DMA4 = 1, GEMM_DMA8 = 2, GEMM_DMA8X3 = 3 };  // X3: three LDS buffers, one workgroup per CU

// Order of the tiles of a lower-triangular product with T tile rows (GemmArgs::tile_map): super-blocks of 8 x 8 tiles,
// row by row; inside a block column by column
static inline std::vector<int> gemm_tri_order(int T) {
  std::vector<int> m;
  m.reserve((size_t)T * (T + 1) / 2);
  const int S = 8;
  for (int I = 0; I < (T + S - 1) / S; I++)
    for (int J = 0; J <= I; J++)
      for (int tn = J * S; tn < std::min(T, (J + 1) * S); tn++)
        for (int tm = std::max(I * S, tn); tm < std::min(T, (I + 1) * S); tm++) m.push_back(tm << 16 | tn);
  return m;
}
// GemmTile<128, 128>::tile_of on the host: tile index -> (tile row, tile column) of an M x N product on 128 x 128 tiles,
// row by row in groups of eight tile rows, the rows of a triangle, or by the tile order `order` (gemm_tri_order)
static inline void gemm_tile_of_host(int M, int N, int lower, const int *order, long long t, int &tm, int &tn) {
  if (order) {
    tm = order[t] >> 16, tn = order[t] & 0xffff;
  } else if (lower) {
    const long long tcols = (N + 127) / 128, tri = tcols * (tcols + 1) / 2;
    if (t < tri) {
      tm = 0;
      while ((long long)(tm + 1) * (tm + 2) / 2 <= t) tm++;
      tn = (int)(t - (long long)tm * (tm + 1) / 2);
    } else
      tm = (int)(tcols + (t - tri) / tcols), tn = (int)((t - tri) % tcols);
  } else {
    const long long tiles_n = (N + 127) / 128, tiles_m = (M + 127) / 128, GM = 8;
    const long long grp = t / (GM * tiles_n), first = grp * GM, rows = std::min(GM, tiles_m - first), in = t - grp * GM * tiles_n;
    tm = (int)(first + in % rows), tn = (int)(in / rows);
  }
}
// The k ranges of the tiles of a product in the profile form, two ints per tile in the launch's tile order: `panel`
// holds the k-slab range [lo, hi) of every 128-wide column panel of the ranged operand, by = 1: B's (tile (tm, tn)
// takes panel tn: W = V+ F), by = 2: A's (panel tm: G = F'W)
static inline std::vector<int> gemm_profile_tile_ranges(int M, int N, int lower, const int *order, const int *panel, int by) {
  const long long tiles = gemm_tiles(M, N, 128, lower);
  std::vector<int> r(2 * (size_t)tiles);
  for (long long t = 0; t < tiles; t++) {
    int tm, tn;
    gemm_tile_of_host(M, N, lower, order, t, tm, tn);
    const int p = by == 2 ? tm : tn;
    r[2 * t] = panel[2 * p], r[2 * t + 1] = panel[2 * p + 1];
  }
  return r;
}

// What the holder of a launch offers: the handle's 128 x 128 variant (HQPKKT_NO_LDSDMA, HQPKKT_DGEMM_WAVES), the CUs, the
// workgroups of the cut forms (0: not used), the tiles the launch rule may give a cut form and the size of the arrival
// counters' array, the workspaces of the first and the second stream (gemm_form), whether the cut form may take unequal
// shares (HQPKKT_SK_TABLE, and never one system over several ranks: gemm_choose_list), and the rule's flags (GEMM_SHARDED,
// GEMM_NO_KS, GEMM_NO_TILE_MAP, GEMM_FORCE_SPLIT)
struct GemmCaps {
  int variant = GEMM_DMA8, cus = 0, grid = 0;
  long long sk_tiles = 0, cnt_elems = 0, ws_elems = 0, ws2_elems = 0;
  bool unequal = true;
  int flags = 0;
};
// What the schedule of a launch depends on, and nothing else (gemm_request makes it of a GemmArgs, staged_gemm.hip.h);
// equal requests share a cache entry.  second: a launch of the second stream; ntiles > 0: the launch computes that many
// 128 x 128 tiles out of a list of the caller's; dma: the operands may be staged by LDS-DMA (gemm_operands_dma_ok);
// mu > 0: the control-row segment is asked for, seg_ok: its operands admit it (gemm_ctrl_rows_ok); by 1 / 2: the profile
// form with the (lo, hi) k-slab ranges of B's / A's 128-column panels in `panel`
struct GemmRequest {
  int M = 0, N = 0, K = 0, K2 = 0, lower = 0, mirror = 0, ntiles = 0;
  bool second = false, dma = false;
  int mu = 0;
  bool seg_ok = false;
  int by = 0;
  std::vector<int> panel;
  bool operator==(const GemmRequest &o) const {
    return M == o.M && N == o.N && K == o.K && K2 == o.K2 && lower == o.lower && mirror == o.mirror && ntiles == o.ntiles && second == o.second &&
           dma == o.dma && mu == o.mu && seg_ok == o.seg_ok && by == o.by && panel == o.panel;
  }
};
static const int SK_LIST_PROFILE = 3;  // (beside sk_table.hpp's SkList: the list of gemm_profile_table)
// nslab: k-slabs of a tile (both segments).  list / tab: the work list of a cut or profile form (SK_LIST_NONE: a cut form
// whose lists' pieces the workspace does not hold - a plain round of whole tiles).  order: the tile order of a large
// triangle, or - seg - that of the control-row segment (bit 31: the augmented form); empty: the kernel's own.  seg: the
// segment is taken; a request for it that is not taken has the schedule of the launch without it
struct GemmSchedule {
  GemmForm f;
  long long nslab = 0;
  int variant = GEMM_REG4;
  int list = SK_LIST_NONE;
  SplitTable tab;
  std::vector<int> order;
  bool seg = false;
  bool cut() const { return f.kind == GEMM_FORM_FRAC || f.kind == GEMM_FORM_CUT; }
  // the launch looks something up on the device (or is counted among the work lists): it needs a cache entry
  bool kept() const { return cut() || f.kind == GEMM_FORM_PROFILE || !order.empty(); }
};
// REFUSED: no form takes the request; CAPACITY: the profile form's list does not fit the counters or the workspace (that
// form has no plain round to fall back to: a round of whole tiles would read what the ranges leave out)
enum GemmSchedStatus { GEMM_SCHED_OK = 0, GEMM_SCHED_REFUSED = 1, GEMM_SCHED_CAPACITY = 2 };

static inline int gemm_schedule(const GemmCaps &c, const GemmRequest &r, GemmSchedule &s) {
  s = GemmSchedule{};
  if (r.M <= 0 || r.N <= 0 || r.K < 0 || r.K2 < 0) return GEMM_SCHED_REFUSED;
  // (a launch with a second k segment counts as one of the depth of both: a multiple of the slab)
  s.nslab = gemm_slabs(r.K) + (r.K2 > 0 ? gemm_slabs(r.K2) : 0);
  const int Kf = r.K2 > 0 ? (int)(s.nslab * GEMM_BK) : r.K, T = (r.M + 127) / 128;
  // operands by LDS-DMA only from 16-byte aligned rows; the others are staged through registers
  s.variant = r.dma ? c.variant : GEMM_REG4;
  const bool dma = s.variant != GEMM_REG4;
  if (r.by) {
    s.f = gemm_form_profile(r.M, r.N, r.lower, c.flags);
    if ((r.by != 1 && r.by != 2) || r.K2 > 0 || c.grid <= 0 || (long long)r.panel.size() != 2LL * (((r.by == 2 ? r.M : r.N) + 127) / 128)) return GEMM_SCHED_REFUSED;
  } else
    s.f = r.ntiles ? gemm_form_tiles(r.ntiles, Kf, c.grid, c.sk_tiles)
                   : gemm_form(r.M, r.N, Kf, r.lower, r.mirror, c.cus, c.grid, c.sk_tiles, c.ws_elems, c.ws2_elems, c.flags | (r.second ? GEMM_SECOND_STREAM : 0));
  if (s.f.kind == GEMM_FORM_NONE) return GEMM_SCHED_REFUSED;
  // the second segment exists in the 128 x 128 LDS-DMA kernels alone
  if (r.K2 > 0 && !(dma && (s.cut() || s.f.kind == GEMM_FORM_PLAIN))) return GEMM_SCHED_REFUSED;
  if (s.f.tile_map) s.order = gemm_tri_order(T);
  const long long slot = 128LL * 128;
  if (r.by) {  // every tile over the k-slabs of its panel of the ranged operand, in the launch's tile order
    const std::vector<int> ranges = gemm_profile_tile_ranges(r.M, r.N, r.lower, s.f.tile_map ? s.order.data() : nullptr, r.panel.data(), r.by);
    if (s.f.tiles > c.cnt_elems - 4 || !gemm_profile_table(ranges.data(), s.f.tiles, c.grid, s.tab) || s.tab.pieces * slot > c.ws_elems) return GEMM_SCHED_CAPACITY;
    s.list = SK_LIST_PROFILE;
    return GEMM_SCHED_OK;
  }
  if (!s.cut()) return GEMM_SCHED_OK;
  const bool frac = s.f.kind == GEMM_FORM_FRAC;
  // The control-row segment (gemm_ctrl_rows_order): a cut form on the 2 x 4 LDS-DMA kernels, tiles + 1 logical tiles in
  // the list the chooser gives that count, within the counters, and the tile order that puts the last tile column first
  // and the augmented row last.  No such list: not taken - the caller forms the control rows by a product of their own
  if (r.mu > 0 && r.seg_ok && !s.f.tile_map && (s.variant == GEMM_DMA8 || s.variant == GEMM_DMA8X3)) {
    const int list = gemm_choose_list(frac, c.unequal, s.f.tiles + 1, s.nslab, c.grid, c.sk_tiles + 1, c.ws_elems, s.tab);
    if (list != SK_LIST_NONE && s.f.tiles + 1 <= c.cnt_elems && gemm_ctrl_rows_order(s.tab, c.grid, T, (int)(s.f.tiles / T), s.order)) {
      s.list = list, s.seg = true;
      return GEMM_SCHED_OK;
    }
  }
  s.list = gemm_choose_list(frac, c.unequal, s.f.tiles, s.nslab, c.grid, c.sk_tiles, c.ws_elems, s.tab);
  if (s.list == SK_LIST_NONE) s.tab = SplitTable{};
  return GEMM_SCHED_OK;
}
}  // namespace stg
