// Host side of the cut form of the STAGED engine's fp64 product (k_dgemm_tn_sk, staged_gemm.hip.h): the kernel walks a
// list of units of work per workgroup, and every schedule is such a list, made here - unequal shares for the two
// workgroups of a CU (gemm_split_table), equal shares in whole rounds and cut phases (gemm_equal_table), the k-slabs of
// all tiles as one sequence (gemm_frac_table), the same for tiles of unequal length (gemm_profile_table) - and chosen in
// one place (gemm_choose_list).  Plain C++ (no device code):
// used by staged_gemm.hip.h and the engine's host code and, through hqpkkt_debug_sk_table, by the CPU tests.
#pragma once
#include <algorithm>
#include <vector>

namespace stg {
// one unit of work of a workgroup: the k-slabs [s0, s1) of tile `tile`; piece j of `pieces` of that tile (pieces == 1:
// the whole tile); the tile's pieces park their partial sums in the slots slot0 ... slot0 + pieces - 1 (order of k)
struct SkUnit {
  int tile;  // < 0: end of the workgroup's list
  unsigned short s0, s1;
  int slot0;
  unsigned short pieces, j;
};
static_assert(sizeof(SkUnit) == 16, "SkUnit is read as one 16-byte word");

// UNEQUAL shares for the two workgroups of a CU.  What the stamps of the headline's products say
// (profiles/r03_dgemm_stamps.txt, r06_sk_stamps.txt; tiles of 313 k-slabs): of the two workgroups a CU holds, the one
// dispatched first (class A: blockIdx.x < grid / 2) finishes a tile in ~1000 us and the second (class B) in ~1530 us
// while both run - the older wavefronts win the arbitration for the matrix pipe -, and a workgroup alone on its CU
// takes ~700 us.  With equal shares (gemm_equal_table: W = 3 whole tiles + an eighth for everybody) class A is done at
// 3090 us and the launch ends when class B is, at 3870 us.  And cut tiles are dear: a plan with 2560 parked pieces
// instead of 256 takes 4.4 instead of 3.76 ms (tools/sk_sweep.py, profiles/r06_sk_sweep.txt) - the pieces' pipeline
// fills, their parked sums and workgroups that no longer walk the same k.  So: WHOLE tiles as far as they go, more of
// them for class A (nA per workgroup) than for class B (nB), and only the remainder of less than grid / 2 tiles cut -
// by class B, by class A or by both, in at most two groups.  The candidates are compared by a model of the pace
// (sk_model_makespan) and the best one is listed per workgroup; within a round the workgroups of a class take
// neighbouring tiles in the order of their position in the XCD (the swizzled index), as the equal-share plan does.
struct SplitTable {
  std::vector<SkUnit> units;  // grid x stride
  int stride = 0;
  long long pieces = 0;   // parking slots
  double makespan = 0.0;  // the model's, in tile times of class A
  int nA = 0, nB = 0;     // whole tiles per workgroup of the two classes
};
static inline int xcd_swizzle_host(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
  return x * q + (x < r ? x : r) + (bid >> 3);
}
// the pace model: work wa / wb (in tiles) of a workgroup of class A / B on one CU; while both run a tile takes A 1.0
// and B 1.55, alone 0.71 (measured: 987 / 1532 / 700 us)
static inline double sk_model_makespan(double wa, double wb) {
  const double rA = 1.0, rB = 1.55, alone = 0.71;
  const double ta = wa * rA, tb = wb * rB;
  return tb <= ta ? tb + (wa - tb / rA) * alone : ta + (wb - ta / rB) * alone;
}
static inline bool gemm_split_table(long long tiles, long long nslab, int grid, SplitTable &best) {
  struct Group {
    long long begin, count;
    int nsplit, cls;  // cls: 3 both classes, 1 A, 2 B
  };
  if (grid < 2 || grid % 2 || nslab >= 65536 || tiles <= 0) return false;
  const long long H = grid / 2, n = tiles / H, R = tiles - n * H;
  const int smax = (int)std::max<long long>(1, std::min<long long>(16, nslab / 16));
  const double piece_cost = 0.04;  // (a cut piece: its pipeline fill and the parked sums, in tile times)
  auto members = [&](int cls) { return (cls == 3 ? 2 : 1) * H; };
  bool have = false;
  double best_t = 0.0;
  std::vector<Group> best_groups;
  for (long long nA = (n + 1) / 2; nA <= n; nA++) {
    const long long nB = n - nA;
    // remainder: R1 tiles cut s1 ways over c1, the other R - R1 tiles cut s2 ways over c2 (s2 as large as its class allows)
    for (int c1 : {2, 1, 3})
      for (int s1 = 1; s1 <= smax; s1 = s1 < 4 ? s1 + 1 : s1 * 2) {
        const long long R1 = std::min(R, members(c1) / s1);
        const long long R2 = R - R1;
        for (int c2 : {0, 1, 2, 3}) {
          if ((R2 == 0) != (c2 == 0)) continue;
          if (c2 == c1) continue;  // (the same class twice: one group of it)
          int s2 = 0;
          if (c2) {
            s2 = (int)std::min<long long>(smax, members(c2) / R2);
            if (s2 < 1) continue;
          }
          double ea = 0.0, eb = 0.0;  // extra work of the busiest workgroup of each class
          if (R1 > 0) {
            const double w = 1.0 / s1 + (s1 > 1 ? piece_cost : 0.0);
            if (c1 & 1) ea += w;
            if (c1 & 2) eb += w;
          }
          if (c2) {
            const double w = 1.0 / s2 + (s2 > 1 ? piece_cost : 0.0);
            if (c2 & 1) ea += w;
            if (c2 & 2) eb += w;
          }
          const double t = sk_model_makespan(nA + ea, nB + eb);
          if (!have || t < best_t - 1e-9) {
            have = true, best_t = t;
            best_groups.clear();
            long long next = 0;
            for (long long r = 0; r < nB; r++) best_groups.push_back({next, 2 * H, 1, 3}), next += 2 * H;
            for (long long r = nB; r < nA; r++) best_groups.push_back({next, H, 1, 1}), next += H;
            if (R1 > 0) best_groups.push_back({next, R1, s1, c1}), next += R1;
            if (c2) best_groups.push_back({next, R2, s2, c2}), next += R2;
            best.nA = (int)nA, best.nB = (int)nB;
          }
        }
      }
  }
  if (!have) return false;
  // per workgroup its units in the order of the groups; rank within the class by the swizzled index
  std::vector<int> rankA(grid, -1), rankB(grid, -1), rankAll(grid, -1), bid_of_v(grid);
  for (int b = 0; b < grid; b++) bid_of_v[xcd_swizzle_host(b, grid)] = b;
  {
    int ra = 0, rb = 0;
    for (int v = 0; v < grid; v++) {
      const int b = bid_of_v[v];
      rankAll[b] = v;
      if (b < H) rankA[b] = ra++; else rankB[b] = rb++;
    }
  }
  std::vector<long long> slot0(tiles, -1);
  long long slots = 0;
  for (const Group &p : best_groups)
    if (p.nsplit > 1)
      for (long long t = p.begin; t < p.begin + p.count; t++) slot0[t] = slots, slots += p.nsplit;
  std::vector<std::vector<SkUnit>> per(grid);
  for (const Group &p : best_groups)
    for (int b = 0; b < grid; b++) {
      const int r = p.cls == 3 ? rankAll[b] : p.cls == 1 ? rankA[b] : rankB[b];
      if (r < 0 || r >= p.count * p.nsplit) continue;
      const long long ti = r % p.count, j = r / p.count, t = p.begin + ti;
      const long long L = (nslab + p.nsplit - 1) / p.nsplit, s0 = std::min(nslab, j * L), s1 = std::min(nslab, s0 + L);
      per[b].push_back(SkUnit{(int)t, (unsigned short)s0, (unsigned short)s1, (int)(p.nsplit > 1 ? slot0[t] : 0), (unsigned short)p.nsplit, (unsigned short)j});
    }
  size_t stride = 1;
  for (int b = 0; b < grid; b++) stride = std::max(stride, per[b].size() + 1);
  best.stride = (int)stride, best.pieces = slots, best.makespan = best_t;
  best.units.assign((size_t)grid * stride, SkUnit{-1, 0, 0, 0, 0, 0});
  for (int b = 0; b < grid; b++)
    for (size_t i = 0; i < per[b].size(); i++) best.units[(size_t)b * stride + i] = per[b][i];
  return true;
}

// EQUAL shares: the plan for `tiles` tiles of `nslab` k-slabs on `grid` workgroups.  The remainder R of the whole
// rounds is cut floor(grid / R) ways; a remainder of more than half a round first gives grid / 2 tiles to
// two workgroups each (a full phase of half the depth) and cuts the rest after that.  A piece holds at
// least 16 slabs (below that the pipeline fill of a piece and the parked partial sums cost more than the
// balance gains) and a tile has at most 16 pieces (the last arriver reads them one after the other).
struct EqualPlan {
  int whole;  // the first `whole` tiles (whole rounds of the grid) are computed whole
  int nphase;
  int begin[2], count[2], split[2];  // phase q: count[q] tiles from begin[q] on, the k range of each in split[q] pieces
};
static inline EqualPlan gemm_split_plan(long long tiles, long long nslab, int grid) {
  EqualPlan sp{};
  const long long smax = std::max<long long>(1, std::min<long long>(16, nslab / 16));
  long long begin = tiles / grid * grid, R = tiles - begin;
  sp.whole = (int)begin;
  while (R > 0 && sp.nphase < 2) {
    long long s = std::min<long long>(smax, grid / R), r = R;
    if (s <= 1) {
      s = 1;
      // (the half round needs an even grid: with an odd one workgroup grid - 1 would start on the next phase's first
      // unit, which workgroup 0 takes as well)
      if (sp.nphase == 0 && smax >= 2 && R > grid / 2 && grid % 2 == 0) s = 2, r = grid / 2;
    }
    sp.begin[sp.nphase] = (int)begin, sp.count[sp.nphase] = (int)r, sp.split[sp.nphase] = (int)s;
    sp.nphase++, begin += r, R -= r;
  }
  return sp;
}
// parked pieces of the plan: the slots of its list (the handle's workspace is sized by this).  A phase that cuts nothing
// (split 1: an odd grid, or too few k-slabs for two pieces) parks nothing
static inline long long gemm_split_plan_pieces(const EqualPlan &sp) {
  long long n = 0;
  for (int q = 0; q < sp.nphase; q++) n += sp.split[q] > 1 ? (long long)sp.count[q] * sp.split[q] : 0;
  return n;
}
// rows of workgroups (by blockIdx.x) -> a table with an end mark behind every row
static inline void sk_table_pack(const std::vector<std::vector<SkUnit>> &per, long long pieces, SplitTable &out) {
  size_t stride = 1;
  for (const auto &row : per) stride = std::max(stride, row.size() + 1);
  out = SplitTable{};
  out.stride = (int)stride, out.pieces = pieces;
  out.units.assign(per.size() * stride, SkUnit{-1, 0, 0, 0, 0, 0});
  for (size_t b = 0; b < per.size(); b++) std::copy(per[b].begin(), per[b].end(), out.units.begin() + b * stride);
}
// The plan as a list.  Units: the whole tiles of the rounds (unit u = tile u), then the pieces of the cut phases (phase q:
// unit j * count[q] + ti = piece j of its tile ti).  The workgroup at position v (after the XCD swizzle) does unit v of
// every round and phase: its neighbours in the XCD work on the neighbouring tiles at the same k and share their operand
// panels in that XCD's L2 (a contiguous range of (tile, k-slab) units per workgroup balances as well but leaves the
// workgroups at as many different k, and the launch then runs at the speed of its operand reads).
static inline bool gemm_equal_table(long long tiles, long long nslab, int grid, SplitTable &out) {
  if (grid < 1 || nslab < 1 || nslab >= 65536 || tiles <= 0) return false;
  const EqualPlan sp = gemm_split_plan(tiles, nslab, grid);
  std::vector<std::vector<SkUnit>> per(grid);
  for (int b = 0; b < grid; b++) {
    const int v = xcd_swizzle_host(b, grid);
    for (long long u = v; u < sp.whole; u += grid) per[b].push_back(SkUnit{(int)u, 0, (unsigned short)nslab, 0, 1, 0});
    long long slots = 0;  // (of the phases before q)
    for (int q = 0; q < sp.nphase; q++) {
      const long long cnt = sp.count[q], pieces = sp.split[q], slot_q = slots;
      if (pieces > 1) slots += cnt * pieces;
      if (v >= cnt * pieces) continue;
      const long long ti = v % cnt, j = v / cnt, L = (nslab + pieces - 1) / pieces;
      const long long s0 = std::min(nslab, j * L), s1 = std::min(nslab, s0 + L);
      per[b].push_back(SkUnit{sp.begin[q] + (int)ti, (unsigned short)s0, (unsigned short)s1, (int)(pieces > 1 ? slot_q + ti * pieces : 0),
                              (unsigned short)pieces, (unsigned short)j});
    }
  }
  sk_table_pack(per, gemm_split_plan_pieces(sp), out);
  return true;
}
// The FRACTIONAL cut: the tiles' k-slabs in one sequence (tile t holds the units t nslab ...), cut into `per` units per
// workgroup - the workgroup at position v takes [v per, (v + 1) per): the end of one tile, whole tiles, the start of
// another.  A tile that several workgroups share is summed by its last arriver in the order of the workgroups; a
// workgroup parks at most two partial tiles, so the list has at most 2 grid slots.  For products of a few hundred tiles
// (stages of 1000 - 3000 states), where whole rounds and cut remainders leave a large part of the chip idle.
static inline bool gemm_frac_table(long long tiles, long long nslab, int grid, SplitTable &out) {
  if (grid < 1 || nslab < 1 || nslab >= 65536 || tiles <= 0) return false;
  const long long U = tiles * nslab, share = (U + grid - 1) / grid;
  auto sharers = [&](long long t, long long &first) {  // the workgroups whose ranges meet tile t
    first = t * nslab / share;
    return ((t + 1) * nslab - 1) / share - first + 1;
  };
  std::vector<long long> slot0(tiles, 0);
  long long slots = 0, first;
  for (long long t = 0; t < tiles; t++) {
    const long long pieces = sharers(t, first);
    if (pieces > 1) slot0[t] = slots, slots += pieces;
  }
  std::vector<std::vector<SkUnit>> per(grid);
  for (int b = 0; b < grid; b++) {
    const long long v = xcd_swizzle_host(b, grid), lo = std::min(U, v * share), hi = std::min(U, lo + share);
    for (long long x = lo; x < hi;) {
      const long long t = x / nslab, s0 = x - t * nslab, s1 = std::min(nslab, s0 + (hi - x)), pieces = sharers(t, first);
      per[b].push_back(SkUnit{(int)t, (unsigned short)s0, (unsigned short)s1, (int)slot0[t], (unsigned short)pieces, (unsigned short)(v - first)});
      x += s1 - s0;
    }
  }
  sk_table_pack(per, slots, out);
  return true;
}
// The same for tiles of UNEQUAL length (the profile form of the stage products, staged_plan.hpp: a tile of W = V+ F or
// G = F'W takes only the k-slabs that hold the stored entries of its panel of F_k): tile t takes the slabs
// [ranges[2 t], ranges[2 t + 1]).  The slabs of all tiles form one sequence in the launch's tile order, every workgroup
// gets an equal, contiguous share of it (the workgroup at position v after the XCD swizzle the v-th), a tile that several
// workgroups share is parked and summed by its last arriver in the order of k, and a workgroup parks at most two
// tiles: at most 2 grid slots.  A tile without slabs is still one unit (s0 = s1, pieces = 1) of the workgroup at whose
// position in the sequence it stands: its zeros must be written.
// A tile weighs its slabs and nothing else: no constant for its pipeline fill and epilogue (none was measured; with
// one a workgroup's share of slabs is no longer bounded by ceil(total / grid)).
static inline bool gemm_profile_table(const int *ranges, long long tiles, int grid, SplitTable &out) {
  if (grid < 1 || tiles <= 0 || !ranges) return false;
  std::vector<long long> pre(tiles + 1, 0);
  for (long long t = 0; t < tiles; t++) {
    const long long lo = ranges[2 * t], hi = ranges[2 * t + 1];
    if (lo < 0 || hi < lo || hi >= 65536) return false;
    pre[t + 1] = pre[t] + (hi - lo);
  }
  const long long U = pre[tiles], share = std::max<long long>(1, (U + grid - 1) / grid);
  std::vector<std::vector<SkUnit>> pos(grid), per(grid);
  long long slots = 0;
  for (long long t = 0; t < tiles; t++) {
    const long long lo = ranges[2 * t], len = pre[t + 1] - pre[t];
    if (len == 0) {
      pos[std::min<long long>(grid - 1, pre[t] / share)].push_back(SkUnit{(int)t, (unsigned short)lo, (unsigned short)lo, 0, 1, 0});
      continue;
    }
    const long long first = pre[t] / share, last = (pre[t + 1] - 1) / share, pieces = last - first + 1;
    for (long long v = first; v <= last; v++) {
      const long long x0 = std::max(pre[t], v * share), x1 = std::min(pre[t + 1], (v + 1) * share);
      pos[v].push_back(SkUnit{(int)t, (unsigned short)(lo + x0 - pre[t]), (unsigned short)(lo + x1 - pre[t]), (int)(pieces > 1 ? slots : 0),
                              (unsigned short)pieces, (unsigned short)(v - first)});
    }
    if (pieces > 1) slots += pieces;
  }
  for (int b = 0; b < grid; b++) per[b] = pos[xcd_swizzle_host(b, grid)];
  sk_table_pack(per, slots, out);
  return true;
}

// Which list a launch of the cut forms walks - decided here alone, for the schedule of a launch (gemm_schedule.hpp: the
// engine in upload's dry walk of the factor sequence, and the self-test hqpkkt_debug_dgemm).  SK_LIST_NONE: no list whose parked pieces fit the workspace of `ws_elems`
// doubles - the launch is a plain round of whole tiles instead.
// `frac`: the launch rule gave the fractional form (gemm_form.hpp).  Otherwise the unequal shares, unless they are
// switched off (HQPKKT_SK_TABLE=0), the system is sharded over several ranks - there the strip's product runs beside the
// second stream's control-sized chain, and the pace of the two workgroups of a CU that the shares are fitted to is not
// the one measured for a launch that has the chip to itself - or they do not build or fit; then the equal shares.
enum SkList { SK_LIST_NONE = -1, SK_LIST_UNEQUAL = 0, SK_LIST_EQUAL = 1, SK_LIST_FRAC = 2 };
static inline bool gemm_list_table(int list, long long tiles, long long nslab, int grid, SplitTable &t) {
  return list == SK_LIST_UNEQUAL ? gemm_split_table(tiles, nslab, grid, t)
         : list == SK_LIST_EQUAL ? gemm_equal_table(tiles, nslab, grid, t)
                                 : list == SK_LIST_FRAC && gemm_frac_table(tiles, nslab, grid, t);
}
static inline int gemm_choose_list(bool frac, bool unequal, long long tiles, long long nslab, int grid, long long sk_tiles, long long ws_elems,
                                   SplitTable &t) {
  const long long slot = 128LL * 128;
  if (frac) return gemm_frac_table(tiles, nslab, grid, t) && t.pieces * slot <= ws_elems ? SK_LIST_FRAC : SK_LIST_NONE;
  if (unequal && gemm_split_table(tiles, nslab, grid, t) && t.pieces * slot <= ws_elems && tiles <= sk_tiles) return SK_LIST_UNEQUAL;
  return gemm_equal_table(tiles, nslab, grid, t) && t.pieces * slot <= ws_elems ? SK_LIST_EQUAL : SK_LIST_NONE;
}

// The control-row segment of a product whose last tile row is ragged (k_dgemm_tn_sk<.., AUG>, GemmArgs::Au): the tiles
// of the last tile ROW (r = M - 128 tm_last valid rows of 128) also multiply the columns [c0, c0 + mu) of C itself - which
// the tiles of the last tile COLUMN of the same launch write - from the free rows of their A panel.  So the launch has
// one more unit of work than tiles, the corner tile twice (early in plain form, late in augmented form), and an order:
//   - the tiles of the last tile column stand at the START of their workgroups' lists (every unit of such a tile has
//     only units of such tiles in front of it),
//   - the augmented tiles at the END of theirs (behind every unit of such a tile come only units of such tiles).
// With fewer of them than workgroups - the headline's W: 40 and 40 on 512 - that is the first and the last unit.
// Nothing else about a list changes: it is built as always for tiles + 1 logical tiles, and only which tile of C a
// logical tile is (GemmArgs::tile_map, bit 31: augmented) is decided here - the logical tiles that end earliest are the
// last tile column, those that start latest the augmented row, all others keep the launch's order (groups of eight tile
// rows, column by column).  Returns false where the list has no such order (a tile count that puts a cut piece of a
// late tile in front of a whole one); the caller then forms the control rows by a product of their own.
static const int SK_TILE_AUG = (int)0x80000000;
static inline bool gemm_ctrl_rows_order(const SplitTable &t, int grid, int tiles_m, int tiles_n, std::vector<int> &map) {
  const long long T = (long long)tiles_m * tiles_n + 1;
  if (tiles_m < 1 || tiles_n < 1 || tiles_m >= 32768 || tiles_n >= 65536 || grid < 1 || t.stride < 1 || (long long)t.units.size() != (long long)grid * t.stride) return false;
  std::vector<int> len(grid, 0), head(T, 0), tail(T, 0), seen(T, 0);
  for (int b = 0; b < grid; b++)
    while (len[b] < t.stride && t.units[(size_t)b * t.stride + len[b]].tile >= 0) len[b]++;
  for (int b = 0; b < grid; b++)
    for (int i = 0; i < len[b]; i++) {
      const int id = t.units[(size_t)b * t.stride + i].tile;
      if (id >= T) return false;
      seen[id] = 1, head[id] = std::max(head[id], i), tail[id] = std::max(tail[id], len[b] - 1 - i);
    }
  std::vector<int> ids(T), role(T, 0);  // role 1: last tile column, 2: augmented
  for (long long i = 0; i < T; i++) {
    if (!seen[i]) return false;
    ids[i] = (int)i;
  }
  std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return head[a] < head[b]; });
  for (int i = 0; i < tiles_m; i++) role[ids[i]] = 1;
  for (long long i = 0; i < T; i++) ids[i] = (int)(T - 1 - i);
  std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return tail[a] < tail[b]; });
  for (int i = 0; i < tiles_n; i++) {
    if (role[ids[i]]) return false;
    role[ids[i]] = 2;
  }
  for (int b = 0; b < grid; b++) {
    int first_other = len[b], last_other = -1;
    for (int i = 0; i < len[b]; i++)
      if (role[t.units[(size_t)b * t.stride + i].tile] != 1) {
        first_other = i;
        break;
      }
    for (int i = len[b] - 1; i >= 0; i--)
      if (role[t.units[(size_t)b * t.stride + i].tile] != 2) {
        last_other = i;
        break;
      }
    for (int i = 0; i < len[b]; i++) {
      const int ro = role[t.units[(size_t)b * t.stride + i].tile];
      if ((ro == 1 && i > first_other) || (ro == 2 && i < last_other)) return false;
    }
  }
  map.assign(T, 0);
  const int GM = 8;
  long long next = 0;  // the launch's own order of the tiles outside the last row and column
  auto next_inner = [&]() {
    for (;; next++) {
      const long long grp = next / ((long long)GM * tiles_n), first = grp * GM, rows = std::min<long long>(GM, tiles_m - first), in = next - grp * GM * tiles_n;
      const int tm = (int)(first + in % rows), tn = (int)(in / rows);
      if (tm != tiles_m - 1 && tn != tiles_n - 1) {
        next++;
        return tm << 16 | tn;
      }
    }
  };
  int col = 0, row = 0;
  for (long long i = 0; i < T; i++)
    map[i] = role[i] == 1 ? (col++) << 16 | (tiles_n - 1) : role[i] == 2 ? (SK_TILE_AUG | (tiles_m - 1) << 16 | (row++)) : next_inner();
  return true;
}
}  // namespace stg
