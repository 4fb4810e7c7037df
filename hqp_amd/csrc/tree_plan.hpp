// What a handle of the tree engine launches: the rule that turns an analysis into launches, as plain host code (no HIP
// call; compiles with g++ like gemm_schedule.hpp and sk_table.hpp).  tree.hip builds one TreePlan per upload and walks
// it in run_factor / run_step; hqpkkt_debug_get 48 returns it, on a machine without a device as well.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/hqpkkt.h"
#include "analysis.hpp"
#include "tree_sizes.hpp"

namespace kktdev {

static const int FWD_FUSED_MAX_SLABS = 1024;  // above: forward step of a level in two launches
static const int SU1_MAX = 768;  // levels of at most this many 64 x 64 update tiles run k_schur_update with 32 x 16 per wave
static const size_t LDS_LIMIT = 160 * 1024;

// The instances of k_factor_blk (tree.hip's table holds their kernels in this order): the pivot blocks on the matrix
// pipe, 8 wavefronts (two workgroups per CU) for levels of <= 128 pivots, 12 wavefronts beyond, each holding as many
// 16 x 16 blocks of the triangle as the level's largest front needs - five per wavefront up to 160 pivots (55 blocks on
// 11 wavefronts), six up to 176 (66 blocks: 16 registers fewer than with eight, no scratch), eight up to 192
struct FbInstance {
  int maxp, threads;
};
static const int FB_INSTANCES = 4;
static const FbInstance fb_instances[FB_INSTANCES] = {{128, 512}, {160, 768}, {176, 768}, {192, 768}};
// the smallest instance that holds a level whose largest front has p pivots
inline int fb_instance(int p) {
  int i = 0;
  while (i + 1 < FB_INSTANCES && p > fb_instances[i].maxp) i++;
  return i;
}

// what the rule reads from outside the analysis: the environment at the time of the upload, and the handle's no_polled
struct TreeSwitches {
  bool no_tree_sweeps = false;   // HQPKKT_NO_TREE_SWEEPS: no whole-tree launches
  bool no_solve_top = false;     // HQPKKT_NO_SOLVE_TOP: no fused top of the solve
  bool solve_top_fused = false;  // HQPKKT_SOLVE_TOP_FUSED: both sweeps of the top in one launch where its fronts allow
  bool no_polled = false;        // a polled launch gave up once: per-level launches only
};

enum { FWD_NONE = 0, FWD_ONE, FWD_AB, FWD_TOP, FWD_TREE };  // LevelPlan::fwd_form

// One tree level of one schedule: what run_factor and run_step launch for it.  A count or grid of 0: no launch.  Ints
// only - hqpkkt_debug_get 48 returns the records as they stand (layout: include/hqpkkt.h).
struct LevelPlan {
  int n = 0, nodes_off = 0;  // fronts of the level; where they start in level_nodes: small fronts, small blocks, the rest
  int fs_n = 0, fs_ldp = 0, fs_ldb = 0, fs_lds = 0;          // k_factor_diag_small<true>
  int sm_n = 0, sm_ldp = 0, sm_lds = 0;                      // k_factor_diag_small<false>
  int blk_n = 0, blk_inst = 0, blk_threads = 0, blk_lds = 0;  // k_factor_blk, instance fb_instances[blk_inst]
  int ps_grid = 0, ps_xps = 0, slabs_off = 0;                // k_panel_solve; offset in pairs of `slabs`
  // k_schur_update<su_variant> on su_n tiles of 64: a wave holds 32 x 32 of a tile while a level fills the chip (<2>),
  // 32 x 16 (two workgroups per tile) on the thin levels above (<1>); offset in triples of `upd_tiles`
  int su_n = 0, su_variant = 0, su_grid = 0, su_xsu = 0, tiles_off = 0;
  int big_n = 0, big_off = 0;  // k_schur_update_big on tiles of 128
  // forward sweep: k_solve_fwd_small<false> on fwd_small_n fronts; the rest by fwd_form: FWD_ONE k_solve_fwd (a handful
  // of fronts: the launch is what costs), FWD_AB k_solve_fwd_a + _b (thousands of slabs: M once per front, then the
  // slabs), FWD_TOP the level belongs to the fused top, FWD_TREE to the whole-tree launches; offset in pairs of `gslabs`
  int fwd_form = FWD_NONE, fwd_small_n = 0, fwd_grid = 0, fwd_a_grid = 0, gslabs_off = 0;
  int bwd_small_n = 0, bwd_b_grid = 0, bwd_a_grid = 0, cblks_off = 0;  // k_solve_bwd_small<false>, k_solve_bwd_b, _a
};
static const int LEVEL_PLAN_INTS = 32;
static_assert(sizeof(LevelPlan) == LEVEL_PLAN_INTS * sizeof(int), "LevelPlan is a record of ints");

struct TreePlan {
  int err = 0;      // HQPKKT_E_MEM, HQPKKT_E_INTERN: no plan
  TreeSwitches sw;  // what it was built from
  std::vector<LevelPlan> levels[2];  // [schedule][tree level]
  // a tree of small fronts only (the double-integrator structure): each sweep of the solve is ONE launch over all levels
  // (k_solve_fwd_small<true> / k_solve_bwd_small<true>); tree_factor: ... and the factorisation too
  // (k_factor_diag_small<true, true>)
  bool small_tree = false, tree_factor = false;
  int tree_ldp = 1, tree_ldb = 1;
  std::vector<int> tree_down;  // the fronts root first
  // the top levels of the tree solved by k_solve_top (solve_top.hip.h): the fronts of the levels >= lt
  struct Top {
    int n = 0, lt = 1 << 30, ns = 3;  // ns: 3 = k_solve_top<3, 11>, 4 = <4, 10>
    size_t lds = 0;
    bool split = false;  // the two sweeps as launches of their own
    std::vector<int> nodes, idx, bpos, up;  // root first; supernode -> place in nodes; border rows' words; leaves first
  } top;
  size_t lds_panel = 0, lds_bwdb = 0, lds_blk = 0;  // dynamic LDS of k_panel_solve, k_solve_bwd_b, k_factor_blk (top.lds: k_solve_top)
};

// a tree of small fronts only: whole-tree sweeps
static inline void plan_whole_tree(const Analysis &an, const TreeSwitches &sw, TreePlan &P) {
  const Analysis::Sched &S = an.sched[0];
  if (sw.no_tree_sweeps || sw.no_polled || an.shard_count != 1 || S.nnodes <= 1 || an.sched[1].nnodes != 0) return;
  for (int l = 0; l < an.nlevels; l++)
    if (S.level_fsmall[l] != S.level_ptr[l + 1] - S.level_ptr[l]) return;
  for (int l = an.nlevels - 1; l >= 0; l--)
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) P.tree_down.push_back(S.level_nodes[q]);
  P.small_tree = true, P.tree_factor = !an.upd_pingpong;
  for (int l = 0; l < an.nlevels; l++) P.tree_ldp = std::max(P.tree_ldp, S.level_fs_p[l] | 1), P.tree_ldb = std::max(P.tree_ldb, S.level_fs_b[l]);
}

// the fused top of the solve sweeps: the highest levels whose fronts all fit one instance of k_solve_top, at most
// ST_MAXSPLIT fronts (single rank: with a sharded tree the two sweeps of a schedule are not adjacent)
static inline void plan_top(const Analysis &an, const TreeSwitches &sw, TreePlan &P) {
  const Analysis::Sched &S = an.sched[0];
  TreePlan::Top &T = P.top;
  if (sw.no_solve_top || sw.no_polled || an.shard_count != 1 || S.nnodes <= 0) return;
  int lt = an.nlevels, cnt = 0, maxp = 0;
  bool ok3 = true, ok4 = true;  // the instances <3, 11> and <4, 10>
  for (int l = an.nlevels - 1; l >= 0; l--) {
    const int nn = S.level_ptr[l + 1] - S.level_ptr[l];
    bool f3 = ok3, f4 = ok4;
    int mp2 = maxp;
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) {
      const int v = S.level_nodes[q];
      f3 = f3 && st_top_fits(an.npiv[v], an.nbor[v], 3, 11), f4 = f4 && st_top_fits(an.npiv[v], an.nbor[v], 4, 10);
      mp2 = std::max(mp2, an.npiv[v]);
    }
    // (levels of small fronts stay with their one-wavefront kernels: a step of k_solve_top costs 16 wavefronts'
    // worth of barriers and reductions whatever the size of the front - measured slower on the DID tree)
    if (cnt + nn > ST_MAXSPLIT || !(f3 || f4) || S.level_fsmall[l] > 0) break;
    cnt += nn, lt = l, maxp = mp2, ok3 = f3, ok4 = f4;
  }
  if (an.nlevels - lt < 2 || cnt < 2) return;
  std::vector<int> owner(an.dim, -1);
  T.idx.assign(an.nnodes, -1);
  for (int l = an.nlevels - 1; l >= lt; l--)
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) T.idx[S.level_nodes[q]] = (int)T.nodes.size(), T.nodes.push_back(S.level_nodes[q]);
  for (size_t t = 0; t < T.nodes.size(); t++)
    for (int k = 0; k < an.npiv[T.nodes[t]]; k++) owner[an.piv_start[T.nodes[t]] + k] = (int)t;
  T.bpos.assign(T.nodes.size() * ST_CS, 0);
  for (size_t t = 0; t < T.nodes.size(); t++)
    for (int i = 0; i < an.nbor[T.nodes[t]]; i++) {
      const int ei = an.bidx[an.bptr[T.nodes[t]] + i], o = owner[ei];
      if (o < 0) {  // (a border row of a fused front belongs to a fused ancestor)
        P.err = HQPKKT_E_INTERN;
        return;
      }
      T.bpos[t * ST_CS + i] = o * ST_XS + (ei - an.piv_start[T.nodes[o]]);
    }
  // level by level, leaves first; inside a level the largest fronts first, as in `nodes`
  for (int l = lt; l < an.nlevels; l++)
    for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) T.up.push_back(S.level_nodes[q]);
  // One launch for both sweeps needs ALL its fronts resident at once (the forward sweep of a front waits for
  // fronts behind it in the launch): safe only while nothing else competes for the CUs.  Several systems in flight
  // on one GPU (bench.py's concurrent systems, scenario trees) could starve each other, so the form in use is the
  // split one - a front waits only for fronts before it - and the fused launch is an option (HQPKKT_SOLVE_TOP_FUSED,
  // 17 us less per solve: M and L21 are read once).
  T.split = (int)T.nodes.size() > ST_MAXFRONTS || !sw.solve_top_fused;
  T.n = (int)T.nodes.size(), T.lt = lt, T.ns = ok3 ? 3 : 4, T.lds = st_top_lds_bytes(maxp, T.ns);
}

// the factorisation's launches of level l of S: small fronts, small blocks, pivot blocks, panel solve, updates
static inline void plan_factor_level(const Analysis &an, const Analysis::Sched &S, int l, LevelPlan &R) {
  const int nfs = S.level_fsmall[l], nsm = S.level_small[l];
  if (nfs > 0)  // small fronts: extend-add, pivot block, panel and update in one kernel
    R.fs_n = nfs, R.fs_ldp = S.level_fs_p[l] | 1, R.fs_ldb = S.level_fs_b[l], R.fs_lds = (int)fs_lds_bytes(true, R.fs_ldp, R.fs_ldb);
  if (nsm > 0) R.sm_n = nsm, R.sm_ldp = S.level_sm_p[l] | 1, R.sm_lds = (int)fs_lds_bytes(false, R.sm_ldp, 1);
  int maxp = 0, maxb = 0;  // the largest pivot count and border among the general fronts of the level
  for (int q = S.level_ptr[l] + nfs + nsm; q < S.level_ptr[l + 1]; q++)
    maxp = std::max(maxp, an.npiv[S.level_nodes[q]]), maxb = std::max(maxb, an.nbor[S.level_nodes[q]]);
  if (R.n > nfs + nsm) {
    R.blk_n = R.n - nfs - nsm, R.blk_inst = fb_instance(maxp);
    R.blk_threads = fb_instances[R.blk_inst].threads, R.blk_lds = (int)fb_lds_bytes(maxp);
  }
  // the work lists go over the XCDs in chunks of about half a front's items (kernels.hip.h, xcd_order; measured on C2:
  // 1.875 -> 1.826 ms per factor + solve; whole fronts per chunk 1.830, contiguous ranges per XCD 1.915)
  const int xtt = (maxb + 63) / 64, xsu = std::max(1, xtt * (xtt + 1) / 4);
  const int ns = S.slab_ptr[l + 1] - S.slab_ptr[l];
  if (ns > 0) R.ps_grid = 2 * ns, R.ps_xps = std::max(1, (maxb + 31) / 32);  // (the schedule lists 32-row slabs; the kernel takes 16 rows per workgroup)
  R.su_n = S.upd_big_ptr[l] - S.upd_tile_ptr[l], R.big_n = S.upd_tile_ptr[l + 1] - S.upd_big_ptr[l];
  if (R.su_n > SU1_MAX)
    R.su_variant = 2, R.su_grid = R.su_n, R.su_xsu = xsu;
  else if (R.su_n > 0)
    R.su_variant = 1, R.su_grid = 2 * R.su_n, R.su_xsu = 2 * xsu;
}

// the per-level launches of the two sweeps of the solve
static inline void plan_solve_level(const Analysis::Sched &S, int l, LevelPlan &R) {
  const int nfs = S.level_fsmall[l], ng = S.gslab_ptr[l + 1] - S.gslab_ptr[l];  // ng: (front, 64-row slab), at least one per front
  R.fwd_small_n = nfs;
  if (ng > 0 && ng <= FWD_FUSED_MAX_SLABS)
    R.fwd_form = FWD_ONE, R.fwd_grid = ng;
  else if (ng > 0)
    R.fwd_form = FWD_AB, R.fwd_a_grid = R.n - nfs, R.fwd_grid = ng;
  R.bwd_small_n = nfs;
  if (R.n > nfs) R.bwd_b_grid = S.cblk_ptr[l + 1] - S.cblk_ptr[l], R.bwd_a_grid = R.n - nfs;
}

inline TreePlan tree_plan(const Analysis &an, const TreeSwitches &sw) {
  TreePlan P;
  P.sw = sw;
  const size_t mp = an.max_npiv;
  P.lds_panel = (PS_LD * mp + 1 + 2 * mp) * sizeof(double) + mp * sizeof(int);
  P.lds_bwdb = ((size_t)an.max_nbor + 2) * sizeof(double);
  P.lds_blk = fb_lds_bytes((int)mp);
  if (P.lds_bwdb > LDS_LIMIT || P.lds_blk > LDS_LIMIT) {
    P.err = HQPKKT_E_MEM;
    return P;
  }
  plan_whole_tree(an, sw, P);
  plan_top(an, sw, P);
  for (int w = 0; w < 2 && !P.err; w++) {
    const Analysis::Sched &S = an.sched[w];
    P.levels[w].assign(an.nlevels, LevelPlan());
    for (int l = 0; l < an.nlevels && S.nnodes; l++) {
      LevelPlan &R = P.levels[w][l];
      R.n = S.level_ptr[l + 1] - S.level_ptr[l], R.nodes_off = S.level_ptr[l];
      R.slabs_off = S.slab_ptr[l], R.tiles_off = S.upd_tile_ptr[l], R.big_off = S.upd_big_ptr[l];
      R.gslabs_off = S.gslab_ptr[l], R.cblks_off = S.cblk_ptr[l];
      if (!(w == 0 && P.tree_factor)) plan_factor_level(an, S, l, R);
      if (w == 0 && P.small_tree)
        R.fwd_form = FWD_TREE;
      else if (w == 0 && P.top.n > 0 && l >= P.top.lt)  // (the levels above: k_solve_top)
        R.fwd_form = FWD_TOP;
      else
        plan_solve_level(S, l, R);
    }
  }
  return P;
}

}  // namespace kktdev
