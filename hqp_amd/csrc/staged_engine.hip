// The STAGED engine (HQPKKT_MODE_STAGED, staged.hip.h / staged_host.hip.h): its entry points of the C ABI, what the
// other units call (factor, step, the dense dynamics' share of the residual products), and the debug entry points that
// read a handle.  The entries on the dense stage Hessians are staged_hess_host.hip.h, the hooks that stand outside a
// handle staged_hooks.hip.h: both parts of this unit.
#include "hqpkkt_handle.hpp"

#include <algorithm>
#include <limits>

#include "staged.hip.h"
#include "staged_gradl.hip.h"
#include "staged_sparse.hip.h"
#include "staged_profile.hip.h"
#include "staged_rows.hip.h"
#include "staged_hess.hip.h"
#include "staged_host.hip.h"

// y = Q x over the dense stage Hessians of all stages: one launch (k_hs_symv) for the stages that keep their dense block,
// a launch pair (k_hp_symv_tiles, k_hp_symv_finish) for those stored as packed lower tiles
static void staged_hess_symv(hqpkkt_t *h, StagedDev &d, const double *x, double *y) {
  const kktdev::StagedPlan &P = d.plan;
  if (d.hess.hs_nz_max > 0 || !P.hess_packed) {
    const int nzmax = std::max(d.hess.hs_nz_max, 1);
    KLAUNCH(h, KC_RESIDUAL, stg::k_hs_symv<<<dim3(std::min((nzmax + 3) / 4, 1024), P.K + 1), 256, 0, h->stream>>>(d.hess.desc.p, d.hess.Q.p, x, y));
  }
  if (d.hess.hp_chunks_max > 0) {
    KLAUNCH(h, KC_RESIDUAL, stg::k_hp_symv_tiles<<<dim3(d.hess.hp_chunks_max, P.K + 1), 256, 0, h->stream>>>(d.hess.hp_desc.p, d.hess.Q.p, x, d.hess.scr.p));
    KLAUNCH(h, KC_RESIDUAL, stg::k_hp_symv_finish<<<dim3(d.hess.hp_nt_max, P.K + 1), stg::HP_T, 0, h->stream>>>(d.hess.hp_desc.p, d.hess.scr.p, y));
  }
}
int staged_dense_products(hqpkkt_t *h, const Vecs &v, const double **x1, const double **x2, int *ndyn, const double **xq) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  if (P.hess_dense) {  // dense stage Hessians: Q dx in place of the walk over Q's rows
    staged_hess_symv(h, d, v.dx, d.hess.y.p);
    *xq = d.hess.y.p;
  }
  if (!P.dense_dyn) return 0;
  int nzmax = 1, npmax = 1;
  for (int k = 0; k < P.K; k++) nzmax = std::max(nzmax, P.hess_order(k)), npmax = std::max(npmax, P.nk[k + 1]);
  nzmax = std::max(nzmax, P.nk[P.K]);
  if (P.sharded) {
    // the rank's share of both products from its local blocks (staged.hip.h, DynLoc), summed over the ranks
    const long long tot = d.dres_sh.sum_x2 + P.ndyn;
    KLAUNCH(h, KC_RESIDUAL, stg::k_st_zero<<<nblk(tot), 256, 0, h->stream>>>(tot, d.dres_sh.sum.p));
    KLAUNCH(h, KC_RESIDUAL, stg::k_st_dynloc_ax<<<dim3(std::min((npmax + 3) / 4, 2048), P.K), 256, 0, h->stream>>>(d.dres_sh.loc.p, d.F.p, v.dx,
                                                                                                           d.dres_sh.sum.p + d.dres_sh.sum_x2));
    KLAUNCH(h, KC_RESIDUAL, stg::k_st_dynloc_aty<<<dim3((nzmax + 255) / 256, P.K + 1), 256, 0, h->stream>>>(d.dres_sh.loc.p, d.F.p, v.dy, d.dres_sh.sum.p));
    int e = exchange(h, HQPKKT_XCHG_ALLREDUCE_SUM, d.dres_sh.sum.p, tot, 1);
    if (e) return e;
    *x1 = d.dres_sh.sum.p, *x2 = d.dres_sh.sum.p + d.dres_sh.sum_x2, *ndyn = P.ndyn;
    return 0;
  }
  // one pass over F for both products (k_st_dyn_both), then the row sums' column blocks (DynResidual::part)
  const int nbc = d.dres.part_cols;
  KLAUNCH(h, KC_RESIDUAL, stg::k_st_dyn_both<<<dim3(nbc, P.K + 1), 256, 0, h->stream>>>(d.dres.desc.p, d.F.p, v.dx, v.dy, d.dres.x1.p,
                                                                                      d.dres.part.p, nbc));
  KLAUNCH(h, KC_RESIDUAL, stg::k_st_dyn_ax_finish<<<dim3((npmax + 255) / 256, P.K), 256, 0, h->stream>>>(d.dres.desc.p, d.dres.part.p, nbc,
                                                                                                   v.dx, d.dres.x2.p));
  *x1 = d.dres.x1.p, *x2 = d.dres.x2.p, *ndyn = P.ndyn;
  return 0;
}
void staged_rows_products(hqpkkt_t *h, const Vecs &v, const double **xcw, const double **cw, CsrDev *CT, CsrDev *C) {
  StagedDev &d = *h->sd;
  if (!d.plan.rows_vec()) return;
  st_rows_cols(h, d, v.dz);
  st_rows_rows(h, d, stg::RowsGemv{nullptr, nullptr, 0, nullptr, nullptr, v.dx, nullptr, nullptr, nullptr, nullptr, nullptr, d.wr.cdx.p});
  *xcw = d.wr.xc.p, *cw = d.wr.cdx.p, *CT = d.wr.CTn.dev(), *C = d.wr.Cn.dev();
}
static bool staged_is_sharded(hqpkkt_t *h) { return h->sd && h->sd->plan.sharded; }
int staged_factor(hqpkkt_t *h, const Vecs &v) {
  if (staged_is_sharded(h)) return staged_run_factor(h, v.z, v.w);  // an exchange per stage: not captured
  return graphed(h, h->gfactor[0], [&]() { return staged_run_factor(h, v.z, v.w); });
}
int staged_step(hqpkkt_t *h, const Vecs &v, int which) {
  if (staged_is_sharded(h)) return staged_run_step(h, v);  // exchanges inside the sweeps: not captured
  return graphed(h, h->gstep[which][0], [&]() { return staged_run_step(h, v); });
}
void StagedDevDelete::operator()(StagedDev *d) const { delete d; }
void staged_reset(StagedDev &d) {
  kktdev::StagedPlan plan = std::move(d.plan);
  d = StagedDev();
  d.plan = std::move(plan);
}

// a 64-bit count as (low, high) ints
static void push_count(std::vector<int> &out, long long c) { out.push_back((int)(unsigned)(c & 0xffffffffLL)), out.push_back((int)(c >> 32)); }

// hqpkkt_debug_get's STAGED items (20 .. 28, 32 .. 39, 41 .. 47); the handle is in HQPKKT_MODE_STAGED and analysed
int staged_debug_get(const hqpkkt_t *h, int what, std::vector<int> &out) {
  if (!h->sd) return HQPKKT_E_INTERN;
  const kktdev::StagedPlan &P = h->sd->plan;
  switch (what) {
    case 20: out = P.nk; break;  // the plan
    case 21: out = P.mk; break;
    case 22: out = P.nmk; break;
    case 23: out = P.eq_ptr; break;
    case 24: out = P.eq_rows; break;
    case 25: out = P.fix_rows; break;
    case 26: out = P.cap; break;
    case 27: out = P.xcut; break;  // over several ranks: column cuts, (K+1) x (ranks+1)
    case 33:  // over several ranks: the blocks of G_xx, 10 ints each: stage, block row, block column, r0, r1, c0,
              // c1, owner, computed in the owner's own rows (1) or transposed (0), offset inside the owner's slot
      for (int k = 0; k < P.K && !P.xrect_ptr.empty(); k++)
        for (int q = P.xrect_ptr[k]; q < P.xrect_ptr[k + 1]; q++) {
          const kktdev::StagedPlan::XRect &x = P.xrects[q];
          for (int val : {k, x.a, x.b, x.r0, x.r1, x.c0, x.c1, x.owner, x.mine_rows ? 1 : 0, (int)x.off}) out.push_back(val);
        }
      break;
    case 34:  // ... and this rank's tiles of its blocks' products: per stage a count, then the tiles (tile row in the strip << 16 | tile column)
      for (int k = 0; k < P.K && !P.gtile_ptr.empty(); k++) {
        out.push_back(P.gtile_ptr[k + 1] - P.gtile_ptr[k]);
        for (int q = P.gtile_ptr[k]; q < P.gtile_ptr[k + 1]; q++) out.push_back(P.gtile[q]);
      }
      break;
    case 28:  // [0] stages whose blocked elimination ran, [1] those of them that fell back to the one-workgroup form
      out.assign(2, 0);
      if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out.data(), h->td.flags.p + 6, sizeof(int) * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return HQPKKT_E_DEVICE;
      break;
    case 32:  // free initial state of many components: [0] blocked inverse ran, [1] fell back to the LU factors
      // ... [2] the pivot block that gave up (1-based, 0: none), [3], [4] |K_jj|, |K_jj^-1| of that block, [5] max |K0 K0^-1 - I|
      // (floats as their bit patterns; the words of the blocked sweep's scratch area as the LAST factorisation left them)
      out.assign(6, 0);
      if (hipDeviceSynchronize() != hipSuccess ||
          hipMemcpy(out.data(), h->td.flags.p + stg::X0_BLOCKED, sizeof(int) * 2, hipMemcpyDeviceToHost) != hipSuccess)
        return HQPKKT_E_DEVICE;
      if (P.big0 &&
          hipMemcpy(out.data() + 2, stg::big_scratch(h->sd->misc.p + P.oScr, P.q0max).flags + 1, sizeof(int) * 4,
                    hipMemcpyDeviceToHost) != hipSuccess)
        return HQPKKT_E_DEVICE;
      break;
    case 35:  // per stage: 1 where V_k comes out of the G_xx launch (staged_stage_fused); decided at the upload
      out.assign(P.K + 1, 0);
      for (size_t k = 0; k < h->sd->prod.fused.size() && k < out.size(); k++) out[k] = h->sd->prod.fused[k];
      break;
    case 36:  // per stage k < K: stored entries of F_k, and 1 where the stage runs the sparse sequence (staged_stage_sparse), 2: the profile sequence
      for (int k = 0; k < P.K; k++) {
        long long nnz = 0;
        if (P.sparse_dyn)
          nnz = P.sp_nnz[k];
        else if (!P.dense_dyn)
          nnz = (long long)(h->pAp[P.nks[k + 1]] - h->pAp[P.nks[k]]) - P.nk[k + 1];
        else
          nnz = (long long)P.nk[k + 1] * P.hess_order(k);  // (dense hand-over: the whole block)
        const kktdev::StageSeq seq = P.stage_seq(k);  // (the plan's answer: the item is asked ahead of the upload too)
        out.push_back((int)std::min<long long>(nnz, 0x7fffffff)), out.push_back(seq == kktdev::SEQ_SPARSE ? 1 : seq == kktdev::SEQ_PROFILE ? 2 : 0);
      }
      break;
    case 37:  // the sparse form's ranges (host only): [first, end) into A's CSR arrays per dynamics row, then [first, end) into
              // the CSR arrays of A' (rows ascending inside a column) per column of the stages k < K; empty on a dense-form handle
      out = P.sp_arow;
      out.insert(out.end(), P.sp_tcol.begin(), P.sp_tcol.end());
      break;
    case 39:  // the sparse form's heavy columns (hqpkkt_set_dense_columns; host only): K + 1 pointers, then the columns of every stage,
              // local to the stage (states, then controls), ascending; empty on a dense-form handle
      out = P.hv_ptr;
      out.insert(out.end(), P.hv_cols.begin(), P.hv_cols.end());
      break;
    case 41:  // the profile form's ranges (host only): K + 1 pointers, then the (lo, hi) k-slab pairs of every stage's 128-column
              // panels of F_k; empty unless the profile form is set
      out = P.pf_ptr;
      out.insert(out.end(), P.pf_rng.begin(), P.pf_rng.end());
      break;
    case 42:  // the packed panels (host only): item 41's K + 1 pointers, then per panel (offset in doubles from the stage's first
              // panel, leading dimension); (-1, 0) for the panels of a stage that keeps its dense block; empty unless the
              // profile form is set
      out = P.pf_ptr;
      for (size_t q = 0; q < P.pf_rng.size() / 2; q++)
        out.push_back(P.packed ? (int)P.pk_off[q] : -1), out.push_back(P.packed ? P.pk_ld[q] : 0);
      break;
    case 43:  // the wide rows of C (hqpkkt_set_dense_rows; host only): K + 2 pointers, then the wide rows of every stage 0 .. K as row
              // indices of C, ascending, then per stage the H terms the plan kept and the terms its wide rows would have added,
              // each a 64-bit count as (low, high) ints; empty unless the analysis had a threshold
      if (P.rows_min > 0) {
        out = P.wr_ptr;
        out.insert(out.end(), P.wr_rows.begin(), P.wr_rows.end());
        for (int k = 0; k <= P.K; k++)
          push_count(out, P.h_kept[k]), push_count(out, P.h_cut[k]);
      }
      break;
    case 44:  // the control-row segment: [0] W launches whose augmented tiles found the control columns unfinished (the guarded
              // thin product formed the control rows of G) since the upload, then per stage 1 where the W launch takes the segment
      out.assign(P.K + 2, 0);
      if (h->sd->prod.ctl.p) {
        unsigned w[3] = {0, 0, 0};
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(w, h->sd->prod.ctl.p, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return HQPKKT_E_DEVICE;
        out[0] = (int)(w[1] + (w[2] ? 1 : 0));
      }
      for (size_t k = 0; k < h->sd->prod.ctrl_rows.size() && k + 1 < out.size(); k++) out[k + 1] = h->sd->prod.ctrl_rows[k];
      break;
    case 45:  // the dense stage Hessians (hqpkkt_set_hessian_form; host only): per stage 0 .. K the block's order, its leading
              // dimension and the H terms left in the lists as (low, high) ints; empty unless the dense form is set
      for (int k = 0; k <= P.K && P.hess_dense; k++) {
        out.push_back(P.hess_order(k)), out.push_back(P.ldQ[k]);
        push_count(out, P.h_kept[k]);
      }
      break;
    case 47:  // the packed lower tiles of the dense Hessians (hqpkkt_set_packed_hessians; host only): per stage 0 .. K eight ints -
              // the tile edge (0: the stage keeps its dense block), the tiles stored, then as (low, high) ints the stage's arena
              // elements, the doubles one dense hand-over of it moves from the caller, its share of the product's scratch;
              // empty unless packing was analysed with the dense form
      for (int k = 0; k <= P.K && P.hess_packed; k++) {
        const int nz = P.hess_order(k);
        const bool pk = P.stage_packed(k);
        const long long nt = (nz + P.HESS_T - 1) / P.HESS_T, tiles = pk ? P.hess_tiles(nz) : 0;
        out.push_back(pk ? P.HESS_T : 0), out.push_back((int)tiles);
        for (long long c : {pk ? tiles * P.HESS_T * P.HESS_T : (long long)nz * P.ldQ[k], P.hess_handover(nz, pk), pk ? P.hess_slots(nt) * P.HESS_T : 0LL})
          push_count(out, c);
      }
      break;
    case 46:  // the wide rows' vector products (host only): 1 where step and residual take the wide rows through the blocks E_k, the
              // number of wide rows, then the stored entries of C left in the narrow copy of the CSR walks and the entries taken
              // out, each as (low, high) ints; empty unless the analysis found wide rows
      if (!P.wr_rows.empty()) {
        out.push_back(P.rows_vec() ? 1 : 0), out.push_back((int)P.wr_rows.size());
        push_count(out, P.c_kept), push_count(out, P.c_cut);
      }
      break;
    case 38:  // the work lists upload made for the cut products, 5 ints each: tiles, k-slabs, form (stg::GemmFormKind), list
              // (stg::SK_LIST_*), launches that looked it up since
              // (the cut forms' entries of StagedDev::Product::gemms in the order they were made, requests with the same list as one; a
              // launch with the control-row segment: form + 100; the profile form's lists are not reported)
      for (const GemmCache::Entry &t : h->sd->prod.gemms.entries) {
        if (!t.s.cut()) continue;
        const int row[3] = {(int)t.s.f.tiles, (int)t.s.nslab, t.s.f.kind + (t.s.seg ? 100 : 0)};
        size_t q = 0;
        while (q < out.size() && !std::equal(row, row + 3, out.begin() + q)) q += 5;
        if (q == out.size()) out.insert(out.end(), {row[0], row[1], row[2], t.s.list, 0});
        out[q + 4] += t.hits;
      }
      break;
    default: return HQPKKT_E_RANGE;
  }
  return 0;
}

// A setter of the request the next analysis picks up (kktdev::StagedRequest): a STAGED handle, the value in range, then
// `set` writes it - and may still refuse
template <class Set>
static int staged_set_request(hqpkkt_t *h, bool in_range, Set set) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (!in_range) return HQPKKT_E_RANGE;
    return set(h->staged_rq);
  });
}
// the forms of an analysed STAGED handle that the entries on the sparse Q ask about (q_entries.hip, qv_prepare)
int staged_form(const hqpkkt_t *h) {
  if (!h->analyzed || h->opts.mode != HQPKKT_MODE_STAGED || !h->sd) return 0;
  const kktdev::StagedPlan &P = h->sd->plan;
  return (P.hess_dense ? STAGED_FORM_HESS_DENSE : 0) | (P.dense_dyn ? STAGED_FORM_DENSE_DYN : 0) | (P.sharded ? STAGED_FORM_SHARDED : 0);
}
// what the entry points of the dense hand-over ask of the handle (hess: of the dense stage Hessians' as well)
static bool staged_dense_ready(const hqpkkt_t *h, bool hess = false) {
  return h->analyzed && h->opts.mode == HQPKKT_MODE_STAGED && h->sd && h->sd->plan.dense_dyn && (!hess || h->sd->plan.hess_dense);
}
// a block handed over out of the library's own staging buffer (hqpkkt_stage_staging): remember when it is free again
static int staged_staging_used(hqpkkt_t *h, const double *src) {
  StagedDev &d = *h->sd;
  for (int b = 0; b < 2; b++)
    if (src == d.hblk[b].p) {
      if (!d.hblk_ev[b]) HIPCHK(hipEventCreateWithFlags(&d.hblk_ev[b].h, hipEventDisableTiming));
      HIPCHK(hipEventRecord(d.hblk_ev[b], h->stream));
    }
  return 0;
}

#include "staged_hess_host.hip.h"

extern "C" {

int hqpkkt_set_dynamics_form(hqpkkt_t *h, int form) {
  return staged_set_request(h, form == HQPKKT_DYN_DENSE || form == HQPKKT_DYN_SPARSE || form == HQPKKT_DYN_PROFILE, [&](kktdev::StagedRequest &rq) {
    rq.want_sparse = form == HQPKKT_DYN_SPARSE, rq.want_profile = form == HQPKKT_DYN_PROFILE;
    return 0;
  });
}

int hqpkkt_set_dense_columns(hqpkkt_t *h, int min_entries) {  // (read by the sparse form alone)
  return staged_set_request(h, min_entries >= -1, [&](kktdev::StagedRequest &rq) { return rq.want_heavy = min_entries, 0; });
}

int hqpkkt_set_dense_rows(hqpkkt_t *h, int min_entries) {  // (a sharded handle keeps its term lists)
  // (-1, the library's threshold: none has been measured yet)
  return staged_set_request(h, min_entries >= 0 || (min_entries == -1 && kktdev::StagedPlan::ROWS_DEFAULT > 0),
                            [&](kktdev::StagedRequest &rq) { return rq.want_rows = min_entries, 0; });
}

int hqpkkt_set_hessian_form(hqpkkt_t *h, int form) {
  return staged_set_request(h, form == HQPKKT_HESS_CSR || form == HQPKKT_HESS_DENSE,
                            [&](kktdev::StagedRequest &rq) { return rq.want_hess_dense = form == HQPKKT_HESS_DENSE, 0; });
}

int hqpkkt_set_packed_hessians(hqpkkt_t *h, int on) {  // (read with HQPKKT_HESS_DENSE alone)
  return staged_set_request(h, on == 0 || on == 1, [&](kktdev::StagedRequest &rq) { return rq.want_hess_packed = on != 0, 0; });
}

int hqpkkt_set_packed_panels(hqpkkt_t *h, int on) {  // (read by the profile form alone)
  return staged_set_request(h, on == 0 || on == 1, [&](kktdev::StagedRequest &rq) { return rq.want_packed = on != 0, 0; });
}

int hqpkkt_set_stages(hqpkkt_t *h, int K, const int *nx, const int *nu) {
  return staged_set_request(h, true, [&](kktdev::StagedRequest &rq) -> int {
    rq.given_nx.clear(), rq.given_nu.clear();
    if (K <= 0) return 0;  // back to detection from the staircase of A
    if (!nx || !nu) return HQPKKT_E_NULL;
    for (int k = 0; k <= K; k++)
      if (nx[k] < 1) return HQPKKT_E_RANGE;
    for (int k = 0; k < K; k++)
      if (nu[k] < 0) return HQPKKT_E_RANGE;
    rq.given_nx.assign(nx, nx + K + 1), rq.given_nu.assign(nu, nu + K);
    return 0;
  });
}

int hqpkkt_analyze_staged(hqpkkt_t *h, int K, const int *nx, const int *nu, int n_total, int me_rest, int m, const int *Qp,
                          const int *Qi, const int *Ep, const int *Ei, const int *Cp, const int *Ci) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (h->staged_rq.want_sparse || h->staged_rq.want_profile) return HQPKKT_E_INTERN;  // (HQPKKT_DYN_SPARSE, _PROFILE: the CSR hand-over alone)
    int e = hqpkkt_set_stages(h, K, nx, nu);
    if (e) return e;
    if (K < 1) return HQPKKT_E_RANGE;
    long long n = nx[K], ndyn = 0;
    for (int k = 0; k < K; k++) n += (long long)nx[k] + nu[k], ndyn += nx[k + 1];
    if (n > 0x7fffffffLL || ndyn + me_rest > 0x7fffffffLL || me_rest < 0 || m < 0) return HQPKKT_E_RANGE;
    if (n != n_total) return HQPKKT_E_SIZES;  // Q, E, C were built for another number of variables
    const bool hess_dense = h->staged_rq.want_hess_dense;  // (the blocks come through hqpkkt_set_stage_hessian: Qp / Qi are not read)
    if ((n > 0 && !hess_dense && (!Qp || (Qp[n] > 0 && !Qi))) || (me_rest > 0 && (!Ep || (Ep[me_rest] > 0 && !Ei))) ||
        (m > 0 && (!Cp || (Cp[m] > 0 && !Ci))))
      return HQPKKT_E_NULL;
    if (h->uploaded) {
      (void)hipSetDevice(h->opts.device);
      (void)hipStreamSynchronize(h->stream);
      h->release_device();
    }
    h->analyzed = false;
    h->ip_hot_valid = h->fr_hot_valid = false;
    const int me = (int)ndyn + me_rest;
    if (hess_dense)
      h->pQp.assign((size_t)n + 1, 0), h->pQi.clear();
    else
      h->pQp.assign(Qp, Qp + n + 1), h->pQi.assign(Qi, Qi + Qp[n]);
    h->pAp.assign((size_t)me + 1, 0);  // the dynamics rows are empty: they come as dense blocks
    for (int i = 0; i <= me_rest; i++) h->pAp[ndyn + i] = me_rest ? Ep[i] : 0;
    h->pAi.clear();
    if (me_rest && Ep[me_rest]) h->pAi.assign(Ei, Ei + Ep[me_rest]);
    h->pCp.clear(), h->pCi.clear();
    if (m) h->pCp.assign(Cp, Cp + m + 1), h->pCi.assign(Ci, Ci + Cp[m]);
    h->zd_decided = true, h->zd_weak = false;
    return staged_analyze(h, (int)n, me, m, true);
  });
}

int hqpkkt_set_values_staged(hqpkkt_t *h, const double *Qx, const double *const *F, const long long *ldF,
                             const double *Ex, const double *Cx) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (!h->analyzed || h->opts.mode != HQPKKT_MODE_STAGED || !h->sd) return HQPKKT_E_INTERN;
    Analysis &an = h->an;
    if ((an.nq && !Qx) || (an.na && !Ex) || (an.nc && !Cx) || (F && !ldF)) return HQPKKT_E_NULL;
    if (!h->sd->plan.dense_dyn) return HQPKKT_E_INTERN;  // analysed for the CSR hand-over
    if (!F) {  // the blocks came one by one (hqpkkt_set_stage_block): every one of them, since the analysis
      const std::vector<char> &bs = h->sd->blocks_set;
      if ((int)bs.size() != h->sd->plan.K || std::find(bs.begin(), bs.end(), 0) != bs.end()) return HQPKKT_E_INTERN;
    }
    if (h->sd->plan.hess_dense) {  // ... and every Hessian block (hqpkkt_set_stage_hessian)
      const std::vector<char> &qs = h->sd->hess.set;
      if ((int)qs.size() != h->sd->plan.K + 1 || std::find(qs.begin(), qs.end(), 0) != qs.end()) return HQPKKT_E_INTERN;
    }
    return staged_set_values(h, Qx, Ex, Cx, F, ldF, true);
  });
}

int hqpkkt_lagrangian_gradient_staged(hqpkkt_t *h, const double *c, const double *y, const double *z, const double *minus, double *out) {
  return guarded([&]() -> int {
    if (!h || !c || !out) return HQPKKT_E_NULL;
    if (h->analyzed && ((h->an.me > 0 && !y) || (h->an.m > 0 && !z))) return HQPKKT_E_NULL;
    if (!h->analyzed || !h->have_values) return HQPKKT_E_INTERN;
    if (!staged_dense_ready(h)) return HQPKKT_E_INTERN;  // (a handle of the CSR hand-over: hqpkkt_lagrangian_gradient)
    if (h->shard_count > 1 || h->an.shard_count > 1 || h->sd->plan.sharded) return HQPKKT_E_INTERN;  // (not built: the ranks' sum)
    int e;
    if ((e = ensure_device(h)) || (e = CallerVecs{h}.ready())) return e;
    const StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    const Analysis &an = h->an;
    const size_t n = (size_t)an.n;
    CallerVecs io{h};
    const double *dc, *dy, *dz, *dm;
    double *dout;
    if ((e = io.in(c, n, &dc)) || (e = io.in(an.me > 0 ? y : nullptr, (size_t)an.me, &dy)) ||
        (e = io.in(an.m > 0 ? z : nullptr, (size_t)an.m, &dz)) || (e = io.in(minus, n, &dm)))
      return e;
    io.out(out, n, &dout);
    // every variable is a column of one stage: (column blocks of the widest stage) x (K + 1) workgroups
    KLAUNCH(h, KC_VECTOR, stg::k_st_grad_l<<<dim3((unsigned)d.dres.part_cols, (unsigned)(P.K + 1)), 256, 0, h->stream>>>(
                              d.dres.desc.p, d.F.p, h->td.AT.dev(), h->td.CT.dev(), dc, dy, dz, dm, dout));
    HIPCHK(hipGetLastError());
    return io.finish();
  });
}

int hqpkkt_detect_stages(int n, int rows, const int *row_len, const int *last_col, const int *prev_col, int cap, int *K,
                         int *nx, int *nu, int *dyn_rows) {
  return guarded([&]() -> int {
    if (!row_len || !last_col || !prev_col || !K || !nx || !nu || !dyn_rows) return HQPKKT_E_NULL;
    if (n < 1 || rows < 1) return HQPKKT_E_FORMAT;
    std::vector<int> st, ct, fc;
    int nd = 0;
    if (kktdev::stages_from_staircase(n, rows, row_len, last_col, prev_col, st, ct, fc, nd)) return HQPKKT_E_FORMAT;
    const int k = (int)ct.size();
    if (k > cap) return HQPKKT_E_SIZES;
    *K = k, *dyn_rows = nd;
    for (int i = 0; i <= k; i++) nx[i] = st[i];
    for (int i = 0; i < k; i++) nu[i] = ct[i];
    return 0;
  });
}

int hqpkkt_stage_staging(hqpkkt_t *h, int which, double **buf, long long *elems) {
  return guarded([&]() -> int {
    if (!h || !buf || !elems || which < 0 || which > 1) return HQPKKT_E_NULL;
    if (!staged_dense_ready(h)) return HQPKKT_E_INTERN;
    int e = ensure_device(h);
    if (e) return e;
    StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    long long mx = 1;
    for (int k = 0; k < P.K; k++) mx = std::max(mx, (long long)P.nk[k + 1] * P.hess_order(k));
    // (dense stage Hessians: a block Q_k comes through the same buffers, hqpkkt_set_stage_hessian)
    for (int k = 0; k <= P.K && P.hess_dense; k++) mx = std::max(mx, (long long)P.hess_order(k) * P.hess_order(k));
    for (auto &b : d.hblk)
      if (b.count < (size_t)mx) HIPCHK(b.alloc((size_t)mx, hipHostMallocDefault));
    // the copy that last read this buffer must be over before the caller refills it
    if (d.hblk_ev[which]) HIPCHK(hipEventSynchronize(d.hblk_ev[which]));
    *buf = d.hblk[which].p, *elems = mx;
    return 0;
  });
}

int hqpkkt_set_stage_block(hqpkkt_t *h, int k, const double *F, long long ldF) {
  return guarded([&]() -> int {
    if (!h || !F) return HQPKKT_E_NULL;
    if (!staged_dense_ready(h)) return HQPKKT_E_INTERN;
    int e;
    if (!h->uploaded && (e = staged_upload(h))) return e;
    StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    if (k < 0 || k >= P.K) return HQPKKT_E_RANGE;
    if (ldF < P.hess_order(k)) return HQPKKT_E_SIZES;
    HIPCHK(hipSetDevice(h->opts.device));
    const hipMemcpyKind kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if ((e = staged_copy_block(h, k, F, ldF, kind))) return e;
    if ((e = staged_staging_used(h, F))) return e;
    if ((int)d.blocks_set.size() != P.K) d.blocks_set.assign(P.K, 0);
    d.blocks_set[k] = 1;
    h->factored = false;
    return 0;
  });
}

// STAGED: rank and number of carried rows of every stage in the last factorisation
// (2 ints per stage, K+1 stages); tests only
int hqpkkt_debug_stage_ranks(hqpkkt_t *h, int *out, int cap) {
  if (!h || !out) return HQPKKT_E_NULL;
  if (!h->sd || !h->uploaded) return HQPKKT_E_INTERN;
  HIPCHK(hipSetDevice(h->opts.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const kktdev::StagedPlan &P = h->sd->plan;
  for (int k = 0; k <= P.K && 2 * k + 1 < cap; k++)
    HIPCHK(hipMemcpy(out + 2 * k, h->sd->tab.dyn.p + P.dyn_off[k], 2 * sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

int hqpkkt_debug_stage_block(hqpkkt_t *h, int k, double *out, long long cap, long long *len) {
  if (!h || !len) return HQPKKT_E_NULL;
  if (!h->sd || !h->uploaded || h->sd->plan.sharded) return HQPKKT_E_INTERN;
  const kktdev::StagedPlan &P = h->sd->plan;
  if (k < 0 || k > P.K) return HQPKKT_E_RANGE;
  const long long n = P.nk[k];
  *len = n * n;
  if (!out) return 0;
  if (cap < n * n) return HQPKKT_E_SIZES;
  HIPCHK(hipSetDevice(h->opts.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (n) HIPCHK(hipMemcpy2D(out, sizeof(double) * n, h->sd->V.p + P.oV[k], sizeof(double) * P.ldv[k], sizeof(double) * n, n, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

#include "staged_hooks.hip.h"
