// The STAGED engine (HQPKKT_MODE_STAGED, staged.hip.h / staged_host.hip.h): its entry points of the C ABI, what the
// other units call (factor, step, the dense dynamics' share of the residual products), and its debug entry points.
#include "hqpkkt_handle.hpp"

#include <algorithm>
#include <limits>

#include "staged.hip.h"
#include "staged_sparse.hip.h"
#include "staged_profile.hip.h"
#include "staged_rows.hip.h"
#include "staged_hess.hip.h"
#include "staged_host.hip.h"

// y = Q x over the dense stage Hessians of all stages: one launch (k_hs_symv) for the stages that keep their dense block,
// a launch pair (k_hp_symv_tiles, k_hp_symv_finish) for those stored as packed lower tiles
static void staged_hess_symv(hqpkkt_t *h, StagedDev &d, const double *x, double *y) {
  const kktdev::StagedPlan &P = d.plan;
  if (d.hs_nz_max > 0 || !P.hess_packed) {
    const int nzmax = std::max(d.hs_nz_max, 1);
    KLAUNCH(h, KC_RESIDUAL, stg::k_hs_symv<<<dim3(std::min((nzmax + 3) / 4, 1024), P.K + 1), 256, 0, h->stream>>>(d.hess_desc.p, d.Qd.p, x, y));
  }
  if (d.hp_chunks_max > 0) {
    KLAUNCH(h, KC_RESIDUAL, stg::k_hp_symv_tiles<<<dim3(d.hp_chunks_max, P.K + 1), 256, 0, h->stream>>>(d.hp_desc.p, d.Qd.p, x, d.hess_scr.p));
    KLAUNCH(h, KC_RESIDUAL, stg::k_hp_symv_finish<<<dim3(d.hp_nt_max, P.K + 1), stg::HP_T, 0, h->stream>>>(d.hp_desc.p, d.hess_scr.p, y));
  }
}
int staged_dense_products(hqpkkt_t *h, const Vecs &v, const double **x1, const double **x2, int *ndyn, const double **xq) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  if (P.hess_dense) {  // dense stage Hessians: Q dx in place of the walk over Q's rows
    staged_hess_symv(h, d, v.dx, d.hess_y.p);
    *xq = d.hess_y.p;
  }
  if (!P.dense_dyn) return 0;
  int nzmax = 1, npmax = 1;
  for (int k = 0; k < P.K; k++) nzmax = std::max(nzmax, P.nk[k] + P.mk[k]), npmax = std::max(npmax, P.nk[k + 1]);
  nzmax = std::max(nzmax, P.nk[P.K]);
  if (P.sharded) {
    // the rank's share of both products from its local blocks (staged.hip.h, DynLoc), summed over the ranks
    const long long tot = d.dyn_sum_x2 + P.ndyn;
    KLAUNCH(h, KC_RESIDUAL, stg::k_st_zero<<<nblk(tot), 256, 0, h->stream>>>(tot, d.dyn_sum.p));
    KLAUNCH(h, KC_RESIDUAL, stg::k_st_dynloc_ax<<<dim3(std::min((npmax + 3) / 4, 2048), P.K), 256, 0, h->stream>>>(d.dyn_loc.p, d.F.p, v.dx,
                                                                                                           d.dyn_sum.p + d.dyn_sum_x2));
    KLAUNCH(h, KC_RESIDUAL, stg::k_st_dynloc_aty<<<dim3((nzmax + 255) / 256, P.K + 1), 256, 0, h->stream>>>(d.dyn_loc.p, d.F.p, v.dy, d.dyn_sum.p));
    int e = exchange(h, HQPKKT_XCHG_ALLREDUCE_SUM, d.dyn_sum.p, tot, 1);
    if (e) return e;
    *x1 = d.dyn_sum.p, *x2 = d.dyn_sum.p + d.dyn_sum_x2, *ndyn = P.ndyn;
    return 0;
  }
  // one pass over F for both products (k_st_dyn_both), then the row sums' column blocks (dyn_part: staged_upload)
  const int nbc = d.dyn_part_cols;
  KLAUNCH(h, KC_RESIDUAL, stg::k_st_dyn_both<<<dim3(nbc, P.K + 1), 256, 0, h->stream>>>(d.dyn_desc.p, d.F.p, v.dx, v.dy, d.dyn_x1.p,
                                                                                      d.dyn_part.p, nbc));
  KLAUNCH(h, KC_RESIDUAL, stg::k_st_dyn_ax_finish<<<dim3((npmax + 255) / 256, P.K), 256, 0, h->stream>>>(d.dyn_desc.p, d.dyn_part.p, nbc,
                                                                                                   v.dx, d.dyn_x2.p));
  *x1 = d.dyn_x1.p, *x2 = d.dyn_x2.p, *ndyn = P.ndyn;
  return 0;
}
void staged_rows_products(hqpkkt_t *h, const Vecs &v, const double **xcw, const double **cw, CsrDev *CT, CsrDev *C) {
  StagedDev &d = *h->sd;
  if (!d.plan.rows_vec()) return;
  st_rows_cols(h, d, v.dz);
  st_rows_rows(h, d, stg::RowsGemv{nullptr, nullptr, 0, nullptr, nullptr, v.dx, nullptr, nullptr, nullptr, nullptr, nullptr, d.wr_cdx.p});
  *xcw = d.wr_xc.p, *cw = d.wr_cdx.p, *CT = d.CTn.dev(), *C = d.Cn.dev();
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

// hqpkkt_debug_get's STAGED items (20 .. 28, 32 .. 39); the handle is in HQPKKT_MODE_STAGED and analysed
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
      for (size_t k = 0; k < h->sd->fused.size() && k < out.size(); k++) out[k] = h->sd->fused[k];
      break;
    case 36:  // per stage k < K: stored entries of F_k, and 1 where the stage runs the sparse sequence (staged_stage_sparse), 2: the profile sequence
      for (int k = 0; k < P.K; k++) {
        long long nnz = 0;
        if (P.sparse_dyn)
          nnz = P.sp_nnz[k];
        else if (!P.dense_dyn)
          nnz = (long long)(h->pAp[P.nks[k + 1]] - h->pAp[P.nks[k]]) - P.nk[k + 1];
        else
          nnz = (long long)P.nk[k + 1] * (P.nk[k] + P.mk[k]);  // (dense hand-over: the whole block)
        out.push_back((int)std::min<long long>(nnz, 0x7fffffff)), out.push_back(P.sparse_dyn ? 1 : P.profile_dyn && P.pf_stage[k] ? 2 : 0);
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
          for (long long c : {P.h_kept[k], P.h_cut[k]}) out.push_back((int)(unsigned)(c & 0xffffffffLL)), out.push_back((int)(c >> 32));
      }
      break;
    case 44:  // the control-row segment: [0] W launches whose augmented tiles found the control columns unfinished (the guarded
              // thin product formed the control rows of G) since the upload, then per stage 1 where the W launch takes the segment
      out.assign(P.K + 2, 0);
      if (h->sd->ctl.p) {
        unsigned w[3] = {0, 0, 0};
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(w, h->sd->ctl.p, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return HQPKKT_E_DEVICE;
        out[0] = (int)(w[1] + (w[2] ? 1 : 0));
      }
      for (size_t k = 0; k < h->sd->ctrl_rows.size() && k + 1 < out.size(); k++) out[k + 1] = h->sd->ctrl_rows[k];
      break;
    case 45:  // the dense stage Hessians (hqpkkt_set_hessian_form; host only): per stage 0 .. K the block's order, its leading
              // dimension and the H terms left in the lists as (low, high) ints; empty unless the dense form is set
      for (int k = 0; k <= P.K && P.hess_dense; k++) {
        out.push_back(P.hess_order(k)), out.push_back(P.ldQ[k]);
        out.push_back((int)(unsigned)(P.h_kept[k] & 0xffffffffLL)), out.push_back((int)(P.h_kept[k] >> 32));
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
          out.push_back((int)(unsigned)(c & 0xffffffffLL)), out.push_back((int)(c >> 32));
      }
      break;
    case 46:  // the wide rows' vector products (host only): 1 where step and residual take the wide rows through the blocks E_k, the
              // number of wide rows, then the stored entries of C left in the narrow copy of the CSR walks and the entries taken
              // out, each as (low, high) ints; empty unless the analysis found wide rows
      if (!P.wr_rows.empty()) {
        out.push_back(P.rows_vec() ? 1 : 0), out.push_back((int)P.wr_rows.size());
        for (long long c : {P.c_kept, P.c_cut}) out.push_back((int)(unsigned)(c & 0xffffffffLL)), out.push_back((int)(c >> 32));
      }
      break;
    case 38:  // the work lists upload made for the cut products, 5 ints each: tiles, k-slabs, form (stg::GemmFormKind), list
              // (stg::SK_LIST_*), launches that looked it up since
              // (the cut forms' entries of StagedDev::gemms in the order they were made, requests with the same list as one; a
              // launch with the control-row segment: form + 100; the profile form's lists are not reported)
      for (const GemmCache::Entry &t : h->sd->gemms.entries) {
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

extern "C" {

int hqpkkt_set_dynamics_form(hqpkkt_t *h, int form) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (form != HQPKKT_DYN_DENSE && form != HQPKKT_DYN_SPARSE && form != HQPKKT_DYN_PROFILE) return HQPKKT_E_RANGE;
    if (!h->sd) h->sd.reset(new StagedDev);
    h->sd->plan.want_sparse = form == HQPKKT_DYN_SPARSE;  // (the next hqpkkt_analyze picks it up)
    h->sd->plan.want_profile = form == HQPKKT_DYN_PROFILE;
    return 0;
  });
}

int hqpkkt_set_dense_columns(hqpkkt_t *h, int min_entries) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (min_entries < -1) return HQPKKT_E_RANGE;
    if (!h->sd) h->sd.reset(new StagedDev);
    h->sd->plan.want_heavy = min_entries;  // (the next hqpkkt_analyze picks it up; read by the sparse form alone)
    return 0;
  });
}

int hqpkkt_set_dense_rows(hqpkkt_t *h, int min_entries) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    // (-1, the library's threshold: none has been measured yet)
    if (min_entries < -1 || (min_entries == -1 && kktdev::StagedPlan::ROWS_DEFAULT <= 0)) return HQPKKT_E_RANGE;
    if (!h->sd) h->sd.reset(new StagedDev);
    h->sd->plan.want_rows = min_entries;  // (the next analysis picks it up; a sharded handle keeps its term lists)
    return 0;
  });
}

int hqpkkt_set_hessian_form(hqpkkt_t *h, int form) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (form != HQPKKT_HESS_CSR && form != HQPKKT_HESS_DENSE) return HQPKKT_E_RANGE;
    if (!h->sd) h->sd.reset(new StagedDev);
    h->sd->plan.want_hess_dense = form == HQPKKT_HESS_DENSE;  // (the next analysis picks it up)
    return 0;
  });
}

int hqpkkt_set_packed_hessians(hqpkkt_t *h, int on) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (on != 0 && on != 1) return HQPKKT_E_RANGE;
    if (!h->sd) h->sd.reset(new StagedDev);
    h->sd->plan.want_hess_packed = on != 0;  // (the next analysis picks it up; read with HQPKKT_HESS_DENSE alone)
    return 0;
  });
}

int hqpkkt_set_packed_panels(hqpkkt_t *h, int on) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (on != 0 && on != 1) return HQPKKT_E_RANGE;
    if (!h->sd) h->sd.reset(new StagedDev);
    h->sd->plan.want_packed = on != 0;  // (the next hqpkkt_analyze picks it up; read by the profile form alone)
    return 0;
  });
}

int hqpkkt_set_stages(hqpkkt_t *h, int K, const int *nx, const int *nu) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (!h->sd) h->sd.reset(new StagedDev);
    kktdev::StagedPlan &P = h->sd->plan;
    P.given_nx.clear(), P.given_nu.clear();
    if (K <= 0) return 0;  // back to detection from the staircase of A
    if (!nx || !nu) return HQPKKT_E_NULL;
    for (int k = 0; k <= K; k++)
      if (nx[k] < 1) return HQPKKT_E_RANGE;
    for (int k = 0; k < K; k++)
      if (nu[k] < 0) return HQPKKT_E_RANGE;
    P.given_nx.assign(nx, nx + K + 1), P.given_nu.assign(nu, nu + K);
    return 0;
  });
}

int hqpkkt_analyze_staged(hqpkkt_t *h, int K, const int *nx, const int *nu, int n_total, int me_rest, int m, const int *Qp,
                          const int *Qi, const int *Ep, const int *Ei, const int *Cp, const int *Ci) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (h->opts.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_INTERN;
    if (h->sd && (h->sd->plan.want_sparse || h->sd->plan.want_profile)) return HQPKKT_E_INTERN;  // (HQPKKT_DYN_SPARSE, _PROFILE: the CSR hand-over alone)
    int e = hqpkkt_set_stages(h, K, nx, nu);
    if (e) return e;
    if (K < 1) return HQPKKT_E_RANGE;
    long long n = nx[K], ndyn = 0;
    for (int k = 0; k < K; k++) n += (long long)nx[k] + nu[k], ndyn += nx[k + 1];
    if (n > 0x7fffffffLL || ndyn + me_rest > 0x7fffffffLL || me_rest < 0 || m < 0) return HQPKKT_E_RANGE;
    if (n != n_total) return HQPKKT_E_SIZES;  // Q, E, C were built for another number of variables
    const bool hess_dense = h->sd && h->sd->plan.want_hess_dense;  // (the blocks come through hqpkkt_set_stage_hessian: Qp / Qi are not read)
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
      const std::vector<char> &qs = h->sd->hess_set;
      if ((int)qs.size() != h->sd->plan.K + 1 || std::find(qs.begin(), qs.end(), 0) != qs.end()) return HQPKKT_E_INTERN;
    }
    return staged_set_values(h, Qx, Ex, Cx, F, ldF, true);
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
    if (!h->analyzed || h->opts.mode != HQPKKT_MODE_STAGED || !h->sd || !h->sd->plan.dense_dyn) return HQPKKT_E_INTERN;
    int e = ensure_device(h);
    if (e) return e;
    StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    long long mx = 1;
    for (int k = 0; k < P.K; k++) mx = std::max(mx, (long long)P.nk[k + 1] * (P.nk[k] + P.mk[k]));
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
    if (!h->analyzed || h->opts.mode != HQPKKT_MODE_STAGED || !h->sd || !h->sd->plan.dense_dyn) return HQPKKT_E_INTERN;
    int e;
    if (!h->uploaded && (e = staged_upload(h))) return e;
    StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    if (k < 0 || k >= P.K) return HQPKKT_E_RANGE;
    const int nz = P.nk[k] + P.mk[k];
    if (ldF < nz) return HQPKKT_E_SIZES;
    HIPCHK(hipSetDevice(h->opts.device));
    const hipMemcpyKind kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if ((e = staged_copy_block(h, k, F, ldF, kind))) return e;
    for (int b = 0; b < 2; b++)
      if (F == d.hblk[b].p) {  // the library's own staging buffer: remember when it is free again
        if (!d.hblk_ev[b]) HIPCHK(hipEventCreateWithFlags(&d.hblk_ev[b].h, hipEventDisableTiming));
        HIPCHK(hipEventRecord(d.hblk_ev[b], h->stream));
      }
    if ((int)d.blocks_set.size() != P.K) d.blocks_set.assign(P.K, 0);
    d.blocks_set[k] = 1;
    h->factored = false;
    return 0;
  });
}

int hqpkkt_set_stage_hessian(hqpkkt_t *h, int k, const double *Q, long long ldQ) {
  return guarded([&]() -> int {
    if (!h || !Q) return HQPKKT_E_NULL;
    if (!h->analyzed || h->opts.mode != HQPKKT_MODE_STAGED || !h->sd || !h->sd->plan.dense_dyn || !h->sd->plan.hess_dense) return HQPKKT_E_INTERN;
    int e;
    if (!h->uploaded && (e = staged_upload(h))) return e;
    StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    if (k < 0 || k > P.K) return HQPKKT_E_RANGE;
    const int nz = P.hess_order(k);
    if (ldQ < nz) return HQPKKT_E_SIZES;
    HIPCHK(hipSetDevice(h->opts.device));
    const hipMemcpyKind kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (nz > 0 && P.stage_packed(k)) {
      // packed lower tiles: k_hp_pack reads a device block where it lies; of a host block the rows come in groups of
      // HESS_COPY_ROWS, every group from its first column on, into the staging block (reused in stream order)
      const double *src = Q;
      long long lds = ldQ;
      if (kind == hipMemcpyHostToDevice) {
        if (d.hess_stage.count < (size_t)P.q_stage_elems && (e = d.hess_stage.alloc((size_t)P.q_stage_elems))) return e;
        lds = P.ldQ[k], src = d.hess_stage.p;
        for (int r = 0; r < nz; r += P.HESS_COPY_ROWS)
          HIPCHK(hipMemcpy2DAsync(d.hess_stage.p + (long long)r * lds + r, sizeof(double) * lds, Q + (long long)r * ldQ + r, sizeof(double) * ldQ,
                                  sizeof(double) * (nz - r), std::min(P.HESS_COPY_ROWS, nz - r), kind, h->stream));
      }
      stg::k_hp_pack<<<dim3((unsigned)P.hess_tiles(nz), 16), 256, 0, h->stream>>>(src, lds, nz, d.Qd.p + P.oQ[k]);
    } else if (nz > 0) {  // the caller's nz columns of every row, then the strict lower triangle from the upper one
      double *dst = d.Qd.p + P.oQ[k];
      HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * P.ldQ[k], Q, sizeof(double) * ldQ, sizeof(double) * nz, nz, kind, h->stream));
      const unsigned T = (unsigned)((nz + stg::HS_TILE - 1) / stg::HS_TILE);
      stg::k_hs_mirror<<<T * (T + 1) / 2, 256, 0, h->stream>>>(dst, P.ldQ[k], nz, (int)T);
    }
    for (int b = 0; b < 2; b++)
      if (Q == d.hblk[b].p) {  // the library's own staging buffer: remember when it is free again
        if (!d.hblk_ev[b]) HIPCHK(hipEventCreateWithFlags(&d.hblk_ev[b].h, hipEventDisableTiming));
        HIPCHK(hipEventRecord(d.hblk_ev[b], h->stream));
      }
    if ((int)d.hess_set.size() != P.K + 1) d.hess_set.assign(P.K + 1, 0);
    d.hess_set[k] = 1;
    h->factored = false;
    return 0;
  });
}

int hqpkkt_debug_stage_hessian(hqpkkt_t *h, int k, double *out, long long cap, long long *len) {
  return guarded([&]() -> int {
    if (!h || !len) return HQPKKT_E_NULL;
    if (!h->sd || !h->uploaded || !h->sd->plan.hess_dense) return HQPKKT_E_INTERN;
    const kktdev::StagedPlan &P = h->sd->plan;
    if (k < 0 || k > P.K) return HQPKKT_E_RANGE;
    const long long elems = (long long)P.hess_order(k) * P.ldQ[k];
    *len = elems;
    if (!out) return 0;
    if (cap < elems) return HQPKKT_E_SIZES;
    HIPCHK(hipSetDevice(h->opts.device));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (elems && P.stage_packed(k)) {  // the unpacked view: entry (i, j) out of its stored tile, zero padding
      const int T = P.HESS_T, nz = P.hess_order(k);
      std::vector<double> t((size_t)P.hess_tiles(nz) * T * T);
      HIPCHK(hipMemcpy(t.data(), h->sd->Qd.p + P.oQ[k], sizeof(double) * t.size(), hipMemcpyDeviceToHost));
      std::fill(out, out + elems, 0.0);
      for (int i = 0; i < nz; i++)
        for (int j = 0; j < nz; j++) {
          const int a = std::max(i, j) / T, b = std::min(i, j) / T;
          const size_t tile = ((size_t)a * (a + 1) / 2 + b) * T * T;
          out[(long long)i * P.ldQ[k] + j] = i / T >= j / T ? t[tile + (size_t)(i % T) * T + j % T] : t[tile + (size_t)(j % T) * T + i % T];
        }
      return 0;
    }
    if (elems) HIPCHK(hipMemcpy(out, h->sd->Qd.p + P.oQ[k], sizeof(double) * elems, hipMemcpyDeviceToHost));
    return 0;
  });
}

int hqpkkt_debug_hess_symv(hqpkkt_t *h, const double *x, double *y) {
  return guarded([&]() -> int {
    if (!h || !x || !y) return HQPKKT_E_NULL;
    if (!h->sd || !h->uploaded || !h->sd->plan.hess_dense) return HQPKKT_E_INTERN;
    StagedDev &d = *h->sd;
    const size_t n = (size_t)d.plan.n;
    HIPCHK(hipSetDevice(h->opts.device));
    int e;
    if (!d.hess_x.p && (e = d.hess_x.alloc(n + 1))) return e;  // (the tests' operand: made here, outside every capture)
    // hess_y is the buffer the residual's launches read: everything here goes to the handle's stream, behind whatever
    // residual is still in it, and is over when this call returns
    HIPCHK(hipMemcpyAsync(d.hess_x.p, x, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    staged_hess_symv(h, d, d.hess_x.p, d.hess_y.p);
    HIPCHK(hipMemcpyAsync(y, d.hess_y.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int hqpkkt_debug_hess_symv_timed(hqpkkt_t *h, const double *x, double *y, int reps, double *ms) {
  return guarded([&]() -> int {
    if (!h || !x || !y || !ms) return HQPKKT_E_NULL;
    if (reps < 1) return HQPKKT_E_RANGE;
    if (!h->sd || !h->uploaded || !h->sd->plan.hess_dense) return HQPKKT_E_INTERN;
    StagedDev &d = *h->sd;
    const size_t n = (size_t)d.plan.n;
    HIPCHK(hipSetDevice(h->opts.device));
    int e;
    if (!d.hess_x.p && (e = d.hess_x.alloc(n + 1))) return e;
    EventOwner t0, t1;
    HIPCHK(hipEventCreate(&t0.h));
    HIPCHK(hipEventCreate(&t1.h));
    HIPCHK(hipMemcpyAsync(d.hess_x.p, x, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    staged_hess_symv(h, d, d.hess_x.p, d.hess_y.p);  // (one product ahead of the timed ones)
    HIPCHK(hipEventRecord(t0, h->stream));
    for (int r = 0; r < reps; r++) staged_hess_symv(h, d, d.hess_x.p, d.hess_y.p);
    HIPCHK(hipEventRecord(t1, h->stream));
    HIPCHK(hipMemcpyAsync(y, d.hess_y.p, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, t0, t1));
    *ms = (double)t / reps;
    return 0;
  });
}

int hqpkkt_hessian_product(hqpkkt_t *h, const double *x, double *y) {
  if (h && h->opts.loc != HQPKKT_LOC_DEVICE) return hqpkkt_debug_hess_symv(h, x, y);  // (host vectors: the hook's own path)
  return guarded([&]() -> int {
    if (!h || !x || !y) return HQPKKT_E_NULL;
    if (!h->sd || !h->uploaded || !h->sd->plan.hess_dense) return HQPKKT_E_INTERN;
    HIPCHK(hipSetDevice(h->opts.device));
    staged_hess_symv(h, *h->sd, x, y);  // (the same launches on the caller's vectors)
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int hqpkkt_update_stage_hessians(hqpkkt_t *h, const hqpkkt_hess_update *u) {
  return guarded([&]() -> int {
    if (!h || !u) return HQPKKT_E_NULL;
    static_assert(stg::HU_RANK == HQPKKT_HESS_UPDATE_RANK, "the kernel's descriptor holds the coefficients");
    const int r = u->r;
    if (r < 0 || r > HQPKKT_HESS_UPDATE_RANK) return HQPKKT_E_RANGE;
    if (r > 0 && (!u->U || !u->coef)) return HQPKKT_E_NULL;
    for (int j = 0; j < r; j++)
      if (!u->U[j]) return HQPKKT_E_NULL;
    if (!h->analyzed || h->opts.mode != HQPKKT_MODE_STAGED || !h->sd || !h->sd->plan.dense_dyn || !h->sd->plan.hess_dense) return HQPKKT_E_INTERN;
    StagedDev &d = *h->sd;
    const kktdev::StagedPlan &P = d.plan;
    const int K1 = P.K + 1;
    for (int k = 0; k < K1; k++) {
      if (u->beta && !std::isfinite(u->beta[k])) return HQPKKT_E_RANGE;
      for (int j = 0; j < r; j++)
        if (!std::isfinite(u->coef[(size_t)k * r + j])) return HQPKKT_E_RANGE;
    }
    // the launch's descriptors; a stage with beta = 1, every coefficient 0 and no diagonal is left alone (units = 0)
    std::vector<stg::HuDesc> hd(K1);
    int units_max = 0;
    for (int k = 0; k < K1; k++) {
      const double beta = u->beta ? u->beta[k] : 1.0;
      const int nz = P.hess_order(k), nt = (nz + stg::HP_T - 1) / stg::HP_T;
      const bool packed = P.stage_packed(k);
      stg::HuDesc &q = hd[k];
      q = stg::HuDesc{P.oQ[k], P.ldQ[k], nt, nz, P.nmk[k], packed ? 1 : 0, 0, beta == 0.0 ? 0 : beta == 1.0 ? 1 : 2, 0, beta, {0.0, 0.0, 0.0, 0.0}};
      bool touched = beta != 1.0 || u->diag;
      for (int j = 0; j < r; j++) q.c[j] = u->coef[(size_t)k * r + j], touched = touched || q.c[j] != 0.0;
      if (!touched || nz == 0) continue;
      // (the hand-over rule: what is kept of a block must have arrived since the analysis)
      if (beta != 0.0 && ((int)d.hess_set.size() != K1 || !d.hess_set[k])) return HQPKKT_E_INTERN;
      q.units = packed ? (int)P.hess_tiles(nz) : nt * nt;
      units_max = std::max(units_max, q.units);
    }
    int e;
    if (!h->uploaded && (e = staged_upload(h))) return e;
    HIPCHK(hipSetDevice(h->opts.device));
    if (units_max > 0) {
      const size_t n = (size_t)P.n;
      stg::HuVecs V{};
      V.r = r;
      if (h->opts.loc == HQPKKT_LOC_DEVICE) {
        for (int j = 0; j < r; j++) V.u[j] = u->U[j];
        V.diag = u->diag;
      } else {  // a host caller's vectors through the handle's own buffer
        if (!d.hu_vec.p && (e = d.hu_vec.alloc((size_t)(stg::HU_RANK + 1) * n + 1))) return e;
        for (int j = 0; j < r; j++) {
          HIPCHK(hipMemcpyAsync(d.hu_vec.p + j * n, u->U[j], sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
          V.u[j] = d.hu_vec.p + j * n;
        }
        if (u->diag) {
          HIPCHK(hipMemcpyAsync(d.hu_vec.p + stg::HU_RANK * n, u->diag, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
          V.diag = d.hu_vec.p + stg::HU_RANK * n;
        }
      }
      if (!d.hu_desc.p) {
        if ((e = d.hu_desc.alloc((size_t)K1))) return e;
        HIPCHK(d.hu_hdesc.alloc((size_t)K1, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&d.hu_ev.h, hipEventDisableTiming));
      } else
        HIPCHK(hipEventSynchronize(d.hu_ev));  // (the copy of the last call's descriptors out of the pinned words)
      std::copy(hd.begin(), hd.end(), d.hu_hdesc.p);
      HIPCHK(hipMemcpyAsync(d.hu_desc.p, d.hu_hdesc.p, sizeof(stg::HuDesc) * K1, hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipEventRecord(d.hu_ev, h->stream));
      KLAUNCH(h, KC_ASSEMBLE, stg::k_hu_update<<<dim3((unsigned)units_max, (unsigned)K1), 256, 0, h->stream>>>(d.hu_desc.p, d.Qd.p, V));
      HIPCHK(hipGetLastError());
      if (h->opts.loc != HQPKKT_LOC_DEVICE) HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's vectors are free again)
    }
    if ((int)d.hess_set.size() != K1) d.hess_set.assign(K1, 0);
    for (int k = 0; k < K1; k++)
      if (hd[k].mode == 0) d.hess_set[k] = 1;  // (beta = 0: the block has been made here)
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
    HIPCHK(hipMemcpy(out + 2 * k, h->sd->dyn.p + P.dyn_off[k], 2 * sizeof(int), hipMemcpyDeviceToHost));
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

// Micro-benchmark and self-check of the dense fp64 product the STAGED engine is made of
// (k_dgemm_tn): C = A'B (+ lower / mirror) on pseudo-random operands, `reps` timed launches;
// *ms = average device time per launch, *max_err = max |C - exact| over 4096 sampled entries
// relative to sum |a||b|.  Used by tests/ and bench.py (roofline of the kernel on its own).
namespace {
__global__ void k_fill_rand(double *p, long long n, unsigned long long seed) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long x = (unsigned long long)i * 0x9E3779B97F4A7C15ULL + seed;
  x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ULL, x ^= x >> 27, x *= 0x94D049BB133111EBULL, x ^= x >> 31;
  p[i] = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}
__global__ void k_gemm_check(stg::GemmArgs g, int nsample, double *err) {
  const int sidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (sidx >= nsample) return;
  unsigned long long x = (unsigned long long)sidx * 0x9E3779B97F4A7C15ULL + 12345;
  x ^= x >> 29, x *= 0xBF58476D1CE4E5B9ULL, x ^= x >> 32;
  int i = (int)(x % (unsigned long long)g.M), j = (int)((x >> 20) % (unsigned long long)g.N);
  // lower: only i >= j is computed; mirror: C[j][i] is a copy of C[i][j] (the product is
  // symmetric in the engine; here the operands are not, so the copy is what gets checked)
  int ci = i, cj = j;
  if (g.lower && i < j) {
    const int t = i;
    i = j, j = t;
    if (!g.mirror) ci = i, cj = j;
  }
  double s = 0.0, sa = 0.0;
  for (int k = 0; k < g.K; k++) {
    const double a = g.A[(long long)k * g.lda + i], b = g.B[(long long)k * g.ldb + j];
    s += a * b, sa += fabs(a * b);
  }
  for (int k = 0; k < g.K2; k++) {  // (the second k segment)
    const double a = g.A2[(long long)k * g.lda2 + i], b = g.B2[(long long)k * g.ldb2 + j];
    s += a * b, sa += fabs(a * b);
  }
  const double e = fabs(g.C[(long long)ci * g.ldc + cj] - g.alpha * s) / (sa + 1e-300);
  atomic_max_pos((unsigned long long *)err, e);
}
__global__ void k_negate_into(long long n, const double *__restrict__ x, double *__restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = -x[i];
}
// entries of a mirrored result that differ in a bit from their image
__global__ void k_gemm_count_asym(stg::GemmArgs g, unsigned long long *count) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)g.M * g.N) return;
  const int i = (int)(e / g.N), j = (int)(e % g.N);
  if (i <= j || i >= g.N) return;
  if (__double_as_longlong(g.C[(long long)i * g.ldc + j]) != __double_as_longlong(g.C[(long long)j * g.ldc + i])) atomicAdd(count, 1ULL);
}
// HQPKKT_DGEMM_STAMPS: one more launch of the product with time stamps (100 MHz constant clock), printed to stderr
static void dgemm_stamps_split(const stg::GemmArgs &g, const stg::GemmForm &f, int variant, int skg, int list, const stg::SplitTable &sk_tab, const stg::SkUnit *tab_dev) {
  // the split form with time stamps: per workgroup its start and, per unit, the end of the k loop, of the
  // parking / summing of partial tiles and of the epilogue (us after the first start)
  DBuf<unsigned long long> st;
  DBuf<double> ws2;
  DBuf<unsigned> cnt2;
  if (st.alloc(32 * (size_t)skg) || ws2.alloc((size_t)std::max<long long>(sk_tab.pieces, 1) * 128 * 128) || cnt2.alloc(f.tiles + 4)) return;
  (void)hipMemset(st.p, 0, sizeof(unsigned long long) * 32 * skg);
  (void)hipMemset(cnt2.p, 0, sizeof(unsigned) * (f.tiles + 4));
  stg::GemmArgs gs = g;
  gs.stamps = st.p;
  stg::gemm_launch_split(variant, skg, 0, gs, stg::SplitPlan{ws2.p, cnt2.p, tab_dev, sk_tab.stride});
  std::vector<unsigned long long> hs(32 * (size_t)skg);
  if (hipMemcpy(hs.data(), st.p, sizeof(unsigned long long) * 32 * skg, hipMemcpyDeviceToHost) != hipSuccess) return;
  unsigned long long tmin = ~0ULL;
  for (int w = 0; w < skg; w++) tmin = std::min(tmin, hs[32 * (size_t)w]);
  fprintf(stderr, "%s shares: %lld parked pieces", list == stg::SK_LIST_UNEQUAL ? "unequal" : "equal", sk_tab.pieces);
  if (list == stg::SK_LIST_UNEQUAL) fprintf(stderr, ", %d / %d whole tiles per first / second workgroup of a CU", sk_tab.nA, sk_tab.nB);
  fprintf(stderr, "; stamps of every %dth workgroup (us): start | per unit: k loop end, parked / summed, epilogue end\n", std::max(1, skg / 32));
  const int nr = std::min(10, sk_tab.stride - 1);
  for (int w = 0; w < skg; w += std::max(1, skg / 32)) {
    fprintf(stderr, "  wg %4d: %7.2f |", w, (hs[32 * (size_t)w] - tmin) * 0.01);
    for (int r = 0; r < nr; r++) {
      for (int c = 1; c <= 3; c++) {
        const unsigned long long x = hs[32 * (size_t)w + 3 * r + c];
        if (x) fprintf(stderr, " %8.2f", (x - tmin) * 0.01); else fprintf(stderr, "        -");
      }
      fprintf(stderr, " |");
    }
    fprintf(stderr, "\n");
  }
  // the end of every workgroup's last unit, per class (first / second half of the launch)
  for (int c = 0; c < 2; c++) {
    double lo = 1e30, hi = 0.0, sum = 0.0;
    int n = 0;
    for (int w = c * skg / 2; w < (c + 1) * skg / 2; w++) {
      unsigned long long last = 0;
      for (int r = 0; r < 10; r++) last = std::max(last, hs[32 * (size_t)w + 3 * r + 3]);
      if (!last) continue;
      const double e = (last - tmin) * 0.01;
      lo = std::min(lo, e), hi = std::max(hi, e), sum += e, n++;
    }
    if (n) fprintf(stderr, "  class %c (blockIdx %s grid / 2): last epilogue ends at %.1f ... %.1f us, mean %.1f\n", c ? 'B' : 'A', c ? ">=" : "<", lo, hi, sum / n);
  }
}
static void dgemm_stamps_plain(const stg::GemmArgs &g, long long tiles, int variant) {
  // one more launch with time stamps per workgroup (100 MHz constant clock): when it started, when its k loop
  // ended, when its epilogue ended - relative to the first start; printed as a histogram over the workgroups
  DBuf<unsigned long long> st;
  if (st.alloc(4 * (size_t)tiles)) return;
  stg::GemmArgs gs = g;
  gs.stamps = st.p;
  stg::gemm_launch_plain(variant, (unsigned)tiles, 0, gs);
  std::vector<unsigned long long> hs(4 * tiles);
  if (hipMemcpy(hs.data(), st.p, sizeof(unsigned long long) * 4 * tiles, hipMemcpyDeviceToHost) != hipSuccess) return;
  unsigned long long tmin = ~0ULL;
  for (long long t = 0; t < tiles; t++) tmin = std::min(tmin, hs[4 * t]);
  // workgroups in the order of their start
  std::vector<long long> ord(tiles);
  for (long long t = 0; t < tiles; t++) ord[t] = t;
  std::sort(ord.begin(), ord.end(), [&](long long a, long long b) { return hs[4 * a] < hs[4 * b]; });
  fprintf(stderr, "stamps (us after the first start; %lld workgroups, every %lldth in start order): start, k loop end, epilogue end, xcc, blockIdx\n", tiles,
          std::max<long long>(1, tiles / 64));
  for (long long q = 0; q < tiles; q += std::max<long long>(1, tiles / 64)) {
    const long long t = ord[q];
    fprintf(stderr, "  %8.2f %8.2f %8.2f  xcc %llu  wg %lld\n", (hs[4 * t] - tmin) * 0.01, (hs[4 * t + 2] - tmin) * 0.01, (hs[4 * t + 3] - tmin) * 0.01,
            hs[4 * t + 1], t);
  }
}
}  // namespace
// One launch of the product outside a handle, for the hooks hqpkkt_debug_dgemm*: the engine's schedule
// (stg::gemm_schedule through a GemmCache of its own) and the engine's launch (stg::gemm_run) with a workspace, arrival
// counters and a zero row of its own.  The schedule sees the capacity the self-test has always stated - counters for
// the tiles of this product, 16 parked pieces per tile - and the buffers hold what the chosen list and form need.
struct DebugGemm {
  DBuf<double> zr, ws, thin_ws;
  DBuf<unsigned> cnt, ctl;
  stg::GemmCaps caps;
  GemmCache cache;
  GemmCache::Entry local, *e = nullptr;
  stg::GemmArgs thin{};
  int thin_split = 1;
  // makes what the launch of g looks up; flags: stg::GEMM_SHARDED, GEMM_NO_KS, GEMM_NO_TILE_MAP, GEMM_FORCE_SPLIT
  // krange / krange_by: the profile form (hqpkkt_dgemm_case): two ints per 128-wide panel of B (1) or A (2)
  // g.Au / mu / Cu set: the control-row segment is asked for, on `grid` workgroups (0: the device's); taken() says
  // whether the launch takes it, as the engine would.  The product Cu = Au'B cut in k runs behind it, guarded, as in the
  // engine's fused stage; not taken: that product alone forms Cu
  int prepare(int device, stg::GemmArgs &g, int flags, const int *krange = nullptr, int krange_by = 0, int grid = 0) {
    const long long t128 = stg::gemm_tiles(g.M, g.N, 128, g.lower), nslab = stg::gemm_slabs_of(g);
    caps.variant = stg::gemm_variant_from_env();
    (void)hipDeviceGetAttribute(&caps.cus, hipDeviceAttributeMultiprocessorCount, device);
    caps.grid = grid > 0 ? grid : stg::gemm_wgs_per_cu(caps.variant) * caps.cus;
    caps.sk_tiles = t128, caps.cnt_elems = t128 + 5;
    caps.ws_elems = std::max<long long>(16 * t128 + 8, 2LL * caps.grid + 2) * 128 * 128;
    caps.unequal = stg::gemm_sk_table_from_env() && !(flags & stg::GEMM_SHARDED), caps.flags = flags;
    if (krange_by) {
      const int npanel = ((krange_by == 2 ? g.M : g.N) + 127) / 128;
      if (!krange || (krange_by != 1 && krange_by != 2)) return HQPKKT_E_RANGE;
      for (int p = 0; p < npanel; p++)
        if (krange[2 * p] < 0 || krange[2 * p + 1] < krange[2 * p] || krange[2 * p + 1] > nslab) return HQPKKT_E_RANGE;
    }
    if (g.Au) {
      if (ctl.alloc(8)) return HQPKKT_E_MEM;
      (void)hipMemset(ctl.p, 0, sizeof(unsigned) * 8);
      g.ctl = ctl.p;
      thin = stg::GemmArgs{g.Au, g.ldau, g.B, g.ldb, nullptr, 0, g.Cu, g.ldcu, g.mu, g.N, g.K, g.alpha, 0.0, 0, 0};
      thin_split = (int)std::max<long long>(1, std::min<long long>(8, stg::gemm_slabs(g.K) / 4));
      if (thin_ws.alloc((size_t)thin_split * g.mu * g.N)) return HQPKKT_E_MEM;
    }
    const stg::PackPanel *apack = g.apack, *bpack = g.bpack;
    g.apack = g.bpack = nullptr;  // (the request is that of the operands as blocks, as the engine's)
    const stg::GemmRequest rq = stg::gemm_request(g, false, 0, krange_by, krange);
    g.apack = apack, g.bpack = bpack;
    if (int err = cache.get(caps, rq, true, local, e)) return err == HQPKKT_E_MEM ? err : HQPKKT_E_RANGE;
    (void)stg::gemm_set_attributes();
    const stg::GemmSchedule &s = e->s;
    if (s.variant != stg::GEMM_REG4) {
      if (zr.alloc(256)) return HQPKKT_E_MEM;
      (void)hipMemset(zr.p, 0, sizeof(double) * 256);
    }
    const long long ws_elems = s.f.kind == stg::GEMM_FORM_KS ? stg::gemm_ks_ws_elems(g, s.f) : std::max<long long>(s.tab.pieces, 1) * 128 * 128;
    if (ws.alloc((size_t)ws_elems) || cnt.alloc((size_t)caps.cnt_elems)) return HQPKKT_E_MEM;
    if (s.seg) thin.guard = ctl.p + 2;
    return 0;
  }
  bool taken() const { return e->s.seg; }
  void launch(const stg::GemmArgs &g) {
    // (its own counters: cleared ahead of every launch)
    if (e->s.list != stg::SK_LIST_NONE) (void)hipMemsetAsync(cnt.p, 0, sizeof(unsigned) * (size_t)caps.cnt_elems, 0);
    stg::gemm_run(e->s, caps, stg::GemmBufs{e->units.p, e->order.p, ws.p, cnt.p, ws.p, zr.p}, 0, g, [](auto &&kernel) { kernel(); });
    if (thin.M > 0) {
      // The control rows as the engine's fused stage forms them: guarded behind a launch with the segment.  A direct launch:
      // the rule does not give the hooks' small shapes the form cut in k (GEMM_FORM_KS), and only that form knows the guard
      stg::k_dgemm_tn_ks<64, 64><<<dim3((unsigned)stg::gemm_tiles(thin.M, thin.N, 64, 0), thin_split), 256, stg::gemm_lds_bytes(64, 64), 0>>>(thin, thin_ws.p, thin_split);
      stg::k_dgemm_ks_finish<<<(unsigned)(((long long)thin.M * thin.N + 255) / 256), 256, 0, 0>>>(thin, thin_ws.p, thin_split);
      if (thin.guard) stg::k_ctrl_rows_end<<<1, 64, 0, 0>>>(ctl.p);
    }
  }
  int fallbacks() {
    unsigned w[3] = {0, 0, 0};
    if (hipMemcpy(w, ctl.p, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)(w[1] + (w[2] ? 1 : 0));
  }
};
// K2 > 0: C = A'B - A2'B2 by a launch with a second k segment (operands A2, -B2); asym: entries of a mirrored result
// that are not bit-identical to their image
static int debug_dgemm(int device, int M, int N, int K, int K2, int lower, int mirror, int reps, double *ms, double *max_err, long long *asym) {
  if (M <= 0 || N <= 0 || K < 0 || K2 < 0 || reps <= 0) return HQPKKT_E_RANGE;
  if (lower && M < N) return HQPKKT_E_RANGE;  // (M > N: the column strip of a lower triangle)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  const long long lda = (M + 7) / 8 * 8, ldb = (N + 7) / 8 * 8, ldc = ldb;
  DBuf<double> A, B, Cm, err, A2, B2, nB2;
  DBuf<unsigned long long> nasym;
  const size_t kk = K > 0 ? K : 1;
  if (A.alloc(kk * lda) || B.alloc(kk * ldb) || Cm.alloc((size_t)std::max(M, N) * ldc) || err.alloc(1)) return HQPKKT_E_MEM;
  k_fill_rand<<<nblk((long long)kk * lda), 256>>>(A.p, (long long)kk * lda, 1);
  k_fill_rand<<<nblk((long long)kk * ldb), 256>>>(B.p, (long long)kk * ldb, 2);
  (void)hipMemset(err.p, 0, 8);
  (void)hipMemset(Cm.p, 0, sizeof(double) * (size_t)std::max(M, N) * ldc);
  stg::GemmArgs g{A.p, lda, B.p, ldb, nullptr, 0, Cm.p, ldc, M, N, K, 1.0, 0.0, lower, mirror, nullptr, nullptr};
  if (K2 > 0) {
    if (A2.alloc((size_t)K2 * lda) || B2.alloc((size_t)K2 * ldb) || nB2.alloc((size_t)K2 * ldb)) return HQPKKT_E_MEM;
    k_fill_rand<<<nblk((long long)K2 * lda), 256>>>(A2.p, (long long)K2 * lda, 3);
    k_fill_rand<<<nblk((long long)K2 * ldb), 256>>>(B2.p, (long long)K2 * ldb, 4);
    k_negate_into<<<nblk((long long)K2 * ldb), 256>>>((long long)K2 * ldb, B2.p, nB2.p);
    g.A2 = A2.p, g.lda2 = lda, g.B2 = nB2.p, g.ldb2 = ldb, g.K2 = K2;  // (the check sums what the launch was given: A'B + A2'(-B2))
  }
  // The engine's rule (gemm_form.hpp) with what this entry point has always done differently: no thin product cut in k, no
  // tile order for large triangles, never sharded, and a workspace of its own
  // (HQPKKT_DGEMM_FORCE_SPLIT: the cut form whatever the launch rules say - same-box comparisons of the two forms)
  // (HQPKKT_DGEMM_CTRL_ROWS=mu, M == K: the launch with the control-row segment for the last mu columns of C and the
  // guarded product behind it, as a fused stage runs W - same-box comparisons with the plain launch)
  DBuf<double> Cu;
  const int mu = getenv("HQPKKT_DGEMM_CTRL_ROWS") ? atoi(getenv("HQPKKT_DGEMM_CTRL_ROWS")) : 0;
  const bool seg = mu > 0 && mu <= N && M == K && K2 == 0 && !lower;
  if (seg) {
    if (Cu.alloc((size_t)mu * ldc)) return HQPKKT_E_MEM;
    g.Au = Cm.p + (N - mu), g.ldau = ldc, g.mu = mu, g.Cu = Cu.p, g.ldcu = ldc;
  }
  DebugGemm run;
  if (int e = run.prepare(device, g, stg::GEMM_NO_KS | stg::GEMM_NO_TILE_MAP | (getenv("HQPKKT_DGEMM_FORCE_SPLIT") ? stg::GEMM_FORCE_SPLIT : 0))) return e;
  if (seg) fprintf(stderr, "control-row segment: %s\n", run.taken() ? "taken" : "not taken (the thin product alone)");
  EventOwner e0, e1;
  (void)hipEventCreate(&e0.h), (void)hipEventCreate(&e1.h);
  for (int r = -1; r < reps; r++) {
    if (r == 0) (void)hipEventRecord(e0, 0);
    run.launch(g);
  }
  (void)hipEventRecord(e1, 0);
  hipError_t se = hipDeviceSynchronize();
  if (mu > 0 && run.ctl.p) fprintf(stderr, "control-row segment: %d of %d launches fell back\n", run.fallbacks(), reps + 1);
  run.ws.release(), run.cnt.release();
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (se != hipSuccess) return HQPKKT_E_DEVICE;
  if (getenv("HQPKKT_DGEMM_STAMPS")) {
    const stg::GemmSchedule &sc = run.e->s;
    const stg::GemmArgs gc = stg::gemm_complete(sc, stg::GemmBufs{nullptr, run.e->order.p, nullptr, nullptr, nullptr, run.zr.p}, g);
    if (sc.f.kind == stg::GEMM_FORM_CUT) dgemm_stamps_split(gc, sc.f, sc.variant, run.caps.grid, sc.list, sc.tab, run.e->units.p);
    if (sc.f.kind == stg::GEMM_FORM_PLAIN) dgemm_stamps_plain(gc, sc.f.tiles, sc.variant);
  }
  k_gemm_check<<<16, 256>>>(g, 4096, err.p);
  double he = 0.0;
  if (hipMemcpy(&he, err.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return HQPKKT_E_DEVICE;
  if (asym) {
    unsigned long long na = 0;
    if (nasym.alloc(1)) return HQPKKT_E_MEM;
    (void)hipMemset(nasym.p, 0, 8);
    if (lower && mirror) k_gemm_count_asym<<<nblk((long long)M * N), 256>>>(g, nasym.p);
    if (hipMemcpy(&na, nasym.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return HQPKKT_E_DEVICE;
    *asym = (long long)na;
  }
  if (ms) *ms = t / reps;
  if (max_err) *max_err = he;
  return 0;
}
// The packed panels a test hook was given (include/hqpkkt.h, hqpkkt_debug_dgemm_packed): `panel` holds (offset, ld) per
// 128-column panel of a K x W operand, `ranges` its (lo, hi) k-slabs.  Every panel's rows must lie inside the buffer of
// `elems` doubles, on 16-byte boundaries.  Out: the kernels' table (offsets less 16 lo ld)
static int debug_pack_table(int K, int W, const long long *panel, const int *ranges, long long elems, std::vector<stg::PackPanel> &tab) {
  const int np = (W + 127) / 128;
  tab.resize(np);
  for (int p = 0; p < np; p++) {
    const long long off = panel[2 * p], ld = panel[2 * p + 1];
    const int lo = ranges[2 * p], hi = ranges[2 * p + 1];
    if (lo < 0 || hi < lo || hi > (K + 15) / 16) return HQPKKT_E_RANGE;
    const long long rows = std::min(16 * hi, K) - 16 * lo;
    if (ld < std::min(128, W - 128 * p) || (ld & 7) || off < 0 || (off & 1) || off + rows * ld > elems) return HQPKKT_E_RANGE;
    tab[p] = stg::PackPanel{off - 16LL * lo * ld, ld};
  }
  return 0;
}
// One product on the caller's operands, all of C back (include/hqpkkt.h): launches and copies, compares nothing
// pk: the ranged operand (c->krange_by) comes from this buffer of packed panels instead (hqpkkt_debug_dgemm_packed)
static int debug_dgemm_full(int device, hqpkkt_dgemm_case *c, const double *pk = nullptr, long long pk_elems = 0, const long long *pk_panel = nullptr) {
  if (!c || !c->C) return HQPKKT_E_NULL;
  if (pk && (!pk_panel || !c->krange || (c->krange_by != 1 && c->krange_by != 2) || c->K2 > 0 || c->K <= 0 || pk_elems <= 0)) return HQPKKT_E_RANGE;
  const bool pkA = pk && c->krange_by == 2, pkB = pk && c->krange_by == 1;
  const int M = c->M, N = c->N, K = c->K, K2 = c->K2;
  if (M <= 0 || N <= 0 || K < 0 || K2 < 0) return HQPKKT_E_RANGE;
  if ((c->lower && M < N) || (c->mirror && !c->lower)) return HQPKKT_E_RANGE;  // (the image of a triangle, or of the column strip of one)
  if (c->flags & ~(stg::GEMM_SHARDED | stg::GEMM_NO_KS | stg::GEMM_NO_TILE_MAP | stg::GEMM_FORCE_SPLIT)) return HQPKKT_E_RANGE;
  // an operand of k rows and w columns: inside its rows, and one row allocated behind those read (a 16-byte load of the
  // register-staged loop reaches one column past an odd leading dimension)
  auto operand_ok = [](const hqpkkt_dgemm_operand &o, int k, int w) {
    return k == 0 || (o.p && o.ld >= 1 && o.col0 >= 0 && o.col0 + w <= o.ld && o.rows >= (long long)k + 1);
  };
  if ((!pkA && !operand_ok(c->A, K, M)) || (!pkB && !operand_ok(c->B, K, N)) || !operand_ok(c->A2, K2, M) || !operand_ok(c->B2, K2, N)) return HQPKKT_E_RANGE;
  std::vector<stg::PackPanel> ptab;
  if (pk && debug_pack_table(K, pkA ? M : N, pk_panel, c->krange, pk_elems, ptab)) return HQPKKT_E_RANGE;
  const int wc = c->mirror ? std::max(M, N) : N;  // (the image of a column strip reaches column M)
  if (c->ldc < 1 || c->c_row0 < 0 || c->c_col0 < 0 || c->c_col0 + wc > c->ldc || c->c_row0 + M > c->c_rows) return HQPKKT_E_RANGE;
  const bool beta = c->beta != 0.0, cin_own = beta && !c->cin_is_c;
  if (cin_own && !(c->Cin.p && c->Cin.ld >= 1 && c->Cin.col0 >= 0 && c->Cin.col0 + N <= c->Cin.ld && c->Cin.rows >= M)) return HQPKKT_E_RANGE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  DBuf<double> dA, dB, dA2, dB2, dCin, dC;
  DBuf<stg::PackPanel> dtab;
  auto up = [](DBuf<double> &d, const double *p, long long elems) -> int {
    if (d.alloc((size_t)elems)) return HQPKKT_E_MEM;
    HIPCHK(hipMemcpy(d.p, p, sizeof(double) * (size_t)elems, hipMemcpyHostToDevice));
    return 0;
  };
  int e;
  if (K > 0 && ((e = pkA ? up(dA, pk, pk_elems) : up(dA, c->A.p, c->A.rows * c->A.ld)) || (e = pkB ? up(dB, pk, pk_elems) : up(dB, c->B.p, c->B.rows * c->B.ld))))
    return e;
  if (pk && dtab.upload(ptab)) return HQPKKT_E_MEM;
  if (K2 > 0 && ((e = up(dA2, c->A2.p, c->A2.rows * c->A2.ld)) || (e = up(dB2, c->B2.p, c->B2.rows * c->B2.ld)))) return e;
  if (cin_own && (e = up(dCin, c->Cin.p, c->Cin.rows * c->Cin.ld))) return e;
  if ((e = up(dC, c->C, c->c_rows * c->ldc))) return e;
  stg::GemmArgs g{};
  if (K > 0) g.A = dA.p + c->A.col0, g.lda = c->A.ld, g.B = dB.p + c->B.col0, g.ldb = c->B.ld;
  if (pkA) g.A = dA.p, g.lda = 8, g.apack = dtab.p;  // (the panels' own leading dimensions count)
  if (pkB) g.B = dB.p, g.ldb = 8, g.bpack = dtab.p;
  if (K2 > 0) g.A2 = dA2.p + c->A2.col0, g.lda2 = c->A2.ld, g.B2 = dB2.p + c->B2.col0, g.ldb2 = c->B2.ld, g.K2 = K2;
  g.C = dC.p + c->c_row0 * c->ldc + c->c_col0, g.ldc = c->ldc;
  if (beta) g.Cin = cin_own ? dCin.p + c->Cin.col0 : g.C, g.ldcin = cin_own ? c->Cin.ld : c->ldc;
  g.M = M, g.N = N, g.K = K, g.alpha = c->alpha, g.beta = c->beta, g.lower = c->lower ? 1 : 0, g.mirror = c->mirror ? 1 : 0;
  DebugGemm run;
  if ((e = run.prepare(device, g, c->flags, c->krange, c->krange_by))) return e;
  run.launch(g);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(c->C, dC.p, sizeof(double) * (size_t)(c->c_rows * c->ldc), hipMemcpyDeviceToHost));
  const stg::GemmSchedule &sc = run.e->s;
  c->form = sc.f.kind, c->tile_map = !sc.order.empty(), c->ldsdma = sc.variant != stg::GEMM_REG4, c->nsplit = sc.f.nsplit;
  c->tiles = sc.f.tiles;
  return 0;
}
int hqpkkt_debug_dgemm(int device, int M, int N, int K, int lower, int mirror, int reps, double *ms, double *max_err) {
  return debug_dgemm(device, M, N, K, 0, lower, mirror, reps, ms, max_err, nullptr);
}
int hqpkkt_debug_dgemm2(int device, int M, int N, int K, int K2, int lower, int mirror, int reps, double *ms, double *max_err, long long *asym) {
  return debug_dgemm(device, M, N, K, K2, lower, mirror, reps, ms, max_err, asym);
}
int hqpkkt_debug_dgemm_full(int device, hqpkkt_dgemm_case *c) {
  return guarded([&]() -> int { return debug_dgemm_full(device, c); });
}
int hqpkkt_debug_dgemm_packed(int device, hqpkkt_dgemm_case *c, const double *packed, long long packed_elems, const long long *panel) {
  return guarded([&]() -> int { return packed ? debug_dgemm_full(device, c, packed, packed_elems, panel) : HQPKKT_E_NULL; });
}

// One launch with the control-row segment on the caller's operands (include/hqpkkt.h)
static int debug_dgemm_ctrl_rows(int device, hqpkkt_ctrl_rows_case *c) {
  if (!c || !c->C || !c->Cu || !c->A.p || !c->B.p) return HQPKKT_E_NULL;
  const int M = c->M, N = c->N, K = c->M, mu = c->mu;
  if (M <= 0 || N <= 0 || mu < 0 || mu > N || c->grid < 0) return HQPKKT_E_RANGE;
  auto operand_ok = [](const hqpkkt_dgemm_operand &o, int k, int w) { return o.ld >= 1 && o.col0 >= 0 && o.col0 + w <= o.ld && o.rows >= (long long)k + 1; };
  if (!operand_ok(c->A, K, M) || !operand_ok(c->B, K, N) || c->ldc < N + 1 || c->c_rows < M + 1 || c->ldcu < N || c->cu_rows < mu) return HQPKKT_E_RANGE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  DBuf<double> dA, dB, dC, dCu;
  auto up = [](DBuf<double> &d, const double *p, long long elems) -> int {
    if (d.alloc((size_t)elems)) return HQPKKT_E_MEM;
    HIPCHK(hipMemcpy(d.p, p, sizeof(double) * (size_t)elems, hipMemcpyHostToDevice));
    return 0;
  };
  int e;
  if ((e = up(dA, c->A.p, c->A.rows * c->A.ld)) || (e = up(dB, c->B.p, c->B.rows * c->B.ld)) || (e = up(dC, c->C, c->c_rows * c->ldc)) ||
      (e = up(dCu, c->Cu, std::max<long long>(1, c->cu_rows * c->ldcu))))
    return e;
  stg::GemmArgs g{dA.p + c->A.col0, c->A.ld, dB.p + c->B.col0, c->B.ld, nullptr, 0, dC.p, c->ldc, M, N, K, 1.0, 0.0, 0, 0};
  if (mu > 0) g.Au = g.C + (N - mu), g.ldau = c->ldc, g.mu = mu, g.Cu = dCu.p, g.ldcu = c->ldcu;
  DebugGemm run;
  if ((e = run.prepare(device, g, stg::GEMM_NO_KS | stg::GEMM_FORCE_SPLIT, nullptr, 0, c->grid))) return e;
  c->taken = run.taken(), c->fallbacks = 0;
  run.launch(g);
  HIPCHK(hipDeviceSynchronize());
  if (mu > 0 && (c->fallbacks = run.fallbacks()) < 0) return HQPKKT_E_DEVICE;
  HIPCHK(hipMemcpy(c->C, dC.p, sizeof(double) * (size_t)(c->c_rows * c->ldc), hipMemcpyDeviceToHost));
  if (c->cu_rows > 0) HIPCHK(hipMemcpy(c->Cu, dCu.p, sizeof(double) * (size_t)(c->cu_rows * c->ldcu), hipMemcpyDeviceToHost));
  c->form = run.e->s.f.kind, c->tiles = run.e->s.f.tiles;
  return 0;
}
int hqpkkt_debug_dgemm_ctrl_rows(int device, hqpkkt_ctrl_rows_case *c) {
  return guarded([&]() -> int { return debug_dgemm_ctrl_rows(device, c); });
}
// a work list for the host-only hooks: six ints per unit (include/hqpkkt.h, hqpkkt_debug_sk_table); false: cap_ints too small
static bool units_out(const stg::SplitTable &t, int *units, long long cap_ints) {
  if (!units) return true;
  if ((long long)t.units.size() * 6 > cap_ints) return false;
  for (size_t i = 0; i < t.units.size(); i++) {
    const stg::SkUnit &u = t.units[i];
    int *o = units + 6 * i;
    o[0] = u.tile, o[1] = u.s0, o[2] = u.s1, o[3] = u.slot0, o[4] = u.pieces, o[5] = u.j;
  }
  return true;
}
int hqpkkt_debug_sk_ctrl_rows(int tiles_m, int tiles_n, int nslab, int grid, int kind, int *units, long long cap_ints, int *tile_map, long long *pieces) {
  stg::SplitTable t;
  std::vector<int> map;
  const long long tiles = (long long)tiles_m * tiles_n + 1;
  if (tiles_m < 1 || tiles_n < 1) return 0;
  if (kind < 0 ? stg::gemm_choose_list(false, true, tiles, nslab, grid, tiles, 1LL << 40, t) == stg::SK_LIST_NONE : !stg::gemm_list_table(kind, tiles, nslab, grid, t)) return 0;
  if (!stg::gemm_ctrl_rows_order(t, grid, tiles_m, tiles_n, map)) return 0;
  if (pieces) *pieces = t.pieces;
  if (!units_out(t, units, cap_ints)) return 0;
  if (tile_map) std::copy(map.begin(), map.end(), tile_map);
  return t.stride;
}

int hqpkkt_debug_gemm_form(int M, int N, int K, int lower, int mirror, int cus, int grid, long long sk_tiles, long long ws_elems,
                           long long ws2_elems, int flags, long long *tiles, int *table, int *tile_map, int *nsplit) {
  const stg::GemmForm f = stg::gemm_form(M, N, K, lower, mirror, cus, grid, sk_tiles, ws_elems, ws2_elems, flags);
  if (tiles) *tiles = f.tiles;
  if (table) *table = f.kind == stg::GEMM_FORM_CUT;
  if (tile_map) *tile_map = f.tile_map;
  if (nsplit) *nsplit = f.nsplit;
  return f.kind;
}

// the request of a launch described by numbers (include/hqpkkt.h): through a GemmArgs, as the engine makes it
static stg::GemmRequest debug_request(const hqpkkt_gemm_launch *l) {
  stg::GemmArgs g{};
  g.A = (const double *)l->a, g.lda = l->lda, g.B = (const double *)l->b, g.ldb = l->ldb, g.C = (double *)l->c, g.ldc = l->ldc;
  g.A2 = (const double *)l->a2, g.lda2 = l->lda2, g.B2 = (const double *)l->b2, g.ldb2 = l->ldb2;
  g.M = l->M, g.N = l->N, g.K = l->K, g.K2 = l->K2, g.lower = l->lower, g.mirror = l->mirror, g.alpha = 1.0;
  if (l->mu > 0) g.Au = g.C + l->c0, g.ldau = l->ldc, g.mu = l->mu, g.Cu = (double *)l->c, g.ldcu = l->ldc, g.ctl = (unsigned *)l->c;
  return stg::gemm_request(g, l->second_stream != 0, l->ntiles, l->panel ? l->by : 0, l->panel);
}
int hqpkkt_debug_gemm_schedule(const hqpkkt_gemm_caps *caps, const hqpkkt_gemm_launch *launch, const hqpkkt_gemm_launch *other,
                               hqpkkt_gemm_schedule_out *out, int *units, long long cap_ints, int *order, long long cap_order) {
  return guarded([&]() -> int {
    if (!caps || !launch || !out) return -1;
    const stg::GemmCaps c{caps->variant, caps->cus, caps->grid, caps->sk_tiles, caps->cnt_elems, caps->ws_elems, caps->ws2_elems, caps->unequal != 0, caps->flags};
    const stg::GemmRequest rq = debug_request(launch);
    stg::GemmSchedule s;
    const int status = stg::gemm_schedule(c, rq, s);
    *out = hqpkkt_gemm_schedule_out{s.f.kind, s.f.nsplit, s.variant, s.list, s.tab.stride, s.seg, other && rq == debug_request(other), s.f.tiles, s.nslab, s.tab.pieces,
                                    (long long)s.order.size()};
    if (status == stg::GEMM_SCHED_OK && (!units_out(s.tab, units, cap_ints) || (order && (long long)s.order.size() > cap_order))) return -1;
    if (status == stg::GEMM_SCHED_OK && order) std::copy(s.order.begin(), s.order.end(), order);
    return status;
  });
}

int hqpkkt_debug_sk_table(long long tiles, int nslab, int grid, int kind, int *units, long long cap_ints, long long *pieces, int *whole_a, int *whole_b) {
  stg::SplitTable t;
  if (!stg::gemm_list_table(kind, tiles, nslab, grid, t)) return 0;
  if (pieces) *pieces = t.pieces;
  if (whole_a) *whole_a = t.nA;
  if (whole_b) *whole_b = t.nB;
  if (!units_out(t, units, cap_ints)) return 0;
  return t.stride;
}

int hqpkkt_debug_sk_profile(const int *ranges, long long tiles, int grid, int *units, long long cap_ints, long long *pieces) {
  stg::SplitTable t;
  if (!stg::gemm_profile_table(ranges, tiles, grid, t)) return 0;
  if (pieces) *pieces = t.pieces;
  if (!units_out(t, units, cap_ints)) return 0;
  return t.stride;
}

// One launch of a product of the profile form's solve (staged_profile.hip.h) on the caller's host arrays
// (panel: A is a buffer of a_rows x ld doubles that holds packed panels, (offset, ld) per panel: hqpkkt_debug_gemv_packed)
static int debug_gemv_profile(int device, int rows_form, int K, int N, const double *A, long long a_rows, long long ld, const int *ranges,
                              const double *x, const double *add, double alpha, double *y, const long long *panel = nullptr) {
  if (!A || !ranges || !x || !y) return HQPKKT_E_NULL;
  if (K <= 0 || N <= 0 || (!panel && (a_rows < K || ld < N || (ld & 7)))) return HQPKKT_E_RANGE;
  std::vector<stg::PackPanel> ptab;
  if (panel && (a_rows < 1 || ld < 1 || debug_pack_table(K, N, panel, ranges, a_rows * ld, ptab))) return HQPKKT_E_RANGE;
  const int np = (N + 127) / 128, nx = rows_form ? N : K, ny = rows_form ? K : N;
  for (int p = 0; p < np; p++)
    if (ranges[2 * p] < 0 || ranges[2 * p + 1] < ranges[2 * p] || ranges[2 * p + 1] > (K + 15) / 16) return HQPKKT_E_RANGE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  DBuf<double> dA, dx, dadd, dy, part;
  DBuf<int> dr;
  DBuf<stg::PackPanel> dtab;
  if (panel && dtab.upload(ptab)) return HQPKKT_E_MEM;
  const int chunks = stg::pf_chunks(ranges, np, K);
  const int guard = 64;  // doubles behind y on the device, checked after the launch: nothing may be written past y
  const std::vector<double> mark(guard, -12345.678);
  if (dA.alloc((size_t)(a_rows * ld)) || dx.alloc(nx) || dy.alloc(ny + guard) || (add && dadd.alloc(ny)) || part.alloc((size_t)chunks * N) ||
      dr.upload(std::vector<int>(ranges, ranges + 2 * np)))
    return HQPKKT_E_MEM;
  HIPCHK(hipMemcpy(dA.p, A, sizeof(double) * (size_t)(a_rows * ld), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dx.p, x, sizeof(double) * nx, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy.p, y, sizeof(double) * ny, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy.p + ny, mark.data(), sizeof(double) * guard, hipMemcpyHostToDevice));
  if (add) HIPCHK(hipMemcpy(dadd.p, add, sizeof(double) * ny, hipMemcpyHostToDevice));
  const stg::PfGemv g{dA.p, ld, K, N, dr.p, dx.p, add ? dadd.p : nullptr, alpha, dy.p, part.p, panel ? dtab.p : nullptr};
  if (rows_form)
    stg::pf_launch_rows(g, 0, [](auto &&kernel) { kernel(); });
  else
    stg::pf_launch_cols(g, ranges, 0, [](auto &&kernel) { kernel(); });
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(y, dy.p, sizeof(double) * ny, hipMemcpyDeviceToHost));
  std::vector<double> back(guard);
  HIPCHK(hipMemcpy(back.data(), dy.p + ny, sizeof(double) * guard, hipMemcpyDeviceToHost));
  return std::memcmp(back.data(), mark.data(), sizeof(double) * guard) ? HQPKKT_E_INTERN : 0;
}
int hqpkkt_debug_gemv_profile(int device, int rows_form, int K, int N, const double *A, long long a_rows, long long ld, const int *ranges,
                              const double *x, const double *add, double alpha, double *y) {
  return guarded([&]() -> int { return debug_gemv_profile(device, rows_form, K, N, A, a_rows, ld, ranges, x, add, alpha, y); });
}

int hqpkkt_debug_gemv_packed(int device, int rows_form, int K, int N, const double *packed, long long packed_elems, const long long *panel,
                             const int *ranges, const double *x, const double *add, double alpha, double *y) {
  return guarded([&]() -> int {
    if (!panel) return HQPKKT_E_NULL;
    return debug_gemv_profile(device, rows_form, K, N, packed, 1, packed_elems, ranges, x, add, alpha, y, panel);
  });
}

// One launch of the carried rows of a packed stage (k_pk_carried) on the caller's host arrays
static int debug_carried_packed(int device, int K, int N, int R, const double *BT, long long bt_rows, long long ldb, const double *packed,
                                long long packed_elems, const long long *panel, const int *ranges, double *Cbuf, long long c_rows, long long ldc,
                                long long c_row0, long long c_col0) {
  if (!BT || !packed || !panel || !ranges || !Cbuf) return HQPKKT_E_NULL;
  if (K <= 0 || N <= 0 || R <= 0 || bt_rows < K || ldb < R || packed_elems < 1 || ldc < 1 || c_row0 < 0 || c_col0 < 0 || c_col0 + N > ldc ||
      c_row0 + R > c_rows)
    return HQPKKT_E_RANGE;
  std::vector<stg::PackPanel> ptab;
  if (debug_pack_table(K, N, panel, ranges, packed_elems, ptab)) return HQPKKT_E_RANGE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  const int np = (N + 127) / 128;
  DBuf<double> dB, dA, dC, part;
  DBuf<int> dr;
  DBuf<stg::PackPanel> dtab;
  if (dB.alloc((size_t)(bt_rows * ldb)) || dA.alloc((size_t)packed_elems) || dC.alloc((size_t)(c_rows * ldc)) ||
      part.alloc((size_t)stg::pk_chunks(ranges, np, K) * R * N) || dr.upload(std::vector<int>(ranges, ranges + 2 * np)) || dtab.upload(ptab))
    return HQPKKT_E_MEM;
  HIPCHK(hipMemcpy(dB.p, BT, sizeof(double) * (size_t)(bt_rows * ldb), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dA.p, packed, sizeof(double) * (size_t)packed_elems, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dC.p, Cbuf, sizeof(double) * (size_t)(c_rows * ldc), hipMemcpyHostToDevice));
  stg::pk_launch_carried(stg::PkCarried{dB.p, ldb, dA.p, dtab.p, dr.p, K, N, R, 0, dC.p + c_row0 * ldc + c_col0, ldc, part.p}, ranges, 0,
                         [](auto &&kernel) { kernel(); });
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(Cbuf, dC.p, sizeof(double) * (size_t)(c_rows * ldc), hipMemcpyDeviceToHost));
  return 0;
}
int hqpkkt_debug_carried_packed(int device, int K, int N, int R, const double *BT, long long bt_rows, long long ldb, const double *packed,
                                long long packed_elems, const long long *panel, const int *ranges, double *C, long long c_rows, long long ldc,
                                long long c_row0, long long c_col0) {
  return guarded([&]() -> int {
    return debug_carried_packed(device, K, N, R, BT, bt_rows, ldb, packed, packed_elems, panel, ranges, C, c_rows, ldc, c_row0, c_col0);
  });
}

// ---- the solve's dense vector products on the caller's host arrays (include/hqpkkt.h): one launch through the engine's
// launch functions (stg::gemv_launch_*, symv_launch, symv_launch_batch); nothing is compared here
namespace {
constexpr int DBG_GUARD = 64;  // marked doubles behind every result vector and scratch area on the device
// a vector the launch writes: the caller's n doubles and the marks behind them
struct DebugOut {
  DBuf<double> d;
  long long n = 0;
  int up(const double *host, long long len) {
    n = len;
    const std::vector<double> mark(DBG_GUARD, -12345.678);
    if (d.alloc((size_t)(n + DBG_GUARD))) return HQPKKT_E_MEM;
    HIPCHK(hipMemcpy(d.p, host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.p + n, mark.data(), sizeof(double) * DBG_GUARD, hipMemcpyHostToDevice));
    return 0;
  }
  int down(double *host) {  // HQPKKT_E_INTERN: a mark has changed
    const std::vector<double> mark(DBG_GUARD, -12345.678);
    std::vector<double> back(DBG_GUARD);
    HIPCHK(hipMemcpy(host, d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(back.data(), d.p + n, sizeof(double) * DBG_GUARD, hipMemcpyDeviceToHost));
    return std::memcmp(back.data(), mark.data(), sizeof(double) * DBG_GUARD) ? HQPKKT_E_INTERN : 0;
  }
};
// partial sums: `elems` doubles as the plan sizes them and the marks, all NaN before the launch (a partial that is read
// but never written shows in y); whatever lies outside the parts in use must come back untouched
struct DebugScratch {
  DBuf<double> d;
  std::vector<double> fill;
  int make(long long elems) {
    fill.assign((size_t)(elems + DBG_GUARD), std::numeric_limits<double>::quiet_NaN());
    if (d.alloc(fill.size())) return HQPKKT_E_MEM;
    HIPCHK(hipMemcpy(d.p, fill.data(), sizeof(double) * fill.size(), hipMemcpyHostToDevice));
    return 0;
  }
  // used: (first, one past last) pairs, ascending, of the doubles the launch may write
  int check(const std::vector<std::pair<long long, long long>> &used) {
    std::vector<double> back(fill.size());
    HIPCHK(hipMemcpy(back.data(), d.p, sizeof(double) * back.size(), hipMemcpyDeviceToHost));
    long long at = 0;
    auto same = [&](long long a, long long b) { return b <= a || !std::memcmp(back.data() + a, fill.data() + a, sizeof(double) * (size_t)(b - a)); };
    for (const auto &u : used) {
      if (!same(at, u.first)) return HQPKKT_E_INTERN;
      at = u.second;
    }
    return same(at, (long long)back.size()) ? 0 : HQPKKT_E_INTERN;
  }
};
int debug_up(DBuf<double> &d, const double *p, long long elems) {
  if (d.alloc((size_t)elems)) return HQPKKT_E_MEM;
  if (elems > 0) HIPCHK(hipMemcpy(d.p, p, sizeof(double) * (size_t)elems, hipMemcpyHostToDevice));
  return 0;
}
// an operand of `rows` rows and w columns inside its buffer
bool debug_block_ok(const hqpkkt_dgemm_operand &o, long long rows, long long w) {
  return o.p && o.ld >= 1 && o.col0 >= 0 && w >= 0 && o.col0 + w <= o.ld && o.rows >= rows && rows >= 1;
}
// the carried rows' block of a case with `rows` rows: 0 fine (or none), else the code
int debug_a2_check(const hqpkkt_gemv_case &c, long long rows) {
  if (!c.A2.p) return 0;
  if (!c.x2) return HQPKKT_E_NULL;
  if (c.n2 < 0 || !debug_block_ok(c.A2, rows, c.n2) || c.x2_len < c.n2) return HQPKKT_E_RANGE;
  return 0;
}
// what a case's second block needs on the device
struct DebugA2 {
  DBuf<double> A, x;
  DBuf<int> n;
  int up(const hqpkkt_gemv_case &c) {
    if (!c.A2.p) return 0;
    int e;
    if ((e = debug_up(A, c.A2.p, c.A2.rows * c.A2.ld)) || (e = debug_up(x, c.x2, c.x2_len))) return e;
    return n.upload(std::vector<int>(1, c.n2));
  }
};
int debug_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  return 0;
}
const auto debug_plain = [](auto &&kernel) { kernel(); };
}  // namespace

static int debug_gemv_dense(int device, int form, hqpkkt_gemv_case *c) {
  if (!c || !c->A.p || !c->x || !c->y) return HQPKKT_E_NULL;
  if (form < 0 || form > 2) return HQPKKT_E_RANGE;
  const bool cols = form == 2;
  const int M = c->M, N = c->N, nx = cols ? M : N, ny = cols ? N : M;
  if (M <= 0 || N <= 0 || !debug_block_ok(c->A, M, N) || c->x_len < nx) return HQPKKT_E_RANGE;
  if (form == 0) {
    if (int e = debug_a2_check(*c, M)) return e;
  } else if (c->A2.p)
    return HQPKKT_E_RANGE;
  if (cols ? (c->part_chunks < 1 || !c->add2 != !c->y2) : (c->add2 || c->y2)) return HQPKKT_E_RANGE;
  int e;
  if ((e = debug_device(device))) return e;
  DBuf<double> dA, dx, dadd, dadd2;
  DebugA2 a2;
  DebugOut y, y2;
  DebugScratch part;
  if ((e = debug_up(dA, c->A.p, c->A.rows * c->A.ld)) || (e = debug_up(dx, c->x, c->x_len)) || (c->add && (e = debug_up(dadd, c->add, ny))) ||
      (c->add2 && (e = debug_up(dadd2, c->add2, ny))) || (e = a2.up(*c)) || (e = y.up(c->y, ny)) || (c->y2 && (e = y2.up(c->y2, ny))))
    return e;
  const double *A = dA.p + c->A.col0;
  std::vector<std::pair<long long, long long>> used;
  if (cols) {
    if ((e = part.make((long long)c->part_chunks * (N + 8)))) return e;
    const stg::GemvCols g{A, c->A.ld, M, N, dx.p, c->add ? dadd.p : nullptr, c->scale, y.d.p, part.d.p, 0, c->add2 ? dadd2.p : nullptr, c->y2 ? y2.d.p : nullptr};
    c->chunks = stg::gemv_launch_cols(g, c->part_chunks, 0, debug_plain);
    c->vec16 = (((size_t)A) & 15) == 0 && (c->A.ld & 1) == 0;
    if (c->chunks > 1) used.push_back({0, (long long)c->chunks * N});
  } else {
    const stg::GemvRows g{A, c->A.ld, M, N, dx.p, c->add ? dadd.p : nullptr, c->A2.p ? a2.A.p + c->A2.col0 : nullptr, c->A2.ld, c->A2.p ? a2.n.p : nullptr,
                          c->A2.p ? a2.x.p : nullptr, y.d.p, c->scale};
    if (form == 0)
      stg::gemv_launch_rows(g, 0, debug_plain);
    else
      stg::gemv_launch_wide(g, 0, debug_plain);
    c->chunks = 1, c->vec16 = 0;
    for (int i = 0; i < M; i++) c->vec16 += (((size_t)(A + (long long)i * c->A.ld)) & 15) == 0;  // (rows that take the 16-byte loads)
  }
  HIPCHK(hipDeviceSynchronize());
  e = y.down(c->y);
  if (c->y2)
    if (int e2 = y2.down(c->y2)) e = e2;
  if (cols)
    if (int e2 = part.check(used)) e = e2;
  return e;
}
int hqpkkt_debug_gemv_dense(int device, int form, hqpkkt_gemv_case *c) {
  return guarded([&]() -> int { return debug_gemv_dense(device, form, c); });
}

// a vector the kernel reads: its n entries and DBG_GUARD NaN doubles behind them
static int debug_up_nan(DBuf<double> &d, const double *p, long long n) {
  std::vector<double> v((size_t)(n + DBG_GUARD), std::numeric_limits<double>::quiet_NaN());
  std::copy(p, p + n, v.begin());
  return d.upload(v);
}
static int debug_rows_gemv(int device, int form, hqpkkt_rows_case *c) {
  if (!c || !c->rows || !c->cols || !c->ld || !c->col0 || !c->off || !c->E || !c->row_index) return HQPKKT_E_NULL;
  if (form < 0 || form > 2) return HQPKKT_E_RANGE;
  if (form == 2 ? (!c->t || !c->xc) : (!c->x || (form == 0 ? !c->y : (!c->tz || !c->zw || !c->r3 || !c->dz || !c->dw)))) return HQPKKT_E_NULL;
  if (c->nblocks < 1 || c->n < 1 || c->m < 1 || c->e_len < 1) return HQPKKT_E_RANGE;
  std::vector<stg::RowsBlock> rb(c->nblocks);
  std::vector<int> of;
  int pairs_max = 0;
  for (int b = 0; b < c->nblocks; b++) {
    const long long r = c->rows[b], nz = c->cols[b], ld = c->ld[b], off = c->off[b], col0 = c->col0[b];
    // (what the kernels take: rows of whole 16-byte pairs - the plan's blocks have ld = up8 - inside E, columns inside x)
    if (r < 0 || nz < 1 || ld < nz || ld % 8 || off < 0 || (off & 1) || off + r * ld > c->e_len || col0 < 0 || col0 + nz > c->n) return HQPKKT_E_RANGE;
    rb[b] = stg::RowsBlock{off, (int)ld, (int)nz, (int)col0, (int)of.size(), (int)r};
    of.insert(of.end(), (size_t)r, b);
    pairs_max = std::max(pairs_max, (int)((nz + 1) / 2));
  }
  const int R = (int)of.size();
  {
    std::vector<char> seen(c->m, 0);
    for (int q = 0; q < R; q++) {
      if (c->row_index[q] < 0 || c->row_index[q] >= c->m || seen[c->row_index[q]]) return HQPKKT_E_RANGE;
      seen[c->row_index[q]] = 1;
    }
  }
  int e;
  if ((e = debug_device(device))) return e;
  DBuf<stg::RowsBlock> dblk;
  DBuf<int> dof, drows;
  DBuf<double> dE, dx, dt, dtz, dzw, dr3;
  DebugOut y, dz, dw, xc;
  if ((e = dblk.upload(rb)) || (e = dof.upload(of)) || (e = drows.upload(std::vector<int>(c->row_index, c->row_index + R))) || (e = debug_up(dE, c->E, c->e_len)))
    return e;
  if (form == 2) {
    if ((e = debug_up_nan(dt, c->t, c->m)) || (e = xc.up(c->xc, c->n))) return e;
    stg::rows_launch_t(stg::RowsGemvT{dblk.p, dE.p, drows.p, dt.p, xc.d.p}, c->nblocks, pairs_max, 0, debug_plain);
  } else {
    if ((e = debug_up_nan(dx, c->x, c->n))) return e;
    if (form == 0 ? (e = y.up(c->y, c->m))
                  : ((e = debug_up_nan(dtz, c->tz, c->m)) || (e = debug_up_nan(dzw, c->zw, c->m)) || (e = debug_up_nan(dr3, c->r3, c->m)) || (e = dz.up(c->dz, c->m)) ||
                     (e = dw.up(c->dw, c->m))))
      return e;
    stg::rows_launch(stg::RowsGemv{dblk.p, dof.p, R, dE.p, drows.p, dx.p, form == 1 ? dtz.p : nullptr, dzw.p, dr3.p, dz.d.p, dw.d.p, y.d.p}, 0, debug_plain);
  }
  HIPCHK(hipDeviceSynchronize());
  if (form == 2) return xc.down(c->xc);
  if (form == 0) return y.down(c->y);
  e = dz.down(c->dz);
  if (int e2 = dw.down(c->dw)) e = e2;
  return e;
}
int hqpkkt_debug_rows_gemv(int device, int form, hqpkkt_rows_case *c) {
  return guarded([&]() -> int { return debug_rows_gemv(device, form, c); });
}

// what the triangle form asks of a case: NULL / RANGE, 0 fine.  vec: the case brings x / y of its own
static int debug_symv_check(const hqpkkt_gemv_case &c, bool own_x, bool own_y) {
  if (!c.A.p || (own_x && !c.x) || (own_y && !c.y)) return HQPKKT_E_NULL;
  if (c.N <= 0 || !debug_block_ok(c.A, c.N, c.N) || (own_x && c.x_len < c.N)) return HQPKKT_E_RANGE;
  if ((c.A.ld & 1) || (c.A.col0 & 1)) return HQPKKT_E_RANGE;  // (what symv_tiles_form refuses: 16-byte loads of every row)
  return debug_a2_check(c, c.N);
}
static int debug_symv(int device, hqpkkt_gemv_case *c) {
  if (!c) return HQPKKT_E_NULL;
  int e;
  if ((e = debug_symv_check(*c, true, true)) || (e = debug_device(device))) return e;
  const int N = c->N;
  DBuf<double> dV, dx, dadd;
  DebugA2 a2;
  DebugOut y;
  DebugScratch part;
  if ((e = debug_up(dV, c->A.p, c->A.rows * c->A.ld)) || (e = debug_up(dx, c->x, c->x_len)) || (c->add && (e = debug_up(dadd, c->add, N))) || (e = a2.up(*c)) ||
      (e = y.up(c->y, N)) || (e = part.make(kktdev::StagedPlan::symv_need(N))))
    return e;
  const stg::GemvRows g{dV.p + c->A.col0, c->A.ld, N, N, dx.p, c->add ? dadd.p : nullptr, c->A2.p ? a2.A.p + c->A2.col0 : nullptr, c->A2.ld,
                        c->A2.p ? a2.n.p : nullptr, c->A2.p ? a2.x.p : nullptr, y.d.p, c->scale};
  stg::symv_launch(g, part.d.p, 0, debug_plain);
  HIPCHK(hipDeviceSynchronize());
  c->chunks = (int)stg::symv_tiles(N), c->vec16 = 1;
  e = y.down(c->y);
  const long long parts = (N + stg::SV_R - 1) / stg::SV_R + (N + stg::SV_C - 1) / stg::SV_C;
  if (int e2 = part.check({{0, parts * N}})) e = e2;
  return e;
}
int hqpkkt_debug_symv(int device, hqpkkt_gemv_case *c) {
  return guarded([&]() -> int { return debug_symv(device, c); });
}

static int debug_symv_batch(int device, int count, hqpkkt_gemv_case *cs, const double *xbase, long long xbase_len, double *ybase, long long ybase_len,
                            int grid_tiles, int grid_fins) {
  if (!cs) return HQPKKT_E_NULL;
  if (count < 1 || grid_tiles < 0 || grid_fins < 0 || xbase_len < 0 || ybase_len < 0) return HQPKKT_E_RANGE;
  auto up16 = [](long long x) { return (x + 15) / 16 * 16; };
  long long arena = 0;
  for (int i = 0; i < count; i++) {
    const hqpkkt_gemv_case &c = cs[i];
    if (int e = debug_symv_check(c, !xbase, !ybase)) return e;
    if (xbase && (c.xoff < 0 || c.xoff + c.N > xbase_len)) return HQPKKT_E_RANGE;
    if (ybase && (c.yoff < 0 || c.yoff + c.N > ybase_len)) return HQPKKT_E_RANGE;
    arena += up16(kktdev::StagedPlan::symv_need(c.N));
  }
  int e;
  if ((e = debug_device(device))) return e;
  std::vector<DBuf<double>> dV(count), dx(count), dadd(count);
  std::vector<DebugA2> a2(count);
  std::vector<DebugOut> y(count);
  DBuf<double> dxb;
  DebugOut yb;
  DebugScratch part;
  DBuf<stg::SymvItem> ditems;
  if ((e = part.make(arena)) || (xbase && (e = debug_up(dxb, xbase, xbase_len))) || (ybase && (e = yb.up(ybase, ybase_len)))) return e;
  std::vector<stg::SymvItem> items(count);
  std::vector<std::pair<long long, long long>> used;
  int tiles = 0, fins = 0;
  long long at = 0;
  for (int i = 0; i < count; i++) {
    const hqpkkt_gemv_case &c = cs[i];
    const int N = c.N;
    if ((e = debug_up(dV[i], c.A.p, c.A.rows * c.A.ld)) || (!xbase && (e = debug_up(dx[i], c.x, c.x_len))) || (c.add && (e = debug_up(dadd[i], c.add, N))) ||
        (e = a2[i].up(c)) || (!ybase && (e = y[i].up(c.y, N))))
      return e;
    double *rowpart, *colpart;
    stg::symv_parts(part.d.p + at, N, rowpart, colpart);
    stg::SymvItem &it = items[i];
    it.a = stg::SymvArgs{dV[i].p + c.A.col0, c.A.ld, N, xbase ? nullptr : dx[i].p, rowpart, colpart};
    it.f = stg::SymvFinish{N, rowpart, colpart, c.add ? dadd[i].p : nullptr, c.A2.p ? a2[i].A.p + c.A2.col0 : nullptr, c.A2.ld, c.A2.p ? a2[i].n.p : nullptr,
                           c.A2.p ? a2[i].x.p : nullptr, ybase ? nullptr : y[i].d.p, c.scale};
    it.tile0 = tiles, it.fin0 = fins;
    it.xrel = xbase != nullptr, it.yrel = ybase != nullptr, it.xoff = c.xoff, it.yoff = c.yoff;
    tiles += (int)stg::symv_tiles(N), fins += (N + 63) / 64;
    used.push_back({at, at + ((N + stg::SV_R - 1) / stg::SV_R + (N + stg::SV_C - 1) / stg::SV_C) * (long long)N});
    at += up16(kktdev::StagedPlan::symv_need(N));
  }
  if ((e = ditems.upload(items))) return e;
  stg::symv_launch_batch(ditems.p, count, tiles, fins, grid_tiles, grid_fins, dxb.p, yb.d.p, 0, debug_plain);
  HIPCHK(hipDeviceSynchronize());
  e = 0;
  if (ybase) e = yb.down(ybase);
  for (int i = 0; i < count && !ybase; i++)
    if (int e2 = y[i].down(cs[i].y)) e = e2;
  if (int e2 = part.check(used)) e = e2;
  cs[0].chunks = tiles;
  return e;
}
int hqpkkt_debug_symv_batch(int device, int count, hqpkkt_gemv_case *cases, const double *xbase, long long xbase_len, double *ybase, long long ybase_len,
                            int grid_tiles, int grid_fins) {
  return guarded([&]() -> int { return debug_symv_batch(device, count, cases, xbase, xbase_len, ybase, ybase_len, grid_tiles, grid_fins); });
}

long long hqpkkt_debug_symv_map(int N, int *pairs, long long cap) {
  if (N <= 0) return 0;
  const long long tiles = stg::symv_tiles(N);
  if (pairs && cap >= 2 * tiles)
    for (long long t = 0; t < tiles; t++) stg::symv_tile_pair((int)t, pairs[2 * t], pairs[2 * t + 1]);
  return tiles;
}

#ifdef HQPKKT_STAMPS
int hqpkkt_debug_gj_stamps(int *out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(stg::g_gj_stamps), sizeof(int) * 32));
  return 0;
}
#endif

}  // extern "C"
