// The tree engine (HQPKKT_MODE_FULL / _REDUCED): device residency of the symbolic structure and the kernel
// sequencing of assemble -> factor -> step -> residual; the vector staging of a call and the posted read-backs
// (both engines use them), and the debug entry points that launch the tree's kernels or read its device arrays.
#include "hqpkkt_handle.hpp"

#include "kernels.hip.h"
#include "factor_blk.hip.h"
#include "solve_top.hip.h"

using namespace kktdev;

int ensure_device(hqpkkt_t *h) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= h->opts.device) {
    std::snprintf(g_last_hip_error, sizeof(g_last_hip_error),
                  "no HIP device %d (gfx950 required; there is no CPU fallback)", h->opts.device);
    return HQPKKT_E_DEVICE;
  }
  HIPCHK(hipSetDevice(h->opts.device));
  if (!h->own_stream) {
    HIPCHK(hipStreamCreateWithFlags(&h->own_stream.h, hipStreamNonBlocking));
    for (EventOwner *ev : {&h->ev0, &h->ev1, &h->evs0, &h->evs1, &h->evt0, &h->evt1}) HIPCHK(hipEventCreate(&ev->h));
  }
  if (!h->stream) h->stream = h->own_stream;
  return 0;
}

// the exchange arrays of k_solve_top in their idle state: every word the sentinel, counters zero
static int reset_solve_top(hqpkkt_t *h) {
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->td.tree_words.p) HIPCHK(hipMemset(h->td.tree_words.p, 0, sizeof(int) * 2));
  auto fill = [&](DBuf<double> &buf, size_t count) -> int {
    std::vector<double> f(count);
    for (auto &x : f) std::memcpy(&x, &XW_SENTINEL, sizeof(double));
    HIPCHK(hipMemcpy(buf.p, f.data(), sizeof(double) * count, hipMemcpyHostToDevice));
    return 0;
  };
  int e;
  if (h->top_n > 0) {
    if ((e = fill(h->td.top_x, 2 * (size_t)h->top_n * (ST_CS + ST_XS)))) return e;
  }
  if (h->small_tree) {
    if ((e = fill(h->td.tree_x, 2 * (size_t)(h->an.cb_elems + h->an.dim)))) return e;
    if (h->tree_factor && (e = fill(h->td.tree_u, 2 * (size_t)std::max<long long>(h->an.upd_elems, 1)))) return e;

  }
  return 0;
}

bool poll_fallback(hqpkkt_t *h, const int *hs) {
  if (!hs[XW_GAVE_UP]) return false;
  (void)reset_solve_top(h);
  (void)hipMemsetAsync(h->td.flags.p + XW_GAVE_UP, 0, sizeof(int), h->stream);
  (void)hipStreamSynchronize(h->stream);
  h->top_n = 0, h->small_tree = false, h->tree_factor = false, h->no_polled = true;  // (no_polled: a later upload stays there)
  h->drop_graphs();
  h->st.n_poll_fallbacks++;
  if (getenv("HQPKKT_TRACE_SOLVE")) fprintf(stderr, "a polled launch gave up: per-level launches from now on\n");
  return true;
}

// the mapped, coherent host words of the read-backs (hqpkkt::Kept::hpin; both engines)
int alloc_hpin(hqpkkt_t *h) {
  PinnedBuf<double> &hp = h->kept.hpin;
  if (hp.p) return 0;
  HIPCHK(hp.alloc(HPIN_DOUBLES, hipHostMallocMapped | hipHostMallocCoherent));
  std::memset(hp.p, 0, sizeof(double) * HPIN_DOUBLES);
  HIPCHK(hp.map());
  h->post_seq = 0;
  int e = h->kept.post_seq_dev.alloc(1);
  if (e) return e;
  HIPCHK(hipMemset(h->kept.post_seq_dev.p, 0, sizeof(unsigned)));
  return 0;
}
int upload(hqpkkt_t *h) {
  int e = ensure_device(h);
  if (e) return e;
  Analysis &an = h->an;
#define UP(buf, vec) \
  if ((e = h->td.buf.upload(an.vec))) return e
  UP(piv_start, piv_start);
  UP(npiv, npiv);
  UP(nbor, nbor);
  UP(parent, parent);
  UP(bidx, bidx);
  UP(rel, rel);
  UP(child_ptr, child_ptr);
  UP(child_idx, child_idx);
  for (int w = 0; w < 2; w++) {
    UP(ds[w].level_nodes, sched[w].level_nodes);
    UP(ds[w].upd_tiles, sched[w].upd_tiles);
    UP(ds[w].slabs, sched[w].slabs);
    UP(ds[w].gslabs, sched[w].gslabs);
    UP(ds[w].cblks, sched[w].cblks);
  }
  UP(zero_panel, zero_panel);
  UP(keep_e, keep_e);
  UP(linv_off, linv_off);
  UP(pinv, pinv);
  UP(pinv_off, pinv_off);
  UP(ent_a, ent_a);
  UP(ent_b, ent_b);
  UP(term_ptr, term_ptr);
  UP(diag_ent, diag_ent);
  UP(q2e, q2e);
  UP(bptr, bptr);
  UP(panel_off, panel_off);
  UP(upd_off, upd_off);
  UP(x_off, x_off);
  UP(cb_off, cb_off);
  UP(ent_dst, ent_dst);
#undef UP
  {
    std::vector<TermDev> t(an.terms.size());
    for (size_t k = 0; k < t.size(); k++)
      t[k] = TermDev{an.terms[k].s1, an.terms[k].s2, an.terms[k].wi, an.terms[k].sgn};
    if ((e = h->td.terms.upload(t))) return e;
    // all entries single terms sgn * vals[s1] * wt[wi] with s2 = the constant 1 (FULL plugin)?
    const int one = an.nq + an.na + an.nc;
    bool simple = an.mode == 0 && an.terms.size() == an.ent_a.size();
    for (size_t k = 0; simple && k < t.size(); k++)
      simple = t[k].s2 == one && (t[k].sgn == 1.0 || t[k].sgn == -1.0);
    if (simple) {
      std::vector<int> ss(t.size()), ww(t.size());
      for (size_t k = 0; k < t.size(); k++) ss[k] = t[k].s1 | (t[k].sgn < 0 ? (int)0x80000000 : 0), ww[k] = t[k].wi;
      if ((e = h->td.simple_src.upload(ss)) || (e = h->td.simple_wi.upload(ww))) return e;
    }
    // sign a perturbed pivot takes: x rows belong to the -Q block, y / slack rows
    // to the zero / +W/Z blocks
    std::vector<signed char> sg(an.dim);
    for (int q = 0; q < an.dim; q++) sg[an.q2e[q]] = q < an.n ? -1 : 1;
    // +-2: no diagonal of its own (see zero_pivot_slot in kernels.hip.h)
    std::vector<char> in_c(an.n, 0);  // REDUCED: C' (Z/W) C gives x_i a diagonal as well
    if (an.mode != 0)
      for (int c : h->pCi) in_c[c] = 1;
    for (int q = 0; q < an.n; q++) {
      bool diag = in_c[q] != 0;
      for (int k = h->pQp[q]; k < h->pQp[q + 1]; k++) diag = diag || h->pQi[k] == q;
      if (!diag) sg[an.q2e[q]] = -2;
    }
    for (int q = an.n; q < an.n + an.me; q++) sg[an.q2e[q]] = 2;
    if ((e = h->td.esign.upload(sg))) return e;
  }
  if ((e = h->td.Qf.upload(an.Qfull)) || (e = h->td.A.upload(an.A)) || (e = h->td.AT.upload(an.AT)) ||
      (e = h->td.C.upload(an.C)) || (e = h->td.CT.upload(an.CT)))
    return e;
  const int n = an.n, me = an.me, m = an.m, dim = an.dim;
  const size_t nv = (size_t)an.nq + an.na + an.nc + 1;
  if ((e = h->td.vals.alloc(nv)) || (e = h->td.wt.alloc(m + 1)) || (e = h->td.sc.alloc(dim)) ||
      (e = h->td.ent_val.alloc(an.ent_a.size())) || (e = h->td.panel.alloc(an.panel_elems)) ||
      (e = h->td.upd.alloc(an.upd_elems)) || (e = h->td.xar.alloc(an.x_elems)) ||
      (e = h->td.dinv.alloc(2 * (size_t)dim)) || (e = h->td.rhs.alloc(dim)) ||
      (e = h->td.xsol.alloc(dim)) || (e = h->td.cb.alloc(an.cb_elems)) || (e = h->td.ytmp.alloc(std::max(dim, 8))) ||
      (e = h->td.vtmp.alloc(dim)) || (e = h->td.linv.alloc(an.linv_elems)) || (e = h->td.ptype.alloc(dim)) ||
      (e = h->td.lperm.alloc(dim)) || (e = h->td.flags.alloc(128)) ||
      (e = h->td.vin.alloc(2 * (size_t)m + n + me + 2 * (size_t)m)) ||
      (e = h->td.vout.alloc((size_t)n + me + 2 * (size_t)m)) ||
      (e = h->td.vres.alloc((size_t)n + me + 2 * (size_t)m)) ||
      (e = h->td.vcor.alloc((size_t)n + me + 2 * (size_t)m)) || (e = h->td.tz.alloc(m)))
    return e;
  h->td.bits.p = (unsigned long long *)(h->td.flags.p + 120);
  HIPCHK(hipMemset(h->td.flags.p, 0, sizeof(int) * 128));
  h->res_read = 122;
  if ((e = alloc_hpin(h))) return e;
  h->td.hstage.release();
  h->td.hstage_in = h->td.hstage_out = 0;
  {
    const size_t nin = 4 * (size_t)m + n + me, nout = (size_t)n + me + 2 * (size_t)m;
    if ((nin + nout) * sizeof(double) <= (size_t)512 * 1024 && nin + nout > 0) {
      HIPCHK(h->td.hstage.alloc(nin + nout, hipHostMallocMapped | hipHostMallocCoherent));
      h->td.hstage_in = nin, h->td.hstage_out = nout;
      if (h->td.hstage.map() != hipSuccess) (void)hipGetLastError();
    }
  }
  {
    std::vector<double> ones(dim, 1.0);
    HIPCHK(hipMemcpy(h->td.sc.p, ones.data(), sizeof(double) * dim, hipMemcpyHostToDevice));
    const double one = 1.0;
    HIPCHK(hipMemcpy(h->td.vals.p + (nv - 1), &one, sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->td.wt.p + m, &one, sizeof(double), hipMemcpyHostToDevice));
  }
  // dynamic LDS budgets
  const size_t mp = an.max_npiv;
  h->lds_panel = (PS_LD * mp + 1 + 2 * mp) * sizeof(double) + mp * sizeof(int);
  h->lds_bwdb = ((size_t)an.max_nbor + 2) * sizeof(double);
  const size_t lds_blk = fb_lds_bytes((int)mp);
  if (h->lds_bwdb > 160 * 1024 || lds_blk > 160 * 1024) return HQPKKT_E_MEM;
  for (int w = 0; w < 2; w++) {
    const Analysis::Sched &S = an.sched[w];
    h->level_maxp[w].assign(an.nlevels, 0), h->level_maxb[w].assign(an.nlevels, 0);
    for (int l = 0; l < an.nlevels && S.nnodes; l++)
      for (int q = S.level_ptr[l] + S.level_fsmall[l] + S.level_small[l]; q < S.level_ptr[l + 1]; q++) {
        h->level_maxp[w][l] = std::max(h->level_maxp[w][l], an.npiv[S.level_nodes[q]]);
        h->level_maxb[w][l] = std::max(h->level_maxb[w][l], an.nbor[S.level_nodes[q]]);
      }
  }
  {  // the counters of the polled exchanges: [0] solves, [1] factorisations so far (k_rhs_*, the assembly kernels count)
    std::vector<int> two(2, 0);
    if ((e = h->td.tree_words.upload(two))) return e;
  }
  {  // tries before a poll gives up (HQPKKT_POLL_LIMIT: a test hook that forces the fall-back of poll_fallback)
    const char *pl = getenv("HQPKKT_POLL_LIMIT");
    const int lim = pl ? atoi(pl) : 1 << 20;
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(xw_poll_limit), &lim, sizeof(int)));
    const double spp = 1e-6;  // (kernels.hip.h, soft_pivot_pert)
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(soft_pivot_pert), &spp, sizeof(double)));
  }
  // a tree of small fronts only: whole-tree sweeps
  h->small_tree = false, h->tree_factor = false;
  if (!getenv("HQPKKT_NO_TREE_SWEEPS") && !h->no_polled && an.shard_count == 1 && an.sched[0].nnodes > 1 && an.sched[1].nnodes == 0) {
    const Analysis::Sched &S = an.sched[0];
    bool all = true;
    for (int l = 0; l < an.nlevels && all; l++) all = S.level_fsmall[l] == S.level_ptr[l + 1] - S.level_ptr[l];
    if (all) {
      std::vector<int> down, one(2, 0);
      for (int l = an.nlevels - 1; l >= 0; l--)
        for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) down.push_back(S.level_nodes[q]);
      if ((e = h->td.tree_down.upload(down)) || (e = h->td.tree_x.alloc(2 * (size_t)(an.cb_elems + an.dim)))) return e;
      h->small_tree = true;
      h->tree_factor = !an.upd_pingpong;
      if (h->tree_factor && (e = h->td.tree_u.alloc(2 * (size_t)std::max<long long>(an.upd_elems, 1)))) return e;
      if ((e = reset_solve_top(h))) return e;
    }
  }
  // the fused top of the solve sweeps: the highest levels whose fronts all fit one instance of k_solve_top, at most
  // ST_MAXFRONTS fronts (single rank: with a sharded tree the two sweeps of a schedule are not adjacent)
  h->top_n = 0, h->top_lt = 1 << 30, h->top_lds = 0;
  if (!getenv("HQPKKT_NO_SOLVE_TOP") && !h->no_polled && an.shard_count == 1 && an.sched[0].nnodes > 0) {
    const Analysis::Sched &S = an.sched[0];
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
    if (an.nlevels - lt >= 2 && cnt >= 2) {
      std::vector<int> nodes, idx(an.nnodes, -1), owner(an.dim, -1);
      for (int l = an.nlevels - 1; l >= lt; l--)
        for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) idx[S.level_nodes[q]] = (int)nodes.size(), nodes.push_back(S.level_nodes[q]);
      for (size_t t = 0; t < nodes.size(); t++)
        for (int k = 0; k < an.npiv[nodes[t]]; k++) owner[an.piv_start[nodes[t]] + k] = (int)t;
      std::vector<int> bpos(nodes.size() * ST_CS, 0);
      for (size_t t = 0; t < nodes.size(); t++)
        for (int i = 0; i < an.nbor[nodes[t]]; i++) {
          const int ei = an.bidx[an.bptr[nodes[t]] + i], o = owner[ei];
          if (o < 0) return HQPKKT_E_INTERN;  // (a border row of a fused front belongs to a fused ancestor)
          bpos[t * ST_CS + i] = o * ST_XS + (ei - an.piv_start[nodes[o]]);
        }
      std::vector<int> up;  // level by level, leaves first; inside a level the largest fronts first, as in `nodes`
      for (int l = lt; l < an.nlevels; l++)
        for (int q = S.level_ptr[l]; q < S.level_ptr[l + 1]; q++) up.push_back(S.level_nodes[q]);
      // One launch for both sweeps needs ALL its fronts resident at once (the forward sweep of a front waits for
      // fronts behind it in the launch): safe only while nothing else competes for the CUs.  Several systems in flight
      // on one GPU (bench.py's concurrent systems, scenario trees) could starve each other, so the form in use is the
      // split one - a front waits only for fronts before it - and the fused launch is an option (HQPKKT_SOLVE_TOP_FUSED,
      // 17 us less per solve: M and L21 are read once).
      h->top_split = (int)nodes.size() > ST_MAXFRONTS || getenv("HQPKKT_SOLVE_TOP_FUSED") == nullptr;
      if ((e = h->td.top_nodes.upload(nodes)) || (e = h->td.top_idx.upload(idx)) || (e = h->td.top_bpos.upload(bpos)) || (e = h->td.top_up.upload(up)) ||
          (e = h->td.top_x.alloc(2 * nodes.size() * (size_t)(ST_CS + ST_XS))))
        return e;
      h->top_n = (int)nodes.size(), h->top_lt = lt, h->top_ns = ok3 ? 3 : 4, h->top_lds = st_top_lds_bytes(maxp, h->top_ns);
      if ((e = reset_solve_top(h))) return e;
    }
  }
  {
    // the attribute is state of the PROCESS, not of the handle: a second handle with smaller fronts must
    // not lower the limit under one that still launches with more (several plugins in one host, the
    // bench's concurrent systems): keep the largest value ever asked for, under a mutex
    // ... and hipFuncSetAttribute acts on the CURRENT device: the largest values are kept per device
    static std::mutex attr_mutex;
    struct PerDev { size_t panel = 0, bwdb = 0, blk = 0, top = 0; };
    static PerDev per_dev[64];
    if (h->opts.device < 0 || h->opts.device >= 64) return HQPKKT_E_RANGE;
    std::lock_guard<std::mutex> lk(attr_mutex);
    size_t &a_panel = per_dev[h->opts.device].panel, &a_bwdb = per_dev[h->opts.device].bwdb,
           &a_blk = per_dev[h->opts.device].blk, &a_top = per_dev[h->opts.device].top;
    if (h->top_lds > a_top) {
      const int l3 = (int)std::min(h->top_lds, st_top_lds_bytes(176, 3)), l4 = (int)std::min(h->top_lds, st_top_lds_bytes(160, 4));
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_top<3, 11, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, l3));
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_top<3, 11, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, l3));
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_top<3, 11, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, l3));
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_top<4, 10, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, l4));
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_top<4, 10, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, l4));
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_top<4, 10, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, l4));
      a_top = h->top_lds;
    }
    if (lds_blk > a_blk) {
      HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<8, 6, 144, 2, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min(lds_blk, fb_lds_bytes(128))));
      HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<12, 8, 208, 3, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_blk));
      HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<12, 6, 208, 3, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min(lds_blk, fb_lds_bytes(176))));
      HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<12, FB_NS160, 208, 3, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::min(lds_blk, fb_lds_bytes(160))));
      a_blk = lds_blk;
    }
    if (h->lds_panel > a_panel) {
      HIPCHK(hipFuncSetAttribute((const void *)k_panel_solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_panel));
      a_panel = h->lds_panel;
    }
    if (h->lds_bwdb > a_bwdb) {
      HIPCHK(hipFuncSetAttribute((const void *)k_solve_bwd_b, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bwdb));
      a_bwdb = h->lds_bwdb;
    }
  }
  {
    const double rows = 2.0 * n + me + m;  // Q, A', C' per x row; A, C rows
    const double nnz = (double)an.Qfull.col.size() + 2.0 * an.A.col.size() + 2.0 * an.C.col.size();
    h->short_rows = rows > 0 && nnz / rows < 8.0;
  }
  h->st.bytes_panels = (long long)sizeof(double) * (an.panel_elems + an.x_elems);
  h->st.bytes_updates = (long long)sizeof(double) * an.upd_elems;
  h->uploaded = true;
  return 0;
}


// (HQPKKT_NO_HOST_KERNEL_COPIES=1: the copy engine as before, for same-box comparisons)
static bool host_kernel_copies(const hqpkkt_t *) {
  return getenv("HQPKKT_NO_HOST_KERNEL_COPIES") == nullptr;
}
// A call with host vectors as one graph (hqpkkt::ghost_factor / ghost_step): the tree engine on one GPU, vectors that
// fit the pinned staging buffer.  (HQPKKT_NO_HOST_GRAPHS=1: launch by launch.)
bool host_graphs_ok(const hqpkkt_t *h) {
  return getenv("HQPKKT_NO_HOST_GRAPHS") == nullptr && host_kernel_copies(h) && !h->lazy && h->opts.loc != HQPKKT_LOC_DEVICE && h->td.hstage_in && h->td.hstage.dev && h->use_graphs &&
         !h->prof.on && h->opts.mode != HQPKKT_MODE_STAGED && h->an.shard_count <= 1;
}
// the caller's vectors packed into the pinned buffer by the CPU (stage_in's layout); returns the doubles in use
size_t stage_pack(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3, const double *r4) {
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  double *q = h->td.hstage.p;
  const double *src[6] = {z, w, r1, r2, r3, r4};
  const int len[6] = {m, m, n, me, m, m};
  size_t used = 0, off = 0;
  for (int k = 0; k < 6; k++) {
    if (src[k] && len[k] > 0) std::memcpy(q + off, src[k], sizeof(double) * len[k]), used = off + len[k];
    off += len[k];
  }
  return used;
}
int stage_in(hqpkkt_t *h, const double *z, const double *w, const double *r1,
             const double *r2, const double *r3, const double *r4, Vecs &v) {
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  double *b = h->td.vin.p;
  double *dz_ = b, *dw_ = b + m, *d1 = b + 2 * (size_t)m, *d2 = d1 + n, *d3 = d2 + me, *d4 = d3 + m;
  if (h->opts.loc == HQPKKT_LOC_DEVICE) {
    CopyList L{{z, w, r1, r2, r3, r4}, {dz_, dw_, d1, d2, d3, d4}, {m, m, n, me, m, m}};
    k_copy_vectors<<<copy_blocks(L), 256, 0, h->stream>>>(L, 6);
  } else if (h->td.hstage_in) {
    // packed by the CPU; the prefix up to the last vector the caller passes
    double *q = h->td.hstage.p;
    const double *src[6] = {z, w, r1, r2, r3, r4};
    const int len[6] = {m, m, n, me, m, m};
    size_t used = 0, off = 0;
    for (int k = 0; k < 6; k++) {
      if (src[k] && len[k] > 0) std::memcpy(q + off, src[k], sizeof(double) * len[k]), used = off + len[k];
      off += len[k];
    }
    if (used && h->td.hstage.dev && host_kernel_copies(h)) {  // read out of the pinned buffer by a kernel: no copy engine in the chain
      CopyList L{{h->td.hstage.dev, nullptr, nullptr, nullptr, nullptr, nullptr}, {b, nullptr, nullptr, nullptr, nullptr, nullptr}, {(int)used, 0, 0, 0, 0, 0}};
      k_copy_vectors<<<copy_blocks(L), 256, 0, h->stream>>>(L, 1);
    } else if (used)
      HIPCHK(hipMemcpyAsync(b, q, sizeof(double) * used, hipMemcpyHostToDevice, h->stream));
  } else {
#define H2D(dst, src, k) \
  if ((src) && (k) > 0) HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * (k), hipMemcpyHostToDevice, h->stream))
    H2D(dz_, z, m);
    H2D(dw_, w, m);
    H2D(d1, r1, n);
    H2D(d2, r2, me);
    H2D(d3, r3, m);
    H2D(d4, r4, m);
#undef H2D
  }
  v.z = dz_, v.w = dw_, v.r1 = d1, v.r2 = d2, v.r3 = d3, v.r4 = d4;
  return 0;
}

void stage_out_ptrs(hqpkkt_t *h, Vecs &v) {
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  v.dx = h->td.vout.p, v.dy = v.dx + n, v.dz = v.dy + me, v.dw = v.dz + m;
}

int stage_out(hqpkkt_t *h, const Vecs &v, double *dx, double *dy, double *dz, double *dw) {
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  if (h->opts.loc == HQPKKT_LOC_DEVICE) {
    CopyList L{{v.dx, v.dy, v.dz, v.dw, nullptr, nullptr}, {dx, dy, dz, dw, nullptr, nullptr}, {n, me, m, m, 0, 0}};
    k_copy_vectors<<<copy_blocks(L), 256, 0, h->stream>>>(L, 4);
    return 0;
  }
  if (h->td.hstage_out) {  // one transfer into pinned memory; unstage() hands it out after the sync
    if (h->td.hstage.dev && host_kernel_copies(h)) {  // ... written by a kernel (coherent host memory: there when the next kernel of the stream starts)
      CopyList L{{v.dx, nullptr, nullptr, nullptr, nullptr, nullptr}, {h->td.hstage.dev + h->td.hstage_in, nullptr, nullptr, nullptr, nullptr, nullptr}, {(int)h->td.hstage_out, 0, 0, 0, 0, 0}};
      k_copy_vectors<<<copy_blocks(L), 256, 0, h->stream>>>(L, 1);
      h->out_by_kernel = true;
    } else {
      HIPCHK(hipMemcpyAsync(h->td.hstage.p + h->td.hstage_in, v.dx, sizeof(double) * h->td.hstage_out, hipMemcpyDeviceToHost,
                            h->stream));
      h->out_by_kernel = false;
    }
    h->out_pending = h->td.hstage.p + h->td.hstage_in;
    return 0;
  }
#define D2H(dst, src, k) \
  if ((dst) && (k) > 0) HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * (k), hipMemcpyDeviceToHost, h->stream))
  D2H(dx, v.dx, n);
  D2H(dy, v.dy, me);
  D2H(dz, v.dz, m);
  D2H(dw, v.dw, m);
#undef D2H
  return 0;
}

// after the stream has been drained: the packed results to the caller's vectors
void unstage(hqpkkt_t *h, double *dx, double *dy, double *dz, double *dw) {
  if (!h->out_pending) return;
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  const double *q = h->out_pending;
  h->out_pending = nullptr;
  if (dx && n) std::memcpy(dx, q, sizeof(double) * n);
  if (dy && me) std::memcpy(dy, q + n, sizeof(double) * me);
  if (dz && m) std::memcpy(dz, q + n + me, sizeof(double) * m);
  if (dw && m) std::memcpy(dw, q + n + me + m, sizeof(double) * m);
}

static const int FWD_FUSED_MAX_SLABS = 1024;  // above: forward step of a level in two launches
static const int SU1_MAX = 768;  // levels of at most this many 64 x 64 update tiles run k_schur_update with 32 x 16 per wave
static_assert(FS_MAXP == kktdev::SMALL_PIVOTS && FS_MAXB == kktdev::SMALL_BORDER, "small-supernode kernels and schedule disagree");
// ------------------------------------------------------------ numeric phases
// phases: 1 = assemble + this rank's subtrees, 2 = replicated top of the tree
// (3 = everything, the single-rank case)
// (HQPKKT_NO_FUSED_VECTORS=1: the vector work around the sweeps and the assembly as the separate launches of round 5 - the
// comparison the bit-identity test makes)
static bool no_fused_vectors() { return getenv("HQPKKT_NO_FUSED_VECTORS") != nullptr; }
static int run_factor(hqpkkt_t *h, const double *z, const double *w, int phases) {
  Analysis &an = h->an;
  hipStream_t s = h->stream;
  const int m = an.m, nent = (int)an.ent_a.size();
  DevTree T = h->td.tree();
  if (phases & 1) {
    if (an.shard_count <= 1) {  // the panel arena, and the status words, counters and the two maxima
      KLAUNCH(h, KC_ASSEMBLE, k_clear<<<(int)std::max<long long>(1, std::min<long long>(2048, (an.panel_elems / 2 + 1023) / 1024)), 256, 0, s>>>(h->td.panel.p, an.panel_elems, h->td.flags.p));
    } else {  // only the blocks this rank writes
      const int np = (int)an.zero_panel.size() / 2;
      if (np) k_zero_ranges<<<dim3(512, np), 256, 0, s>>>(h->td.panel.p, h->td.zero_panel.p);
      k_clear<<<1, 256, 0, s>>>(nullptr, 0, h->td.flags.p);
    }
    if (!h->capturing) HIPCHK(hipEventRecord(h->ev0, s));
    if (m > 0 && (h->td.simple_src.count || no_fused_vectors()))
      KLAUNCH(h, KC_ASSEMBLE, k_weights<<<nblk(m), 256, 0, s>>>(an.mode, m, an.n + an.me, z, w, h->td.wt.p, h->td.sc.p, h->td.flags.p));
    if (h->td.simple_src.count) {  // FULL: one pass
      KLAUNCH(h, KC_ASSEMBLE, k_assemble_simple<<<std::min(nblk(nent), 2048), 256, 0, s>>>(
                                  nent, h->td.simple_src.p, h->td.simple_wi.p, h->td.ent_a.p, h->td.ent_b.p, h->td.ent_dst.p,
                                  h->td.vals.p, h->td.wt.p, h->td.sc.p, h->td.panel.p, h->td.bits.p, h->td.tree_words.p + 1));
    } else {
      // weights + entry values, scales + scatter: one launch each (kernels.hip.h, k_wt_entry / k_scale_scatter)
      if (no_fused_vectors()) {
        KLAUNCH(h, KC_ASSEMBLE, k_entry_values<<<nblk(nent), 256, 0, s>>>(nent, h->td.term_ptr.p, h->td.terms.p, h->td.vals.p, h->td.wt.p,
                                                  h->td.ent_val.p, h->td.tree_words.p + 1));
        if (an.mode == 1 && an.n > 0)
          KLAUNCH(h, KC_ASSEMBLE, k_red_scale<<<nblk(an.n), 256, 0, s>>>(an.n, h->td.diag_ent.p, h->td.ent_val.p, h->td.sc.p));
        KLAUNCH(h, KC_ASSEMBLE, k_scatter<<<std::min(nblk(nent), 2048), 256, 0, s>>>(nent, h->td.ent_a.p, h->td.ent_b.p, h->td.ent_dst.p, h->td.ent_val.p,
                                             h->td.sc.p, h->td.panel.p, h->td.bits.p));
      } else {
      KLAUNCH(h, KC_ASSEMBLE, k_wt_entry<<<nblk(nent) + (m > 0 ? nblk(m) : 0), 256, 0, s>>>(an.mode, m, an.n + an.me, nent, nblk(nent), z, w, h->td.wt.p, h->td.sc.p,
                                                h->td.flags.p, h->td.term_ptr.p, h->td.terms.p, h->td.vals.p, h->td.ent_val.p, h->td.tree_words.p + 1));
      const int nsc = std::min(nblk(nent), 2048);
      if (an.mode == 1 && an.n > 0)
        KLAUNCH(h, KC_ASSEMBLE, k_scale_scatter<<<nsc + nblk(an.n), 256, 0, s>>>(an.n, nent, nsc, h->td.diag_ent.p, h->td.ent_a.p, h->td.ent_b.p, h->td.ent_dst.p,
                                                 h->td.ent_val.p, h->td.sc.p, h->td.panel.p, h->td.bits.p));
      else
        KLAUNCH(h, KC_ASSEMBLE, k_scatter<<<nsc, 256, 0, s>>>(nent, h->td.ent_a.p, h->td.ent_b.p, h->td.ent_dst.p, h->td.ent_val.p,
                                             h->td.sc.p, h->td.panel.p, h->td.bits.p));
      }
    }
    if (!h->capturing) HIPCHK(hipEventRecord(h->ev1, s));
  }
  const double alpha = h->opts.tol * 0.6403882032022076;  // tol (1+sqrt 17)/8, hqp/spBKP.C:392
  for (int which = 0; which < 2; which++) {
    if (!(phases & (1 << which))) continue;
    const Analysis::Sched &S = an.sched[which];
    const TreeDev::DevSched &D = h->td.ds[which];
    if (S.nnodes == 0) continue;
    const TreeXchgF txf{h->td.tree_u.p, an.upd_elems, h->td.tree_words.p + 1};
    if (which == 0 && h->tree_factor) {  // a tree of small fronts: all levels in one launch
      int ldp = 1, ldb = 1;
      for (int l = 0; l < an.nlevels; l++) ldp = std::max(ldp, S.level_fs_p[l] | 1), ldb = std::max(ldb, S.level_fs_b[l]);
      KLAUNCH(h, KC_FACTOR_DIAG, (k_factor_diag_small<true, true><<<S.nnodes, 64, fs_lds_bytes(true, ldp, ldb), s>>>(T, D.level_nodes.p, h->td.panel.p,
                                               h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                               h->td.flags.p + 1, h->td.upd.p, h->td.xar.p, ldp, ldb, txf)));
      continue;
    }
    for (int l = 0; l < an.nlevels; l++) {
      const int nn = S.level_ptr[l + 1] - S.level_ptr[l], nfs = S.level_fsmall[l], nsm = S.level_small[l];
      if (nfs > 0) {  // small fronts: extend-add, pivot block, panel and update in one kernel
        const int ldp = S.level_fs_p[l] | 1, ldb = S.level_fs_b[l];
        KLAUNCH(h, KC_FACTOR_DIAG, k_factor_diag_small<true><<<nfs, 64, fs_lds_bytes(true, ldp, ldb), s>>>(T, D.level_nodes.p + S.level_ptr[l], h->td.panel.p,
                                                 h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                                 h->td.flags.p + 1, h->td.upd.p, h->td.xar.p, ldp, ldb, txf));
      }
      if (nsm > 0) {
        const int ldp = S.level_sm_p[l] | 1;
        KLAUNCH(h, KC_FACTOR_DIAG, k_factor_diag_small<false><<<nsm, 64, fs_lds_bytes(false, ldp, 1), s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs, h->td.panel.p,
                                                 h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                                 h->td.flags.p + 1, h->td.upd.p, h->td.xar.p, ldp, 1, txf));
      }
      if (nn > nfs + nsm) {
        // the pivot blocks on the matrix pipe: 8 wavefronts (two workgroups per CU) for levels of <= 128 pivots, 12
        // wavefronts beyond, each holding as many 16 x 16 blocks of the triangle as the level's largest front needs
        const int lmp = h->level_maxp[which][l];
        if (lmp <= 128)
          KLAUNCH(h, KC_FACTOR_DIAG, (k_factor_blk<8, 6, 144, 2, FB_OWNSIMD><<<nn - nfs - nsm, 512, fb_lds_bytes(lmp), s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs + nsm, h->td.panel.p,
                                                 h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                                 h->td.flags.p + 1, h->td.upd.p)));
        else if (lmp <= 160)  // (55 blocks on 11 wavefronts: five per wavefront)
          KLAUNCH(h, KC_FACTOR_DIAG, (k_factor_blk<12, FB_NS160, 208, 3, FB_OWNSIMD><<<nn - nfs - nsm, 768, fb_lds_bytes(lmp), s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs + nsm, h->td.panel.p,
                                                 h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                                 h->td.flags.p + 1, h->td.upd.p)));
        else if (lmp <= 176)  // (66 blocks of the triangle on 11 wavefronts: six per wavefront - 16 registers fewer than with eight, no scratch)
          KLAUNCH(h, KC_FACTOR_DIAG, (k_factor_blk<12, 6, 208, 3, FB_OWNSIMD><<<nn - nfs - nsm, 768, fb_lds_bytes(lmp), s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs + nsm, h->td.panel.p,
                                                 h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                                 h->td.flags.p + 1, h->td.upd.p)));
        else
          KLAUNCH(h, KC_FACTOR_DIAG, (k_factor_blk<12, 8, 208, 3, FB_OWNSIMD><<<nn - nfs - nsm, 768, fb_lds_bytes(lmp), s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs + nsm, h->td.panel.p,
                                                 h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p, alpha, h->opts.pivot_eps, h->td.bits.p,
                                                 h->td.flags.p + 1, h->td.upd.p)));
      }
      const int ns = S.slab_ptr[l + 1] - S.slab_ptr[l];
      // the work lists go over the XCDs in chunks of about half a front's items (kernels.hip.h, xcd_order; measured on C2:
      // 1.875 -> 1.826 ms per factor + solve; whole fronts per chunk 1.830, contiguous ranges per XCD 1.915)
      const int lmb = h->level_maxb[which][l];
      const int xps = std::max(1, (lmb + 31) / 32);
      const int xtt = (lmb + 63) / 64, xsu = std::max(1, xtt * (xtt + 1) / 4);
      if (ns > 0)  // (the schedule lists 32-row slabs; the kernel takes 16 rows per workgroup)
        KLAUNCH(h, KC_PANEL_SOLVE, k_panel_solve<<<2 * ns, 256, h->lds_panel, s>>>(T, D.slabs.p + 2 * (size_t)S.slab_ptr[l],
                                                    h->td.panel.p, h->td.xar.p, h->td.dinv.p, h->td.ptype.p,
                                                    h->td.lperm.p, h->td.linv.p, h->td.linv_off.p, h->td.upd.p, xps));
      const int nt = S.upd_big_ptr[l] - S.upd_tile_ptr[l], ntb = S.upd_tile_ptr[l + 1] - S.upd_big_ptr[l];
      // a wave holds 32 x 32 of a tile while a level fills the chip; 32 x 16 (two workgroups per tile) on the thin levels above
      if (nt > 0 && nt > SU1_MAX)
        KLAUNCH(h, KC_SCHUR_UPDATE, k_schur_update<2><<<nt, 256, 0, s>>>(T, D.upd_tiles.p + 3 * (size_t)S.upd_tile_ptr[l],
                                          h->td.panel.p, h->td.xar.p, h->td.upd.p, xsu));
      else if (nt > 0)
        KLAUNCH(h, KC_SCHUR_UPDATE, k_schur_update<1><<<2 * nt, 256, 0, s>>>(T, D.upd_tiles.p + 3 * (size_t)S.upd_tile_ptr[l],
                                          h->td.panel.p, h->td.xar.p, h->td.upd.p, 2 * xsu));
      if (ntb > 0)
        KLAUNCH(h, KC_SCHUR_UPDATE, (k_schur_update_big<2, 2, 4, 4, 2, 2><<<ntb, 256, 0, s>>>(T, D.upd_tiles.p + 3 * (size_t)S.upd_big_ptr[l],
                                          h->td.panel.p, h->td.xar.p, h->td.upd.p)));
    }
  }
  if (!h->capturing) HIPCHK(hipEventRecord(h->evs1, s));
  HIPCHK(hipGetLastError());
  return 0;
}

// phases: 1 = right-hand side + forward sweep over this rank's subtrees,
// 2 = forward / backward over the replicated top, backward over the subtrees,
// 4 = unscale + scatter of the solution (7 = everything, the single-rank case)
static int run_step(hqpkkt_t *h, const Vecs &v, int phases) {
  Analysis &an = h->an;
  hipStream_t s = h->stream;
  const int n = an.n, me = an.me, m = an.m, dim = an.dim;
  DevTree T = h->td.tree();
  auto forward = [&](int which) -> int {
    const Analysis::Sched &S = an.sched[which];
    const TreeDev::DevSched &D = h->td.ds[which];
    const TreeXchg tx{h->td.tree_x.p, h->td.tree_x.p + 2 * an.cb_elems, an.cb_elems, an.dim, h->td.tree_words.p, h->td.flags.p};
    if (which == 0 && h->small_tree) {  // all levels in one launch
      KLAUNCH(h, KC_SOLVE_FWD,
              k_solve_fwd_small<true><<<S.nnodes, 64, 0, s>>>(T, D.level_nodes.p, h->td.panel.p, h->td.linv.p, h->td.linv_off.p, h->td.dinv.p, h->td.ptype.p,
                                                              h->td.lperm.p, h->td.rhs.p, h->td.xsol.p, h->td.ytmp.p, h->td.cb.p, tx));
      return 0;
    }
    const int lend = which == 0 && h->top_n > 0 ? h->top_lt : an.nlevels;  // (the levels above: k_solve_top)
    for (int l = 0; l < lend && S.nnodes; l++) {
      const int nn = S.level_ptr[l + 1] - S.level_ptr[l], nfs = S.level_fsmall[l];
      if (nfs > 0)
        KLAUNCH(h, KC_SOLVE_FWD,
                k_solve_fwd_small<false><<<nfs, 64, 0, s>>>(T, D.level_nodes.p + S.level_ptr[l], h->td.panel.p, h->td.linv.p,
                                                     h->td.linv_off.p, h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.rhs.p,
                                                     h->td.xsol.p, h->td.ytmp.p, h->td.cb.p, tx));
      const int ng = S.gslab_ptr[l + 1] - S.gslab_ptr[l];  // (front, 64-row slab), at least one per front
      if (ng > 0 && ng <= FWD_FUSED_MAX_SLABS)  // a handful of fronts: the launch is what costs
        KLAUNCH(h, KC_SOLVE_FWD,
                k_solve_fwd<<<ng, 256, 0, s>>>(T, D.gslabs.p + 2 * (size_t)S.gslab_ptr[l], h->td.panel.p, h->td.linv.p,
                                               h->td.linv_off.p, h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.rhs.p,
                                               h->td.xsol.p, h->td.ytmp.p, h->td.cb.p));
      else if (ng > 0) {  // thousands of slabs: M once per front, then the slabs
        KLAUNCH(h, KC_SOLVE_FWD,
                k_solve_fwd_a<<<nn - nfs, 256, 0, s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs, h->td.linv.p,
                                                 h->td.linv_off.p, h->td.dinv.p, h->td.ptype.p, h->td.lperm.p,
                                                 h->td.rhs.p, h->td.xsol.p, h->td.ytmp.p, h->td.cb.p));
        KLAUNCH(h, KC_SOLVE_FWD,
                k_solve_fwd_b<<<ng, 256, 0, s>>>(T, D.gslabs.p + 2 * (size_t)S.gslab_ptr[l], h->td.panel.p,
                                                 h->td.ytmp.p, h->td.cb.p));
      }
    }
    return 0;
  };
  auto backward = [&](int which) -> int {
    const Analysis::Sched &S = an.sched[which];
    const TreeDev::DevSched &D = h->td.ds[which];
    const TreeXchg tx{h->td.tree_x.p, h->td.tree_x.p + 2 * an.cb_elems, an.cb_elems, an.dim, h->td.tree_words.p, h->td.flags.p};
    if (which == 0 && h->small_tree) {
      KLAUNCH(h, KC_SOLVE_BWD, k_solve_bwd_small<true><<<S.nnodes, 64, 0, s>>>(T, h->td.tree_down.p, h->td.panel.p, h->td.linv.p, h->td.linv_off.p, h->td.lperm.p,
                                                                               h->td.xsol.p, tx));
      return 0;
    }
    const int lbeg = which == 0 && h->top_n > 0 ? h->top_lt - 1 : an.nlevels - 1;
    for (int l = lbeg; l >= 0 && S.nnodes; l--) {
      const int nn = S.level_ptr[l + 1] - S.level_ptr[l], nfs = S.level_fsmall[l];
      const int ncb = S.cblk_ptr[l + 1] - S.cblk_ptr[l];
      if (nn <= 0) continue;
      if (nfs > 0)
        KLAUNCH(h, KC_SOLVE_BWD,
                k_solve_bwd_small<false><<<nfs, 64, 0, s>>>(T, D.level_nodes.p + S.level_ptr[l], h->td.panel.p, h->td.linv.p,
                                                     h->td.linv_off.p, h->td.lperm.p, h->td.xsol.p, tx));
      if (nn <= nfs) continue;
      // (one workgroup per front doing both steps was measured slower: L21' x needs the
      // column blocks spread over the chip)
      KLAUNCH(h, KC_SOLVE_BWD,
              k_solve_bwd_b<<<ncb, 256, h->lds_bwdb, s>>>(T, D.cblks.p + 2 * (size_t)S.cblk_ptr[l],
                                                          h->td.panel.p, h->td.xsol.p, h->td.vtmp.p));
      KLAUNCH(h, KC_SOLVE_BWD,
              k_solve_bwd_a<<<nn - nfs, 256, 0, s>>>(T, D.level_nodes.p + S.level_ptr[l] + nfs, h->td.linv.p,
                                               h->td.linv_off.p, h->td.lperm.p, h->td.vtmp.p, h->td.xsol.p));
    }
    return 0;
  };
  if (phases & 1) {
    if (an.mode == 0) {
      KLAUNCH(h, KC_VECTOR, k_rhs_full<<<nblk(dim), 256, 0, s>>>(n, me, m, h->td.q2e.p, h->td.sc.p, v.z, v.r1, v.r2, v.r3, v.r4,
                                           h->td.rhs.p, h->td.tree_words.p));
    } else {
      // (tz and the right-hand side that needs it in one launch: kernels.hip.h, k_rhs_red_t; HQPKKT_NO_FUSED_VECTORS=1: two)
      if (no_fused_vectors()) {
        if (m > 0) KLAUNCH(h, KC_VECTOR, k_red_t<<<nblk(m), 256, 0, s>>>(m, v.w, h->td.wt.p, v.r3, v.r4, h->td.tz.p));
        KLAUNCH(h, KC_VECTOR, k_rhs_red<<<nblk(dim), 256, 0, s>>>(n, me, h->td.q2e.p, h->td.sc.p, h->td.CT.ptr.p, h->td.CT.col.p,
                                            h->td.CT.src.p, h->td.vals.p, h->td.tz.p, v.r1, v.r2, h->td.rhs.p,
                                            h->td.tree_words.p));
      } else
        KLAUNCH(h, KC_VECTOR, k_rhs_red_t<<<nblk(dim) + (m > 0 ? nblk(m) : 0), 256, 0, s>>>(n, me, m, nblk(dim), h->td.q2e.p, h->td.sc.p, h->td.CT.ptr.p, h->td.CT.col.p,
                                            h->td.CT.src.p, h->td.vals.p, v.w, h->td.wt.p, v.r3, v.r4, h->td.tz.p, v.r1, v.r2, h->td.rhs.p,
                                            h->td.tree_words.p));
    }
    forward(0);
  }
  if (phases & 2) {
    forward(1);
    if (h->top_n > 0) {  // the top levels, up and down: one launch, or one per sweep (k_solve_top)
      TopArgs ta{h->td.top_nodes.p, h->td.top_idx.p, h->td.top_bpos.p, h->td.top_x.p, h->td.top_x.p + 2 * (size_t)h->top_n * ST_CS, h->td.tree_words.p, h->top_n, h->top_stamps};
#define TOP_LAUNCH(NS, NU, MODE)                                                                                                          \
  KLAUNCH(h, KC_SOLVE_TOP, (k_solve_top<NS, NU, MODE><<<h->top_n, ST_THREADS, h->top_lds, s>>>(T, ta, h->td.panel.p, h->td.linv.p, h->td.linv_off.p, \
                                                            h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.rhs.p, h->td.xsol.p, h->td.cb.p, h->td.flags.p)))
      if (!h->top_split) {
        if (h->top_ns == 3) TOP_LAUNCH(3, 11, 0); else TOP_LAUNCH(4, 10, 0);
      } else {
        ta.nodes = h->td.top_up.p;
        if (h->top_ns == 3) TOP_LAUNCH(3, 11, 1); else TOP_LAUNCH(4, 10, 1);
        ta.nodes = h->td.top_nodes.p;
        if (h->top_ns == 3) TOP_LAUNCH(3, 11, 2); else TOP_LAUNCH(4, 10, 2);
      }
#undef TOP_LAUNCH
    }
    backward(1);
    backward(0);
    if (an.shard_count > 1)  // leave only this rank's share for the all-reduce
      KLAUNCH(h, KC_VECTOR, k_mask_vector<<<nblk(dim), 256, 0, s>>>(dim, h->td.keep_e.p, h->td.xsol.p));
  }
  if (phases & 4) {
    if (an.mode == 0) {
      KLAUNCH(h, KC_VECTOR, k_unpack_full<<<nblk(dim), 256, 0, s>>>(n, me, m, h->td.q2e.p, h->td.sc.p, h->td.xsol.p, v.dx, v.dy,
                                              v.dz));
      if (m > 0)
        KLAUNCH(h, KC_VECTOR, k_dw<<<nblk(m), 256, 0, s>>>(m, h->td.C.ptr.p, h->td.C.col.p, h->td.C.src.p, h->td.vals.p, v.dx, v.r3,
                                     v.z, v.w, v.r4, v.dz, v.dw));
    } else {
      // (dx, dy and the dz, dw that need dx in one launch: kernels.hip.h, k_unpack_dzdw)
      const int nb_dzdw = m > 0 ? nblk(m) : 0;
      if (no_fused_vectors()) {
        KLAUNCH(h, KC_VECTOR, k_unpack_red<<<nblk(dim), 256, 0, s>>>(n, me, h->td.q2e.p, h->td.sc.p, h->td.xsol.p, v.dx, v.dy));
        if (m > 0)
          KLAUNCH(h, KC_VECTOR, k_red_dzdw<<<nblk(m), 256, 0, s>>>(m, h->td.C.ptr.p, h->td.C.col.p, h->td.C.src.p, h->td.vals.p, v.dx,
                                             h->td.wt.p, h->td.tz.p, v.r3, v.dz, v.dw));
      } else
      KLAUNCH(h, KC_VECTOR, k_unpack_dzdw<<<nb_dzdw + nblk(dim), 256, 0, s>>>(n, me, m, nb_dzdw, h->td.q2e.p, h->td.sc.p, h->td.xsol.p, v.dx, v.dy, h->td.C.ptr.p,
                                           h->td.C.col.p, h->td.C.src.p, h->td.vals.p, h->td.wt.p, h->td.tz.p, v.r3, v.dz, v.dw));
    }
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The exchange steps of a sharded system: the handle's stream is
// drained, the caller's collective runs, and the next phase starts afterwards.
int exchange(hqpkkt_t *h, int op, double *buf, long long slot, int nslots, hipStream_t on) {
  // (profiled as the class "exchange": in the stream-ordered form the time between the collective's place in
  // the stream and its completion - the wait for the slowest rank and the transfer)
  if (h->listing) return 0;
  if (h->xchg_sfn) {  // the collective is put into the handle's stream (or `on`) behind the kernels that fill `buf`
    hipStream_t st = on ? on : h->stream;
    h->prof.begin(KC_XCHG, st);
    const int rc = h->xchg_sfn(h->xchg_ctx, op, buf, slot, nslots, (void *)st);
    h->prof.end(st);
    return rc ? HQPKKT_E_DEVICE : 0;
  }
  if (!h->xchg_fn) return HQPKKT_E_INTERN;
  h->prof.begin(KC_XCHG, h->stream);
  HIPCHK(hipStreamSynchronize(h->stream));
  const int rc = h->xchg_fn(h->xchg_ctx, op, buf, slot, nslots);
  h->prof.end(h->stream);
  return rc ? HQPKKT_E_DEVICE : 0;
}

int do_factor(hqpkkt_t *h, const Vecs &v) {
  Analysis &an = h->an;
  int e;
  if (h->opts.mode == HQPKKT_MODE_STAGED) return staged_factor(h, v);
  if (an.shard_count <= 1) {
    if (an.m > 0 && v.z != h->td.vin.p) {  // the caller's device vectors themselves (direct_vectors)
      const void *key[10] = {v.z, v.w};
      return graphed(h, h->direct_slot(h->gdirect_factor, key), [&]() { return run_factor(h, v.z, v.w, 3); });
    }
    return graphed(h, h->gfactor[0], [&]() { return run_factor(h, v.z, v.w, 3); });
  }
  if ((e = graphed(h, h->gfactor[0], [&]() { return run_factor(h, v.z, v.w, 1); }))) return e;
  if (an.upd_x_slot > 0 &&
      (e = exchange(h, HQPKKT_XCHG_ALLGATHER, h->td.upd.p + an.upd_x_off, an.upd_x_slot, an.shard_count)))
    return e;
  if ((e = graphed(h, h->gfactor[1], [&]() { return run_factor(h, v.z, v.w, 2); }))) return e;
  // A zero pivot inside a subtree is seen by its owner only: agree on the status words (one small
  // all-reduce), so that every rank returns the same code and nobody waits in a collective alone
  k_status_pack<<<1, 64, 0, h->stream>>>(h->td.flags.p, h->td.bits.p, h->td.ytmp.p);
  if ((e = exchange(h, HQPKKT_XCHG_ALLREDUCE_SUM, h->td.ytmp.p, 4, 1))) return e;
  k_status_unpack<<<1, 64, 0, h->stream>>>(h->td.ytmp.p, h->td.flags.p, h->td.bits.p);
  return 0;
}

int do_step(hqpkkt_t *h, const Vecs &v, int which) {
  Analysis &an = h->an;
  int e;
  if (h->opts.mode == HQPKKT_MODE_STAGED) return staged_step(h, v, which);
  if (an.shard_count <= 1) {
    // the caller's device vectors themselves (direct_vectors): also the refinement's sequence (which == 1: residual and
    // correction vectors are the handle's, z and w the caller's)
    if ((which == 0 && v.dx != h->td.vout.p) || (an.m > 0 && v.z != h->td.vin.p)) {
      const void *key[10] = {v.z, v.w, v.r1, v.r2, v.r3, v.r4, v.dx, v.dy, v.dz, v.dw};
      return graphed(h, h->direct_slot(h->gdirect_step, key), [&]() { return run_step(h, v, 7); });
    }
    return graphed(h, h->gstep[which][0], [&]() { return run_step(h, v, 7); });
  }
  if ((e = graphed(h, h->gstep[which][0], [&]() { return run_step(h, v, 1); }))) return e;
  if (an.cb_x_slot > 0 &&
      (e = exchange(h, HQPKKT_XCHG_ALLGATHER, h->td.cb.p + an.cb_x_off, an.cb_x_slot, an.shard_count)))
    return e;
  if ((e = graphed(h, h->gstep[which][1], [&]() { return run_step(h, v, 2); }))) return e;
  if ((e = exchange(h, HQPKKT_XCHG_ALLREDUCE_SUM, h->td.xsol.p, an.dim, 1))) return e;
  return graphed(h, h->gstep[which][2], [&]() { return run_step(h, v, 4); });
}

// residual of (d) for rhs (r); leaves the residual vectors in h->td.vres
// out != nullptr: the caller's copy of (d) is put into the stream before the read-back, so
// that a solve that needs no refinement round is over with this one round trip
// ---- read-backs through mapped host memory (hqpkkt::Kept::hpin)
// the status words (and, with `out`, n_out <= 40 of the IP loop's scalars) as they stand at this point of the stream
int post_words(hqpkkt_t *h, const double *out, int n_out, bool residual) {
  h->post_seq++;
  if (h->capturing) h->cap_posts++;
  k_post_words<<<1, 64, 0, h->stream>>>(h->td.flags.p, out, n_out, h->kept.hpin.dev, h->kept.post_seq_dev.p, residual ? 1 : 0);
  return 0;
}
// waits until the last posted words have arrived (every earlier post of the stream has then arrived as well)
int post_wait(hqpkkt_t *h) {
  volatile unsigned *seq = (volatile unsigned *)(h->kept.hpin.p + HPIN_SEQ);
  for (long long spin = 0;; spin++) {
    if (*seq == h->post_seq) break;
    if ((spin & 0xfffff) == 0xfffff) {  // (about every millisecond: has the stream died or drained without the word?)
      const hipError_t q = hipStreamQuery(h->stream);
      if (q == hipSuccess) {
        if (*seq == h->post_seq) break;
        (void)snprintf(g_last_hip_error, sizeof(g_last_hip_error), "posted read-back: the stream is empty and the sequence word is %u, not %u", *seq, h->post_seq);
        return HQPKKT_E_DEVICE;
      }
      if (q != hipErrorNotReady) HIPCHK(q);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}


// the residual kernel alone (what run_residual puts into the stream first)
int residual_launch(hqpkkt_t *h, const Vecs &v) {
  Analysis &an = h->an;
  hipStream_t s = h->stream;
  const int n = an.n, me = an.me, m = an.m;
  double *o1 = h->td.vres.p, *o2 = o1 + n, *o3 = o2 + me, *o4 = o3 + m;
  // the maximum is accumulated in the ints 122-123 of the flags buffer; the posting kernel behind every residual kernel
  // clears it (and a factorisation clears the whole buffer).  (rb_next: the word the kernel zeroes for its successor - a
  // spare one since the posting kernel does that.)
  unsigned long long *const rb_now = h->td.bits.p + 1, *const rb_next = h->td.bits.p - 1;
  const double *x1 = nullptr, *x2 = nullptr;  // STAGED, dense dynamics: their share of A dx and A'dy
  const double *xq = nullptr;                  // STAGED, dense stage Hessians: Q dx
  // STAGED, wide rows of C: C_wide' dz and the wide rows' C dx, with the narrow copies of C' and C for the walks
  const double *xcw = nullptr, *cw = nullptr;
  CsrDev CT = h->td.CT.dev(), C = h->td.C.dev();
  int ndyn = 0;
  if (h->opts.mode == HQPKKT_MODE_STAGED) {
    int e1 = staged_dense_products(h, v, &x1, &x2, &ndyn, &xq);
    if (e1) return e1;
    staged_rows_products(h, v, &xcw, &cw, &CT, &C);
  }
  if (h->short_rows)
    KLAUNCH(h, KC_RESIDUAL, k_residual<4><<<std::min(nblk(4LL * ((long long)n + me + m)), 1024), 256, 0, s>>>(
        n, me, m, h->td.Qf.dev(), h->td.AT.dev(), CT, h->td.A.dev(), C, h->td.vals.p, v.z, v.w,
        v.r1, v.r2, v.r3, v.r4, v.dx, v.dy, v.dz, v.dw, o1, o2, o3, o4, rb_now, rb_next, x1, x2, ndyn, xq, xcw, cw));
  else
    KLAUNCH(h, KC_RESIDUAL, k_residual<16><<<std::min(nblk(16LL * ((long long)n + me + m)), 1024), 256, 0, s>>>(
        n, me, m, h->td.Qf.dev(), h->td.AT.dev(), CT, h->td.A.dev(), C, h->td.vals.p, v.z, v.w,
        v.r1, v.r2, v.r3, v.r4, v.dx, v.dy, v.dz, v.dw, o1, o2, o3, o4, rb_now, rb_next, x1, x2, ndyn, xq, xcw, cw));
  return 0;
}
int run_residual(hqpkkt_t *h, const Vecs &v, double *res, const OutPtrs *out) {
  hipStream_t s = h->stream;
  {
    const int e1 = residual_launch(h, v);
    if (e1) return e1;
  }
  if (out) {
    int e2 = stage_out(h, v, out->dx, out->dy, out->dz, out->dw);
    if (e2) return e2;
  }
  // one read-back: the residual maximum and the status of the factorisation this solve belongs to
  int ep;
  if ((ep = post_words(h, nullptr, 0, true))) return ep;
  if (h->defer_residual && !out) {  // the caller queues more work and waits once (collect_residual)
    h->residual_pending = true;
    *res = 0.0;
    return 0;
  }
  if (out && !(h->out_pending && h->out_by_kernel)) HIPCHK(hipStreamSynchronize(s));  // (the caller's vectors: copies into pageable memory have landed)
  if ((ep = post_wait(h))) return ep;
  return collect_residual(h, res);
}

// the words run_residual copied to the pinned buffer, after the stream has been waited for
int collect_residual(hqpkkt_t *h, double *res) {
  h->residual_pending = false;
  const bool check = h->factor_unchecked;
  int *hs = (int *)h->kept.hpin.p;
  int flags[4] = {hs[0], hs[1], hs[2], hs[3]};
  if (poll_fallback(h, hs)) {  // a polled launch gave up waiting for a word: no result, and per-level launches from now on
    if (h->factor_unchecked) h->factor_unchecked = false, h->factored = false;  // (the factorisation may be the one that gave up)
    return HQPKKT_E_POLL;
  }
  unsigned long long kb, bits;
  std::memcpy(&kb, hs + 120, sizeof(kb)), std::memcpy(&bits, hs + h->res_read, sizeof(bits));
  double r;
  std::memcpy(&r, &bits, sizeof(r));
  *res = r;
  if (check) {
    h->factor_unchecked = false;
    std::memcpy(&h->st.kmax, &kb, sizeof(kb));
    h->st.n_2x2 = flags[1], h->st.n_perturbed = flags[2], h->st.n_slow_pivots = flags[3];
    h->soft_singular = hs[4] != 0;
    h->soft_tiny = hs[5] != 0;
    if (getenv("HQPKKT_TRACE_SOLVE") && (flags[0] || hs[4] || hs[5]))
      fprintf(stderr, "factor (checked with the solve): status %d, perturbed %d, zero pivot perturbed %d, tiny multiplier pivot %d\n", flags[0],
              flags[2], hs[4], hs[5]);
    if (flags[0] || std::isinf(h->st.kmax)) {
      h->factored = false;
      return flags[0] ? flags[0] : HQPKKT_E_SING;
    }
  }
  return 0;
}

extern "C" {

// diagnostics: run the solve `reps` times with time stamps inside k_solve_top (eager launches) and return, per fused
// front, level and six times in microseconds after the launch's first stamp: start, static data in, children arrived,
// forward done, border solution arrived, backward done (out: top_n x 8 doubles, [0] = tree level, [1..6] the times)
int hqpkkt_debug_solve_top_stamps(hqpkkt_t *h, double *out, int cap) {
  if (!h || !out) return HQPKKT_E_NULL;
  if (!h->factored || h->top_n <= 0) return HQPKKT_E_INTERN;
  if (cap < h->top_n * 8) return HQPKKT_E_SIZES;
  HIPCHK(hipSetDevice(h->opts.device));
  DBuf<unsigned long long> st;
  if (st.alloc(8 * (size_t)h->top_n)) return HQPKKT_E_MEM;
  (void)hipMemset(st.p, 0, sizeof(unsigned long long) * 8 * h->top_n);
  const bool graphs = h->use_graphs;
  h->use_graphs = false, h->top_stamps = st.p;
  Vecs v{};
  {  // the staged vectors of the last solve (the layout of stage_in)
    const int n = h->an.n, me = h->an.me, m = h->an.m;
    double *b = h->td.vin.p;
    v.z = b, v.w = b + m, v.r1 = b + 2 * (size_t)m, v.r2 = v.r1 + n, v.r3 = v.r2 + me, v.r4 = v.r3 + m;
  }
  stage_out_ptrs(h, v);
  int e = do_step(h, v, 0);
  if (!e && hipStreamSynchronize(h->stream) != hipSuccess) e = HQPKKT_E_DEVICE;
  h->use_graphs = graphs, h->top_stamps = nullptr;
  if (!e) {  // stamps of a sweep that gave up on a poll mean nothing
    int gave_up[XW_GAVE_UP + 1] = {};
    if (hipMemcpy(gave_up + XW_GAVE_UP, h->td.flags.p + XW_GAVE_UP, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess || poll_fallback(h, gave_up)) e = HQPKKT_E_DEVICE;
  }
  std::vector<unsigned long long> hs(8 * (size_t)h->top_n);
  if (!e && hipMemcpy(hs.data(), st.p, sizeof(unsigned long long) * hs.size(), hipMemcpyDeviceToHost) != hipSuccess) e = HQPKKT_E_DEVICE;
  if (e) return e;
  std::vector<int> nodes(h->top_n);
  HIPCHK(hipMemcpy(nodes.data(), h->td.top_nodes.p, sizeof(int) * h->top_n, hipMemcpyDeviceToHost));
  unsigned long long t0 = ~0ULL;
  for (int t = 0; t < h->top_n; t++) t0 = std::min(t0, hs[8 * (size_t)t]);
  for (int t = 0; t < h->top_n; t++) {
    out[8 * t] = h->an.level[nodes[t]];
    // split form: the backward launch has its own start (slot 6) and static-data (slot 7) stamps; they are returned in
    // place of nothing - out[7] = start of the backward launch of this front
    for (int k = 0; k < 6; k++) out[8 * t + 1 + k] = (double)(hs[8 * (size_t)t + k] - t0) * 0.01;  // 100 MHz
    out[8 * t + 7] = hs[8 * (size_t)t + 6] ? (double)(hs[8 * (size_t)t + 6] - t0) * 0.01 : 0.0;
  }
  return 0;
}

#ifdef HQPKKT_STAMPS
int hqpkkt_debug_fb_stamps(int *out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(kktdev::g_fb_stamps), sizeof(int) * 256));
  return 0;
}
int hqpkkt_debug_ps_stamps(int *out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(kktdev::g_ps_stamps), sizeof(int) * 64));
  return 0;
}
#endif

// One dense symmetric p x p block through the pivot-block kernel on its own (tests, tools): A row-major;
// variant 0 = k_factor_blk as run_factor launches it (8 wavefronts for p <= 128, 12 beyond: five blocks per wavefront up to
// 160 pivots, six up to 176, eight up to 192), 1 = k_factor_diag (p <= 128), 2 = the 12-wavefront instance with eight blocks whatever p,
// 3 = the 12-wavefront instance with six blocks (p <= 176).  Out: the block's panel (p x p column-major: unit lower L11
// below the diagonal), D^-1 (2 p), pivot types, pivot order, M = L11^-1 (p x p column-major), the counters
// (2x2 pivots, perturbed, slow pivots, ...), and the average time of `reps` launches of one workgroup.
int hqpkkt_debug_factor_block(int device, int p, const double *A, double tol, double pivot_eps, int variant,
                              int reps, double *Lout, double *dinv_out, int *ptype_out, int *lperm_out,
                              double *Wout, int *counters_out, double *ms_out) {
  if (!A || p < 1 || p > 192 || (variant == 1 && p > 128)) return HQPKKT_E_RANGE;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  if (reps < 1) reps = 1;
  const size_t pp2 = (size_t)p * p;
  std::vector<double> P(pp2 * reps);
  double kmax = 0.0;
  for (int j = 0; j < p; j++)
    for (int i = 0; i < p; i++) {
      P[(size_t)j * p + i] = i >= j ? A[(size_t)i * p + j] : 0.0;
      kmax = std::fmax(kmax, std::fabs(A[(size_t)i * p + j]));
    }
  for (int rp = 1; rp < reps; rp++) std::memcpy(P.data() + pp2 * rp, P.data(), sizeof(double) * pp2);
  std::vector<int> piv_start(reps), npiv(reps, p), nbor(reps, 0), parent(reps, -1), child_ptr(reps + 1, 0), nodes(reps);
  std::vector<long long> zeros(reps + 1, 0), poff(reps), loff(reps);
  std::vector<signed char> sg((size_t)p * reps);
  for (int rp = 0; rp < reps; rp++) {
    piv_start[rp] = rp * p, nodes[rp] = rp, poff[rp] = (long long)pp2 * rp, loff[rp] = (long long)pp2 * rp;
    for (int i = 0; i < p; i++) sg[(size_t)rp * p + i] = A[(size_t)i * p + i] < 0.0 ? -1 : 1;
  }
  DBuf<int> d_ps, d_np, d_nb, d_par, d_cp, d_nodes, d_pt, d_lp, d_flags, d_one;
  DBuf<long long> d_zero, d_poff, d_loff;
  DBuf<double> d_P, d_dinv, d_W, d_upd;
  DBuf<signed char> d_sg;
  std::vector<int> fl(128, 0), onei(4, 0);
  std::memcpy(fl.data() + 120, &kmax, sizeof(double));
  int e;
  if ((e = d_ps.upload(piv_start)) || (e = d_np.upload(npiv)) || (e = d_nb.upload(nbor)) || (e = d_par.upload(parent)) ||
      (e = d_cp.upload(child_ptr)) || (e = d_nodes.upload(nodes)) || (e = d_zero.upload(zeros)) || (e = d_poff.upload(poff)) ||
      (e = d_loff.upload(loff)) || (e = d_P.upload(P)) || (e = d_sg.upload(sg)) || (e = d_flags.upload(fl)) ||
      (e = d_one.upload(onei)) || (e = d_dinv.alloc(2 * (size_t)p * reps)) || (e = d_W.alloc(pp2 * reps)) ||
      (e = d_upd.alloc(8)) || (e = d_pt.alloc((size_t)p * reps)) || (e = d_lp.alloc((size_t)p * reps)))
    return e;
  HIPCHK(hipMemset(d_W.p, 0, sizeof(double) * pp2 * reps));
  DevTree T{d_ps.p, d_np.p, d_nb.p, d_par.p, d_zero.p, d_one.p, d_one.p, d_poff.p, d_zero.p, d_zero.p, d_zero.p,
            d_cp.p, d_one.p, d_one.p, d_zero.p};
  const double alpha = tol * 0.6403882032022076;
  const unsigned long long *kb = (const unsigned long long *)(d_flags.p + 120);
  const size_t mpd = p, ldm = mpd | 1;
  const size_t lds_old = (std::max<size_t>(ldm * mpd, 2 * FD_PLD * FD_PANEL) + 5 * 128 + 2 * mpd) * sizeof(double) + 2 * mpd * sizeof(int) + 16;
  if (variant == 1)
    HIPCHK(hipFuncSetAttribute((const void *)k_factor_diag, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>(lds_old, 64 * 1024)));
  HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<8, 6, 144, 2, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fb_lds_bytes(128)));
  HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<12, 8, 208, 3, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fb_lds_bytes(192)));
  HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<12, 6, 208, 3, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fb_lds_bytes(192)));
  HIPCHK(hipFuncSetAttribute((const void *)k_factor_blk<12, FB_NS160, 208, 3, FB_OWNSIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fb_lds_bytes(192)));
  EventOwner e0, e1;
  HIPCHK(hipEventCreate(&e0.h));
  HIPCHK(hipEventCreate(&e1.h));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(e0, 0));
  for (int rp = 0; rp < reps; rp++) {
    if (variant == 1)
      k_factor_diag<<<1, FD_THREADS, lds_old, 0>>>(T, d_nodes.p + rp, d_P.p, d_dinv.p, d_pt.p, d_lp.p, d_sg.p, d_W.p, d_loff.p,
                                                  alpha, pivot_eps, kb, d_flags.p + 1, d_upd.p);
    else if (variant == 0 && p <= 128)
      k_factor_blk<8, 6, 144, 2, FB_OWNSIMD><<<1, 512, fb_lds_bytes(p), 0>>>(T, d_nodes.p + rp, d_P.p, d_dinv.p, d_pt.p, d_lp.p, d_sg.p, d_W.p,
                                                        d_loff.p, alpha, pivot_eps, kb, d_flags.p + 1, d_upd.p);
    else if (variant == 0 && p <= 160)  // (as run_factor chooses: five blocks per wavefront up to 160 pivots, six up to 176)
      k_factor_blk<12, FB_NS160, 208, 3, FB_OWNSIMD><<<1, 768, fb_lds_bytes(std::max(p, 129)), 0>>>(T, d_nodes.p + rp, d_P.p, d_dinv.p, d_pt.p, d_lp.p, d_sg.p, d_W.p,
                                                          d_loff.p, alpha, pivot_eps, kb, d_flags.p + 1, d_upd.p);
    else if ((variant == 0 || variant == 3) && p <= 176)
      k_factor_blk<12, 6, 208, 3, FB_OWNSIMD><<<1, 768, fb_lds_bytes(std::max(p, 129)), 0>>>(T, d_nodes.p + rp, d_P.p, d_dinv.p, d_pt.p, d_lp.p, d_sg.p, d_W.p,
                                                          d_loff.p, alpha, pivot_eps, kb, d_flags.p + 1, d_upd.p);
    else
      k_factor_blk<12, 8, 208, 3, FB_OWNSIMD><<<1, 768, fb_lds_bytes(std::max(p, 129)), 0>>>(T, d_nodes.p + rp, d_P.p, d_dinv.p, d_pt.p, d_lp.p, d_sg.p, d_W.p,
                                                          d_loff.p, alpha, pivot_eps, kb, d_flags.p + 1, d_upd.p);
  }
  HIPCHK(hipEventRecord(e1, 0));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipGetLastError());
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  if (ms_out) *ms_out = ms / reps;
  const size_t last = (size_t)(reps - 1);
  if (Lout) HIPCHK(hipMemcpy(Lout, d_P.p + pp2 * last, sizeof(double) * pp2, hipMemcpyDeviceToHost));
  if (Wout) HIPCHK(hipMemcpy(Wout, d_W.p + pp2 * last, sizeof(double) * pp2, hipMemcpyDeviceToHost));
  if (dinv_out) HIPCHK(hipMemcpy(dinv_out, d_dinv.p + 2 * (size_t)p * last, sizeof(double) * 2 * p, hipMemcpyDeviceToHost));
  if (ptype_out) HIPCHK(hipMemcpy(ptype_out, d_pt.p + (size_t)p * last, sizeof(int) * p, hipMemcpyDeviceToHost));
  if (lperm_out) HIPCHK(hipMemcpy(lperm_out, d_lp.p + (size_t)p * last, sizeof(int) * p, hipMemcpyDeviceToHost));
  if (counters_out) HIPCHK(hipMemcpy(counters_out, d_flags.p, sizeof(int) * 128, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
