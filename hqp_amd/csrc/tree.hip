// The tree engine (HQPKKT_MODE_FULL / _REDUCED): device residency of the symbolic structure (upload, a sequence of named
// steps) and the kernel sequencing of assemble -> factor -> step -> residual; the vector staging of a call and the posted
// read-backs (both engines use them), and the debug entry points that launch the tree's kernels or read its device arrays.
// WHAT is launched for a tree level is decided once per upload by tree_plan() (tree_plan.hpp, plain host code) and kept in
// hqpkkt::plan; run_factor and run_step walk it.  The instances of the templated kernels stand in one table per family
// (fb_kernels, top_kernels), the pointer lists the kernels share in one launch function each (launch_factor, launch_fwd).
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
  const TreePlan &P = h->plan;
  int e;
  if (P.top.n > 0 && (e = fill(h->td.top_x, 2 * (size_t)P.top.n * (ST_CS + ST_XS)))) return e;
  if (P.small_tree && (e = fill(h->td.tree_x, 2 * (size_t)(h->an.cb_elems + h->an.dim)))) return e;
  if (P.tree_factor && (e = fill(h->td.tree_u, 2 * (size_t)std::max<long long>(h->an.upd_elems, 1)))) return e;
  return 0;
}

TreeSwitches tree_switches(const hqpkkt_t *h) {
  return TreeSwitches{getenv("HQPKKT_NO_TREE_SWEEPS") != nullptr, getenv("HQPKKT_NO_SOLVE_TOP") != nullptr,
                      getenv("HQPKKT_SOLVE_TOP_FUSED") != nullptr, h->no_polled};
}

bool poll_fallback(hqpkkt_t *h, const int *hs) {
  if (!hs[XW_GAVE_UP]) return false;
  (void)reset_solve_top(h);
  (void)hipMemsetAsync(h->td.flags.p + XW_GAVE_UP, 0, sizeof(int), h->stream);
  (void)hipStreamSynchronize(h->stream);
  h->no_polled = true;  // (a later upload stays there)
  TreeSwitches sw = h->plan.sw;
  sw.no_polled = true;
  h->plan = tree_plan(h->an, sw);  // per-level launches from now on
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
// ------------------------------------------------------------ one table per templated kernel family
// the instances of k_factor_blk, in the order of fb_instances (tree_plan.hpp: pivots held and threads of each)
using FactorBlkFn = decltype(&k_factor_blk<8, 6, 144, 2, FB_OWNSIMD>);
static const FactorBlkFn fb_kernels[FB_INSTANCES] = {k_factor_blk<8, 6, 144, 2, FB_OWNSIMD>, k_factor_blk<12, FB_NS160, 208, 3, FB_OWNSIMD>,
                                                     k_factor_blk<12, 6, 208, 3, FB_OWNSIMD>, k_factor_blk<12, 8, 208, 3, FB_OWNSIMD>};
// the instances of k_solve_top by [ns - 3][mode], and the pivots an instance holds (16 nu)
using SolveTopFn = decltype(&k_solve_top<3, 11, 0>);
static const SolveTopFn top_kernels[2][3] = {{k_solve_top<3, 11, 0>, k_solve_top<3, 11, 1>, k_solve_top<3, 11, 2>},
                                             {k_solve_top<4, 10, 0>, k_solve_top<4, 10, 1>, k_solve_top<4, 10, 2>}};
static const int top_maxp[2] = {176, 160};

static int set_max_lds(const void *kernel, size_t bytes) {
  HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}
// every instance of k_factor_blk may launch with `want` bytes of LDS, or with what its largest front needs
static int raise_fb_lds(size_t want) {
  int e = 0;
  for (int i = 0; i < FB_INSTANCES && !e; i++) e = set_max_lds((const void *)fb_kernels[i], std::min(want, fb_lds_bytes(fb_instances[i].maxp)));
  return e;
}

// ------------------------------------------------------------ upload, step by step
static int upload_structure(hqpkkt_t *h) {
  Analysis &an = h->an;
  int e;
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
  return 0;
}

// the terms of the entries, and the sign a perturbed pivot takes
static int upload_terms_and_signs(hqpkkt_t *h) {
  Analysis &an = h->an;
  int e;
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
  return h->td.esign.upload(sg);
}

// the SpMV blocks, the arenas of the factors and the vectors, the status words
static int alloc_numeric(hqpkkt_t *h) {
  Analysis &an = h->an;
  int e;
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
  std::vector<double> ones(dim, 1.0);
  HIPCHK(hipMemcpy(h->td.sc.p, ones.data(), sizeof(double) * dim, hipMemcpyHostToDevice));
  const double one = 1.0;
  HIPCHK(hipMemcpy(h->td.vals.p + (nv - 1), &one, sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->td.wt.p + m, &one, sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// the mapped words of the read-backs, and the pinned buffer the vectors of a small system go through
static int alloc_staging(hqpkkt_t *h) {
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  int e;
  if ((e = alloc_hpin(h))) return e;
  h->td.hstage.release();
  h->td.hstage_in = h->td.hstage_out = 0;
  const size_t nin = 4 * (size_t)m + n + me, nout = (size_t)n + me + 2 * (size_t)m;
  if ((nin + nout) * sizeof(double) <= (size_t)512 * 1024 && nin + nout > 0) {
    HIPCHK(h->td.hstage.alloc(nin + nout, hipHostMallocMapped | hipHostMallocCoherent));
    h->td.hstage_in = nin, h->td.hstage_out = nout;
    if (h->td.hstage.map() != hipSuccess) (void)hipGetLastError();
  }
  return 0;
}

// what the handle launches (tree_plan.hpp), the device arrays of its polled launches and their idle state
static int upload_plan(hqpkkt_t *h) {
  Analysis &an = h->an;
  int e;
  h->plan = tree_plan(an, tree_switches(h));
  const TreePlan &P = h->plan;
  if (P.err) return P.err;
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
  if (P.small_tree) {
    if ((e = h->td.tree_down.upload(P.tree_down)) || (e = h->td.tree_x.alloc(2 * (size_t)(an.cb_elems + an.dim)))) return e;
    if (P.tree_factor && (e = h->td.tree_u.alloc(2 * (size_t)std::max<long long>(an.upd_elems, 1)))) return e;
  }
  if (P.top.n > 0 &&
      ((e = h->td.top_nodes.upload(P.top.nodes)) || (e = h->td.top_idx.upload(P.top.idx)) || (e = h->td.top_bpos.upload(P.top.bpos)) ||
       (e = h->td.top_up.upload(P.top.up)) || (e = h->td.top_x.alloc(2 * (size_t)P.top.n * (ST_CS + ST_XS)))))
    return e;
  return P.small_tree || P.top.n > 0 ? reset_solve_top(h) : 0;
}

// The dynamic-LDS limits of the kernels.  The attribute is state of the PROCESS, not of the handle: a second handle with
// smaller fronts must not lower the limit under one that still launches with more (several plugins in one host, the
// bench's concurrent systems): keep the largest value ever asked for, under a mutex ... and hipFuncSetAttribute acts on
// the CURRENT device: the largest values are kept per device
static int raise_lds_limits(hqpkkt_t *h) {
  static std::mutex attr_mutex;
  struct PerDev { size_t panel = 0, bwdb = 0, blk = 0, top = 0; };
  static PerDev per_dev[64];
  if (h->opts.device < 0 || h->opts.device >= 64) return HQPKKT_E_RANGE;
  std::lock_guard<std::mutex> lk(attr_mutex);
  PerDev &a = per_dev[h->opts.device];
  const TreePlan &P = h->plan;
  int e;
  if (P.top.lds > a.top) {
    for (int i = 0; i < 2; i++)
      for (int mode = 0; mode < 3; mode++)
        if ((e = set_max_lds((const void *)top_kernels[i][mode], std::min(P.top.lds, st_top_lds_bytes(top_maxp[i], 3 + i))))) return e;
    a.top = P.top.lds;
  }
  if (P.lds_blk > a.blk) {
    if ((e = raise_fb_lds(P.lds_blk))) return e;
    a.blk = P.lds_blk;
  }
  if (P.lds_panel > a.panel) {
    if ((e = set_max_lds((const void *)k_panel_solve, P.lds_panel))) return e;
    a.panel = P.lds_panel;
  }
  if (P.lds_bwdb > a.bwdb) {
    if ((e = set_max_lds((const void *)k_solve_bwd_b, P.lds_bwdb))) return e;
    a.bwdb = P.lds_bwdb;
  }
  return 0;
}

int upload(hqpkkt_t *h) {
  int e;
  if ((e = ensure_device(h)) || (e = upload_structure(h)) || (e = upload_terms_and_signs(h)) || (e = alloc_numeric(h)) ||
      (e = alloc_staging(h)) || (e = upload_plan(h)) || (e = raise_lds_limits(h)))
    return e;
  const Analysis &an = h->an;
  const double rows = 2.0 * an.n + an.me + an.m;  // Q, A', C' per x row; A, C rows
  const double nnz = (double)an.Qfull.col.size() + 2.0 * an.A.col.size() + 2.0 * an.C.col.size();
  h->short_rows = rows > 0 && nnz / rows < 8.0;
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

static_assert(FS_MAXP == kktdev::SMALL_PIVOTS && FS_MAXB == kktdev::SMALL_BORDER, "small-supernode kernels and schedule disagree");
// ------------------------------------------------------------ numeric phases
// run_factor and run_step walk the handle's plan (tree_plan.hpp): which kernel instance a level takes, its grid and LDS
// were decided there.
// (HQPKKT_NO_FUSED_VECTORS=1: the vector work around the sweeps and the assembly as the separate launches of round 5 - the
// comparison the bit-identity test makes)
static bool no_fused_vectors() { return getenv("HQPKKT_NO_FUSED_VECTORS") != nullptr; }

// The pointer list the factor kernels share (k_factor_blk, k_factor_diag, k_factor_diag_small), written once: `tail` is
// what a kernel takes behind it.
struct FactorArgs {
  DevTree T;
  double *panel, *dinv;
  int *ptype, *lperm;
  const signed char *esign;
  double *linv;
  const long long *linv_off;
  double alpha, pivot_eps;
  const unsigned long long *kmax_bits;
  int *counters;
  double *upd;
};
template <class K, class... Tail>
static void launch_factor(K kernel, int grid, int block, size_t lds, hipStream_t s, const FactorArgs &a, const int *nodes, Tail... tail) {
  kernel<<<grid, block, lds, s>>>(a.T, nodes, a.panel, a.dinv, a.ptype, a.lperm, a.esign, a.linv, a.linv_off, a.alpha, a.pivot_eps, a.kmax_bits,
                                  a.counters, a.upd, tail...);
}
static FactorArgs factor_args(hqpkkt_t *h) {
  const double alpha = h->opts.tol * 0.6403882032022076;  // tol (1+sqrt 17)/8, hqp/spBKP.C:392
  return FactorArgs{h->td.tree(), h->td.panel.p, h->td.dinv.p, h->td.ptype.p, h->td.lperm.p, h->td.esign.p, h->td.linv.p, h->td.linv_off.p,
                    alpha, h->opts.pivot_eps, h->td.bits.p, h->td.flags.p + 1, h->td.upd.p};
}

// clears the panel arena and the status words, then the entries of the matrix into the panels
static int assemble(hqpkkt_t *h, const double *z, const double *w) {
  Analysis &an = h->an;
  TreeDev &d = h->td;
  hipStream_t s = h->stream;
  const int m = an.m, nent = (int)an.ent_a.size();
  if (an.shard_count <= 1) {  // the panel arena, and the status words, counters and the two maxima
    KLAUNCH(h, KC_ASSEMBLE, k_clear<<<(int)std::max<long long>(1, std::min<long long>(2048, (an.panel_elems / 2 + 1023) / 1024)), 256, 0, s>>>(d.panel.p, an.panel_elems, d.flags.p));
  } else {  // only the blocks this rank writes
    const int np = (int)an.zero_panel.size() / 2;
    if (np) k_zero_ranges<<<dim3(512, np), 256, 0, s>>>(d.panel.p, d.zero_panel.p);
    k_clear<<<1, 256, 0, s>>>(nullptr, 0, d.flags.p);
  }
  if (!h->capturing) HIPCHK(hipEventRecord(h->ev0, s));
  if (m > 0 && (d.simple_src.count || no_fused_vectors()))
    KLAUNCH(h, KC_ASSEMBLE, k_weights<<<nblk(m), 256, 0, s>>>(an.mode, m, an.n + an.me, z, w, d.wt.p, d.sc.p, d.flags.p));
  const int nsc = std::min(nblk(nent), 2048);
  if (d.simple_src.count) {  // FULL: one pass
    KLAUNCH(h, KC_ASSEMBLE, k_assemble_simple<<<nsc, 256, 0, s>>>(nent, d.simple_src.p, d.simple_wi.p, d.ent_a.p, d.ent_b.p, d.ent_dst.p, d.vals.p, d.wt.p,
                                                                  d.sc.p, d.panel.p, d.bits.p, d.tree_words.p + 1));
  } else if (no_fused_vectors()) {
    KLAUNCH(h, KC_ASSEMBLE, k_entry_values<<<nblk(nent), 256, 0, s>>>(nent, d.term_ptr.p, d.terms.p, d.vals.p, d.wt.p, d.ent_val.p, d.tree_words.p + 1));
    if (an.mode == 1 && an.n > 0) KLAUNCH(h, KC_ASSEMBLE, k_red_scale<<<nblk(an.n), 256, 0, s>>>(an.n, d.diag_ent.p, d.ent_val.p, d.sc.p));
    KLAUNCH(h, KC_ASSEMBLE, k_scatter<<<nsc, 256, 0, s>>>(nent, d.ent_a.p, d.ent_b.p, d.ent_dst.p, d.ent_val.p, d.sc.p, d.panel.p, d.bits.p));
  } else {
    // weights + entry values, scales + scatter: one launch each (kernels.hip.h, k_wt_entry / k_scale_scatter)
    KLAUNCH(h, KC_ASSEMBLE, k_wt_entry<<<nblk(nent) + (m > 0 ? nblk(m) : 0), 256, 0, s>>>(an.mode, m, an.n + an.me, nent, nblk(nent), z, w, d.wt.p, d.sc.p, d.flags.p,
                                                                                       d.term_ptr.p, d.terms.p, d.vals.p, d.ent_val.p, d.tree_words.p + 1));
    if (an.mode == 1 && an.n > 0)
      KLAUNCH(h, KC_ASSEMBLE, k_scale_scatter<<<nsc + nblk(an.n), 256, 0, s>>>(an.n, nent, nsc, d.diag_ent.p, d.ent_a.p, d.ent_b.p, d.ent_dst.p, d.ent_val.p, d.sc.p,
                                                                            d.panel.p, d.bits.p));
    else
      KLAUNCH(h, KC_ASSEMBLE, k_scatter<<<nsc, 256, 0, s>>>(nent, d.ent_a.p, d.ent_b.p, d.ent_dst.p, d.ent_val.p, d.sc.p, d.panel.p, d.bits.p));
  }
  if (!h->capturing) HIPCHK(hipEventRecord(h->ev1, s));
  return 0;
}

// one level of schedule `which`: small fronts, small blocks, pivot blocks, panel solve, updates
static void factor_level(hqpkkt_t *h, int which, const LevelPlan &R, const FactorArgs &a, const TreeXchgF &txf) {
  const TreeDev::DevSched &D = h->td.ds[which];
  TreeDev &d = h->td;
  hipStream_t s = h->stream;
  const int *nodes = D.level_nodes.p + R.nodes_off;
  if (R.fs_n > 0)
    KLAUNCH(h, KC_FACTOR_DIAG, launch_factor(k_factor_diag_small<true>, R.fs_n, 64, R.fs_lds, s, a, nodes, d.xar.p, R.fs_ldp, R.fs_ldb, txf));
  if (R.sm_n > 0)
    KLAUNCH(h, KC_FACTOR_DIAG, launch_factor(k_factor_diag_small<false>, R.sm_n, 64, R.sm_lds, s, a, nodes + R.fs_n, d.xar.p, R.sm_ldp, 1, txf));
  if (R.blk_n > 0)
    KLAUNCH(h, KC_FACTOR_DIAG, launch_factor(fb_kernels[R.blk_inst], R.blk_n, R.blk_threads, R.blk_lds, s, a, nodes + R.fs_n + R.sm_n));
  if (R.ps_grid > 0)
    KLAUNCH(h, KC_PANEL_SOLVE, k_panel_solve<<<R.ps_grid, 256, h->plan.lds_panel, s>>>(a.T, D.slabs.p + 2 * (size_t)R.slabs_off, d.panel.p, d.xar.p, d.dinv.p, d.ptype.p,
                                                                                    d.lperm.p, d.linv.p, d.linv_off.p, d.upd.p, R.ps_xps));
  const int *tiles = D.upd_tiles.p + 3 * (size_t)R.tiles_off;
  if (R.su_variant == 2)
    KLAUNCH(h, KC_SCHUR_UPDATE, k_schur_update<2><<<R.su_grid, 256, 0, s>>>(a.T, tiles, d.panel.p, d.xar.p, d.upd.p, R.su_xsu));
  else if (R.su_variant == 1)
    KLAUNCH(h, KC_SCHUR_UPDATE, k_schur_update<1><<<R.su_grid, 256, 0, s>>>(a.T, tiles, d.panel.p, d.xar.p, d.upd.p, R.su_xsu));
  if (R.big_n > 0)
    KLAUNCH(h, KC_SCHUR_UPDATE, (k_schur_update_big<2, 2, 4, 4, 2, 2><<<R.big_n, 256, 0, s>>>(a.T, D.upd_tiles.p + 3 * (size_t)R.big_off, d.panel.p, d.xar.p, d.upd.p)));
}

// phases: 1 = assemble + this rank's subtrees, 2 = replicated top of the tree
// (3 = everything, the single-rank case)
static int run_factor(hqpkkt_t *h, const double *z, const double *w, int phases) {
  const TreePlan &P = h->plan;
  int e;
  if ((phases & 1) && (e = assemble(h, z, w))) return e;
  const FactorArgs a = factor_args(h);
  const TreeXchgF txf{h->td.tree_u.p, h->an.upd_elems, h->td.tree_words.p + 1};
  for (int which = 0; which < 2; which++) {
    if (!(phases & (1 << which)) || h->an.sched[which].nnodes == 0) continue;
    if (which == 0 && P.tree_factor)  // a tree of small fronts: all levels in one launch
      KLAUNCH(h, KC_FACTOR_DIAG, launch_factor(k_factor_diag_small<true, true>, h->an.sched[0].nnodes, 64, fs_lds_bytes(true, P.tree_ldp, P.tree_ldb), h->stream, a,
                                               h->td.ds[0].level_nodes.p, h->td.xar.p, P.tree_ldp, P.tree_ldb, txf));
    else
      for (const LevelPlan &R : P.levels[which]) factor_level(h, which, R, a, txf);
  }
  if (!h->capturing) HIPCHK(hipEventRecord(h->evs1, h->stream));
  HIPCHK(hipGetLastError());
  return 0;
}

// The pointer list the forward kernels share (k_solve_fwd_small, k_solve_fwd), written once: `tail` is the exchange
// arrays of the one-wavefront kernel.
template <class K, class... Tail>
static void launch_fwd(hqpkkt_t *h, K kernel, int grid, int block, const int *list, Tail... tail) {
  TreeDev &d = h->td;
  kernel<<<grid, block, 0, h->stream>>>(d.tree(), list, d.panel.p, d.linv.p, d.linv_off.p, d.dinv.p, d.ptype.p, d.lperm.p, d.rhs.p, d.xsol.p, d.ytmp.p, d.cb.p,
                                        tail...);
}
// ... and k_solve_bwd_small<TREE> of a level, or of the whole tree
template <class K>
static void launch_bwd_small(hqpkkt_t *h, K kernel, int grid, const int *nodes, const TreeXchg &tx) {
  TreeDev &d = h->td;
  kernel<<<grid, 64, 0, h->stream>>>(d.tree(), nodes, d.panel.p, d.linv.p, d.linv_off.p, d.lperm.p, d.xsol.p, tx);
}
static TreeXchg tree_xchg(hqpkkt_t *h) {
  return TreeXchg{h->td.tree_x.p, h->td.tree_x.p + 2 * h->an.cb_elems, h->an.cb_elems, h->an.dim, h->td.tree_words.p, h->td.flags.p};
}

static void forward_level(hqpkkt_t *h, int which, const LevelPlan &R, const TreeXchg &tx) {
  const TreeDev::DevSched &D = h->td.ds[which];
  TreeDev &d = h->td;
  hipStream_t s = h->stream;
  const int *nodes = D.level_nodes.p + R.nodes_off, *gslabs = D.gslabs.p + 2 * (size_t)R.gslabs_off;
  if (R.fwd_small_n > 0) KLAUNCH(h, KC_SOLVE_FWD, launch_fwd(h, k_solve_fwd_small<false>, R.fwd_small_n, 64, nodes, tx));
  if (R.fwd_form == FWD_ONE) {
    KLAUNCH(h, KC_SOLVE_FWD, launch_fwd(h, k_solve_fwd, R.fwd_grid, 256, gslabs));
  } else if (R.fwd_form == FWD_AB) {
    KLAUNCH(h, KC_SOLVE_FWD, k_solve_fwd_a<<<R.fwd_a_grid, 256, 0, s>>>(d.tree(), nodes + R.fwd_small_n, d.linv.p, d.linv_off.p, d.dinv.p, d.ptype.p, d.lperm.p, d.rhs.p,
                                                                       d.xsol.p, d.ytmp.p, d.cb.p));
    KLAUNCH(h, KC_SOLVE_FWD, k_solve_fwd_b<<<R.fwd_grid, 256, 0, s>>>(d.tree(), gslabs, d.panel.p, d.ytmp.p, d.cb.p));
  }
}
static void backward_level(hqpkkt_t *h, int which, const LevelPlan &R, const TreeXchg &tx) {
  const TreeDev::DevSched &D = h->td.ds[which];
  TreeDev &d = h->td;
  hipStream_t s = h->stream;
  const int *nodes = D.level_nodes.p + R.nodes_off;
  if (R.bwd_small_n > 0) KLAUNCH(h, KC_SOLVE_BWD, launch_bwd_small(h, k_solve_bwd_small<false>, R.bwd_small_n, nodes, tx));
  if (R.bwd_a_grid <= 0) return;
  // (one workgroup per front doing both steps was measured slower: L21' x needs the
  // column blocks spread over the chip)
  KLAUNCH(h, KC_SOLVE_BWD, k_solve_bwd_b<<<R.bwd_b_grid, 256, h->plan.lds_bwdb, s>>>(d.tree(), D.cblks.p + 2 * (size_t)R.cblks_off, d.panel.p, d.xsol.p, d.vtmp.p));
  KLAUNCH(h, KC_SOLVE_BWD, k_solve_bwd_a<<<R.bwd_a_grid, 256, 0, s>>>(d.tree(), nodes + R.bwd_small_n, d.linv.p, d.linv_off.p, d.lperm.p, d.vtmp.p, d.xsol.p));
}
// the sweeps of schedule `which` below the fused top: one launch each for a tree of small fronts, else level by level
static void forward(hqpkkt_t *h, int which) {
  const TreeXchg tx = tree_xchg(h);
  if (which == 0 && h->plan.small_tree)
    KLAUNCH(h, KC_SOLVE_FWD, launch_fwd(h, k_solve_fwd_small<true>, h->an.sched[0].nnodes, 64, h->td.ds[0].level_nodes.p, tx));
  else
    for (const LevelPlan &R : h->plan.levels[which]) forward_level(h, which, R, tx);
}
static void backward(hqpkkt_t *h, int which) {
  const TreeXchg tx = tree_xchg(h);
  const std::vector<LevelPlan> &L = h->plan.levels[which];
  if (which == 0 && h->plan.small_tree)
    KLAUNCH(h, KC_SOLVE_BWD, launch_bwd_small(h, k_solve_bwd_small<true>, h->an.sched[0].nnodes, h->td.tree_down.p, tx));
  else
    for (size_t l = L.size(); l-- > 0;) backward_level(h, which, L[l], tx);
}

// the top levels, up and down: one launch, or one per sweep (k_solve_top)
static void solve_top(hqpkkt_t *h) {
  const TreePlan::Top &P = h->plan.top;
  TreeDev &d = h->td;
  TopArgs ta{d.top_nodes.p, d.top_idx.p, d.top_bpos.p, d.top_x.p, d.top_x.p + 2 * (size_t)P.n * ST_CS, d.tree_words.p, P.n, h->top_stamps};
  auto launch = [&](int mode, const int *nodes) {
    ta.nodes = nodes;
    KLAUNCH(h, KC_SOLVE_TOP, top_kernels[P.ns - 3][mode]<<<P.n, ST_THREADS, P.lds, h->stream>>>(d.tree(), ta, d.panel.p, d.linv.p, d.linv_off.p, d.dinv.p, d.ptype.p, d.lperm.p,
                                                                                            d.rhs.p, d.xsol.p, d.cb.p, d.flags.p));
  };
  if (!P.split)
    launch(0, d.top_nodes.p);
  else
    launch(1, d.top_up.p), launch(2, d.top_nodes.p);
}

// the right-hand side in elimination order, scaled
static void rhs(hqpkkt_t *h, const Vecs &v) {
  Analysis &an = h->an;
  TreeDev &d = h->td;
  hipStream_t s = h->stream;
  const int n = an.n, me = an.me, m = an.m, dim = an.dim;
  if (an.mode == 0) {
    KLAUNCH(h, KC_VECTOR, k_rhs_full<<<nblk(dim), 256, 0, s>>>(n, me, m, d.q2e.p, d.sc.p, v.z, v.r1, v.r2, v.r3, v.r4, d.rhs.p, d.tree_words.p));
  } else if (no_fused_vectors()) {
    if (m > 0) KLAUNCH(h, KC_VECTOR, k_red_t<<<nblk(m), 256, 0, s>>>(m, v.w, d.wt.p, v.r3, v.r4, d.tz.p));
    KLAUNCH(h, KC_VECTOR, k_rhs_red<<<nblk(dim), 256, 0, s>>>(n, me, d.q2e.p, d.sc.p, d.CT.ptr.p, d.CT.col.p, d.CT.src.p, d.vals.p, d.tz.p, v.r1, v.r2, d.rhs.p,
                                                             d.tree_words.p));
  } else {
    // (tz and the right-hand side that needs it in one launch: kernels.hip.h, k_rhs_red_t; HQPKKT_NO_FUSED_VECTORS=1: two)
    KLAUNCH(h, KC_VECTOR, k_rhs_red_t<<<nblk(dim) + (m > 0 ? nblk(m) : 0), 256, 0, s>>>(n, me, m, nblk(dim), d.q2e.p, d.sc.p, d.CT.ptr.p, d.CT.col.p, d.CT.src.p, d.vals.p,
                                                                                     v.w, d.wt.p, v.r3, v.r4, d.tz.p, v.r1, v.r2, d.rhs.p, d.tree_words.p));
  }
}

// unscale + scatter of the solution into dx, dy; dz and dw from dx
static void unpack(hqpkkt_t *h, const Vecs &v) {
  Analysis &an = h->an;
  TreeDev &d = h->td;
  hipStream_t s = h->stream;
  const int n = an.n, me = an.me, m = an.m, dim = an.dim;
  if (an.mode == 0) {
    KLAUNCH(h, KC_VECTOR, k_unpack_full<<<nblk(dim), 256, 0, s>>>(n, me, m, d.q2e.p, d.sc.p, d.xsol.p, v.dx, v.dy, v.dz));
    if (m > 0) KLAUNCH(h, KC_VECTOR, k_dw<<<nblk(m), 256, 0, s>>>(m, d.C.ptr.p, d.C.col.p, d.C.src.p, d.vals.p, v.dx, v.r3, v.z, v.w, v.r4, v.dz, v.dw));
  } else if (no_fused_vectors()) {
    KLAUNCH(h, KC_VECTOR, k_unpack_red<<<nblk(dim), 256, 0, s>>>(n, me, d.q2e.p, d.sc.p, d.xsol.p, v.dx, v.dy));
    if (m > 0)
      KLAUNCH(h, KC_VECTOR, k_red_dzdw<<<nblk(m), 256, 0, s>>>(m, d.C.ptr.p, d.C.col.p, d.C.src.p, d.vals.p, v.dx, d.wt.p, d.tz.p, v.r3, v.dz, v.dw));
  } else {
    // (dx, dy and the dz, dw that need dx in one launch: kernels.hip.h, k_unpack_dzdw)
    const int nb_dzdw = m > 0 ? nblk(m) : 0;
    KLAUNCH(h, KC_VECTOR, k_unpack_dzdw<<<nb_dzdw + nblk(dim), 256, 0, s>>>(n, me, m, nb_dzdw, d.q2e.p, d.sc.p, d.xsol.p, v.dx, v.dy, d.C.ptr.p, d.C.col.p, d.C.src.p,
                                                                          d.vals.p, d.wt.p, d.tz.p, v.r3, v.dz, v.dw));
  }
}

// phases: 1 = right-hand side + forward sweep over this rank's subtrees,
// 2 = forward / backward over the replicated top, backward over the subtrees,
// 4 = unscale + scatter of the solution (7 = everything, the single-rank case)
static int run_step(hqpkkt_t *h, const Vecs &v, int phases) {
  if (phases & 1) {
    rhs(h, v);
    forward(h, 0);
  }
  if (phases & 2) {
    forward(h, 1);
    if (h->plan.top.n > 0) solve_top(h);
    backward(h, 1);
    backward(h, 0);
    if (h->an.shard_count > 1)  // leave only this rank's share for the all-reduce
      KLAUNCH(h, KC_VECTOR, k_mask_vector<<<nblk(h->an.dim), 256, 0, h->stream>>>(h->an.dim, h->td.keep_e.p, h->td.xsol.p));
  }
  if (phases & 4) unpack(h, v);
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
  const long long lpr = h->short_rows ? 4 : 16;  // lanes per CSR row
  const auto kernel = h->short_rows ? &k_residual<4> : &k_residual<16>;
  KLAUNCH(h, KC_RESIDUAL, kernel<<<std::min(nblk(lpr * ((long long)n + me + m)), 1024), 256, 0, s>>>(
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
  const int ntop = h->plan.top.n;  // (as it stands now: a poll that gives up below drops the top from the plan)
  if (!h->factored || ntop <= 0) return HQPKKT_E_INTERN;
  if (cap < ntop * 8) return HQPKKT_E_SIZES;
  HIPCHK(hipSetDevice(h->opts.device));
  DBuf<unsigned long long> st;
  if (st.alloc(8 * (size_t)ntop)) return HQPKKT_E_MEM;
  (void)hipMemset(st.p, 0, sizeof(unsigned long long) * 8 * ntop);
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
  std::vector<unsigned long long> hs(8 * (size_t)ntop);
  if (!e && hipMemcpy(hs.data(), st.p, sizeof(unsigned long long) * hs.size(), hipMemcpyDeviceToHost) != hipSuccess) e = HQPKKT_E_DEVICE;
  if (e) return e;
  std::vector<int> nodes(ntop);
  HIPCHK(hipMemcpy(nodes.data(), h->td.top_nodes.p, sizeof(int) * ntop, hipMemcpyDeviceToHost));
  unsigned long long t0 = ~0ULL;
  for (int t = 0; t < ntop; t++) t0 = std::min(t0, hs[8 * (size_t)t]);
  for (int t = 0; t < ntop; t++) {
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
// variant 0 = k_factor_blk as run_factor launches it (the instance fb_instance(p) of tree_plan.hpp), 1 = k_factor_diag
// (p <= 128), 2 = the 12-wavefront instance with eight blocks whatever p, 3 = the 12-wavefront instance with six blocks
// (where it holds p).  Out: the block's panel (p x p column-major: unit lower L11
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
  if ((e = raise_fb_lds(fb_lds_bytes(fb_instances[FB_INSTANCES - 1].maxp)))) return e;
  // variant 0: the rule's choice; 3: the six-block instance where it holds p; 2 (and 3 beyond): the eight-block instance.
  // (The 12-wavefront instances lay their images out with the leading dimension of more than fb_instances[0].maxp pivots.)
  const int inst = variant == 0 ? fb_instance(p) : variant == 3 && p <= fb_instances[2].maxp ? 2 : 3;
  const size_t lds_blk = fb_lds_bytes(inst == 0 ? p : std::max(p, fb_instances[0].maxp + 1));
  const FactorArgs a{T, d_P.p, d_dinv.p, d_pt.p, d_lp.p, d_sg.p, d_W.p, d_loff.p, alpha, pivot_eps, kb, d_flags.p + 1, d_upd.p};
  EventOwner e0, e1;
  HIPCHK(hipEventCreate(&e0.h));
  HIPCHK(hipEventCreate(&e1.h));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(e0, 0));
  for (int rp = 0; rp < reps; rp++) {
    if (variant == 1)
      launch_factor(k_factor_diag, 1, FD_THREADS, lds_old, 0, a, d_nodes.p + rp);
    else
      launch_factor(fb_kernels[inst], 1, fb_instances[inst].threads, lds_blk, 0, a, d_nodes.p + rp);
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
