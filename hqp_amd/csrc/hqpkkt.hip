// C ABI of the MI355X KKT path (include/hqpkkt.h): handle management, symbolic phase and values, factor / step /
// residual / solve with the refinement of Hqp_IpMatrix::solve, getters and setters, profile, statistics.  The engines,
// the interior-point loops and the entries on the sparse Q are units of their own (hqpkkt_handle.hpp); the entry points
// here have C linkage by their declarations in include/hqpkkt.h.
#include "hqpkkt_handle.hpp"

char g_last_hip_error[512] = "";
std::atomic<long long> g_live_bufs[2];

namespace kktdev {
// MFMA layout self-test: C(16x16) = A(16x16) * B(16x16), all row-major
__global__ void k_mfma_selftest(const double *A, const double *B, double *C) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < 16; k0 += 4)
    acc = mfma_f64(A[lr * 16 + k0 + lk], B[(k0 + lk) * 16 + lr], acc);
  for (int rg = 0; rg < 4; rg++) C[(lk + 4 * rg) * 16 + lr] = acc[rg];
}
}  // namespace kktdev

int hqpkkt_default_opts(hqpkkt_opts *o) {
  if (!o) return HQPKKT_E_NULL;
  std::memset(o, 0, sizeof(*o));
  o->mode = HQPKKT_MODE_FULL;
  o->device = 0;
  o->loc = HQPKKT_LOC_HOST;
  o->tol = 1.0;    // hqp/Hqp_IpSpBKP.C:46
  o->eps = 1e-10;  // hqp/Hqp_IpMatrix.C:45
  o->pivot_eps = 1e-20;  // only (near-)exact zeros are replaced: the reference accepts any non-zero pivot
  o->leaf_size = 0;
  o->max_pivots = 0;
  o->zd_policy = -1;  // by the values (hqpkkt_set_values)
  o->slack_policy = 2;
  return 0;
}

int hqpkkt_create(const hqpkkt_opts *opts, hqpkkt_t **out) {
  if (!out) return HQPKKT_E_NULL;
  hqpkkt_opts o;
  if (opts)
    o = *opts;
  else
    hqpkkt_default_opts(&o);
  if (o.mode != HQPKKT_MODE_FULL && o.mode != HQPKKT_MODE_REDUCED && o.mode != HQPKKT_MODE_STAGED) return HQPKKT_E_RANGE;
  if (!(o.tol > 0.0 && o.tol <= 1.0)) return HQPKKT_E_RANGE;  // hqp/spBKP.C:389-390
  if (o.loc != HQPKKT_LOC_HOST && o.loc != HQPKKT_LOC_DEVICE) return HQPKKT_E_RANGE;
  hqpkkt_t *h = new (std::nothrow) hqpkkt;
  if (!h) return HQPKKT_E_MEM;
  h->opts = o;
  std::memset(&h->st, 0, sizeof(h->st));
  h->st.sbw = -1;
  *out = h;
  return 0;
}

int hqpkkt_destroy(hqpkkt_t *h) {
  if (!h) return 0;
  if (h->own_stream) {
    (void)hipSetDevice(h->opts.device);
    (void)hipStreamSynchronize(h->own_stream);
  }
  delete h;  // (the members free what they own: buffers and graphs first, the stream last)
  return 0;
}

static int run_analysis(hqpkkt_t *h, int n, int me, int m, int zd);

int hqpkkt_analyze(hqpkkt_t *h, int n, int me, int m, const int *Qp, const int *Qi,
                   const int *Ap, const int *Ai, const int *Cp, const int *Ci, int *sbw) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if ((n > 0 && (!Qp || (Qp[n] > 0 && !Qi))) || (me > 0 && (!Ap || (Ap[me] > 0 && !Ai))) ||
        (m > 0 && (!Cp || (Cp[m] > 0 && !Ci))))
      return HQPKKT_E_NULL;
    if (h->uploaded) {
      (void)hipSetDevice(h->opts.device);
      (void)hipStreamSynchronize(h->stream);
      h->release_device();
    }
    h->analyzed = false;
    h->ip_hot_valid = h->fr_hot_valid = false;
    auto keep = [](std::vector<int> &dst, const int *src, size_t k) {
      dst.clear();
      if (src && k) dst.assign(src, src + k);
    };
    keep(h->pQp, Qp, n ? (size_t)n + 1 : 0), keep(h->pQi, Qi, n ? (size_t)Qp[n] : 0);
    keep(h->pAp, Ap, me ? (size_t)me + 1 : 0), keep(h->pAi, Ai, me ? (size_t)Ap[me] : 0);
    keep(h->pCp, Cp, m ? (size_t)m + 1 : 0), keep(h->pCi, Ci, m ? (size_t)Cp[m] : 0);
    h->zd_decided = h->opts.zd_policy >= 0;
    h->zd_weak = false;
    if (h->opts.mode == HQPKKT_MODE_STAGED) {
      h->zd_decided = true;
      int es = staged_analyze(h, n, me, m);
      if (es) return es;
      if (sbw) *sbw = -1;
      return 0;
    }
    int e = run_analysis(h, n, me, m, h->zd_decided ? h->opts.zd_policy : 2);
    if (e) return e;
    if (sbw) *sbw = h->an.sbw;
    return 0;
  });
}

// the symbolic phase with the zero-diagonal policy zd (hqpkkt_analyze; once more from
// hqpkkt_set_values when zd_policy -1 sees weak Hessian diagonals)
static int run_analysis(hqpkkt_t *h, int n, int me, int m, int zd) {
  h->an = Analysis();
  h->an.shard_rank = h->shard_rank, h->an.shard_count = h->shard_count;
  h->an.slack_policy = h->opts.slack_policy;
  h->an.small_fronts = !h->opts.no_small_fronts;
  h->an.amalgamation = h->opts.amalgamation != 0;
  h->an.ordering = (h->opts.ordering == 1 || h->opts.ordering == 2) ? h->opts.ordering : 0;
  if (h->opts.upd_pingpong_mb > 0) h->an.upd_pingpong_bytes = (long long)h->opts.upd_pingpong_mb << 20;
  if (h->opts.upd_pingpong_mb < 0) h->an.upd_pingpong_bytes = 0;
  // pivots per supernode: the caller's number (k_factor_blk takes up to 192), or 160 - ten blocks of 16, the widest
  // front whose M = L11^-1 stays in LDS next to L21 in registers for both sweeps of k_solve_top, so that ALL levels of
  // a banded system's tree go through its two launches (C2: 2.27 ms per factor + solve against 2.33 with 192, where
  // the leaf level stays outside).  HQPKKT_MAX_PIVOTS for same-box comparisons; k_factor_diag of rounds 1-3
  // (hqpkkt_debug_factor_block only) takes 128.
  // Separators of >= LONG_CHAIN_VERTS vertices (irregular graphs) are cut into pieces of 192 all the same: their fronts go
  // through the per-level kernels anyway, and the update blocks are rewritten 17 % less often (1e6-cell mesh with far
  // couplings: 154 ms per factor + solve against 162).
  int maxp = h->opts.max_pivots;
  h->an.long_chain_pivots = (maxp <= 0 && !getenv("HQPKKT_MAX_PIVOTS")) ? 192 : 0;
  if (maxp <= 0) maxp = getenv("HQPKKT_MAX_PIVOTS") ? std::atoi(getenv("HQPKKT_MAX_PIVOTS")) : 160;
  int e = h->an.run(h->opts.mode, n, me, m, h->pQp.data(), h->pQi.data(), h->pAp.data(), h->pAi.data(),
                    h->pCp.data(), h->pCi.data(), h->opts.leaf_size, maxp, zd);
  if (e) return e;
  h->zd_used = zd;
  h->analyzed = true;
  Analysis &an = h->an;
  h->st.dim = an.dim, h->st.sbw = an.sbw, h->st.n_supernodes = an.nnodes;
  h->st.n_levels = an.nlevels, h->st.max_front = an.max_front;
  h->st.nnz_kkt = (long long)an.ent_a.size();
  h->st.nnz_factor = an.nnz_factor, h->st.flops_factor = an.flops_factor;
  h->st.bytes_panels = (long long)sizeof(double) * (an.panel_elems + an.x_elems);
  h->st.bytes_updates = (long long)sizeof(double) * an.upd_elems;
  h->st.shard_rank = an.shard_rank, h->st.shard_count = an.shard_count;
  h->st.n_top = an.sched[1].nnodes, h->st.n_exchange_blocks = (int)an.xroots.size();
  h->st.flops_local = an.sched[0].flops, h->st.flops_top = an.sched[1].flops;
  h->st.bytes_exchange_factor = (long long)sizeof(double) * an.upd_x_slot * (an.xroots.empty() ? 0 : an.shard_count);
  h->st.bytes_exchange_step =
      an.shard_count > 1 ? (long long)sizeof(double) * (an.cb_x_slot * an.shard_count + an.dim) : 0;
  return 0;
}

// The values Qx | Ax | Cx are in the handle (tree engine): the CSR copies, the weak-diagonal test of zd_policy -1 and
// the host copies it keeps.  Qx, Ax, Cx: the caller's arrays the values came from.  q_only (the hqpkkt_q_* entries that
// write Q): A and C are as they were - of the copies Qf alone is gathered again, and the kept host copies come from
// the device.
int values_changed(hqpkkt_t *h, bool q_only, const double *Qx, const double *Ax, const double *Cx) {
  Analysis &an = h->an;
  int e;
  for (CsrBuf *c : {&h->td.Qf, &h->td.A, &h->td.AT, &h->td.C, &h->td.CT})
    if (c->src.count && (!q_only || c == &h->td.Qf))
      k_gather_values<<<nblk((long long)c->src.count), 256, 0, h->stream>>>((int)c->src.count, c->src.p, h->td.vals.p, c->val.p);
  if (h->opts.zd_policy < 0 && h->zd_used != 0) {
    // zd_policy -1: an x whose Hessian diagonal is weak against its coupling to an equality needs the
    // 2x2 pivot with that equality's multiplier inside its own pivot block.  Tested on EVERY update (the
    // values of an SQP run change: an identity Hessian may turn weak later), on the device: one pass
    // over Q's diagonal and the columns of A, one word read back.
    h->zd_decided = true;
    int *flag = h->td.flags.p + 100;
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), h->stream));
    if (an.n > 0 && an.me > 0)
      k_zd_weak<<<nblk(an.n), 256, 0, h->stream>>>(an.n, h->td.Qf.dev(), h->td.AT.dev(), flag);
    int *hs = (int *)h->kept.hpin.p;
    HIPCHK(hipMemcpyAsync(hs, flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->zd_weak = hs[0] != 0;
    if (h->zd_weak) {  // what the switch to policy 0 will need: the values on the host
      auto keep = [&](std::vector<double> &dst, const double *src, size_t k) -> int {
        dst.resize(k);
        if (!k) return 0;
        if (h->opts.loc == HQPKKT_LOC_DEVICE || q_only)
          HIPCHK(hipMemcpy(dst.data(), src, sizeof(double) * k, hipMemcpyDeviceToHost));
        else
          std::memcpy(dst.data(), src, sizeof(double) * k);
        return 0;
      };
      if (q_only) Qx = h->td.vals.p, Ax = Qx + an.nq, Cx = Ax + an.na;
      if ((e = keep(h->hQ, Qx, an.nq)) || (e = keep(h->hA, Ax, an.na)) || (e = keep(h->hC, Cx, an.nc))) return e;
    }
  }
  if (!q_only || h->opts.loc != HQPKKT_LOC_DEVICE) HIPCHK(hipStreamSynchronize(h->stream));
  h->have_values = true;
  h->factored = false;
  return 0;
}

int hqpkkt_set_values(hqpkkt_t *h, const double *Qx, const double *Ax, const double *Cx) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (!h->analyzed) return HQPKKT_E_INTERN;
    Analysis &an = h->an;
    if ((an.nq && !Qx) || (an.na && !Ax) || (an.nc && !Cx)) return HQPKKT_E_NULL;
    int e;
    if (h->opts.mode == HQPKKT_MODE_STAGED) return staged_set_values(h, Qx, Ax, Cx);
    if (!h->uploaded && (e = upload(h))) return e;
    HIPCHK(hipSetDevice(h->opts.device));
    hipMemcpyKind kind =
        h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (an.nq) HIPCHK(hipMemcpyAsync(h->td.vals.p, Qx, sizeof(double) * an.nq, kind, h->stream));
    if (an.na) HIPCHK(hipMemcpyAsync(h->td.vals.p + an.nq, Ax, sizeof(double) * an.na, kind, h->stream));
    if (an.nc)
      HIPCHK(hipMemcpyAsync(h->td.vals.p + an.nq + an.na, Cx, sizeof(double) * an.nc, kind, h->stream));
    return values_changed(h, false, Qx, Ax, Cx);
  });
}

// zd_policy -1, weak Hessian diagonals, a solve whose refinement did not reach mat_eps: from now
// on every multiplier right behind a matched neighbour (policy 0).  Symbolic phase, upload and
// values again (hqpkkt_mehrotra's vectors stay); the caller factorises and solves once more.
static int switch_to_policy0(hqpkkt_t *h) {
  if (getenv("HQPKKT_TRACE_SOLVE")) fprintf(stderr, "solve: refinement failed with weak Hessian diagonals: zero-diagonal placement 2 -> 0, factorising again\n");
  HIPCHK(hipSetDevice(h->opts.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  const bool lazy = h->lazy, hot = h->ip_hot_valid;
  const int loc = h->opts.loc;
  h->release_device(true);
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  int e = run_analysis(h, n, me, m, 0);
  if (e) return e;
  h->opts.loc = HQPKKT_LOC_HOST;  // the kept values are host copies
  h->lazy = false;
  e = hqpkkt_set_values(h, h->hQ.data(), h->hA.data(), h->hC.data());
  h->opts.loc = loc, h->lazy = lazy, h->ip_hot_valid = hot;
  return e;
}

// inside the device-resident loops (lazy) of the tree engine on one GPU: no staging copies, the sequences are captured
// on the caller's device vectors (hqpkkt_t::DirectGraph)
static bool direct_vectors(const hqpkkt_t *h) {
  return getenv("HQPKKT_NO_DIRECT_VECTORS") == nullptr && (h->lazy || h->direct_now) && h->opts.loc == HQPKKT_LOC_DEVICE &&
         h->opts.mode != HQPKKT_MODE_STAGED && h->an.shard_count <= 1 && h->use_graphs;
}
// A caller's own factor / solve calls (not the device-resident loops): direct from the SECOND call in a row with the same
// set of pointers (a caller that passes fresh vectors every time would pay a graph capture per call), and only if no
// two of the vectors overlap (the staging copies read every input before any output is written; the sequences do not).
struct DirectCall {
  hqpkkt_t *h;
  DirectCall(hqpkkt_t *h_, const void *const *ptr, const int *len, int count, const void **last) : h(h_) {
    bool same = !h->lazy && h->an.m > 0;
    for (int i = 0; i < count; i++) same = same && ptr[i] == last[i] && (ptr[i] != nullptr || len[i] == 0);
    for (int i = 0; i < count; i++) last[i] = ptr[i];
    for (int i = 0; same && i < count; i++)
      for (int j = i + 1; j < count; j++) {
        const char *a = (const char *)ptr[i], *b = (const char *)ptr[j];
        if (len[i] > 0 && len[j] > 0 && a < b + sizeof(double) * (size_t)len[j] && b < a + sizeof(double) * (size_t)len[i]) same = false;
      }
    h->direct_now = same;
  }
  ~DirectCall() { h->direct_now = false; }
};
// the vectors a solve works on: the caller's (direct_vectors) or the staging buffers, filled
int solve_vecs(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
               const double *r4, double *dx, double *dy, double *dz, double *dw, Vecs &v) {
  if (direct_vectors(h)) {
    v.z = z, v.w = w, v.r1 = r1, v.r2 = r2, v.r3 = r3, v.r4 = r4, v.dx = dx, v.dy = dy, v.dz = dz, v.dw = dw;
    return 0;
  }
  int e = stage_in(h, z, w, r1, r2, r3, r4, v);
  if (e) return e;
  stage_out_ptrs(h, v);
  return 0;
}

static int factor_once(hqpkkt_t *h, const double *z, const double *w);
// (a polled launch that gave up has switched the handle to the per-level launches: once more, then)
int hqpkkt_factor(hqpkkt_t *h, const double *z, const double *w) {
  int e = factor_once(h, z, w);
  if (e == HQPKKT_E_POLL) e = factor_once(h, z, w);
  return e == HQPKKT_E_POLL ? HQPKKT_E_DEVICE : e;
}
static int factor_once(hqpkkt_t *h, const double *z, const double *w) {
  if (!h) return HQPKKT_E_NULL;
  if (!h->analyzed || !h->have_values) return HQPKKT_E_INTERN;
  if (h->an.m > 0 && (!z || !w)) return HQPKKT_E_NULL;
  HIPCHK(hipSetDevice(h->opts.device));
  const void *const fp[2] = {z, w};
  const int fl[2] = {h->an.m, h->an.m};
  DirectCall direct_call(h, fp, fl, 2, h->last_f);
  Vecs v{};
  int e = 0;
  // a caller's own call on its DEVICE vectors (from the second one in a row with the same pointers: DirectCall): the
  // sequence and the posted status words as one graph as well, no timing events in the chain
  const bool devg = !h->lazy && direct_vectors(h) && h->use_graphs && !h->prof.on && getenv("HQPKKT_NO_HOST_GRAPHS") == nullptr;
  const bool hostg = devg || (host_graphs_ok(h) && !direct_vectors(h));
  const auto wall0 = std::chrono::steady_clock::now();
  if (devg) {
    v.z = z, v.w = w;
    h->factored = false;
    const void *key[10] = {z, w, (const void *)(intptr_t)1};
    if ((e = graphed(h, h->direct_slot(h->gdirect_call, key), [&]() {
           const int e2 = do_factor(h, v);
           return e2 ? e2 : post_words(h, nullptr, 0);
         })))
      return e;
  } else if (hostg) {
    // packed by the CPU, then ONE graph: the copy out of the pinned buffer, the factorisation, the posted status words
    const size_t used = stage_pack(h, z, w, nullptr, nullptr, nullptr, nullptr);
    const int m = h->an.m;
    v.z = h->td.vin.p, v.w = h->td.vin.p + m;
    h->factored = false;
    if ((e = graphed(h, h->ghost_factor, [&]() {
           if (used) {
             CopyList L{{h->td.hstage.dev, nullptr, nullptr, nullptr, nullptr, nullptr}, {h->td.vin.p, nullptr, nullptr, nullptr, nullptr, nullptr}, {(int)used, 0, 0, 0, 0, 0}};
             k_copy_vectors<<<copy_blocks(L), 256, 0, h->stream>>>(L, 1);
           }
           const int e2 = do_factor(h, v);
           return e2 ? e2 : post_words(h, nullptr, 0);
         })))
      return e;
  } else {
  if (direct_vectors(h))
    v.z = z, v.w = w;
  else if ((e = stage_in(h, z, w, nullptr, nullptr, nullptr, nullptr, v)))
    return e;
  h->factored = false;
  // (inside the device-resident loops - lazy - nobody reads these times, and an event record between two graph launches
  // is a packet the queue stops at: 22 us between the factorisation and the first solve of an iteration with three of
  // them, profiles/r06_ip_did_timeline.txt)
  if (!h->lazy) HIPCHK(hipEventRecord(h->ev0, h->stream));
  if ((e = do_factor(h, v))) return e;
  if (h->use_graphs && !h->prof.on && !h->lazy) {  // phases are not timed separately inside a graph replay
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventRecord(h->evs1, h->stream));
  }
  if (h->lazy) {
    h->factor_unchecked = true, h->factored = true;
    return 0;
  }
  }
  int *hs = (int *)h->kept.hpin.p;
  {  // the status words, posted (k_post_words) and waited for
    int ep = hostg ? 0 : post_words(h, nullptr, 0);
    if (ep || (ep = post_wait(h))) return ep;
  }
  if (poll_fallback(h, hs)) return HQPKKT_E_POLL;  // (factored stays false)
  const int flags[4] = {hs[0], hs[1], hs[2], hs[3]};
  std::memcpy(&h->st.kmax, hs + 120, sizeof(double));
  h->prof.collect();
  if (hostg) {  // (no events in the chain: the call's wall time, copies and read-back included)
    h->st.ms_assemble = 0.f;
    h->st.ms_factor = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  } else if (h->use_graphs && !h->prof.on) {
    h->st.ms_assemble = 0.f;  // inside the replayed graph
    h->st.ms_factor = elapsed(h->ev0, h->evs1);
  } else {
    h->st.ms_assemble = elapsed(h->ev0, h->ev1);
    h->st.ms_factor = elapsed(h->ev1, h->evs1);
  }
  h->st.n_2x2 = flags[1], h->st.n_perturbed = flags[2], h->st.n_slow_pivots = flags[3];
  h->soft_singular = hs[4] != 0;
  h->soft_tiny = hs[5] != 0;
  if (getenv("HQPKKT_TRACE_SOLVE") && (flags[0] || hs[4] || hs[5]))
    fprintf(stderr, "factor: status %d, 2x2 %d, perturbed %d, zero pivot perturbed %d, tiny multiplier pivot %d, kmax %.3e\n", flags[0],
            flags[1], flags[2], hs[4], hs[5], h->st.kmax);
  if (flags[0]) return flags[0];
  if (!(h->st.kmax == h->st.kmax) || std::isinf(h->st.kmax)) return HQPKKT_E_SING;
  h->factored = true;
  return 0;
}

static int step_once(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
                     const double *r4, double *dx, double *dy, double *dz, double *dw);
int hqpkkt_step(hqpkkt_t *h, const double *z, const double *w, const double *r1,
                const double *r2, const double *r3, const double *r4, double *dx, double *dy,
                double *dz, double *dw) {
  int e = step_once(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw);
  if (e == HQPKKT_E_POLL) e = step_once(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw);
  return e == HQPKKT_E_POLL ? HQPKKT_E_DEVICE : e;
}
static int step_once(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
                     const double *r4, double *dx, double *dy, double *dz, double *dw) {
  if (!h) return HQPKKT_E_NULL;
  if (!h->factored) return HQPKKT_E_INTERN;
  HIPCHK(hipSetDevice(h->opts.device));
  Vecs v{};
  int e = stage_in(h, z, w, r1, r2, r3, r4, v);
  if (e) return e;
  stage_out_ptrs(h, v);
  HIPCHK(hipEventRecord(h->evs0, h->stream));
  if ((e = do_step(h, v, 0))) return e;
  HIPCHK(hipEventRecord(h->evs1, h->stream));
  if ((e = stage_out(h, v, dx, dy, dz, dw))) return e;
  int *hs = (int *)h->kept.hpin.p;  // the give-up word of the polled sweeps comes back with the result
  HIPCHK(hipMemcpyAsync(hs + XW_GAVE_UP, h->td.flags.p + XW_GAVE_UP, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (poll_fallback(h, hs)) return HQPKKT_E_POLL;
  unstage(h, dx, dy, dz, dw);
  h->prof.collect();
  h->st.ms_step = elapsed(h->evs0, h->evs1);
  return 0;
}

int hqpkkt_residual(hqpkkt_t *h, const double *z, const double *w, const double *r1,
                    const double *r2, const double *r3, const double *r4, const double *dx,
                    const double *dy, const double *dz, const double *dw, double *res) {
  if (!h || !res) return HQPKKT_E_NULL;
  if (!h->have_values) return HQPKKT_E_INTERN;
  HIPCHK(hipSetDevice(h->opts.device));
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  Vecs v{};
  int e = stage_in(h, z, w, r1, r2, r3, r4, v);
  if (e) return e;
  stage_out_ptrs(h, v);
  if (h->opts.loc == HQPKKT_LOC_DEVICE) {
    CopyList L{{dx, dy, dz, dw, nullptr, nullptr}, {v.dx, v.dy, v.dz, v.dw, nullptr, nullptr}, {n, me, m, m, 0, 0}};
    k_copy_vectors<<<copy_blocks(L), 256, 0, h->stream>>>(L, 4);
  } else {
    if (n) HIPCHK(hipMemcpyAsync(v.dx, dx, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    if (me) HIPCHK(hipMemcpyAsync(v.dy, dy, sizeof(double) * me, hipMemcpyHostToDevice, h->stream));
    if (m) HIPCHK(hipMemcpyAsync(v.dz, dz, sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
    if (m) HIPCHK(hipMemcpyAsync(v.dw, dw, sizeof(double) * m, hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipEventRecord(h->evs0, h->stream));
  e = run_residual(h, v, res);
  if (e == HQPKKT_E_POLL) e = HQPKKT_E_DEVICE;  // (a stale word: the residual kernels poll nothing)
  HIPCHK(hipEventRecord(h->evs1, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->prof.collect();
  h->st.ms_residual = elapsed(h->evs0, h->evs1);
  return e;
}

// Hqp_IpMatrix::solve (hqp/Hqp_IpMatrix.C:65-128)
static int solve_once(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
                      const double *r4, double *dx, double *dy, double *dz, double *dw, double *res_out);
int hqpkkt_solve(hqpkkt_t *h, const double *z, const double *w, const double *r1,
                 const double *r2, const double *r3, const double *r4, double *dx, double *dy,
                 double *dz, double *dw, double *res_out) {
  int e = solve_once(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, res_out);
  // a polled sweep gave up: the factors are those of the per-level kernels as well (bit-identical), the solve runs again
  // on the per-level launches.  (Inside the device-resident loops - lazy - the loop itself is run again.)
  if (e == HQPKKT_E_POLL && h->factored && !h->lazy) e = solve_once(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, res_out);
  return e == HQPKKT_E_POLL && !h->lazy ? HQPKKT_E_DEVICE : e;
}
static int solve_once(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
                      const double *r4, double *dx, double *dy, double *dz, double *dw, double *res_out) {
  if (!h) return HQPKKT_E_NULL;
  if (!h->factored) return HQPKKT_E_INTERN;
  HIPCHK(hipSetDevice(h->opts.device));
  hipStream_t s = h->stream;
  const void *const sp[10] = {z, w, r1, r2, r3, r4, dx, dy, dz, dw};
  const int sl[10] = {h->an.m, h->an.m, h->an.n, h->an.me, h->an.m, h->an.m, h->an.n, h->an.me, h->an.m, h->an.m};
  DirectCall direct_call(h, sp, sl, 10, h->last_s);
  Vecs v{};
  int e = 0;
  if (!h->lazy && direct_vectors(h) && h->use_graphs && !h->prof.on && getenv("HQPKKT_NO_HOST_GRAPHS") == nullptr) {
    // a caller's own solve on its DEVICE vectors: sweeps, residual and the posted words as one graph
    const auto wall0 = std::chrono::steady_clock::now();
    if ((e = solve_vecs(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, v))) return e;
    const void *key[10] = {z, w, r1, r2, r3, r4, dx, dy, dz, (const void *)((const char *)dw + 1)};  // (+ 1: not the key of the sequence's own graph)
    if ((e = graphed(h, h->direct_slot(h->gdirect_call, key), [&]() {
           int e2 = do_step(h, v, 0);
           if (e2 || (e2 = residual_launch(h, v))) return e2;
           return post_words(h, nullptr, 0, true);
         })))
      return e;
    double res = 0.0;
    if ((e = post_wait(h)) || (e = collect_residual(h, &res))) return e;
    h->host_graph_call = true;
    e = solve_tail(h, v, z, w, r1, r2, r3, r4, dx, dy, dz, dw, res, res_out);
    h->host_graph_call = false;
    h->st.ms_solve = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return e;
  }
  {
    bool all = host_graphs_ok(h) && !direct_vectors(h) && h->td.hstage_out;
    for (int k = 0; k < 10; k++) all = all && (sp[k] != nullptr || sl[k] == 0);
    if (all) {
      // packed by the CPU, then ONE graph: the copy out of the pinned buffer, the sweeps, the residual, the result into
      // the pinned buffer, the posted words (residual and status); the CPU hands the result out when they have arrived
      const auto wall0 = std::chrono::steady_clock::now();
      const size_t used = stage_pack(h, z, w, r1, r2, r3, r4);
      const int n = h->an.n, me = h->an.me, m = h->an.m;
      double *b = h->td.vin.p;
      v.z = b, v.w = b + m, v.r1 = b + 2 * (size_t)m, v.r2 = v.r1 + n, v.r3 = v.r2 + me, v.r4 = v.r3 + m;
      stage_out_ptrs(h, v);
      if ((e = graphed(h, h->ghost_step, [&]() {
             if (used) {
               CopyList L{{h->td.hstage.dev, nullptr, nullptr, nullptr, nullptr, nullptr}, {b, nullptr, nullptr, nullptr, nullptr, nullptr}, {(int)used, 0, 0, 0, 0, 0}};
               k_copy_vectors<<<copy_blocks(L), 256, 0, s>>>(L, 1);
             }
             int e2 = do_step(h, v, 0);
             if (e2 || (e2 = residual_launch(h, v))) return e2;
             CopyList O{{v.dx, nullptr, nullptr, nullptr, nullptr, nullptr}, {h->td.hstage.dev + h->td.hstage_in, nullptr, nullptr, nullptr, nullptr, nullptr}, {(int)h->td.hstage_out, 0, 0, 0, 0, 0}};
             k_copy_vectors<<<copy_blocks(O), 256, 0, s>>>(O, 1);
             return post_words(h, nullptr, 0, true);
           })))
        return e;
      h->out_pending = h->td.hstage.p + h->td.hstage_in, h->out_by_kernel = true;
      double res = 0.0;
      if ((e = post_wait(h)) || (e = collect_residual(h, &res))) return e;
      h->host_graph_call = true;
      e = solve_tail(h, v, z, w, r1, r2, r3, r4, dx, dy, dz, dw, res, res_out);
      h->host_graph_call = false;
      h->st.ms_solve = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
      return e;
    }
  }
  if ((e = solve_vecs(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, v))) return e;
  if (!h->lazy) HIPCHK(hipEventRecord(h->ev0, s));
  if ((e = do_step(h, v, 0))) return e;
  double res = 0.0;
  const OutPtrs outp{dx, dy, dz, dw};
  if ((e = run_residual(h, v, &res, (h->lazy || v.dx == dx) ? nullptr : &outp))) return e;
  if (h->residual_pending) {  // (hqpkkt_franke: solve_tail follows if the residual, once read, asks for it)
    if (res_out) *res_out = 0.0;
    return v.dx == dx ? 0 : stage_out(h, v, dx, dy, dz, dw);
  }
  return solve_tail(h, v, z, w, r1, r2, r3, r4, dx, dy, dz, dw, res, res_out);
}

// refinement and the checks of hqpkkt_solve, from the residual `res` of the first solution on
int solve_tail(hqpkkt_t *h, Vecs &v, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
               const double *r4, double *dx, double *dy, double *dz, double *dw, double res, double *res_out) {
  const int n = h->an.n, me = h->an.me, m = h->an.m;
  hipStream_t s = h->stream;
  int e;
  double res_last;
  const double target = h->refine_target > 0.0 ? std::fmin(h->opts.eps, h->refine_target) : h->opts.eps;
  const bool refined = res > target;  // otherwise the caller's copy is already complete
  const double res_first = res;
  double res_acc = res;  // residual of the solution as it stands (res is the last TRIAL's when that one was rejected, as in the reference)
  double res_acc_prev = HUGE_VAL;  // ... and before the last round
  // correction solve: rhs = residual vectors, result = vcor
  Vecs c = v;
  c.r1 = h->td.vres.p, c.r2 = c.r1 + n, c.r3 = c.r2 + me, c.r4 = c.r3 + m;
  c.dx = h->td.vcor.p, c.dy = c.dx + n, c.dz = c.dy + me, c.dw = c.dz + m;
  const int ntot = n + me + 2 * m;
  int rounds = 0;
  // (the reference makes at most five rounds, hqp/Hqp_IpMatrix.C:84: its factors come from a pivot search over the whole
  // remaining column.  Where THIS factorisation had to perturb a pivot, or met a multiplier pivot at rounding level -
  // the pivot search is confined to the supernode's block - the factors are those of a nearby matrix and the rounds
  // contract more slowly: up to fifteen then, as long as they still gain, so that solve() returns what the caller's
  // optimality test expects of an accurate factorisation - Hqp_IpsFranke compares the returned residual with its
  // eps, hqp/Hqp_IpsFranke.C:372)
  // (not behind a cancelled pivot that was USED as it was - soft_tiny alone: five rounds leave such factors at a residual
  // that says "singular", fifteen can drag a consistent singular system below mat_eps, and the reference reports it)
  // Only inside the device-resident loops (h->lazy): a caller's own hqpkkt_solve - the reference's solvers through the
  // shim - gets the reference's five rounds and with them the residual the reference's plugin contract describes
  // (ADVICE r5).  Rounds beyond five show in hqpkkt_stats.refine_rounds.
  const int max_rounds = (h->st.n_perturbed > 0 && h->lazy) ? 15 : 5;
  for (int it = 0; it < max_rounds && res > target; it++) {
    if (it >= 5 && !(res < 0.5 * res_acc_prev)) break;  // beyond the reference's five: only while a round still halves the residual
    res_last = res;
    if ((e = do_step(h, c, 1))) return e;
    rounds++;
    double alpha = 1.0;
    do {
      KLAUNCH(h, KC_VECTOR, k_axpy4<<<nblk(ntot), 256, 0, s>>>(n, me, m, alpha, c.dx, c.dy, c.dz, c.dw, v.dx, v.dy, v.dz,
                                         v.dw));
      if ((e = run_residual(h, v, &res))) return e;
      if (res > res_last) {
        KLAUNCH(h, KC_VECTOR, k_axpy4<<<nblk(ntot), 256, 0, s>>>(n, me, m, -alpha, c.dx, c.dy, c.dz, c.dw, v.dx, v.dy,
                                           v.dz, v.dw));
        alpha -= 0.3;
      }
    } while (res > res_last && alpha > 0.0);
    if (alpha <= 0.0) break;
    res_acc_prev = res_acc, res_acc = res;
  }
  if (!(res <= h->opts.eps) && h->zd_weak && h->zd_used == 2) {  // (sharded: every rank sees the same residual and switches)
    // the refinement did not reach mat_eps: weak Hessian diagonals and every multiplier behind
    // ALL its neighbours is the placement that loses accuracy when z/w spreads (hqpkkt_opts.
    // zd_policy); switch the handle to the matching rule and do this factor + solve again
    if ((e = switch_to_policy0(h)) || (e = hqpkkt_factor(h, z, w))) return e;
    return hqpkkt_solve(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, res_out);
  }
  if (!h->lazy && !h->host_graph_call) HIPCHK(hipEventRecord(h->ev1, s));
  if (h->lazy) {
    if (v.dx != dx && (e = stage_out(h, v, dx, dy, dz, dw))) return e;
  } else {
    if (refined && v.dx != dx) {
      if ((e = stage_out(h, v, dx, dy, dz, dw))) return e;
    }
    // (a call whose result a kernel has put into the pinned buffer in front of the posted words, and no refinement: it is there)
    if (!h->host_graph_call || rounds > 0 || refined) HIPCHK(hipStreamSynchronize(s));  // (returns at once when nothing was queued after the read-back)
    unstage(h, dx, dy, dz, dw);
    h->prof.collect();
    if (!h->host_graph_call) h->st.ms_solve = elapsed(h->ev0, h->ev1);
  }
  h->st.refine_rounds = rounds;
  if (getenv("HQPKKT_TRACE_SOLVE")) fprintf(stderr, "solve: first residual %.3e, %d rounds, final %.3e\n", res_first, rounds, res);
  if (res_out) *res_out = res;
  if (res != res) return HQPKKT_E_SING;
  // an exactly zero pivot outside a root front was perturbed: singular if the refinement failed
  if (h->soft_singular && !(res <= h->opts.eps)) return HQPKKT_E_SING;
  // a multiplier-type pivot below 1e-13 max|K| and a solve that ends no nearer to a solution than the zero
  // vector is: the rank-deficient equality block the reference reports as E_SING (hqp/spBKP.C:699-700).
  // (Not: a late interior-point system whose refinement stalls at 1e-4 - the reference goes on there.)
  if (h->soft_tiny && !(res_acc <= 1e-4)) {
    double rnorm = 0.0;
    Vecs vz = v;
    vz.dx = h->td.vcor.p, vz.dy = vz.dx + n, vz.dz = vz.dy + me, vz.dw = vz.dz + m;
    HIPCHK(hipMemsetAsync(h->td.vcor.p, 0, sizeof(double) * (size_t)ntot, s));
    if ((e = run_residual(h, vz, &rnorm))) return e;
    if (!(res_acc < rnorm)) return HQPKKT_E_SING;
  }
  return 0;
}

int hqpkkt_get_sbw(const hqpkkt_t *h, int *sbw) {
  if (!h || !sbw) return HQPKKT_E_NULL;
  *sbw = h->analyzed ? h->an.sbw : -1;
  return 0;
}

int hqpkkt_get_perm(const hqpkkt_t *h, int *perm) {
  if (!h || !perm) return HQPKKT_E_NULL;
  if (!h->analyzed) return HQPKKT_E_INTERN;
  if ((int)h->an.qp2j.size() != h->an.dim) return HQPKKT_E_INTERN;  // STAGED: stage order, no RCM
  std::memcpy(perm, h->an.qp2j.data(), sizeof(int) * h->an.dim);
  return 0;
}

int hqpkkt_set_tol(hqpkkt_t *h, double tol) {
  if (!h) return HQPKKT_E_NULL;
  if (!(tol > 0.0 && tol <= 1.0)) return HQPKKT_E_RANGE;
  if (tol != h->opts.tol) h->drop_graphs();  // alpha is baked into the captured launches
  h->opts.tol = tol;
  return 0;
}

int hqpkkt_set_eps(hqpkkt_t *h, double eps) {
  if (!h) return HQPKKT_E_NULL;
  h->opts.eps = eps;
  return 0;
}

int hqpkkt_set_stream(hqpkkt_t *h, void *hip_stream) {
  if (!h) return HQPKKT_E_NULL;
  int e = ensure_device(h);
  if (e) return e;
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  h->drop_graphs();
  return 0;
}

int hqpkkt_set_shard(hqpkkt_t *h, int rank, int count, hqpkkt_exchange_fn fn, void *ctx) {
  if (!h) return HQPKKT_E_NULL;
  if (count < 1 || rank < 0 || rank >= count) return HQPKKT_E_RANGE;
  if (count > 1 && !fn) return HQPKKT_E_NULL;
  if (h->analyzed && (rank != h->shard_rank || count != h->shard_count)) return HQPKKT_E_INTERN;
  h->shard_rank = rank, h->shard_count = count;
  h->xchg_fn = fn, h->xchg_sfn = nullptr, h->xchg_ctx = ctx;
  return 0;
}
int hqpkkt_set_shard_stream(hqpkkt_t *h, int rank, int count, hqpkkt_exchange_stream_fn fn, void *ctx) {
  if (!h) return HQPKKT_E_NULL;
  if (count < 1 || rank < 0 || rank >= count) return HQPKKT_E_RANGE;
  if (count > 1 && !fn) return HQPKKT_E_NULL;
  if (h->analyzed && (rank != h->shard_rank || count != h->shard_count)) return HQPKKT_E_INTERN;
  h->shard_rank = rank, h->shard_count = count;
  h->xchg_fn = nullptr, h->xchg_sfn = fn, h->xchg_ctx = ctx;
  return 0;
}

int hqpkkt_values_staging(hqpkkt_t *h, double **Qx, double **Ax, double **Cx) {
  if (!h || !Qx || !Ax || !Cx) return HQPKKT_E_NULL;
  if (!h->analyzed) return HQPKKT_E_INTERN;
  int e = ensure_device(h);
  if (e) return e;
  const Analysis &an = h->an;
  const size_t need = (size_t)an.nq + an.na + an.nc + 1;
  PinnedBuf<double> &hv = h->kept.hvals;
  if (hv.count != need) HIPCHK(hv.alloc(need, hipHostMallocDefault));  // (none yet, or analysed again for another pattern)
  *Qx = hv.p, *Ax = hv.p + an.nq, *Cx = hv.p + an.nq + an.na;
  return 0;
}


int hqpkkt_set_profile(hqpkkt_t *h, int on) {
  if (!h) return HQPKKT_E_NULL;
  h->prof.on = on != 0;
  h->prof.reset();
  return 0;
}

int hqpkkt_get_profile(const hqpkkt_t *h, int n_classes, double *ms, long long *launches) {
  if (!h || !ms || !launches) return HQPKKT_E_NULL;
  for (int c = 0; c < n_classes && c < KC_COUNT; c++) ms[c] = h->prof.ms[c], launches[c] = h->prof.launches[c];
  return KC_COUNT;
}

const char *hqpkkt_profile_class_name(int c) { return (c >= 0 && c < KC_COUNT) ? kc_names[c] : ""; }

int hqpkkt_get_stats(const hqpkkt_t *h, hqpkkt_stats *out) {
  if (!h || !out) return HQPKKT_E_NULL;
  *out = h->st;
  return 0;
}

const char *hqpkkt_strerror(int status) {
  switch (status) {
    case HQPKKT_OK: return "ok";
    case HQPKKT_E_SIZES: return "sizes of arguments mismatch";
    case HQPKKT_E_MEM: return "out of memory";
    case HQPKKT_E_SING: return "matrix is singular";
    case HQPKKT_E_FORMAT: return "CSR input not sorted / out of range";
    case HQPKKT_E_NULL: return "NULL objects passed";
    case HQPKKT_E_RANGE: return "parameter out of range";
    case HQPKKT_E_INTERN: return "call order violated";
    case HQPKKT_E_DEVICE: return g_last_hip_error[0] ? g_last_hip_error : "HIP device error";
    default: return "unknown status";
  }
}


int hqpkkt_debug_get(const hqpkkt_t *h, int what, int *out, long long *len) {
  if (!h || !len) return HQPKKT_E_NULL;
  if (!h->analyzed && what != 40) return HQPKKT_E_INTERN;
  const Analysis &an = h->an;
  const std::vector<int> *v = nullptr;
  std::vector<int> tmp;
  switch (what) {
    case 0: v = &an.q2e; break;
    case 1: v = &an.piv_start; break;
    case 2: v = &an.npiv; break;
    case 3: v = &an.nbor; break;
    case 4: v = &an.parent; break;
    case 5: v = &an.level; break;
    case 6:
      tmp.assign(an.bptr.begin(), an.bptr.end());
      v = &tmp;
      break;
    case 7: v = &an.bidx; break;
    case 8: v = &an.ent_er; break;
    case 9: v = &an.ent_ec; break;
    case 10: v = &an.node_owner; break;
    case 11: v = &an.xroots; break;
    case 20: case 21: case 22: case 23: case 24: case 25: case 26: case 27: case 28: case 32: case 33: case 34: case 35: case 36: case 37: case 38: case 39: case 41: case 42: case 43: case 44: case 45: case 46: case 47: {  // STAGED
      const int e = staged_debug_get(h, what, tmp);
      if (e) return e;
      v = &tmp;
      break;
    }
    case 30:  // zero-diagonal placement in use, and whether the last values have weak Hessian diagonals
      tmp = {h->zd_used, h->zd_weak ? 1 : 0};
      v = &tmp;
      break;
    case 31: case 48: {  // what the handle launches (tree_plan.hpp): the plan in use, or before the upload the one the switches give now
      TreePlan fly;
      if (!h->uploaded && h->opts.mode != HQPKKT_MODE_STAGED) fly = tree_plan(an, tree_switches(h));
      const TreePlan &P = h->uploaded ? h->plan : fly;
      if (P.err) return P.err;
      tmp = {P.top.n, P.top.n ? P.top.lt : an.nlevels, (int)P.top.lds, P.top.ns, P.small_tree ? 1 : 0, P.tree_factor ? 1 : 0, P.top.split ? 1 : 0};
      if (what == 31) {  // the solve's fused top (k_solve_top): number of fronts, first fused level, LDS bytes, ...
        v = &tmp;
        break;
      }
      for (int x : {P.tree_ldp, P.tree_ldb, (int)P.lds_panel, (int)P.lds_bwdb, (int)P.lds_blk, an.nlevels, LEVEL_PLAN_INTS, an.sched[0].nnodes, an.sched[1].nnodes}) tmp.push_back(x);
      for (int w = 0; w < 2; w++)
        for (int l = 0; l < an.nlevels; l++) {
          const LevelPlan R = l < (int)P.levels[w].size() ? P.levels[w][l] : LevelPlan();
          const int *r = (const int *)&R;
          tmp.insert(tmp.end(), r, r + LEVEL_PLAN_INTS);
        }
      v = &tmp;
      break;
    }
    case 40:  // live device / pinned host buffers of the process (DBuf / PinnedBuf, over all handles)
      tmp = {(int)g_live_bufs[0].load(), (int)g_live_bufs[1].load()};
      v = &tmp;
      break;
    default: return HQPKKT_E_RANGE;
  }
  *len = (long long)v->size();
  if (out && !v->empty()) std::memcpy(out, v->data(), sizeof(int) * v->size());
  return 0;
}

#ifdef HQPKKT_STAMPS
extern "C" int hqpkkt_debug_stamps(hqpkkt_t *h, int *out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, h->td.flags.p, sizeof(int) * 64, hipMemcpyDeviceToHost));
  return 0;
}
#endif

int hqpkkt_debug_read(hqpkkt_t *h, int what, int node, double *out, long long cap, long long *len) {
  if (!h || !len) return HQPKKT_E_NULL;
  if (!h->uploaded) return HQPKKT_E_INTERN;
  const Analysis &an = h->an;
  if (node < 0 || node >= an.nnodes) return HQPKKT_E_RANGE;
  const long long p = an.npiv[node], b = an.nbor[node];
  const double *src = nullptr;
  long long n = 0;
  switch (what) {
    case 0: src = h->td.panel.p + an.panel_off[node], n = (p + b) * p; break;
    case 1: src = h->td.linv.p + an.linv_off[node], n = p * p; break;
    case 2: src = h->td.xar.p + an.x_off[node], n = b * p; break;
    case 3: src = h->td.upd.p + an.upd_off[node], n = b * b; break;
    case 4: src = h->td.dinv.p + 2 * (long long)an.piv_start[node], n = 2 * p; break;
    case 5: case 6: n = p; break;  // ptype, lperm: ints, returned as doubles
    case 7: src = h->td.sc.p, n = an.dim; break;
    default: return HQPKKT_E_RANGE;
  }
  *len = n;
  if (!out) return 0;
  if (cap < n) return HQPKKT_E_SIZES;
  HIPCHK(hipSetDevice(h->opts.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (what == 5 || what == 6) {
    std::vector<int> iv((size_t)n);
    const int *isrc = (what == 5 ? h->td.ptype.p : h->td.lperm.p) + an.piv_start[node];
    if (n) HIPCHK(hipMemcpy(iv.data(), isrc, sizeof(int) * n, hipMemcpyDeviceToHost));
    for (long long t = 0; t < n; t++) out[t] = (double)iv[(size_t)t];
    return 0;
  }
  if (what == 3 && h->plan.tree_factor) {  // the block is in the exchange copy of the last factorisation (lower triangle; the rest idle)
    int ep = 0;
    HIPCHK(hipMemcpy(&ep, h->td.tree_words.p + 1, sizeof(int), hipMemcpyDeviceToHost));
    src = h->td.tree_u.p + (long long)(ep & 1) * an.upd_elems + an.upd_off[node];
  }
  if (n) HIPCHK(hipMemcpy(out, src, sizeof(double) * n, hipMemcpyDeviceToHost));
  if (what == 3 && h->plan.tree_factor)
    for (long long t = 0; t < n; t++)
      if (std::memcmp(out + t, &XW_SENTINEL, sizeof(double)) == 0) out[t] = 0.0;
  return 0;
}


int hqpkkt_selftest_mfma(int device, double *max_err) {
  if (!max_err) return HQPKKT_E_NULL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) return HQPKKT_E_DEVICE;
  HIPCHK(hipSetDevice(device));
  double A[256], B[256], Cx[256], Cd[256];
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 16; j++) {
      A[i * 16 + j] = (double)((i * 7 + j * 3) % 11 - 5);
      B[i * 16 + j] = (double)((i * 5 + j * 13) % 17 - 8);
    }
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 16; j++) {
      double s = 0;
      for (int k = 0; k < 16; k++) s += A[i * 16 + k] * B[k * 16 + j];
      Cx[i * 16 + j] = s;
    }
  DBuf<double> dA, dB, dC;
  if (dA.alloc(256) || dB.alloc(256) || dC.alloc(256)) return HQPKKT_E_MEM;
  HIPCHK(hipMemcpy(dA.p, A, sizeof(A), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dB.p, B, sizeof(B), hipMemcpyHostToDevice));
  k_mfma_selftest<<<1, 64>>>(dA.p, dB.p, dC.p);
  HIPCHK(hipMemcpy(Cd, dC.p, sizeof(Cd), hipMemcpyDeviceToHost));
  double err = 0;
  for (int i = 0; i < 256; i++) err = std::fmax(err, std::fabs(Cd[i] - Cx[i]));
  *max_err = err;
  return 0;
}
