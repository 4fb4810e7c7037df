// The device-resident interior-point loops of the C ABI (hqpkkt_mehrotra, hqpkkt_franke; their vector kernels in
// ipdriver.hip.h): they drive the handle through hqpkkt_factor / hqpkkt_solve and the posted read-backs.
#include "hqpkkt_handle.hpp"

#include "ipdriver.hip.h"

// The attempts of a device-resident loop (hqpkkt_mehrotra / hqpkkt_franke; `loop` reads the caller's `opts` through the
// reference it captured).  ONE rule ("Pivoting"): the factors are first those the reference's own
// loop gets from this plugin through the shim - a multiplier pivot that cancelled to rounding level is used as it
// stands -, and STATIC PIVOTING is the fall-back: a run that ends "degenerate" (or singular) is made again, from a cold
// start, with such pivots replaced (kernels.hip.h, TINY_REPLACE_WORD; what the reference's own PARDISO plugin is
// configured to do, hqp/Hqp_IpPARDISO.C:138-142).  hqpkkt_ip_result.attempts says which happened; plugin calls and device
// time are the totals over the attempts, `iters` is the count of the run that produced the result.  HQPKKT_TINY_IN_LOOP=1 / =0 (campaign switches): static
// pivoting from the first attempt on / never.
template <class Loop>
static int ip_attempts(hqpkkt_t *h, const hqpkkt_ip_opts *&opts, hqpkkt_ip_result *res, Loop loop) {
  hqpkkt_ip_opts again;
  auto cold = [&]() {  // (a first attempt has used up what a hot start would start from; "2" keeps what the NEXT call needs)
    if (opts && opts->hot_start == 1) {
      again = *opts;
      again.hot_start = 2;
      opts = &again;
    }
  };
  // (a polled launch that gave up has switched the handle to the per-level launches: the loop runs once more - from a cold
  // start: the aborted pass has left its own iterates in the loop's vectors and may have overwritten the hot-start candidates)
  auto attempt = [&]() {
    int rc = guarded(loop);
    if (rc == HQPKKT_E_POLL) {
      cold();
      if (h) h->ip_hot_valid = false, h->fr_hot_valid = false;
      rc = guarded(loop);
    }
    return rc == HQPKKT_E_POLL ? HQPKKT_E_DEVICE : rc;
  };
  static const char *const pol = getenv("HQPKKT_TINY_IN_LOOP");
  if (h) h->tiny_replace_in_loop = pol && atoi(pol) == 1;
  int rc = attempt();
  if (res && rc == 0) res->attempts = 1;
  if (h && res && !h->tiny_replace_in_loop && !(pol && atoi(pol) == 0) && (rc == HQPKKT_E_SING || (rc == 0 && res->result == 4))) {
    const hqpkkt_ip_result first = *res;  // (all zero but `result` when the first attempt ended with E_SING before its finish())
    const bool counted = rc == 0;
    h->tiny_replace_in_loop = true;
    cold();
    rc = attempt();
    h->tiny_replace_in_loop = false;
    if (rc == 0) {
      res->attempts = 2;
      if (counted)  // the work of both runs; `iters` stays the count of the run that gave the result (what the reference's count is compared with)
        res->n_factor += first.n_factor, res->n_solve += first.n_solve, res->ms_total += first.ms_total;
    }
  }
  return rc;
}

// ---- device-resident Mehrotra predictor-corrector loop ----------------------
// Restatement of hqp/Hqp_IpsMehrotra.C: cold_start (:209-327), step (:355-693),
// solve (:696-735, cold start only).  Scalars are reduced on the device in a fixed
// order and read back; vectors stay on the device.
namespace {
struct IpCtx {
  hqpkkt_t *h;
  int n, me, m;
  double *x, *y, *z, *w, *r1, *r2, *r3, *r4, *dxa, *dya, *dza, *dwa, *dx, *dy, *dz, *dw, *c, *b, *d, *part, *out;
  double *zh, *wh;  // hot-start candidates (hqp/Hqp_IpsMehrotra.C:475-478)
  double *hout;  // pinned (h->kept.hpin.p + 64)
  int reduce(const int (&ops)[IP_SLOTS], int nout) {
    IpOps o;
    for (int k = 0; k < IP_SLOTS; k++) o.op[k] = ops[k];
    k_ip_final<<<1, 256, 0, h->stream>>>(part, o, out, IpEpi{0, 0, 0.0, 0.0, 0.0, nullptr, nullptr});
    int e = post_words(h, out, nout);  // (hout = hpin + 64: where the posting kernel puts them)
    return e ? e : post_wait(h);
  }
};
}  // namespace

extern "C" {

int hqpkkt_default_ip_opts(hqpkkt_ip_opts *o) {
  if (!o) return HQPKKT_E_NULL;
  std::memset(o, 0, sizeof(*o));
  o->eps = 1e-10;       // hqp/Hqp_Solver.C:53
  o->max_iters = 200;   // hqp/Hqp_Solver.C:52
  o->gammaf = 0.01;     // hqp/Hqp_IpsMehrotra.C:95
  return 0;
}

int hqpkkt_mehrotra(hqpkkt_t *h, const hqpkkt_ip_opts *opts, const double *c, const double *b,
                    const double *d, double *x, double *y, double *z, double *w, hqpkkt_ip_result *res) {
  auto loop = [&]() -> int {
    if (!h || !res) return HQPKKT_E_NULL;
    if (!h->analyzed || !h->have_values) return HQPKKT_E_INTERN;
    if (opts && opts->max_iters < 0) return HQPKKT_E_RANGE;
      if (h->an.shard_count > 1) return HQPKKT_E_INTERN;
    hqpkkt_ip_opts o;
    if (opts)
      o = *opts;
    else
      hqpkkt_default_ip_opts(&o);
    Analysis &an = h->an;
    const int n = an.n, me = an.me, m = an.m;
    if ((n && !c) || (me && !b) || (m && !d) || (n && !x) || (me && !y) || (m && (!z || !w))) return HQPKKT_E_NULL;
    HIPCHK(hipSetDevice(h->opts.device));
    hipStream_t s = h->stream;
    const size_t nv = (size_t)n + me + 2 * (size_t)m;
    const size_t need = 4 * nv + (size_t)n + me + m + (size_t)IP_BLOCKS * IP_SLOTS + 64 + 2 * (size_t)m;
    int e;
    if (h->kept.ipv.count < need) {
      if ((e = h->kept.ipv.alloc(need))) return e;
      h->ip_hot_valid = false;
    }
    h->fr_hot_valid = false;  // the arena is shared with hqpkkt_franke
    IpCtx C;
    C.h = h, C.n = n, C.me = me, C.m = m, C.hout = h->kept.hpin.p + 64;
    double *q = h->kept.ipv.p;
    auto take = [&](size_t k) { double *r = q; q += k; return r; };
    C.x = take(n), C.y = take(me), C.z = take(m), C.w = take(m);
    C.r1 = take(n), C.r2 = take(me), C.r3 = take(m), C.r4 = take(m);
    C.dxa = take(n), C.dya = take(me), C.dza = take(m), C.dwa = take(m);
    C.dx = take(n), C.dy = take(me), C.dz = take(m), C.dw = take(m);
    C.c = take(n), C.b = take(me), C.d = take(m);
    C.part = take((size_t)IP_BLOCKS * IP_SLOTS), C.out = take(64);
    C.zh = take(m), C.wh = take(m);
    // out: 0..7 reductions (k_ip_final), 16..27 the blocking components (k_ip_minratio_final),
    // 32..39 the step's scalars (IPS_*)
    double *const Bk = C.out + 16, *const S = C.out + 32;
    const hipMemcpyKind in_kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n) HIPCHK(hipMemcpyAsync(C.c, c, sizeof(double) * n, in_kind, s));
    if (me) HIPCHK(hipMemcpyAsync(C.b, b, sizeof(double) * me, in_kind, s));
    if (m) HIPCHK(hipMemcpyAsync(C.d, d, sizeof(double) * m, in_kind, s));
    // the plugin entry points below take the driver's DEVICE vectors
    const int saved_loc = h->opts.loc;
    struct Restore {
      hqpkkt_t *h;
      int loc;
      ~Restore() {
        h->opts.loc = loc, h->lazy = false, h->factor_unchecked = false;
        (void)hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, 0, sizeof(int), h->stream);  // (kernels.hip.h: cancelled pivots are replaced inside the loop only)
      }
    } restore{h, saved_loc};
    h->opts.loc = HQPKKT_LOC_DEVICE;
    h->lazy = true;  // no host round trip where the loop does not need the answer at once
    // STAGED with dense dynamics: their share of A x and A'y for the right-hand sides (k_ip_rhs)
    const double *dx1 = nullptr, *dx2 = nullptr, *dxq = nullptr;  // (dxq: Q x with dense stage Hessians)
    int dndyn = 0;
    auto dyn_products = [&]() -> int {
      if (h->opts.mode != HQPKKT_MODE_STAGED) return 0;
      Vecs vv{};
      vv.dx = C.x, vv.dy = C.y;
      return staged_dense_products(h, vv, &dx1, &dx2, &dndyn, &dxq);
    };
    hipEvent_t t0 = h->ev0;  // total time: own pair of events (the plugin calls reuse the handle's)
    const hipEvent_t tb = h->evt0, te = h->evt1;  // owned by the handle: no early return can leak them
    (void)t0;
    HIPCHK(hipEventRecord(tb, s));
    std::memset(res, 0, sizeof(*res));
    res->result = 2;  // Hqp_Infeasible until decided (hqp/Hqp_IpsMehrotra.C:219)
    const int total = n + me + m;
    double resid = 0.0;
    int iter = 0, n_factor = 0, n_solve = 0;
    auto finish = [&](int result) -> int {
      res->result = result, res->iters = iter, res->n_factor = n_factor, res->n_solve = n_solve;
      if (n) HIPCHK(hipMemcpyAsync(x, C.x, sizeof(double) * n, out_kind, s));
      if (me) HIPCHK(hipMemcpyAsync(y, C.y, sizeof(double) * me, out_kind, s));
      if (m) HIPCHK(hipMemcpyAsync(z, C.z, sizeof(double) * m, out_kind, s));
      if (m) HIPCHK(hipMemcpyAsync(w, C.w, sizeof(double) * m, out_kind, s));
      HIPCHK(hipEventRecord(te, s));
      HIPCHK(hipStreamSynchronize(s));
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, tb, te);
      res->ms_total = ms;
      return 0;
    };
    auto factor = [&]() -> int { n_factor++; return hqpkkt_factor(h, C.z, C.w); };
    auto solve = [&](double *ox, double *oy, double *oz, double *ow) -> int {
      n_solve++;
      return hqpkkt_solve(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, ox, oy, oz, ow, &resid);
    };
    const int OPS_NONE[IP_SLOTS] = {IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM};
    // small QPs: an iteration's vector work between its solves in one workgroup each (ipdriver.hip.h, k_ip_pred_small)
    const bool ip_small = !getenv("HQPKKT_NO_IP_SMALL") && m > 0 && m <= IP_SMALL_M && (long long)n + me + m <= 4 * IP_SMALL_M;
  
    // ------------------------------------------------------------ iterations
    std::vector<double> phimin((size_t)o.max_iters + 2, 0.0);
    double mu0 = 0.0, norm_r0 = 0.0, norm_data = 1.0;
    // hot start (hqp/Hqp_IpsMehrotra.C:330-352, 475-478, 696-733): x, y of the last solve and
    // the (z, w) kept from its last iteration far enough from the solution; a hot start that
    // does not reduce phi by 1.2 per iteration, takes a step below 1e-5, runs max_warm_iters or
    // does not end optimal is thrown away and the QP solved again from a cold start
    const bool keep_hot = o.hot_start != 0 && m > 0;  // 1: hot start if possible, 2: cold, but prepare the next
    bool hot = o.hot_start == 1 && m > 0 && h->ip_hot_valid;
    const int max_warm = o.max_warm_iters > 0 ? o.max_warm_iters : 25;
    const double hot_thresh = std::pow(o.eps, 0.3333);
    int fail_iters = 0;
    double test1 = 0.0;
    const double gamma = std::pow(1.0e-4, 0.25);
    int result = 2;
    bool sing_hot = false;  // E_SING inside a hot-started run: restart cold like any failed hot start
    bool stepped = false, pending = false;  // pending: a step is in the stream whose scalars were not read yet
    double mu_pending = 0.0;
    // The rare second corrector (hqp/Hqp_IpsMehrotra.C:612-624: the first corrector's own
    // step is tiny): safe sigma, then Mehrotra's step rule with the host in the loop.
    auto second_corrector = [&](double mu) -> int {
      int e2;
      const double smm = gamma / (1.0 - gamma) * mu;
      k_ip_corr_rhs<<<nblk(m), 256, 0, s>>>(m, C.z, C.w, C.dza, C.dwa, smm, nullptr, C.r4);
      if ((e2 = solve(C.dx, C.dy, C.dz, C.dw))) return e2;
      k_ip_minratio_part<<<IP_BLOCKS, 256, 0, s>>>(m, C.z, C.w, C.dz, C.dw, C.part);
      k_ip_minratio_final<<<1, 256, 0, s>>>(C.part, C.z, C.w, C.dz, C.dw, Bk, m, gamma, nullptr);
      HIPCHK(hipMemcpyAsync(C.hout, Bk, sizeof(double) * 12, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      const double zmin = C.hout[0], wmin = C.hout[6];
      const int izmin = (int)C.hout[1], iwmin = (int)C.hout[7];
      const double z_iz = C.hout[2], dz_iz = C.hout[3], w_iz = C.hout[4], dw_iz = C.hout[5];
      const double z_iw = C.hout[8], dz_iw = C.hout[9], w_iw = C.hout[10], dw_iw = C.hout[11];
      double alpha;
      if (izmin < 0 && iwmin < 0)
        alpha = 1.0;
      else {
        alpha = izmin < 0 ? wmin : iwmin < 0 ? zmin : std::fmin(zmin, wmin);
        k_ip_mupl<<<IP_BLOCKS, 256, 0, s>>>(m, alpha, nullptr, C.z, C.w, C.dz, C.dw, C.part);
        if ((e2 = C.reduce(OPS_NONE, 1))) return e2;
        const double mu_pl = C.hout[0] / m;
        double fpd;
        if (iwmin >= 0 && alpha == wmin && z_iw > -alpha * dz_iw)
          fpd = (o.gammaf * mu_pl / (z_iw + alpha * dz_iw) - w_iw) / (alpha * dw_iw);
        else if (izmin >= 0 && alpha == zmin && w_iz > -alpha * dw_iz)
          fpd = (o.gammaf * mu_pl / (w_iz + alpha * dw_iz) - z_iz) / (alpha * dz_iz);
        else
          fpd = 0.0;
        alpha = std::fmax(0.0, std::fmin(std::fmax(1.0 - o.gammaf, fpd) * alpha, 1.0));
      }
      res->alpha = alpha;
      k_ip_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, alpha, nullptr, C.x, C.y, C.z, C.w, C.dx, C.dy, C.dz, C.dw, C.part);
      return 0;
    };
    // before leaving the loop with a step still in the stream: was it taken?
    auto settle = [&]() -> int {
      if (!pending) return 0;
      pending = false;
      HIPCHK(hipMemcpyAsync(C.hout + 32, S, sizeof(double) * 8, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      res->alpha = C.hout[32 + IPS_ALPHA];
      if (C.hout[32 + IPS_NEED2] != 0.0) return second_corrector(mu_pending);
      return 0;
    };
    // The iteration's launches between two read-backs as ONE captured graph each (small QPs on the tree engine: an
    // iteration of the double-integrator QP is 27 launches and 0.3 ms, and every boundary between a graph and the next
    // launch costs the queue 5 - 20 us, profiles/r06_ip_did_timeline.txt):
    //   A: factorisation + predictor solve + its residual + the posting kernel
    //   B: predictor statistics + corrector solve + residual + post
    //   C: the step + the next iterate's right-hand sides and reductions + post
    // Whatever the read-back then asks for - refinement rounds, the second corrector - runs as before, launch by launch.
    const bool seg_ok = ip_small && h->use_graphs && !h->prof.on && h->opts.mode != HQPKKT_MODE_STAGED && h->an.shard_count <= 1 &&
                        !getenv("HQPKKT_NO_IP_SEGMENTS");
    auto seg_slot = [&](int tag) -> hqpkkt::GraphSlot & {
      unsigned long long gf;
      std::memcpy(&gf, &o.gammaf, sizeof(gf));
      const void *key[10] = {(const void *)(intptr_t)tag, (const void *)(uintptr_t)gf, C.x, C.z, C.r1, C.dx, C.dxa, C.out, nullptr, nullptr};
      return h->direct_slot(h->gdirect_seg, key);
    };
    // a solve whose first residual is in the stream (run_residual with defer_residual): wait, read, and finish it as
    // hqpkkt_solve does (refinement, the checks behind a perturbed pivot)
    auto finish_solve = [&](double *ox, double *oy, double *oz, double *ow) -> int {
      int e2 = post_wait(h);
      if (e2) return e2;
      if ((e2 = collect_residual(h, &resid))) return e2;
      Vecs v{};
      if ((e2 = solve_vecs(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, ox, oy, oz, ow, v))) return e2;
      return solve_tail(h, v, C.z, C.w, C.r1, C.r2, C.r3, C.r4, ox, oy, oz, ow, resid, &resid);
    };
    auto enqueue_head = [&]() -> int {
      if (h->short_rows)
        k_ip_rhs<4><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.Qf.dev(), h->td.AT.dev(), h->td.CT.dev(), h->td.A.dev(), h->td.C.dev(),
                                              h->td.vals.p, C.c, C.b, C.d, C.x, C.y, C.z, C.w, C.r1, C.r2, C.r3, C.r4,
                                              C.part, dx1, dx2, dndyn, dxq);
      else
        k_ip_rhs<16><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.Qf.dev(), h->td.AT.dev(), h->td.CT.dev(), h->td.A.dev(), h->td.C.dev(),
                                               h->td.vals.p, C.c, C.b, C.d, C.x, C.y, C.z, C.w, C.r1, C.r2, C.r3, C.r4,
                                               C.part, dx1, dx2, dndyn, dxq);
      if (m == 0) return 0;
      // the reductions of this iterate and what the step before left behind, one round trip
      const int ops2[IP_SLOTS] = {IP_SUM, IP_SUM, IP_SUM, IP_MAX, IP_MIN, IP_MIN, IP_SUM, IP_SUM};
      IpOps o2;
      for (int k = 0; k < IP_SLOTS; k++) o2.op[k] = ops2[k];
      k_ip_final<<<1, 256, 0, s>>>(C.part, o2, C.out, IpEpi{0, 0, 0.0, 0.0, 0.0, nullptr, nullptr});
      return post_words(h, C.out, 40);  // (C.hout = hpin + 64: where the posting kernel puts them)
    };
    bool head_in_stream = false;  // segment C of the iteration before has queued this iterate's head already
    for (;;) {  // hot first (if asked for and possible), cold after a failed hot start
    iter = 0, result = 2, stepped = false, pending = false, sing_hot = false, head_in_stream = false;
    std::fill(phimin.begin(), phimin.end(), 0.0);
    res->alpha = 1.0;
    if (hot) {
      CopyList L{{C.zh, C.wh, nullptr, nullptr, nullptr, nullptr}, {C.z, C.w, nullptr, nullptr, nullptr, nullptr}, {m, m, 0, 0, 0, 0}};
      k_copy_vectors<<<copy_blocks(L), 256, 0, s>>>(L, 2);
    } else {
        // (x = y = 0 until the cold start's solve has succeeded: what the caller gets back when the
        // very first factorisation is singular, as from the reference)
        if (n) HIPCHK(hipMemsetAsync(C.x, 0, sizeof(double) * n, s));
        if (me) HIPCHK(hipMemsetAsync(C.y, 0, sizeof(double) * me, s));
        if (m > 0) {
      // qp_init_method (:226-250, 294-297): 0 z = w = 1, r4 = 0; 1, 2 w = a ratio of the data's norms;
      // 3 as 0 with r4 = -z.*w and the solve's dz, dw added to z, w
      double w0 = 1.0;
      if (o.init_method == 1) w0 = std::fmax(o.norm_d, 1e-10) * o.norm_Q / o.norm_C;
      if (o.init_method == 2) w0 = o.norm_C / std::fmax(o.norm_d, 1e-10) / o.norm_Q;
      k_ip_cold_rhs<<<nblk(total), 256, 0, s>>>(n, me, m, C.c, C.b, C.d, C.z, C.w, C.r1, C.r2, C.r3, C.r4, w0,
                                                o.init_method ? -w0 : 0.0);
          if ((e = factor()) || (e = solve(C.dx, C.dy, C.dz, C.dw))) {
            if (e == HQPKKT_E_SING) return finish(4);  // Hqp_Degenerate (:262-269)
            return e;
          }
          HIPCHK(hipMemcpyAsync(C.x, C.dx, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
          if (me) HIPCHK(hipMemcpyAsync(C.y, C.dy, sizeof(double) * me, hipMemcpyDeviceToDevice, s));
      if (o.init_method == 3) k_ip_shift<<<nblk(m), 256, 0, s>>>(m, C.dz, C.dw, 1.0, 1.0, C.dz, C.dw);  // :294-297
      k_ip_cold_stats<<<IP_BLOCKS, 256, 0, s>>>(m, C.dz, C.dw, C.part);
          const int ops1[IP_SLOTS] = {IP_MIN, IP_MIN, IP_MAX, IP_MAX, IP_SUM, IP_SUM, IP_SUM, IP_SUM};
          if ((e = C.reduce(ops1, 6))) return e;
          double mindz = C.hout[0], mindw = C.hout[1], sumdz = C.hout[4], sumdw = C.hout[5];
          if (C.hout[2] == 0.0) {  // :301-304
            k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0e-10, C.dz);
            mindz = 1.0e-10, sumdz = 1.0e-10 * m;
          }
          if (C.hout[3] == 0.0) {
            k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0e-10, C.dw);
            mindw = 1.0e-10, sumdw = 1.0e-10 * m;
          }
          double delz = std::fmax(-1.5 * mindz, 0.0), delw = std::fmax(-1.5 * mindw, 0.0);
          // gap = (dz + delz)'(dw + delw): k_ip_mupl with alpha = 1 on (delz, dz), (delw, dw) shifted vectors
          k_ip_shift<<<nblk(m), 256, 0, s>>>(m, C.dz, C.dw, delz, delw, C.z, C.w);
          k_ip_mupl<<<IP_BLOCKS, 256, 0, s>>>(m, 0.0, nullptr, C.z, C.w, C.dz, C.dw, C.part);
          if ((e = C.reduce(OPS_NONE, 1))) return e;
          const double gap0 = C.hout[0];
          delz += 0.5 * gap0 / (sumdw + m * delw);
          delw += 0.5 * gap0 / (sumdz + m * delz);
          k_ip_shift<<<nblk(m), 256, 0, s>>>(m, C.dz, C.dw, delz, delw, C.z, C.w);
        }
  
      if (keep_hot) {  // :318-319
        k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0, C.zh);
        k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0, C.wh);
      }
    }
    // the cold start's factorisation has succeeded (or a hot start carries on): the matrix is regular, cancelled multiplier
    // pivots are replaced from here on (kernels.hip.h, TINY_REPLACE_WORD)
    // (2: exactly zero pivots as well - only where the factorisation just checked met no cancelled multiplier pivot: kernels.hip.h)
    if (h->tiny_replace_in_loop) HIPCHK(hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, (!hot && !h->soft_tiny) ? 2 : 1, sizeof(int), s));
    bool restart_cold = false;
    while (true) {
      double phi = 0.0;
      bool redo = false;  // the second corrector replaced the step: same step() call, new right-hand sides
      do {
      // ---- one step (hqp/Hqp_IpsMehrotra.C:355-693)
      if (!head_in_stream) {
        if ((e = dyn_products()) || (e = enqueue_head())) return e;
      }
      head_in_stream = false;
      if (m == 0) {  // equality-constrained QP: one Newton step (:364-413)
        if ((e = factor()) || (e = solve(C.dx, C.dy, C.dz, C.dw))) {
          if (e == HQPKKT_E_SING) return finish(4);
          return e;
        }
        k_ip_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, 1.0, nullptr, C.x, C.y, C.z, C.w, C.dx, C.dy, C.dz, C.dw, C.part);
        iter++;
        return finish(0);
      }
      if ((e = post_wait(h))) return e;
      if (pending) {
        pending = false;
        res->alpha = C.hout[32 + IPS_ALPHA];
        if (C.hout[32 + IPS_NEED2] != 0.0) {  // that step was not taken (alpha 0): second corrector first
          iter--;
          if ((e = second_corrector(mu_pending))) {
              if (e == HQPKKT_E_SING && hot) {
              sing_hot = true;
              break;
            }
            if (e == HQPKKT_E_SING) return finish(4);
            return e;
          }
          iter++;
          redo = true;  // right-hand sides and reductions of the new iterate
          break;
        }
      }
      const double gap = C.hout[0], mu = C.hout[2] / m, norm_r = C.hout[3];
      if (stepped && (!std::isfinite(mu) || !std::isfinite(norm_r) || !std::isfinite(gap))) {
        iter--;  // the reference leaves the failed step uncounted
        result = 4;
        break;
      }
      res->gap = gap, res->mu = mu, res->pcost = C.hout[1];
      if (iter == 0) {
        mu0 = mu, norm_r0 = norm_r;
        norm_data = o.norm_data > 0.0 ? o.norm_data : 1.0;
      }
      phi = (norm_r + std::fabs(gap)) / norm_data;
      phimin[iter] = phi;
      res->phi = phi;
      if (keep_hot && phi > hot_thresh) {  // prepare the next hot start (:475-478)
        CopyList L{{C.z, C.w, nullptr, nullptr, nullptr, nullptr}, {C.zh, C.wh, nullptr, nullptr, nullptr, nullptr}, {m, m, 0, 0, 0, 0}};
        k_copy_vectors<<<copy_blocks(L), 256, 0, s>>>(L, 2);
      }
      if (mu <= o.eps && norm_r <= o.eps * norm_data) {  // :487-490
        result = 0;
        break;
      }
      double pm = phimin[0];
      for (int i = 1; i <= iter; i++) pm = std::fmin(pm, phimin[i]);
      if (phi > o.eps && phi >= 1.0e4 * pm) {  // :494-502
        result = 3;
        break;
      }
      if (iter >= 30) {  // slow convergence (:506-516)
        double pm30 = phimin[1];
        for (int i = 2; i <= iter - 30; i++) pm30 = std::fmin(pm30, phimin[i]);
        if (pm >= 0.5 * pm30) {
          result = 3;
          break;
        }
      }
      if (norm_r > o.eps * norm_data && norm_r / mu >= 1.0e8 * norm_r0 / mu0) result = 3;  // :520-524 (no return)
      // factorise; predictor (affine) step
      if (seg_ok) {
        h->defer_residual = true;
        e = graphed(h, seg_slot(1), [&]() {
          const int e2 = hqpkkt_factor(h, C.z, C.w);
          return e2 ? e2 : hqpkkt_solve(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, C.dxa, C.dya, C.dza, C.dwa, &resid);
        });
        h->defer_residual = false;
        n_factor++, n_solve++;
        if (!e) {
          h->factor_unchecked = true, h->factored = true, h->residual_pending = true;  // (what the two calls leave, replayed or not)
          e = finish_solve(C.dxa, C.dya, C.dza, C.dwa);
        }
      } else if (!(e = factor()))
        e = solve(C.dxa, C.dya, C.dza, C.dwa);
      if (e) {
        if (e == HQPKKT_E_SING && hot) {  // a hot start that ends degenerate is thrown away (:723-727)
          sing_hot = true;
          break;
        }
        if (e == HQPKKT_E_SING) return finish(4);
        return e;
      }
      // From here to the step itself nothing is read back: sigma (Terlaky's modification,
      // :583-590; the safe value when the predictor step is short and the reference skips the
      // first corrector, :612-616), the corrector's blocking components, the damped step length
      // (:629-672) are computed by thread 0 of the reduction kernels and consumed through device pointers.
      if (seg_ok) {
        h->defer_residual = true;
        e = graphed(h, seg_slot(2), [&]() {
          k_ip_pred_small<<<1, 1024, 0, s>>>(m, C.z, C.w, C.dza, C.dwa, C.out + 2, gamma, S, C.r4);
          return hqpkkt_solve(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, C.dx, C.dy, C.dz, C.dw, &resid);
        });
        h->defer_residual = false;
        n_solve++;
        if (!e) {
          h->residual_pending = true;
          e = finish_solve(C.dx, C.dy, C.dz, C.dw);
        }
      } else {
      if (ip_small) {  // one workgroup: the three launches below, same arithmetic (ipdriver.hip.h)
        k_ip_pred_small<<<1, 1024, 0, s>>>(m, C.z, C.w, C.dza, C.dwa, C.out + 2, gamma, S, C.r4);
      } else {
      k_ip_ratio<<<IP_BLOCKS, 256, 0, s>>>(m, C.z, C.w, C.dza, C.dwa, C.part);
      {
        const int ops3[IP_SLOTS] = {IP_MIN, IP_MAX, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM};
        IpOps o3;
        for (int k = 0; k < IP_SLOTS; k++) o3.op[k] = ops3[k];
        k_ip_final<<<1, 256, 0, s>>>(C.part, o3, C.out, IpEpi{1, m, mu, gamma, 0.0, nullptr, S});
      }
      k_ip_corr_rhs<<<nblk(m), 256, 0, s>>>(m, C.z, C.w, C.dza, C.dwa, 0.0, S + IPS_SMM, C.r4);
      }
      e = solve(C.dx, C.dy, C.dz, C.dw);
      }
      if (e) {
        if (e == HQPKKT_E_SING && hot) {
          sing_hot = true;
          break;
        }
        if (e == HQPKKT_E_SING) return finish(4);
        return e;
      }
      if (seg_ok) {  // the step and the head of the next pass through this loop
        if ((e = graphed(h, seg_slot(3), [&]() {
               k_ip_step_small<<<1, 1024, 0, s>>>(n, me, m, C.x, C.y, C.z, C.w, C.dx, C.dy, C.dz, C.dw, Bk, gamma, o.gammaf, S);
               return enqueue_head();
             })))
          return e;
        head_in_stream = true;
      } else if (ip_small) {  // one workgroup: the five launches below, same arithmetic
        k_ip_step_small<<<1, 1024, 0, s>>>(n, me, m, C.x, C.y, C.z, C.w, C.dx, C.dy, C.dz, C.dw, Bk, gamma, o.gammaf, S);
      } else {
      k_ip_minratio_part<<<IP_BLOCKS, 256, 0, s>>>(m, C.z, C.w, C.dz, C.dw, C.part);
      k_ip_minratio_final<<<1, 256, 0, s>>>(C.part, C.z, C.w, C.dz, C.dw, Bk, m, gamma, S);
      k_ip_mupl<<<IP_BLOCKS, 256, 0, s>>>(m, 0.0, S + IPS_ALPHA_PRE, C.z, C.w, C.dz, C.dw, C.part);
      {
        IpOps on;
        for (int k = 0; k < IP_SLOTS; k++) on.op[k] = IP_SUM;
        k_ip_final<<<1, 256, 0, s>>>(C.part, on, C.out, IpEpi{2, m, 0.0, 0.0, o.gammaf, Bk, S});
      }
      k_ip_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, 0.0, S + IPS_ALPHA, C.x, C.y, C.z, C.w, C.dx, C.dy, C.dz, C.dw,
                                            C.part);
      }
      // (:684-690: a non-finite mu or x ends the solve as degenerate; seen here by the next
      // pass through k_ip_rhs, whose sums and maximum carry the NaN / inf)
      iter++;
      stepped = true, pending = true, mu_pending = mu;
      } while (0);
      if (sing_hot) {
        result = 4;
        break;
      }
      if (redo) continue;
      // ---- what solve() does after every step() call (:703-718)
      const bool leave = result == 0 || result == 3 || result == 4 || iter + fail_iters >= o.max_iters ||
                         (hot && iter >= max_warm);
      if (hot || leave) {  // the step's own scalars are needed now: was it taken, how long was it
        if ((e = settle())) {
          if (e == HQPKKT_E_SING && hot) {
            result = 4;
            break;
          }
          if (e == HQPKKT_E_SING) return finish(4);
          return e;
        }
      }
      if (hot) {
        if (iter == 1)
          test1 = phi;
        else if (phi > test1 / std::pow(1.2, iter - 1.0) || res->alpha < 1.0e-5) {
          fail_iters += iter;
          restart_cold = true;
          break;
        }
      }
      if (leave) break;
    }
    if (restart_cold || (hot && result != 0)) {  // bad hot start: its iterations are lost (:723-727)
      if (!restart_cold) fail_iters += iter;
      hot = false;
      continue;
    }
    break;
    }
    iter += fail_iters;
    if (m > 0) h->ip_hot_valid = keep_hot;
    return finish(result);
  };
  return ip_attempts(h, opts, res, loop);
}

// ---- device-resident Franke loop ----------------------------------------------
// Restatement of hqp/Hqp_IpsFranke.C: cold_start (:156-216), step (:271-378), solve
// (:381-416, cold start only).  One factor + one solve per iteration; the scalars (mu from
// the gap and rhomin, the step length, zeta) live on the host as in the reference.
int hqpkkt_franke(hqpkkt_t *h, const hqpkkt_ip_opts *opts, const double *c, const double *b,
                  const double *d, double *x, double *y, double *z, double *w, hqpkkt_ip_result *res) {
  auto loop = [&]() -> int {
    if (!h || !res) return HQPKKT_E_NULL;
    if (!h->analyzed || !h->have_values) return HQPKKT_E_INTERN;
    if (opts && opts->max_iters < 0) return HQPKKT_E_RANGE;
      if (h->an.shard_count > 1) return HQPKKT_E_INTERN;
    hqpkkt_ip_opts o;
    if (opts)
      o = *opts;
    else
      hqpkkt_default_ip_opts(&o);
    Analysis &an = h->an;
    const int n = an.n, me = an.me, m = an.m;
    if ((n && !c) || (me && !b) || (m && !d) || (n && !x) || (me && !y) || (m && (!z || !w))) return HQPKKT_E_NULL;
    HIPCHK(hipSetDevice(h->opts.device));
    hipStream_t s = h->stream;
    const size_t nv = (size_t)n + me + 2 * (size_t)m;
    // same arena as hqpkkt_mehrotra (its hot-start data does not survive this call)
    const size_t need = 5 * nv + (size_t)n + me + m + (size_t)IP_BLOCKS * IP_SLOTS + 64 + 2 * (size_t)m;  // (+ nv: the iterate before a step)
    int e;
    if (h->kept.ipv.count < need) {
      if ((e = h->kept.ipv.alloc(need))) return e;
      h->fr_hot_valid = false;
    }
    h->ip_hot_valid = false;
    IpCtx C;
    C.h = h, C.n = n, C.me = me, C.m = m, C.hout = h->kept.hpin.p + 64;
    double *q = h->kept.ipv.p;
    auto take = [&](size_t k) { double *r = q; q += k; return r; };
    C.x = take(n), C.y = take(me), C.z = take(m), C.w = take(m);
    C.r1 = take(n), C.r2 = take(me), C.r3 = take(m), C.r4 = take(m);
    double *a1 = take(n), *a2 = take(me), *a3 = take(m);
    (void)take(m);
    C.dx = take(n), C.dy = take(me), C.dz = take(m), C.dw = take(m);
    C.c = take(n), C.b = take(me), C.d = take(m);
    C.part = take((size_t)IP_BLOCKS * IP_SLOTS), C.out = take(64);
    (void)take(2 * (size_t)m);
    double *const keep = take(nv);  // x, y, z, w before the step of an iteration (see below)
    const hipMemcpyKind in_kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out_kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n) HIPCHK(hipMemcpyAsync(C.c, c, sizeof(double) * n, in_kind, s));
    if (me) HIPCHK(hipMemcpyAsync(C.b, b, sizeof(double) * me, in_kind, s));
    if (m) HIPCHK(hipMemcpyAsync(C.d, d, sizeof(double) * m, in_kind, s));
    const int saved_loc = h->opts.loc;
    struct Restore {
      hqpkkt_t *h;
      int loc;
      ~Restore() {
        h->opts.loc = loc, h->lazy = false, h->factor_unchecked = false, h->defer_residual = false, h->residual_pending = false;
        (void)hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, 0, sizeof(int), h->stream);
      }
    } restore{h, saved_loc};
    h->opts.loc = HQPKKT_LOC_DEVICE;
    h->lazy = true;
    // STAGED with dense dynamics: their share of A x and A'y for the right-hand sides (k_ip_rhs)
    const double *dx1 = nullptr, *dx2 = nullptr, *dxq = nullptr;  // (dxq: Q x with dense stage Hessians)
    int dndyn = 0;
    auto dyn_products = [&]() -> int {
      if (h->opts.mode != HQPKKT_MODE_STAGED) return 0;
      Vecs vv{};
      vv.dx = C.x, vv.dy = C.y;
      return staged_dense_products(h, vv, &dx1, &dx2, &dndyn, &dxq);
    };
    const hipEvent_t tb = h->evt0, te = h->evt1;  // owned by the handle: no early return can leak them
    HIPCHK(hipEventRecord(tb, s));
    std::memset(res, 0, sizeof(*res));
    res->result = 2;
    int iter = 0, n_factor = 0, n_solve = 0;
    auto finish = [&](int result) -> int {
      res->result = result, res->iters = iter, res->n_factor = n_factor, res->n_solve = n_solve;
      if (n) HIPCHK(hipMemcpyAsync(x, C.x, sizeof(double) * n, out_kind, s));
      if (me) HIPCHK(hipMemcpyAsync(y, C.y, sizeof(double) * me, out_kind, s));
      if (m) HIPCHK(hipMemcpyAsync(z, C.z, sizeof(double) * m, out_kind, s));
      if (m) HIPCHK(hipMemcpyAsync(w, C.w, sizeof(double) * m, out_kind, s));
      HIPCHK(hipEventRecord(te, s));
      HIPCHK(hipStreamSynchronize(s));
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, tb, te);
      res->ms_total = ms;
      return 0;
    };
    const int total = n + me + m;
    const double beta = 0.995;  // qp_beta (:77)
    const int max_warm = o.max_warm_iters > 0 ? o.max_warm_iters : 15;  // qp_max_warm_iters (:81)
    bool hot = o.hot_start == 1 && m > 0 && h->fr_hot_valid;
    int fail_iters = 0, result = 2;
    double rhomin = 0.0, Ltilde = 0.0, zeta = 1.0, gap = 0.0, alpha = 1.0, alphabar = 1.0, gap1 = 0.0;
    const int OPS_SUM[IP_SLOTS] = {IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM};
    for (;;) {  // hot first (if asked for and possible), cold after a failed hot start (:381-416)
    iter = 0, alpha = 1.0, zeta = 1.0, result = 2;
    if (hot) {
      // hot_start (:222-266): x, y, z, w of the last solve, w += 1e-10, the slack vectors a1..a3
      // of that point - which are the right-hand sides r1..r3 of Mehrotra's loop
      k_ip_shift<<<nblk(m), 256, 0, s>>>(m, C.z, C.w, 0.0, 1e-10, C.z, C.w);
      if ((e = dyn_products())) return e;
      if (h->short_rows)
        k_ip_rhs<4><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.Qf.dev(), h->td.AT.dev(), h->td.CT.dev(), h->td.A.dev(), h->td.C.dev(),
                                              h->td.vals.p, C.c, C.b, C.d, C.x, C.y, C.z, C.w, a1, a2, a3, C.r4, C.part, dx1, dx2, dndyn, dxq);
      else
        k_ip_rhs<16><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.Qf.dev(), h->td.AT.dev(), h->td.CT.dev(), h->td.A.dev(), h->td.C.dev(),
                                               h->td.vals.p, C.c, C.b, C.d, C.x, C.y, C.z, C.w, a1, a2, a3, C.r4, C.part, dx1, dx2, dndyn, dxq);
      if ((e = C.reduce(OPS_SUM, 3))) return e;
      gap = C.hout[2] + 1.0;  // in_prod(z, w) + 1 (:248)
      if (rhomin == 0.0) rhomin = h->fr_rhomin;
    } else {
    // ---- cold start (:156-216)
    if (m > 0) {
      rhomin = 1000.0 * m;
      k_fr_dstats<<<IP_BLOCKS, 256, 0, s>>>(m, C.d, C.part);
      const int opsd[IP_SLOTS] = {IP_MIN, IP_MAX, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM, IP_SUM};
      if ((e = C.reduce(opsd, 3))) return e;
      const double min_d = C.hout[0], norm_d = C.hout[1];
      if (o.qp_mu0 > 0.0) {  // "choose Ltilde according _mu0" (:167-173)
        const double mean_d_h = 0.5 * C.hout[2] / (double)m;
        Ltilde = -mean_d_h + std::sqrt(mean_d_h * mean_d_h + (double)m * rhomin * o.qp_mu0);
        Ltilde = std::fmax(Ltilde, -min_d);
      } else {  // "according Wright" (:175-182)
        Ltilde = std::fmax(norm_d, -min_d);
        Ltilde = std::fmax(Ltilde, 1e2 * m);
      }
    }
    if (h->short_rows)
      k_fr_cold<4><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.CT.dev(), Ltilde, C.c, C.b, C.d, C.x, C.y, C.z, C.w, a1, a2, a3, C.part);
    else
      k_fr_cold<16><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.CT.dev(), Ltilde, C.c, C.b, C.d, C.x, C.y, C.z, C.w, a1, a2, a3, C.part);
    gap = 0.0;
    if (m > 0) {
      if ((e = C.reduce(OPS_SUM, 1))) return e;
      gap = C.hout[0];
    }
    }
    bool restart_cold = false;
    // ---- iterations (:381-416 around :271-378)
    while (true) {
      if (iter == 0) alphabar = 1.0;
      if (iter == 1 && h->tiny_replace_in_loop)
        HIPCHK(hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, h->soft_tiny ? 1 : 2, sizeof(int), s));  // (the first factorisation + solve has succeeded; 2: exact zeros too, kernels.hip.h)
      double mu;
      if (1.0 / gap < rhomin || alpha < 1.0) {
        mu = alphabar * gap / rhomin;             // potential reduction
        mu += (1.0 - alphabar) * gap / (double)m;  // centering
      } else
        mu = gap * gap;  // quadratic convergence
      if (m == 0) mu = 0.0;
      h->kept.hpin.p[HPIN_ZM] = zeta, h->kept.hpin.p[HPIN_ZM + 1] = mu;
      std::atomic_thread_fence(std::memory_order_release);
      // The whole step - right-hand sides, factorisation, solve, its residual, the step length, the update, the new gap,
      // both posts - as ONE captured graph (the launches take nothing from the host that changes from step to step)
      const bool seg_ok = h->use_graphs && !h->prof.on && h->opts.mode != HQPKKT_MODE_STAGED && h->an.shard_count <= 1 &&
                          !getenv("HQPKKT_NO_IP_SEGMENTS") && !getenv("HQPKKT_FRANKE_TWO_READS");
      if (!seg_ok) k_fr_rhs<<<nblk(total), 256, 0, s>>>(n, me, m, h->kept.hpin.dev + HPIN_ZM, a1, a2, a3, C.z, C.w, C.r1, C.r2, C.r3, C.r4);
      double resid = 0.0;
      n_factor++, n_solve++;
      // The step length below compares dw = C dx - r3 with w, whose active components are of the
      // order gap / m: a residual of mat_eps = 1e-10, which the reference's global pivoting stays
      // far below without refinement, lets that noise block the step near the solution (the loop
      // then creeps on with alpha -> 0).  Ask the solve for a residual below the slacks.
      h->refine_target = m > 0 ? std::fmax(0.05 * gap / (double)m, 2e-12) : 0.0;
      // One read-back per iteration: the solve leaves its first residual (and the status of the factorisation) in
      // the stream, the step length is computed and consumed on the device, and residual, status, step length and
      // the new gap come back together.  When the words then say that the solve was not finished (refinement wanted,
      // a perturbed pivot to judge, an error), the iterate of before the step is put back, the solve is finished as
      // hqpkkt_solve would have, and the step is taken again.
      double *const Sfr = C.out + 32;
      auto take_step_enqueue = [&]() -> int {
        if (m > 0) {
          k_fr_ratio<<<IP_BLOCKS, 256, 0, s>>>(m, C.z, C.w, C.dz, C.dw, C.part);
          IpOps orat;
          orat.op[0] = IP_MIN;
          for (int k = 1; k < IP_SLOTS; k++) orat.op[k] = IP_SUM;
          k_ip_final<<<1, 256, 0, s>>>(C.part, orat, C.out, IpEpi{3, m, 0.0, 0.0, beta, nullptr, Sfr});
        }
        k_fr_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, 1.0, m > 0 ? Sfr + IPS_ALPHA : nullptr, C.x, C.y, C.z, C.w, C.dx,
                                              C.dy, C.dz, C.dw, C.part);
        IpOps ou;
        for (int k = 0; k < IP_SLOTS; k++) ou.op[k] = IP_SUM;
        ou.op[1] = IP_MAX;
        k_ip_final<<<1, 256, 0, s>>>(C.part, ou, C.out, IpEpi{0, 0, 0.0, 0.0, 0.0, nullptr, nullptr});
        return post_words(h, C.out, 40);  // (the residual of the solve has gone to the host with the post behind its kernel)
      };
      auto take_step = [&]() -> int {
        const int ep = take_step_enqueue();
        return ep ? ep : post_wait(h);
      };
      const double target = h->refine_target > 0.0 ? std::fmin(h->opts.eps, h->refine_target) : h->opts.eps;  // (as solve_tail)
      const CopyList Lkeep{{C.x, C.y, C.z, C.w, nullptr, nullptr}, {keep, keep + n, keep + n + me, keep + n + me + m, nullptr, nullptr}, {n, me, m, m, 0, 0}};
      if (seg_ok) {
        h->defer_residual = true;
        {
          unsigned long long kb;
          std::memcpy(&kb, &beta, sizeof(kb));
          const void *key[10] = {(const void *)(intptr_t)4, (const void *)(uintptr_t)kb, C.x, C.z, C.r1, C.dx, keep, C.out, a1, nullptr};
          e = graphed(h, h->direct_slot(h->gdirect_seg, key), [&]() {
            k_fr_rhs<<<nblk(total), 256, 0, s>>>(n, me, m, h->kept.hpin.dev + HPIN_ZM, a1, a2, a3, C.z, C.w, C.r1, C.r2, C.r3, C.r4);
            int e2 = hqpkkt_factor(h, C.z, C.w);
            if (!e2) e2 = hqpkkt_solve(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, C.dx, C.dy, C.dz, C.dw, &resid);
            if (e2) return e2;
            k_copy_vectors<<<copy_blocks(Lkeep), 256, 0, s>>>(Lkeep, 4);
            return take_step_enqueue();
          });
        }
        h->defer_residual = false;
        if (!e) {
          h->factor_unchecked = true, h->factored = true, h->residual_pending = true;  // (what the calls leave, replayed or not)
          e = post_wait(h);
        }
      } else {
        h->defer_residual = !getenv("HQPKKT_FRANKE_TWO_READS");
        e = hqpkkt_factor(h, C.z, C.w);
        if (!e) e = hqpkkt_solve(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, C.dx, C.dy, C.dz, C.dw, &resid);
        h->defer_residual = false;
        if (!e && h->residual_pending) {
          k_copy_vectors<<<copy_blocks(Lkeep), 256, 0, s>>>(Lkeep, 4);
          if ((e = take_step())) return e;
        }
      }
      if (!e && h->residual_pending) {
        e = collect_residual(h, &resid);
        const bool unfinished = e || !(resid <= target) || h->soft_singular || h->soft_tiny;
        if (unfinished) {
          CopyList B{{keep, keep + n, keep + n + me, keep + n + me + m, nullptr, nullptr}, {C.x, C.y, C.z, C.w, nullptr, nullptr}, {n, me, m, m, 0, 0}};
          k_copy_vectors<<<copy_blocks(B), 256, 0, s>>>(B, 4);
          if (!e) {
            Vecs v{};
            if ((e = solve_vecs(h, C.z, C.w, C.r1, C.r2, C.r3, C.r4, C.dx, C.dy, C.dz, C.dw, v))) return e;
            e = solve_tail(h, v, C.z, C.w, C.r1, C.r2, C.r3, C.r4, C.dx, C.dy, C.dz, C.dw, resid, &resid);
          }
          if (!e && (e = take_step())) return e;
        }
      } else if (!e) {
        if ((e = take_step())) return e;
      }
      h->refine_target = 0.0;
      if (e == HQPKKT_E_SING && hot) {  // Hqp_Degenerate inside a hot start: thrown away (:405-411)
        result = 4;
        break;
      }
      if (e) {
        if (e == HQPKKT_E_SING) return finish(4);  // Hqp_Degenerate (:308-310)
        return e;
      }
      alpha = m > 0 ? C.hout[32 + IPS_ALPHA] : std::fmin(1.0, 2.0 * beta);
      alphabar = 0.5 * alphabar + 0.5 * alpha;
      if (alphabar == 1.0)
        rhomin *= 2.0;
      else if (alphabar < 0.5 && rhomin > 100.0 * m)
        rhomin /= 2.0;
      zeta *= (1.0 - alpha);
      gap = m > 0 ? C.hout[0] : 0.0;
      res->gap = gap, res->alpha = alpha, res->mu = mu, res->phi = zeta;
      {
        static const bool trace_ip = getenv("HQPKKT_TRACE_IP") != nullptr;  // (diagnosis: the loop's scalars after every step)
        if (trace_ip)
          fprintf(stderr, "franke: step %d gap %.17g alpha %.17g alphabar %.17g zeta %.17g rhomin %.17g resid %.3e mu %.6e hot %d\n", iter + 1, gap, alpha,
                  alphabar, zeta, rhomin, resid, mu, hot ? 1 : 0);
      }
      if (!std::isfinite(gap) || !std::isfinite(C.hout[1])) {  // :351-354
        result = 4;
      } else {
        iter++;
        if (!(zeta < o.eps))  // (:361-374, comparisons written to filter out NaN)
          result = alpha < o.eps ? 3 : 2;
        else if (!(gap < o.eps) || !(resid < o.eps))
          result = 1;  // Hqp_Feasible
        else
          result = 0;
      }
      // ---- what solve() does after every step() (:388-403)
      if (hot) {
        if (iter == 1)
          gap1 = gap;
        else if (gap > gap1) {
          fail_iters += iter;
          restart_cold = true;
          break;
        }
      }
      if (iter + fail_iters >= o.max_iters) break;
      if (hot && iter >= max_warm) break;
      if (result == 0 || result == 3 || result == 4) break;
    }
    if (restart_cold || (hot && result != 0)) {  // bad hot start (:405-411)
      if (!restart_cold) fail_iters += iter;
      hot = false;
      continue;
    }
    break;
    }
    iter += fail_iters;
    h->fr_hot_valid = m > 0 && result != 4;
    h->fr_rhomin = rhomin;
    return finish(result);
  };
  return ip_attempts(h, opts, res, loop);
}

}  // extern "C"
