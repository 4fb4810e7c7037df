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

namespace {

// What a step of a loop tells the loop.  Every other value is an HQPKKT_* error code (they are positive, HQPKKT_E_POLL far
// below these): the call ends with it.
enum : int {
  GO_ON = 0,
  REDO_HEAD = -1,     // the second corrector replaced the step: same step() call, new right-hand sides and reductions
  LEAVE = -2,         // `result` is decided: on to what solve() does after a step, or out of the iterations
  FINISH = -3,        // the call ends here, with finish(result)
  SING_HOT = -4,      // E_SING inside a hot-started run: thrown away like any failed hot start
  RESTART_COLD = -5,  // a bad hot start, its iterations counted in fail_iters: once more from a cold start
};

// how the reductions of the loops combine the slots of the partials (k_ip_final); the slots not named are sums
static_assert(IP_SUM == 0, "the slots a pattern leaves out are sums");
constexpr IpOps OPS_SUM{}, OPS_HEAD{{IP_SUM, IP_SUM, IP_SUM, IP_MAX, IP_MIN, IP_MIN}}, OPS_COLD{{IP_MIN, IP_MIN, IP_MAX, IP_MAX}},
    OPS_MIN_MAX{{IP_MIN, IP_MAX}}, OPS_MIN{{IP_MIN}}, OPS_SUM_MAX{{IP_SUM, IP_MAX}};

// One call of a device-resident loop: the handle, the caller's vectors, the loop's own vectors in h->kept.ipv, the
// counters, and what both loops do with them.  Lives on the stack of the call.
struct IpRun {
  hqpkkt_t *h = nullptr;
  hqpkkt_ip_opts o;  // the caller's, or the defaults
  int n = 0, me = 0, m = 0;
  hipStream_t s = nullptr;
  double *ux, *uy, *uz, *uw;  // the caller's vectors (finish) and result
  hqpkkt_ip_result *res = nullptr;
  hipMemcpyKind out_kind;
  // The arena, in this order.  hqpkkt_franke keeps its slack vectors a1..a3 where hqpkkt_mehrotra keeps dxa..dza, leaves
  // dwa, zh, wh unused and adds `keep`; every vector has the same place in both, a place the hot-start data of the call
  // before and the keys of the captured graphs depend on.
  double *x, *y, *z, *w, *r1, *r2, *r3, *r4, *dxa, *dya, *dza, *dwa, *dx, *dy, *dz, *dw, *c, *b, *d, *part;
  // out: 0..7 reductions (k_ip_final), 16..27 the blocking components (k_ip_minratio_final), 32..39 the step's scalars (IPS_*)
  double *out, *Bk, *S;
  double *zh, *wh;  // hot-start candidates (hqp/Hqp_IpsMehrotra.C:475-478)
  double *keep;     // hqpkkt_franke only: x, y, z, w before the step of an iteration
  double *hout;     // pinned (h->kept.hpin.p + 64): where the posting kernel puts `out`
  int iter = 0, n_factor = 0, n_solve = 0;
  double resid = 0.0;
  // STAGED with dense dynamics: their share of A x and A'y for the right-hand sides (k_ip_rhs); dxq: Q x with dense stage Hessians
  const double *dx1 = nullptr, *dx2 = nullptr, *dxq = nullptr;
  int dndyn = 0;
  // hot first (if asked for and possible), cold after a failed hot start, whose iterations are lost (fail_iters)
  bool hot = false;
  int fail_iters = 0, result = 2;

  // the plugin entry points take the loop's DEVICE vectors; lazy: no host round trip where the loop does not need the
  // answer at once.  Whatever way the call ends, the handle is the caller's again.
  struct Restore {
    hqpkkt_t *h = nullptr;
    int loc = 0;
    void arm(hqpkkt_t *h_) {
      h = h_, loc = h->opts.loc;
      h->opts.loc = HQPKKT_LOC_DEVICE, h->lazy = true;
    }
    ~Restore() {
      if (!h) return;
      h->opts.loc = loc, h->lazy = false, h->factor_unchecked = false, h->defer_residual = false, h->residual_pending = false;
      (void)hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, 0, sizeof(int), h->stream);  // (kernels.hip.h: cancelled pivots are replaced inside the loop only)
    }
  } guard;

  // Checks, arena, the caller's c, b, d in, the guard, the start of the clock.  `franke`: the arena with `keep`; the call
  // invalidates the other loop's hot-start data (the arena is shared) and, where the arena had to grow, its own.
  int begin(hqpkkt_t *h_, const hqpkkt_ip_opts *opts, const double *c_, const double *b_, const double *d_, double *x_, double *y_,
            double *z_, double *w_, hqpkkt_ip_result *res_, bool franke) {
    if (!h_ || !res_) return HQPKKT_E_NULL;
    if (!h_->analyzed || !h_->have_values) return HQPKKT_E_INTERN;
    if (opts && opts->max_iters < 0) return HQPKKT_E_RANGE;
    if (h_->an.shard_count > 1) return HQPKKT_E_INTERN;
    if (opts)
      o = *opts;
    else
      hqpkkt_default_ip_opts(&o);
    h = h_, res = res_, ux = x_, uy = y_, uz = z_, uw = w_;
    n = h->an.n, me = h->an.me, m = h->an.m;
    if ((n && !c_) || (me && !b_) || (m && !d_) || (n && !x_) || (me && !y_) || (m && (!z_ || !w_))) return HQPKKT_E_NULL;
    HIPCHK(hipSetDevice(h->opts.device));
    s = h->stream;
    const size_t nv = (size_t)n + me + 2 * (size_t)m;
    const size_t need = 4 * nv + (size_t)n + me + m + (size_t)IP_BLOCKS * IP_SLOTS + 64 + 2 * (size_t)m + (franke ? nv : 0);
    bool &own_hot = franke ? h->fr_hot_valid : h->ip_hot_valid, &other_hot = franke ? h->ip_hot_valid : h->fr_hot_valid;
    if (h->kept.ipv.count < need) {
      const int e = h->kept.ipv.alloc(need);
      if (e) return e;
      own_hot = false;
    }
    other_hot = false;
    double *q = h->kept.ipv.p;
    auto take = [&](size_t k) { double *r = q; q += k; return r; };
    x = take(n), y = take(me), z = take(m), w = take(m);
    r1 = take(n), r2 = take(me), r3 = take(m), r4 = take(m);
    dxa = take(n), dya = take(me), dza = take(m), dwa = take(m);
    dx = take(n), dy = take(me), dz = take(m), dw = take(m);
    c = take(n), b = take(me), d = take(m);
    part = take((size_t)IP_BLOCKS * IP_SLOTS), out = take(64), Bk = out + 16, S = out + 32;
    zh = take(m), wh = take(m);
    keep = franke ? take(nv) : nullptr;
    hout = h->kept.hpin.p + 64;
    const bool dev = h->opts.loc == HQPKKT_LOC_DEVICE;
    const hipMemcpyKind in_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    out_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n) HIPCHK(hipMemcpyAsync(c, c_, sizeof(double) * n, in_kind, s));
    if (me) HIPCHK(hipMemcpyAsync(b, b_, sizeof(double) * me, in_kind, s));
    if (m) HIPCHK(hipMemcpyAsync(d, d_, sizeof(double) * m, in_kind, s));
    guard.arm(h);
    // total time: the handle's own pair of events (the plugin calls reuse its others; no early return can leak them)
    HIPCHK(hipEventRecord(h->evt0, s));
    std::memset(res, 0, sizeof(*res));
    res->result = 2;  // Hqp_Infeasible until decided (hqp/Hqp_IpsMehrotra.C:219)
    return 0;
  }
  int finish(int result_) {
    res->result = result_, res->iters = iter, res->n_factor = n_factor, res->n_solve = n_solve;
    if (n) HIPCHK(hipMemcpyAsync(ux, x, sizeof(double) * n, out_kind, s));
    if (me) HIPCHK(hipMemcpyAsync(uy, y, sizeof(double) * me, out_kind, s));
    if (m) HIPCHK(hipMemcpyAsync(uz, z, sizeof(double) * m, out_kind, s));
    if (m) HIPCHK(hipMemcpyAsync(uw, w, sizeof(double) * m, out_kind, s));
    HIPCHK(hipEventRecord(h->evt1, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, h->evt0, h->evt1);
    res->ms_total = ms;
    return 0;
  }
  int factor() { n_factor++; return hqpkkt_factor(h, z, w); }
  int solve(double *ox, double *oy, double *oz, double *ow) {
    n_solve++;
    return hqpkkt_solve(h, z, w, r1, r2, r3, r4, ox, oy, oz, ow, &resid);
  }
  // a solve whose first residual is in the stream (run_residual with defer_residual): wait, read, and finish it as
  // hqpkkt_solve does (refinement, the checks behind a perturbed pivot)
  int finish_solve(double *ox, double *oy, double *oz, double *ow) {
    int e = post_wait(h);
    if (e || (e = collect_residual(h, &resid))) return e;
    Vecs v{};
    if ((e = solve_vecs(h, z, w, r1, r2, r3, r4, ox, oy, oz, ow, v))) return e;
    return solve_tail(h, v, z, w, r1, r2, r3, r4, ox, oy, oz, ow, resid, &resid);
  }
  int dyn_products() {
    if (h->opts.mode != HQPKKT_MODE_STAGED) return 0;
    Vecs vv{};
    vv.dx = x, vv.dy = y;
    return staged_dense_products(h, vv, &dx1, &dx2, &dndyn, &dxq);
  }
  int reduce(const IpOps &ops, int nout) {
    k_ip_final<<<1, 256, 0, s>>>(part, ops, out, IpEpi{0, 0, 0.0, 0.0, 0.0, nullptr, nullptr});
    const int e = post_words(h, out, nout);
    return e ? e : post_wait(h);
  }
  // the right-hand sides of the iterate (x, y, z, w) into t1..t3 and r4, their reductions into `part`
  void rhs(double *t1, double *t2, double *t3) {
    if (h->short_rows)
      k_ip_rhs<4><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.Qf.dev(), h->td.AT.dev(), h->td.CT.dev(), h->td.A.dev(), h->td.C.dev(),
                                            h->td.vals.p, c, b, d, x, y, z, w, t1, t2, t3, r4, part, dx1, dx2, dndyn, dxq);
    else
      k_ip_rhs<16><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.Qf.dev(), h->td.AT.dev(), h->td.CT.dev(), h->td.A.dev(), h->td.C.dev(),
                                             h->td.vals.p, c, b, d, x, y, z, w, t1, t2, t3, r4, part, dx1, dx2, dndyn, dxq);
  }
  // A factorisation or solve that failed with E_SING: inside a hot start the hot start is thrown away
  // (hqp/Hqp_IpsMehrotra.C:723-727, hqp/Hqp_IpsFranke.C:405-411), otherwise the QP is Hqp_Degenerate
  // (Hqp_IpsMehrotra.C:262-269, Hqp_IpsFranke.C:308-310).  Any other error ends the call.
  int failed(int e) {
    if (e != HQPKKT_E_SING) return e;
    if (hot) return SING_HOT;
    result = 4;
    return FINISH;
  }
  // how a run ended: RESTART_COLD (hot is off now), LEAVE (on to the end of the call), FINISH or an error
  int judge(int g) {
    if (g == SING_HOT) result = 4, g = LEAVE;
    if (g == LEAVE && hot && result != 0) fail_iters += iter, g = RESTART_COLD;  // bad hot start: its iterations are lost
    if (g == RESTART_COLD) hot = false;
    return g;
  }
};

// ---- device-resident Mehrotra predictor-corrector loop ----------------------
// Restatement of hqp/Hqp_IpsMehrotra.C: cold_start (:209-327), step (:355-693),
// solve (:696-735, cold start only).  Scalars are reduced on the device in a fixed
// order and read back; vectors stay on the device.
struct Mehrotra : IpRun {
  // hot start (hqp/Hqp_IpsMehrotra.C:330-352, 475-478, 696-733): x, y of the last solve and
  // the (z, w) kept from its last iteration far enough from the solution; a hot start that
  // does not reduce phi by 1.2 per iteration, takes a step below 1e-5, runs max_warm_iters or
  // does not end optimal is thrown away and the QP solved again from a cold start
  bool keep_hot = false;  // hot_start 1: hot start if possible, 2: cold, but prepare the next
  double test1 = 0.0, hot_thresh = 0.0;
  int max_warm = 25;
  std::vector<double> phimin;
  double mu0 = 0.0, norm_r0 = 0.0, norm_data = 1.0;
  bool stepped = false, pending = false;  // pending: a step is in the stream whose scalars were not read yet
  double mu_pending = 0.0;
  bool head_in_stream = false;  // segment C of the iteration before has queued this iterate's head already
  bool seg_ok = false, ip_small = false;
  double gamma = 0.0;
  double phi = 0.0, mu = 0.0;  // of the head that step() has read

  int run() {
    // small QPs: an iteration's vector work between its solves in one workgroup each (ipdriver.hip.h, k_ip_pred_small)
    ip_small = !getenv("HQPKKT_NO_IP_SMALL") && m > 0 && m <= IP_SMALL_M && (long long)n + me + m <= 4 * IP_SMALL_M;
    phimin.assign((size_t)o.max_iters + 2, 0.0);
    keep_hot = o.hot_start != 0 && m > 0;
    hot = o.hot_start == 1 && m > 0 && h->ip_hot_valid;
    max_warm = o.max_warm_iters > 0 ? o.max_warm_iters : 25;
    hot_thresh = std::pow(o.eps, 0.3333);
    gamma = std::pow(1.0e-4, 0.25);
    // The iteration's launches between two read-backs as ONE captured graph each (small QPs on the tree engine: an
    // iteration of the double-integrator QP is 27 launches and 0.3 ms, and every boundary between a graph and the next
    // launch costs the queue 5 - 20 us, profiles/r06_ip_did_timeline.txt):
    //   A: factorisation + predictor solve + its residual + the posting kernel
    //   B: predictor statistics + corrector solve + residual + post
    //   C: the step + the next iterate's right-hand sides and reductions + post
    // Whatever the read-back then asks for - refinement rounds, the second corrector - runs as before, launch by launch.
    seg_ok = ip_small && h->use_graphs && !h->prof.on && h->opts.mode != HQPKKT_MODE_STAGED && h->an.shard_count <= 1 &&
             !getenv("HQPKKT_NO_IP_SEGMENTS");
    int g;
    do g = judge(attempt()); while (g == RESTART_COLD);
    if (g != LEAVE) return g == FINISH ? finish(result) : g;
    iter += fail_iters;
    if (m > 0) h->ip_hot_valid = keep_hot;
    return finish(result);
  }
  // one run from a hot or a cold start to a result
  int attempt() {
    iter = 0, result = 2, stepped = false, pending = false, head_in_stream = false;
    std::fill(phimin.begin(), phimin.end(), 0.0);
    res->alpha = 1.0;
    int g;
    if (hot) {
      CopyList L{{zh, wh, nullptr, nullptr, nullptr, nullptr}, {z, w, nullptr, nullptr, nullptr, nullptr}, {m, m, 0, 0, 0, 0}};
      k_copy_vectors<<<copy_blocks(L), 256, 0, s>>>(L, 2);
    } else if ((g = cold_start()))
      return g;
    // the cold start's factorisation has succeeded (or a hot start carries on): the matrix is regular, cancelled multiplier
    // pivots are replaced from here on (kernels.hip.h, TINY_REPLACE_WORD)
    // (2: exactly zero pivots as well - only where the factorisation just checked met no cancelled multiplier pivot: kernels.hip.h)
    if (h->tiny_replace_in_loop)
      HIPCHK(hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, (!hot && !h->soft_tiny) ? 2 : 1, sizeof(int), s));
    do {
      phi = 0.0;
      g = step();
      if (g == REDO_HEAD)
        g = GO_ON;
      else if (g == GO_ON || g == LEAVE)
        g = after_step();
    } while (g == GO_ON);
    return g;
  }
  int cold_start() {
    int e;
    // (x = y = 0 until the cold start's solve has succeeded: what the caller gets back when the
    // very first factorisation is singular, as from the reference)
    if (n) HIPCHK(hipMemsetAsync(x, 0, sizeof(double) * n, s));
    if (me) HIPCHK(hipMemsetAsync(y, 0, sizeof(double) * me, s));
    if (m > 0) {
      // qp_init_method (:226-250, 294-297): 0 z = w = 1, r4 = 0; 1, 2 w = a ratio of the data's norms;
      // 3 as 0 with r4 = -z.*w and the solve's dz, dw added to z, w
      double w0 = 1.0;
      if (o.init_method == 1) w0 = std::fmax(o.norm_d, 1e-10) * o.norm_Q / o.norm_C;
      if (o.init_method == 2) w0 = o.norm_C / std::fmax(o.norm_d, 1e-10) / o.norm_Q;
      k_ip_cold_rhs<<<nblk(n + me + m), 256, 0, s>>>(n, me, m, c, b, d, z, w, r1, r2, r3, r4, w0, o.init_method ? -w0 : 0.0);
      if ((e = factor()) || (e = solve(dx, dy, dz, dw))) return failed(e);  // E_SING: Hqp_Degenerate (:262-269)
      HIPCHK(hipMemcpyAsync(x, dx, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
      if (me) HIPCHK(hipMemcpyAsync(y, dy, sizeof(double) * me, hipMemcpyDeviceToDevice, s));
      if (o.init_method == 3) k_ip_shift<<<nblk(m), 256, 0, s>>>(m, dz, dw, 1.0, 1.0, dz, dw);  // :294-297
      k_ip_cold_stats<<<IP_BLOCKS, 256, 0, s>>>(m, dz, dw, part);
      if ((e = reduce(OPS_COLD, 6))) return e;
      double mindz = hout[0], mindw = hout[1], sumdz = hout[4], sumdw = hout[5];
      if (hout[2] == 0.0) {  // :301-304
        k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0e-10, dz);
        mindz = 1.0e-10, sumdz = 1.0e-10 * m;
      }
      if (hout[3] == 0.0) {
        k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0e-10, dw);
        mindw = 1.0e-10, sumdw = 1.0e-10 * m;
      }
      double delz = std::fmax(-1.5 * mindz, 0.0), delw = std::fmax(-1.5 * mindw, 0.0);
      // gap = (dz + delz)'(dw + delw): k_ip_mupl with alpha = 1 on (delz, dz), (delw, dw) shifted vectors
      k_ip_shift<<<nblk(m), 256, 0, s>>>(m, dz, dw, delz, delw, z, w);
      k_ip_mupl<<<IP_BLOCKS, 256, 0, s>>>(m, 0.0, nullptr, z, w, dz, dw, part);
      if ((e = reduce(OPS_SUM, 1))) return e;
      const double gap0 = hout[0];
      delz += 0.5 * gap0 / (sumdw + m * delw);
      delw += 0.5 * gap0 / (sumdz + m * delz);
      k_ip_shift<<<nblk(m), 256, 0, s>>>(m, dz, dw, delz, delw, z, w);
    }
    if (keep_hot) {  // :318-319
      k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0, zh);
      k_ip_fill<<<nblk(m), 256, 0, s>>>(m, 1.0, wh);
    }
    return GO_ON;
  }
  // ---- one step (hqp/Hqp_IpsMehrotra.C:355-693)
  int step() {
    int g;
    if (!head_in_stream && ((g = dyn_products()) || (g = enqueue_head()))) return g;
    head_in_stream = false;
    if (m == 0) return equality_step();
    if ((g = read_head()) || (g = predictor()) || (g = corrector())) return g;
    return take_step();
  }
  // the right-hand sides of the iterate and, in one round trip, its reductions and what the step before left behind
  int enqueue_head() {
    rhs(r1, r2, r3);
    if (m == 0) return 0;
    k_ip_final<<<1, 256, 0, s>>>(part, OPS_HEAD, out, IpEpi{0, 0, 0.0, 0.0, 0.0, nullptr, nullptr});
    return post_words(h, out, 40);
  }
  int equality_step() {  // equality-constrained QP: one Newton step (:364-413)
    int e;
    if ((e = factor()) || (e = solve(dx, dy, dz, dw))) return failed(e);
    k_ip_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, 1.0, nullptr, x, y, z, w, dx, dy, dz, dw, part);
    iter++;
    result = 0;
    return FINISH;
  }
  // the scalars of the head: was the step before taken, and the tests of the new iterate
  int read_head() {
    int e;
    if ((e = post_wait(h))) return e;
    if (pending) {
      pending = false;
      res->alpha = hout[32 + IPS_ALPHA];
      if (hout[32 + IPS_NEED2] != 0.0) {  // that step was not taken (alpha 0): second corrector first
        iter--;
        if ((e = second_corrector(mu_pending))) return failed(e);
        iter++;
        return REDO_HEAD;
      }
    }
    const double gap = hout[0], norm_r = hout[3];
    mu = hout[2] / m;
    if (stepped && (!std::isfinite(mu) || !std::isfinite(norm_r) || !std::isfinite(gap))) {
      iter--;  // the reference leaves the failed step uncounted
      result = 4;
      return LEAVE;
    }
    res->gap = gap, res->mu = mu, res->pcost = hout[1];
    if (iter == 0) {
      mu0 = mu, norm_r0 = norm_r;
      norm_data = o.norm_data > 0.0 ? o.norm_data : 1.0;
    }
    phi = (norm_r + std::fabs(gap)) / norm_data;
    phimin[iter] = phi;
    res->phi = phi;
    if (keep_hot && phi > hot_thresh) {  // prepare the next hot start (:475-478)
      CopyList L{{z, w, nullptr, nullptr, nullptr, nullptr}, {zh, wh, nullptr, nullptr, nullptr, nullptr}, {m, m, 0, 0, 0, 0}};
      k_copy_vectors<<<copy_blocks(L), 256, 0, s>>>(L, 2);
    }
    if (mu <= o.eps && norm_r <= o.eps * norm_data) {  // :487-490
      result = 0;
      return LEAVE;
    }
    double pm = phimin[0];
    for (int i = 1; i <= iter; i++) pm = std::fmin(pm, phimin[i]);
    if (phi > o.eps && phi >= 1.0e4 * pm) {  // :494-502
      result = 3;
      return LEAVE;
    }
    if (iter >= 30) {  // slow convergence (:506-516)
      double pm30 = phimin[1];
      for (int i = 2; i <= iter - 30; i++) pm30 = std::fmin(pm30, phimin[i]);
      if (pm >= 0.5 * pm30) {
        result = 3;
        return LEAVE;
      }
    }
    if (norm_r > o.eps * norm_data && norm_r / mu >= 1.0e8 * norm_r0 / mu0) result = 3;  // :520-524 (no return)
    return GO_ON;
  }
  hqpkkt::GraphSlot &seg_slot(int tag) {
    unsigned long long gf;
    std::memcpy(&gf, &o.gammaf, sizeof(gf));
    const void *key[10] = {(const void *)(intptr_t)tag, (const void *)(uintptr_t)gf, x, z, r1, dx, dxa, out, nullptr, nullptr};
    return h->direct_slot(h->gdirect_seg, key);
  }
  // factorise; predictor (affine) step
  int predictor() {
    int e;
    if (seg_ok) {
      h->defer_residual = true;
      e = graphed(h, seg_slot(1), [&]() {
        const int e2 = hqpkkt_factor(h, z, w);
        return e2 ? e2 : hqpkkt_solve(h, z, w, r1, r2, r3, r4, dxa, dya, dza, dwa, &resid);
      });
      h->defer_residual = false;
      n_factor++, n_solve++;
      if (!e) {
        h->factor_unchecked = true, h->factored = true, h->residual_pending = true;  // (what the two calls leave, replayed or not)
        e = finish_solve(dxa, dya, dza, dwa);
      }
    } else if (!(e = factor()))
      e = solve(dxa, dya, dza, dwa);
    return e ? failed(e) : GO_ON;  // (E_SING: a hot start that ends degenerate is thrown away, :723-727)
  }
  // From here to the step itself nothing is read back: sigma (Terlaky's modification,
  // :583-590; the safe value when the predictor step is short and the reference skips the
  // first corrector, :612-616), the corrector's blocking components, the damped step length
  // (:629-672) are computed by thread 0 of the reduction kernels and consumed through device pointers.
  int corrector() {
    int e;
    if (seg_ok) {
      h->defer_residual = true;
      e = graphed(h, seg_slot(2), [&]() {
        k_ip_pred_small<<<1, 1024, 0, s>>>(m, z, w, dza, dwa, out + 2, gamma, S, r4);
        return hqpkkt_solve(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, &resid);
      });
      h->defer_residual = false;
      n_solve++;
      if (!e) {
        h->residual_pending = true;
        e = finish_solve(dx, dy, dz, dw);
      }
    } else {
      if (ip_small) {  // one workgroup: the three launches below, same arithmetic (ipdriver.hip.h)
        k_ip_pred_small<<<1, 1024, 0, s>>>(m, z, w, dza, dwa, out + 2, gamma, S, r4);
      } else {
        k_ip_ratio<<<IP_BLOCKS, 256, 0, s>>>(m, z, w, dza, dwa, part);
        k_ip_final<<<1, 256, 0, s>>>(part, OPS_MIN_MAX, out, IpEpi{1, m, mu, gamma, 0.0, nullptr, S});
        k_ip_corr_rhs<<<nblk(m), 256, 0, s>>>(m, z, w, dza, dwa, 0.0, S + IPS_SMM, r4);
      }
      e = solve(dx, dy, dz, dw);
    }
    return e ? failed(e) : GO_ON;
  }
  // the step and, with segments, the head of the next pass through step()
  int take_step() {
    if (seg_ok) {
      const int e = graphed(h, seg_slot(3), [&]() {
        k_ip_step_small<<<1, 1024, 0, s>>>(n, me, m, x, y, z, w, dx, dy, dz, dw, Bk, gamma, o.gammaf, S);
        return enqueue_head();
      });
      if (e) return e;
      head_in_stream = true;
    } else if (ip_small) {  // one workgroup: the five launches below, same arithmetic
      k_ip_step_small<<<1, 1024, 0, s>>>(n, me, m, x, y, z, w, dx, dy, dz, dw, Bk, gamma, o.gammaf, S);
    } else {
      k_ip_minratio_part<<<IP_BLOCKS, 256, 0, s>>>(m, z, w, dz, dw, part);
      k_ip_minratio_final<<<1, 256, 0, s>>>(part, z, w, dz, dw, Bk, m, gamma, S);
      k_ip_mupl<<<IP_BLOCKS, 256, 0, s>>>(m, 0.0, S + IPS_ALPHA_PRE, z, w, dz, dw, part);
      k_ip_final<<<1, 256, 0, s>>>(part, OPS_SUM, out, IpEpi{2, m, 0.0, 0.0, o.gammaf, Bk, S});
      k_ip_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, 0.0, S + IPS_ALPHA, x, y, z, w, dx, dy, dz, dw, part);
    }
    // (:684-690: a non-finite mu or x ends the solve as degenerate; seen here by the next
    // pass through k_ip_rhs, whose sums and maximum carry the NaN / inf)
    iter++;
    stepped = true, pending = true, mu_pending = mu;
    return GO_ON;
  }
  // The rare second corrector (hqp/Hqp_IpsMehrotra.C:612-624: the first corrector's own
  // step is tiny): safe sigma, then Mehrotra's step rule with the host in the loop.
  int second_corrector(double mu_) {
    int e;
    const double smm = gamma / (1.0 - gamma) * mu_;
    k_ip_corr_rhs<<<nblk(m), 256, 0, s>>>(m, z, w, dza, dwa, smm, nullptr, r4);
    if ((e = solve(dx, dy, dz, dw))) return e;
    k_ip_minratio_part<<<IP_BLOCKS, 256, 0, s>>>(m, z, w, dz, dw, part);
    k_ip_minratio_final<<<1, 256, 0, s>>>(part, z, w, dz, dw, Bk, m, gamma, nullptr);
    HIPCHK(hipMemcpyAsync(hout, Bk, sizeof(double) * 12, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const double zmin = hout[0], wmin = hout[6];
    const int izmin = (int)hout[1], iwmin = (int)hout[7];
    const double z_iz = hout[2], dz_iz = hout[3], w_iz = hout[4], dw_iz = hout[5];
    const double z_iw = hout[8], dz_iw = hout[9], w_iw = hout[10], dw_iw = hout[11];
    double alpha;
    if (izmin < 0 && iwmin < 0)
      alpha = 1.0;
    else {
      alpha = izmin < 0 ? wmin : iwmin < 0 ? zmin : std::fmin(zmin, wmin);
      k_ip_mupl<<<IP_BLOCKS, 256, 0, s>>>(m, alpha, nullptr, z, w, dz, dw, part);
      if ((e = reduce(OPS_SUM, 1))) return e;
      const double mu_pl = hout[0] / m;
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
    k_ip_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, alpha, nullptr, x, y, z, w, dx, dy, dz, dw, part);
    return 0;
  }
  // before leaving the loop with a step still in the stream: was it taken?
  int settle() {
    if (!pending) return 0;
    pending = false;
    HIPCHK(hipMemcpyAsync(hout + 32, S, sizeof(double) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    res->alpha = hout[32 + IPS_ALPHA];
    if (hout[32 + IPS_NEED2] != 0.0) return second_corrector(mu_pending);
    return 0;
  }
  // ---- what solve() does after every step() call (:703-718)
  int after_step() {
    const bool leave = result == 0 || result == 3 || result == 4 || iter + fail_iters >= o.max_iters || (hot && iter >= max_warm);
    int e;
    // the step's own scalars are needed now: was it taken, how long was it
    if ((hot || leave) && (e = settle())) return failed(e);
    if (hot) {
      if (iter == 1)
        test1 = phi;
      else if (phi > test1 / std::pow(1.2, iter - 1.0) || res->alpha < 1.0e-5) {
        fail_iters += iter;
        return RESTART_COLD;
      }
    }
    return leave ? LEAVE : GO_ON;
  }
};

// ---- device-resident Franke loop ----------------------------------------------
// Restatement of hqp/Hqp_IpsFranke.C: cold_start (:156-216), step (:271-378), solve
// (:381-416, cold start only).  One factor + one solve per iteration; the scalars (mu from
// the gap and rhomin, the step length, zeta) live on the host as in the reference.
struct Franke : IpRun {
  static constexpr double beta = 0.995;  // qp_beta (:77)
  int max_warm = 15;                     // qp_max_warm_iters (:81)
  double rhomin = 0.0, Ltilde = 0.0, zeta = 1.0, gap = 0.0, alpha = 1.0, alphabar = 1.0, gap1 = 0.0, mu = 0.0;
  double *a1() const { return dxa; }  // the slack vectors of the iterate: the right-hand sides r1..r3 of Mehrotra's loop
  double *a2() const { return dya; }
  double *a3() const { return dza; }

  int run() {
    max_warm = o.max_warm_iters > 0 ? o.max_warm_iters : 15;
    hot = o.hot_start == 1 && m > 0 && h->fr_hot_valid;
    int g;
    do g = judge(attempt()); while (g == RESTART_COLD);  // (:381-416)
    if (g != LEAVE) return g == FINISH ? finish(result) : g;
    iter += fail_iters;
    h->fr_hot_valid = m > 0 && result != 4;
    h->fr_rhomin = rhomin;
    return finish(result);
  }
  // one run from a hot or a cold start to a result: the iterations (:381-416 around :271-378)
  int attempt() {
    iter = 0, alpha = 1.0, zeta = 1.0, result = 2;
    int g = hot ? hot_start() : cold_start();
    if (g) return g;
    do {
      if ((g = mu_of_step()) || (g = step())) return g;
      update_scalars();
      g = after_step();
    } while (g == GO_ON);
    return g;
  }
  // hot_start (:222-266): x, y, z, w of the last solve, w += 1e-10, the slack vectors a1..a3 of that point
  int hot_start() {
    int e;
    k_ip_shift<<<nblk(m), 256, 0, s>>>(m, z, w, 0.0, 1e-10, z, w);
    if ((e = dyn_products())) return e;
    rhs(a1(), a2(), a3());
    if ((e = reduce(OPS_SUM, 3))) return e;
    gap = hout[2] + 1.0;  // in_prod(z, w) + 1 (:248)
    if (rhomin == 0.0) rhomin = h->fr_rhomin;
    return 0;
  }
  int cold_start() {  // (:156-216)
    int e;
    if (m > 0) {
      rhomin = 1000.0 * m;
      k_fr_dstats<<<IP_BLOCKS, 256, 0, s>>>(m, d, part);
      if ((e = reduce(OPS_MIN_MAX, 3))) return e;
      const double min_d = hout[0], norm_d = hout[1];
      if (o.qp_mu0 > 0.0) {  // "choose Ltilde according _mu0" (:167-173)
        const double mean_d_h = 0.5 * hout[2] / (double)m;
        Ltilde = -mean_d_h + std::sqrt(mean_d_h * mean_d_h + (double)m * rhomin * o.qp_mu0);
        Ltilde = std::fmax(Ltilde, -min_d);
      } else {  // "according Wright" (:175-182)
        Ltilde = std::fmax(norm_d, -min_d);
        Ltilde = std::fmax(Ltilde, 1e2 * m);
      }
    }
    if (h->short_rows)
      k_fr_cold<4><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.CT.dev(), Ltilde, c, b, d, x, y, z, w, a1(), a2(), a3(), part);
    else
      k_fr_cold<16><<<IP_BLOCKS, 256, 0, s>>>(n, me, m, h->td.CT.dev(), Ltilde, c, b, d, x, y, z, w, a1(), a2(), a3(), part);
    gap = 0.0;
    if (m > 0) {
      if ((e = reduce(OPS_SUM, 1))) return e;
      gap = hout[0];
    }
    return 0;
  }
  // mu of the step (:271-290); zeta and mu travel through two words of mapped host memory that k_fr_rhs reads
  int mu_of_step() {
    if (iter == 0) alphabar = 1.0;
    // (the first factorisation + solve has succeeded; 2: exact zeros too, kernels.hip.h)
    if (iter == 1 && h->tiny_replace_in_loop)
      HIPCHK(hipMemsetAsync(h->td.flags.p + TINY_REPLACE_WORD, h->soft_tiny ? 1 : 2, sizeof(int), s));
    if (1.0 / gap < rhomin || alpha < 1.0) {
      mu = alphabar * gap / rhomin;             // potential reduction
      mu += (1.0 - alphabar) * gap / (double)m;  // centering
    } else
      mu = gap * gap;  // quadratic convergence
    if (m == 0) mu = 0.0;
    h->kept.hpin.p[HPIN_ZM] = zeta, h->kept.hpin.p[HPIN_ZM + 1] = mu;
    std::atomic_thread_fence(std::memory_order_release);
    return 0;
  }
  // step length, update, the new gap and the post of the iteration's scalars
  int take_step_enqueue() {
    if (m > 0) {
      k_fr_ratio<<<IP_BLOCKS, 256, 0, s>>>(m, z, w, dz, dw, part);
      k_ip_final<<<1, 256, 0, s>>>(part, OPS_MIN, out, IpEpi{3, m, 0.0, 0.0, beta, nullptr, S});
    }
    k_fr_update<<<IP_BLOCKS, 256, 0, s>>>(n, me, m, 1.0, m > 0 ? S + IPS_ALPHA : nullptr, x, y, z, w, dx, dy, dz, dw, part);
    k_ip_final<<<1, 256, 0, s>>>(part, OPS_SUM_MAX, out, IpEpi{0, 0, 0.0, 0.0, 0.0, nullptr, nullptr});
    return post_words(h, out, 40);  // (the residual of the solve has gone to the host with the post behind its kernel)
  }
  int take_step() {
    const int e = take_step_enqueue();
    return e ? e : post_wait(h);
  }
  void fr_rhs() {
    k_fr_rhs<<<nblk(n + me + m), 256, 0, s>>>(n, me, m, h->kept.hpin.dev + HPIN_ZM, a1(), a2(), a3(), z, w, r1, r2, r3, r4);
  }
  // The whole step - right-hand sides, factorisation, solve, its residual, the step length, the update, the new gap,
  // both posts - as ONE captured graph (the launches take nothing from the host that changes from step to step)
  int step_graphed(const CopyList &Lkeep) {
    unsigned long long kb;
    const double bt = beta;
    std::memcpy(&kb, &bt, sizeof(kb));
    const void *key[10] = {(const void *)(intptr_t)4, (const void *)(uintptr_t)kb, x, z, r1, dx, keep, out, a1(), nullptr};
    h->defer_residual = true;
    int e = graphed(h, h->direct_slot(h->gdirect_seg, key), [&]() {
      fr_rhs();
      int e2 = hqpkkt_factor(h, z, w);
      if (!e2) e2 = hqpkkt_solve(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, &resid);
      if (e2) return e2;
      k_copy_vectors<<<copy_blocks(Lkeep), 256, 0, s>>>(Lkeep, 4);
      return take_step_enqueue();
    });
    h->defer_residual = false;
    if (!e) {
      h->factor_unchecked = true, h->factored = true, h->residual_pending = true;  // (what the calls leave, replayed or not)
      e = post_wait(h);
    }
    return e;
  }
  // One read-back per iteration: the solve leaves its first residual (and the status of the factorisation) in
  // the stream, the step length is computed and consumed on the device, and residual, status, step length and
  // the new gap come back together.  When the words then say that the solve was not finished (refinement wanted,
  // a perturbed pivot to judge, an error), the iterate of before the step is put back, the solve is finished as
  // hqpkkt_solve would have, and the step is taken again.
  int step() {
    const bool seg_ok = h->use_graphs && !h->prof.on && h->opts.mode != HQPKKT_MODE_STAGED && h->an.shard_count <= 1 &&
                        !getenv("HQPKKT_NO_IP_SEGMENTS") && !getenv("HQPKKT_FRANKE_TWO_READS");
    if (!seg_ok) fr_rhs();
    resid = 0.0;
    n_factor++, n_solve++;
    // The step length below compares dw = C dx - r3 with w, whose active components are of the
    // order gap / m: a residual of mat_eps = 1e-10, which the reference's global pivoting stays
    // far below without refinement, lets that noise block the step near the solution (the loop
    // then creeps on with alpha -> 0).  Ask the solve for a residual below the slacks.
    h->refine_target = m > 0 ? std::fmax(0.05 * gap / (double)m, 2e-12) : 0.0;
    const double target = h->refine_target > 0.0 ? std::fmin(h->opts.eps, h->refine_target) : h->opts.eps;  // (as solve_tail)
    const CopyList Lkeep{{x, y, z, w, nullptr, nullptr}, {keep, keep + n, keep + n + me, keep + n + me + m, nullptr, nullptr}, {n, me, m, m, 0, 0}};
    int e;
    if (seg_ok)
      e = step_graphed(Lkeep);
    else {
      h->defer_residual = !getenv("HQPKKT_FRANKE_TWO_READS");
      e = hqpkkt_factor(h, z, w);
      if (!e) e = hqpkkt_solve(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, &resid);
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
        CopyList B{{keep, keep + n, keep + n + me, keep + n + me + m, nullptr, nullptr}, {x, y, z, w, nullptr, nullptr}, {n, me, m, m, 0, 0}};
        k_copy_vectors<<<copy_blocks(B), 256, 0, s>>>(B, 4);
        if (!e) {
          Vecs v{};
          if ((e = solve_vecs(h, z, w, r1, r2, r3, r4, dx, dy, dz, dw, v))) return e;
          e = solve_tail(h, v, z, w, r1, r2, r3, r4, dx, dy, dz, dw, resid, &resid);
        }
        if (!e && (e = take_step())) return e;
      }
    } else if (!e) {
      if ((e = take_step())) return e;
    }
    h->refine_target = 0.0;
    return e ? failed(e) : GO_ON;
  }
  // alpha, alphabar, rhomin, zeta and the result code after the step (:312-374)
  void update_scalars() {
    alpha = m > 0 ? hout[32 + IPS_ALPHA] : std::fmin(1.0, 2.0 * beta);
    alphabar = 0.5 * alphabar + 0.5 * alpha;
    if (alphabar == 1.0)
      rhomin *= 2.0;
    else if (alphabar < 0.5 && rhomin > 100.0 * m)
      rhomin /= 2.0;
    zeta *= (1.0 - alpha);
    gap = m > 0 ? hout[0] : 0.0;
    res->gap = gap, res->alpha = alpha, res->mu = mu, res->phi = zeta;
    static const bool trace_ip = getenv("HQPKKT_TRACE_IP") != nullptr;  // (diagnosis: the loop's scalars after every step)
    if (trace_ip)
      fprintf(stderr, "franke: step %d gap %.17g alpha %.17g alphabar %.17g zeta %.17g rhomin %.17g resid %.3e mu %.6e hot %d\n", iter + 1, gap, alpha,
              alphabar, zeta, rhomin, resid, mu, hot ? 1 : 0);
    if (!std::isfinite(gap) || !std::isfinite(hout[1])) {  // :351-354
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
  }
  // ---- what solve() does after every step() (:388-403)
  int after_step() {
    if (hot) {
      if (iter == 1)
        gap1 = gap;
      else if (gap > gap1) {
        fail_iters += iter;
        return RESTART_COLD;
      }
    }
    if (iter + fail_iters >= o.max_iters) return LEAVE;
    if (hot && iter >= max_warm) return LEAVE;
    return result == 0 || result == 3 || result == 4 ? LEAVE : GO_ON;
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
  return ip_attempts(h, opts, res, [&]() -> int {
    Mehrotra run;
    const int e = run.begin(h, opts, c, b, d, x, y, z, w, res, false);
    return e ? e : run.run();
  });
}

int hqpkkt_franke(hqpkkt_t *h, const hqpkkt_ip_opts *opts, const double *c, const double *b,
                  const double *d, double *x, double *y, double *z, double *w, hqpkkt_ip_result *res) {
  return ip_attempts(h, opts, res, [&]() -> int {
    Franke run;
    const int e = run.begin(h, opts, c, b, d, x, y, z, w, res, true);
    return e ? e : run.run();
  });
}

}  // extern "C"
