// The entries of the C ABI (include/hqpkkt.h) on the sparse Q of the program where it lies on the device, 16 of them:
// hqpkkt_q_values .. hqpkkt_q_dscale_report (kernels: q_values.hip.h), hqpkkt_q_blocks, hqpkkt_q_bfgs_update and its report
// (q_bfgs.hip.h), hqpkkt_q_eigen_control and its report (q_eigen.hip.h) and hqpkkt_lagrangian_gradient.  Their state is
// TreeDev::QVal; everything else they use of the handle is declared in hqpkkt_handle.hpp.
// The damped updates - Hqp_HL_DScale::update on the diagonal, Hqp_HL_BFGS on the blocks - are ONE pipeline over the plan of
// a partition (qb_plan): the sums of the units, the decision per block, v and s'v, the outcome per block, and then the
// update's own write (k_qv_ds_apply per variable, k_qb_apply per stored entry).  The eigenvalue control runs over the
// same plans.
#include "hqpkkt_handle.hpp"
#include "q_values.hip.h"
#include "q_bfgs.hip.h"
#include "q_eigen.hip.h"

using QPlan = TreeDev::QVal::BfgsPlan;

// one of the two instances of a kernel template, chosen where it is launched
template <class F>
static F pick(bool second, F a, F b) {
  return second ? b : a;
}

// The checks that follow an entry's own NULL and RANGE tests, in the header's order: call order and refused handles
// (HQPKKT_E_INTERN), the diagonal rule of the entries that write a diagonal (HQPKKT_E_FORMAT; decided on the host from the
// pattern the handle keeps, tables made once), the device, and what the first call makes on it.
static int qv_refused(hqpkkt_t *h, bool touches_q) {
  if (!h->analyzed || !h->have_values) return HQPKKT_E_INTERN;
  if (h->shard_count > 1 || h->an.shard_count > 1) return HQPKKT_E_INTERN;
  if (h->opts.mode == HQPKKT_MODE_STAGED) {
    const int f = staged_form(h);
    if ((f & STAGED_FORM_SHARDED) || (f & (touches_q ? STAGED_FORM_HESS_DENSE : STAGED_FORM_DENSE_DYN))) return HQPKKT_E_INTERN;
  }
  return 0;
}
static int qv_prepare(hqpkkt_t *h, bool touches_q, bool writes_diag) {
  int e = qv_refused(h, touches_q);
  if (e) return e;
  const Analysis &an = h->an;
  TreeDev::QVal &q = h->td.qv;
  if (touches_q && !q.mapped) {
    q.h_didx.assign((size_t)an.n, -1), q.h_kind.assign((size_t)an.nq, qv::QV_LOWER);
    q.bad_diag = false;
    for (int i = 0; i < an.n; i++) {
      for (int k = h->pQp[i]; k < h->pQp[i + 1]; k++) {
        const int c = h->pQi[k];
        if (c > i) q.h_kind[k] = qv::QV_UPPER;
        if (c != i) continue;
        if (q.h_didx[i] >= 0) q.bad_diag = true;  // stored twice
        q.h_didx[i] = k, q.h_kind[k] = i;
      }
      if (q.h_didx[i] < 0) q.bad_diag = true;
    }
    q.mapped = true;
  }
  if (writes_diag && q.bad_diag) return HQPKKT_E_FORMAT;
  if ((e = ensure_device(h))) return e;
  if (touches_q && !q.didx.p && ((e = q.didx.upload(q.h_didx)) || (e = q.kind.upload(q.h_kind)))) return e;
  return CallerVecs{h}.ready();
}

// lanes per row of the walk over Qf, from its mean row length (as short_rows chooses for the residual's kernels)
static bool qv_short_q(const hqpkkt_t *h) { return h->an.n > 0 && (double)h->an.Qfull.col.size() / h->an.n < 8.0; }
static void qv_rows(hqpkkt_t *h, bool stats, const double *x, double *y, double *diag) {
  const int n = h->an.n;
  if (n <= 0) return;
  const TreeDev::QVal &q = h->td.qv;
  const bool sh = qv_short_q(h);
  const auto rows = stats ? pick(sh, qv::k_qv_rows<16, true>, qv::k_qv_rows<4, true>) : pick(sh, qv::k_qv_rows<16, false>, qv::k_qv_rows<4, false>);
  rows<<<nblk(n, sh ? 64 : 16), 256, 0, h->stream>>>(n, h->td.Qf.dev(), x, y, q.didx.p, h->td.vals.p, diag);
}
// Q's values have been written on the device: the state hqpkkt_set_values would leave with them
static int qv_written(hqpkkt_t *h) {
  HIPCHK(hipGetLastError());
  return h->opts.mode == HQPKKT_MODE_STAGED ? staged_values_changed(h, true) : values_changed(h, true, nullptr, nullptr, nullptr);
}

int hqpkkt_q_values(hqpkkt_t *h, double *Qx) {
  return guarded([&]() -> int {
    if (!h || !Qx) return HQPKKT_E_NULL;
    int e = qv_prepare(h, true, false);
    if (e) return e;
    const hipMemcpyKind kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (h->an.nq) HIPCHK(hipMemcpyAsync(Qx, h->td.vals.p, sizeof(double) * h->an.nq, kind, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  });
}

int hqpkkt_q_product(hqpkkt_t *h, const double *x, double *y) {
  return guarded([&]() -> int {
    if (!h || !x || !y) return HQPKKT_E_NULL;
    int e = qv_prepare(h, true, false);
    if (e) return e;
    CallerVecs io{h};
    const double *dx;
    double *dy;
    if ((e = io.in(x, (size_t)h->an.n, &dx))) return e;
    io.out(y, (size_t)h->an.n, &dy);
    qv_rows(h, false, dx, dy, nullptr);
    HIPCHK(hipGetLastError());
    return io.finish();
  });
}

int hqpkkt_q_row_stats(hqpkkt_t *h, double *diag, double *offsum) {
  return guarded([&]() -> int {
    if (!h || (!diag && !offsum)) return HQPKKT_E_NULL;
    int e = qv_prepare(h, true, false);
    if (e) return e;
    CallerVecs io{h};
    double *dd, *ds;
    io.out(diag, (size_t)h->an.n, &dd), io.out(offsum, (size_t)h->an.n, &ds);
    qv_rows(h, true, nullptr, ds, dd);
    HIPCHK(hipGetLastError());
    return io.finish();
  });
}

int hqpkkt_q_set_diagonal(hqpkkt_t *h, const double *d) {
  return guarded([&]() -> int {
    if (!h || !d) return HQPKKT_E_NULL;
    int e = qv_prepare(h, true, true);
    if (e) return e;
    CallerVecs io{h};
    const double *dd;
    if ((e = io.in(d, (size_t)h->an.n, &dd))) return e;
    if (h->an.nq) qv::k_qv_reset<<<nblk(h->an.nq), 256, 0, h->stream>>>(h->an.nq, h->td.qv.kind.p, h->td.vals.p, dd, 0.0, 0);
    if ((e = qv_written(h))) return e;
    return io.finish();
  });
}

int hqpkkt_q_dscale_setup(hqpkkt_t *h, double eps) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (!std::isfinite(eps) || !(eps > 0.0)) return HQPKKT_E_RANGE;
    int e = qv_prepare(h, true, true);
    if (e) return e;
    if (h->an.nq) qv::k_qv_reset<<<nblk(h->an.nq), 256, 0, h->stream>>>(h->an.nq, h->td.qv.kind.p, h->td.vals.p, nullptr, eps, 1);
    return qv_written(h);
  });
}

int hqpkkt_q_gerschgorin(hqpkkt_t *h, double eps) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (!std::isfinite(eps) || !(eps > 0.0)) return HQPKKT_E_RANGE;
    int e = qv_prepare(h, true, true);
    if (e) return e;
    TreeDev::QVal &q = h->td.qv;
    const int n = h->an.n;
    if (!q.offsum.p && (e = q.offsum.alloc((size_t)n + 1))) return e;
    qv_rows(h, true, nullptr, q.offsum.p, nullptr);
    if (n) qv::k_qv_gerschgorin<<<nblk(n), 256, 0, h->stream>>>(n, q.didx.p, q.offsum.p, eps, h->td.vals.p);
    return qv_written(h);
  });
}

// ---- partitions and their plans: what the damped updates and the eigenvalue control share (q_bfgs.hip.h)

// Hqp_HL_BFGS::next_block on the analysed pattern of Q: the blocks' first indices, n behind them; and per block whether
// every (i, j), i <= j, of it is stored (the rows are strictly ascending: a count decides)
static void qb_partition(const hqpkkt_t *h, int bsize, std::vector<int> &first, std::vector<unsigned char> &full) {
  const int n = h->an.n;
  const int *Qp = h->pQp.data(), *Qi = h->pQi.data();
  first.clear(), full.clear();
  for (int b = 0; b < n;) {
    first.push_back(b);
    if (bsize < 0) {
      int end = b;
      for (; b <= end; b++) {
        const int last = Qp[b + 1] > Qp[b] ? Qi[Qp[b + 1] - 1] : b;
        end = std::max(end, last);
      }
    } else
      b += bsize > 0 ? std::min(bsize, n - b) : n - b;
  }
  first.push_back(n);
  if (n == 0) first.clear();
  for (size_t k = 0; k + 1 < first.size(); k++) {
    const int a = first[k], e = first[k + 1];
    long long stored = 0;
    for (int i = a; i < e; i++)
      for (int j = Qp[i]; j < Qp[i + 1]; j++) stored += Qi[j] >= i && Qi[j] < e;
    full.push_back(stored == (long long)(e - a) * (e - a + 1) / 2);
  }
}
static int qb_key(const hqpkkt_t *h, int bsize) { return bsize < 0 ? -1 : (bsize >= h->an.n ? 0 : bsize); }

int hqpkkt_q_blocks(hqpkkt_t *h, int bsize, int *first, int *full, long long cap, long long *n_blocks) {
  return guarded([&]() -> int {
    if (!h || !n_blocks) return HQPKKT_E_NULL;
    if (!h->analyzed) return HQPKKT_E_INTERN;
    std::vector<int> f;
    std::vector<unsigned char> fl;
    qb_partition(h, qb_key(h, bsize), f, fl);
    *n_blocks = (long long)fl.size();
    if (!first) return 0;
    if (cap < *n_blocks) return HQPKKT_E_RANGE;
    std::copy(f.begin(), f.end(), first);
    if (full) std::copy(fl.begin(), fl.end(), full);
    return 0;
  });
}

// the plan of one bsize: the host's partition, then (with_device) its tables, partial sums and the BFGS update's report on
// the device
static int qb_plan(hqpkkt_t *h, int bsize, bool with_device, int *index) {
  TreeDev::QVal &q = h->td.qv;
  const int key = qb_key(h, bsize), n = h->an.n;
  int at = -1;
  for (size_t k = 0; k < q.bfgs_plans.size(); k++)
    if (q.bfgs_plans[k].bsize == key) at = (int)k;
  if (at < 0) {
    QPlan p;
    p.bsize = key;
    qb_partition(h, key, p.first, p.full);
    p.nblocks = (int)p.full.size();
    p.all_full = true;
    for (int b = 0; b < p.nblocks; b++) {
      const int len = p.first[b + 1] - p.first[b];
      p.max_len = std::max(p.max_len, len), p.nunits += (len + qv::QV_CHUNK - 1) / qv::QV_CHUNK;
      p.all_full = p.all_full && p.full[b];
    }
    q.bfgs_plans.push_back(std::move(p));
    at = (int)q.bfgs_plans.size() - 1;
  }
  *index = at;
  QPlan &p = q.bfgs_plans[at];
  if (!with_device || p.blk_of.p || n <= 0) return 0;
  std::vector<int> blk_of((size_t)n), bunit((size_t)p.nblocks + 1), ublk((size_t)p.nunits);
  for (int b = 0, u = 0; b < p.nblocks; b++) {
    const int len = p.first[b + 1] - p.first[b];
    std::fill(blk_of.begin() + p.first[b], blk_of.begin() + p.first[b + 1], b);
    bunit[b] = u;
    for (int j = 0; j < (len + qv::QV_CHUNK - 1) / qv::QV_CHUNK; j++) ublk[u++] = b;
    bunit[b + 1] = u;
  }
  int e;
  if ((e = p.boff.upload(p.first)) || (e = p.bunit.upload(bunit)) || (e = p.ublk.upload(ublk)) || (e = p.part.alloc(3 * (size_t)p.nunits)) ||
      (e = p.rep.alloc((size_t)qv::QV_REPORT * p.nblocks)))
    return e;
  return p.blk_of.upload(blk_of);  // (last: it says the plan is complete)
}

// a plan's launch shape: lanes per row as hqpkkt_q_product; a wavefront per unit where no block is longer than 64
// (q_values.hip.h), four of them a workgroup; the grids of the unit passes and of the row passes; the kernels' tables
struct QShape {
  bool short_rows, wave_units;
  unsigned ugrid, rgrid;
  qv::BfgsTables g;
  QShape(const hqpkkt_t *h, const QPlan &p)
      : short_rows(qv_short_q(h)), wave_units(p.max_len <= 64), ugrid((unsigned)(wave_units ? (p.nunits + 3) / 4 : p.nunits)),
        rgrid((unsigned)nblk(h->an.n, short_rows ? 64 : 16)), g{h->an.n, p.nblocks, p.nunits, p.blk_of.p, p.boff.p, p.bunit.p, p.ublk.p} {}
};

// The passes of a damped update over plan p, four launches: the units' sums, the decision per block into `rep`, v and the
// units' s'v, the outcome per block.  DIAG (Hqp_HL_DScale): src are the handle's values, didx the diagonals' indices, v
// optional; otherwise src is Q s and v the handle's own vector.  The plan's `part` is scratch: the stream orders its users.
template <bool DIAG>
static void qb_passes(hqpkkt_t *h, const QPlan &p, const QShape &L, const double *s, const double *y, const double *src, const int *didx,
                      double gamma, double *rep, double *v) {
  const int B = p.max_len;  // (DIAG: the block length of the uniform partition)
  double *part = p.part.p, *part2 = p.part.p + 2 * (size_t)p.nunits;
  hipStream_t st = h->stream;
  pick(L.wave_units, qv::k_qb_sums<4, DIAG>, qv::k_qb_sums<1, DIAG>)<<<L.ugrid, 256, 0, st>>>(L.g, s, y, src, didx, B, part);
  qv::k_qb_decide<<<nblk(p.nblocks), 256, 0, st>>>(L.g, part, gamma, rep);
  pick(L.wave_units, qv::k_qb_damped<4, DIAG>, qv::k_qb_damped<1, DIAG>)<<<L.ugrid, 256, 0, st>>>(L.g, s, y, src, didx, B, rep, part2, v);
  qv::k_qb_outcome<<<nblk(p.nblocks), 256, 0, st>>>(L.g, part2, rep);
}

// The read-back of a report.  `last`: the plan of the last update or control of its kind since the analysis (-1: none yet,
// HQPKKT_E_INTERN); `rep`: its words on that plan, `words` per block.  *n_blocks (and *t_steps) are set before the capacity
// test.  T, t_steps: what hqpkkt_q_eigen_report returns beside the words.
static int qv_report(hqpkkt_t *h, int TreeDev::QVal::*last, DBuf<double> QPlan::*rep, int words, double *out, long long cap_blocks,
                     long long *n_blocks, double *T = nullptr, int *t_steps = nullptr) {
  return guarded([&]() -> int {
    if (!h || !out || !n_blocks) return HQPKKT_E_NULL;
    int e = qv_prepare(h, true, false);
    if (e) return e;
    const TreeDev::QVal &q = h->td.qv;
    if (q.*last < 0) return HQPKKT_E_INTERN;
    const QPlan &p = q.bfgs_plans[q.*last];
    *n_blocks = p.nblocks;
    if (t_steps) *t_steps = p.eig_steps;
    if (cap_blocks < p.nblocks) return HQPKKT_E_RANGE;
    if (p.nblocks) {
      HIPCHK(hipMemcpyAsync(out, (p.*rep).p, sizeof(double) * words * (size_t)p.nblocks, hipMemcpyDeviceToHost, h->stream));
      if (T) HIPCHK(hipMemcpyAsync(T, p.eig_T.p, sizeof(double) * 2 * (size_t)p.eig_steps * p.nblocks, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  });
}

// ---- Hqp_HL_DScale::update: the damped update of a Q that is its diagonal

int hqpkkt_q_dscale_update(hqpkkt_t *h, const hqpkkt_dscale_update *u) {
  return guarded([&]() -> int {
    if (!h || !u || !u->s || !u->y) return HQPKKT_E_NULL;
    static_assert(qv::QV_REPORT == HQPKKT_DSCALE_REPORT, "the kernels write the report's words");
    if (!std::isfinite(u->gamma) || u->gamma < 0.0) return HQPKKT_E_RANGE;
    int e = qv_prepare(h, true, true), at = -1;
    // the uniform partition of bsize is a plan like any other; bsize <= 0 never means detected blocks here: one block
    if (e || (e = qb_plan(h, u->bsize > 0 ? u->bsize : 0, true, &at))) return e;
    TreeDev::QVal &q = h->td.qv;
    QPlan &p = q.bfgs_plans[at];
    const int n = h->an.n;
    if (n <= 0) {
      q.ds_last = at;
      return 0;
    }
    if (!p.ds_rep.p && (e = p.ds_rep.alloc((size_t)qv::QV_REPORT * p.nblocks))) return e;
    CallerVecs io{h};
    const double *ds, *dy;
    double *dv;
    if ((e = io.in(u->s, (size_t)n, &ds)) || (e = io.in(u->y, (size_t)n, &dy))) return e;
    io.out(u->v, (size_t)n, &dv);
    const QShape L(h, p);
    qb_passes<true>(h, p, L, ds, dy, h->td.vals.p, q.didx.p, u->gamma, p.ds_rep.p, dv);
    qv::k_qv_ds_apply<<<nblk(n), 256, 0, h->stream>>>(n, p.max_len, q.didx.p, ds, dy, p.ds_rep.p, h->td.vals.p);  // (uniform: every block but the last is max_len long)
    q.ds_last = at;
    if ((e = qv_written(h))) return e;
    return io.finish();
  });
}

int hqpkkt_q_dscale_report(hqpkkt_t *h, double *out, long long cap_blocks, long long *n_blocks) {
  return qv_report(h, &TreeDev::QVal::ds_last, &QPlan::ds_rep, qv::QV_REPORT, out, cap_blocks, n_blocks);
}

// ---- Hqp_HL_BFGS and the pattern-kept update on the sparse Q

int hqpkkt_q_bfgs_update(hqpkkt_t *h, const hqpkkt_q_bfgs_update_args *u) {
  return guarded([&]() -> int {
    if (!h || !u || !u->s || !u->y) return HQPKKT_E_NULL;
    static_assert(qv::QV_REPORT == HQPKKT_QBFGS_REPORT, "the kernels write the report's words");
    if (!std::isfinite(u->gamma) || (u->gamma < 0.0 && !std::isfinite(u->alpha))) return HQPKKT_E_RANGE;
    if (u->fill != HQPKKT_QBFGS_FULL && u->fill != HQPKKT_QBFGS_PATTERN) return HQPKKT_E_RANGE;
    int e = qv_refused(h, true), at = -1;
    if (e || (e = qb_plan(h, u->bsize, false, &at))) return e;
    if (u->fill == HQPKKT_QBFGS_FULL && !h->td.qv.bfgs_plans[at].all_full) return HQPKKT_E_FORMAT;
    if ((e = qv_prepare(h, true, false))) return e;
    TreeDev::QVal &q = h->td.qv;
    const int n = h->an.n, nq = h->an.nq;
    if (n <= 0) {
      q.bfgs_last = at;
      return 0;
    }
    if (!q.erow.p) {  // what every plan shares: the entries' rows and columns, Q s and v
      std::vector<int> erow((size_t)nq);
      for (int i = 0; i < n; i++) std::fill(erow.begin() + h->pQp[i], erow.begin() + h->pQp[i + 1], i);
      if ((e = q.ecol.upload(h->pQi)) || (e = q.bfgs_qs.alloc((size_t)n)) || (e = q.bfgs_v.alloc((size_t)n)) || (e = q.erow.upload(erow))) return e;
    }
    if ((e = qb_plan(h, u->bsize, true, &at))) return e;
    const QPlan &p = q.bfgs_plans[at];
    CallerVecs io{h};
    const double *ds, *dy;
    if ((e = io.in(u->s, (size_t)n, &ds)) || (e = io.in(u->y, (size_t)n, &dy))) return e;
    double *Qs = q.bfgs_qs.p, *v = q.bfgs_v.p;
    hipStream_t s = h->stream;
    const QShape L(h, p);
    pick(L.short_rows, qv::k_qb_rows<16>, qv::k_qb_rows<4>)<<<L.rgrid, 256, 0, s>>>(n, h->td.Qf.dev(), p.blk_of.p, ds, Qs);
    qb_passes<false>(h, p, L, ds, dy, Qs, nullptr, bfgs_gamma_eff(u->gamma, u->alpha), p.rep.p, v);
    if (nq) qv::k_qb_apply<<<nblk(nq), 256, 0, s>>>(nq, q.erow.p, q.ecol.p, q.kind.p, p.blk_of.p, Qs, v, p.rep.p, h->td.vals.p);
    q.bfgs_last = at;
    // v and Q s are the handle's own vectors (the update reads them): a caller who asks gets a copy, in the stream
    const hipMemcpyKind back = io.host() ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (u->v) HIPCHK(hipMemcpyAsync(u->v, v, sizeof(double) * (size_t)n, back, s));
    if (u->Qs) HIPCHK(hipMemcpyAsync(u->Qs, Qs, sizeof(double) * (size_t)n, back, s));
    if ((e = qv_written(h))) return e;
    return io.finish();
  });
}

int hqpkkt_q_bfgs_report(hqpkkt_t *h, double *out, long long cap_blocks, long long *n_blocks) {
  return qv_report(h, &TreeDev::QVal::bfgs_last, &QPlan::rep, qv::QV_REPORT, out, cap_blocks, n_blocks);
}

// ---- the eigenvalue control of Hqp_HL_BFGS on the blocks of the sparse Q (q_eigen.hip.h)

// what a control with `steps` steps needs on the device beside the plan's tables: made or grown here, all or nothing - a
// failed allocation leaves the plan as it was
static int qe_buffers(hqpkkt_t *h, QPlan &p, int steps) {
  TreeDev::QVal &q = h->td.qv;
  const size_t n = (size_t)h->an.n;
  int e;
  if (!q.eig_w.p && (e = q.eig_w.alloc(2 * n))) return e;  // w, and behind it the row pass
  if (p.eig_V.p && p.eig_cap >= steps) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));  // (a report or a control still in the stream reads the old ones)
  DBuf<double> V, part, T, rep, st, flr;
  if ((e = V.alloc((size_t)steps * n)) || (e = part.alloc(((size_t)steps + 4) * p.nunits)) || (e = T.alloc(2 * (size_t)steps * p.nblocks)) ||
      (e = rep.alloc((size_t)qv::QE_REPORT * p.nblocks)) || (e = st.alloc(2 * (size_t)qv::QE_STATE * p.nblocks)) || (e = flr.alloc((size_t)p.nblocks)))
    return e;
  p.eig_V = std::move(V), p.eig_part = std::move(part), p.eig_T = std::move(T), p.eig_rep = std::move(rep), p.eig_st = std::move(st),
  p.eig_floor = std::move(flr);
  p.eig_cap = steps;
  return 0;
}

int hqpkkt_q_eigen_control(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec) {
  return guarded([&]() -> int {
    if (!h || !ec) return HQPKKT_E_NULL;
    static_assert(eig::MAX_STEPS == HQPKKT_EIG_MAX_STEPS && eig::REPORT == HQPKKT_EIG_REPORT, "the kernels size T and the report");
    if (!std::isfinite(ec->eps) || !(ec->eps > 0.0) || ec->max_steps < 0 || ec->max_steps > HQPKKT_EIG_MAX_STEPS) return HQPKKT_E_RANGE;
    if (ec->floor_from_bfgs != 0 && ec->floor_from_bfgs != 1) return HQPKKT_E_RANGE;
    int e = qv_refused(h, true), at = -1;
    if (e || (e = qb_plan(h, ec->bsize, false, &at))) return e;
    TreeDev::QVal &q = h->td.qv;
    if (ec->floor_from_bfgs && q.bfgs_last != at) return HQPKKT_E_INTERN;
    for (int b = 0; ec->floor && b < q.bfgs_plans[at].nblocks; b++)
      if (!std::isfinite(ec->floor[b])) return HQPKKT_E_RANGE;
    if ((e = qv_prepare(h, true, true))) return e;
    const int n = h->an.n;
    if (n <= 0) {
      q.eig_last = at, q.bfgs_plans[at].eig_steps = 0;
      return 0;
    }
    if ((e = qb_plan(h, ec->bsize, true, &at))) return e;
    QPlan &p = q.bfgs_plans[at];
    const int steps = std::min(ec->max_steps ? ec->max_steps : 64, p.max_len);
    if ((e = qe_buffers(h, p, steps))) return e;
    hipStream_t s = h->stream;
    if (ec->floor) {  // (a host array of the caller's, in the stream behind the last control's reads; it is the caller's again on return)
      HIPCHK(hipMemcpyAsync(p.eig_floor.p, ec->floor, sizeof(double) * (size_t)p.nblocks, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    // the partials of a unit: its products against the basis (steps), then v'w, w'w, the row pass' minimum and the start vector's sum
    double *V = p.eig_V.p, *T = p.eig_T.p, *rep = p.eig_rep.p, *w = q.eig_w.p, *offs = q.eig_w.p + n;
    double *partc = p.eig_part.p, *parta = partc + (size_t)steps * p.nunits, *partb = parta + p.nunits, *partg = partb + p.nunits, *partf = partg + p.nunits;
    double *st[2] = {p.eig_st.p, p.eig_st.p + (size_t)qv::QE_STATE * p.nblocks};
    const QShape L(h, p);
    const bool sh = L.short_rows, wu = L.wave_units;
    // the basis, `steps` vectors of n, and T are cleared: a block that is done keeps v = 0, words past a block's steps are 0
    HIPCHK(hipMemsetAsync(V, 0, sizeof(double) * (size_t)steps * n, s));
    HIPCHK(hipMemsetAsync(T, 0, sizeof(double) * 2 * (size_t)steps * p.nblocks, s));
    pick(sh, qv::k_qe_rows<16>, qv::k_qe_rows<4>)<<<L.rgrid, 256, 0, s>>>(n, h->td.Qf.dev(), p.blk_of.p, offs);
    pick(wu, qv::k_qe_unit0<4>, qv::k_qe_unit0<1>)<<<L.ugrid, 256, 0, s>>>(L.g, q.didx.p, h->td.vals.p, offs, partg, partf);
    qv::k_qe_begin<<<nblk(p.nblocks), 256, 0, s>>>(L.g, partg, ec->floor ? p.eig_floor.p : nullptr, ec->eps * ec->eps,
                                                   ec->floor_from_bfgs ? p.rep.p : nullptr, st[0], rep);
    pick(wu, qv::k_qe_v0<4>, qv::k_qe_v0<1>)<<<L.ugrid, 256, 0, s>>>(L.g, partf, st[0], V);
    for (int j = 0; j < steps; j++) {  // (nothing is read back: a unit of a block that has ended returns at once)
      const double *sj = st[j & 1];
      pick(sh, qv::k_qb_rows<16>, qv::k_qb_rows<4>)<<<L.rgrid, 256, 0, s>>>(n, h->td.Qf.dev(), p.blk_of.p, V + (size_t)j * n, w);
      pick(wu, qv::k_qe_alpha<4>, qv::k_qe_alpha<1>)<<<L.ugrid, 256, 0, s>>>(L.g, sj, V + (size_t)j * n, w, parta);
      pick(wu, qv::k_qe_resid<4>, qv::k_qe_resid<1>)<<<L.ugrid, 256, 0, s>>>(L.g, sj, V, (long long)n, j, steps, w, parta, partc);
      pick(wu, qv::k_qe_ortho<4>, qv::k_qe_ortho<1>)<<<L.ugrid, 256, 0, s>>>(L.g, sj, V, (long long)n, j, steps, w, partc, partb);
      pick(wu, qv::k_qe_next<4>, qv::k_qe_next<1>)<<<L.ugrid, 256, 0, s>>>(L.g, sj, st[(j + 1) & 1], V, (long long)n, j, j + 1 == steps ? 1 : 0, steps, w, parta, partb, T);
    }
    qv::k_qe_ritz<<<(unsigned)p.nblocks, 64, 0, s>>>(st[steps & 1], T, steps, rep);
    qv::k_qe_shift<<<nblk(n), 256, 0, s>>>(n, p.blk_of.p, q.didx.p, rep, h->td.vals.p);
    q.eig_last = at, p.eig_steps = steps;
    return qv_written(h);
  });
}

int hqpkkt_q_eigen_report(hqpkkt_t *h, double *out, double *T, long long cap_blocks, long long *n_blocks, int *t_steps) {
  if (!t_steps) return HQPKKT_E_NULL;
  return qv_report(h, &TreeDev::QVal::eig_last, &QPlan::eig_rep, qv::QE_REPORT, out, cap_blocks, n_blocks, T, t_steps);
}

int hqpkkt_lagrangian_gradient(hqpkkt_t *h, const double *c, const double *y, const double *z, const double *minus, double *out) {
  return guarded([&]() -> int {
    if (!h || !c || !out) return HQPKKT_E_NULL;
    if (h->analyzed && ((h->an.me > 0 && !y) || (h->an.m > 0 && !z))) return HQPKKT_E_NULL;
    int e = qv_prepare(h, false, false);
    if (e) return e;
    const Analysis &an = h->an;
    const int n = an.n;
    CallerVecs io{h};
    const double *dc, *dy, *dz, *dm;
    double *dout;
    if ((e = io.in(c, (size_t)n, &dc)) || (e = io.in(an.me > 0 ? y : nullptr, (size_t)an.me, &dy)) ||
        (e = io.in(an.m > 0 ? z : nullptr, (size_t)an.m, &dz)) || (e = io.in(minus, (size_t)n, &dm)))
      return e;
    io.out(out, (size_t)n, &dout);
    if (n > 0) {
      if ((double)(an.na + an.nc) / n < 8.0)
        qv::k_qv_grad_l<4><<<nblk(n, 64), 256, 0, h->stream>>>(n, h->td.AT.dev(), h->td.CT.dev(), dc, dy, dz, dm, dout);
      else
        qv::k_qv_grad_l<16><<<nblk(n, 16), 256, 0, h->stream>>>(n, h->td.AT.dev(), h->td.CT.dev(), dc, dy, dz, dm, dout);
    }
    HIPCHK(hipGetLastError());
    return io.finish();
  });
}
