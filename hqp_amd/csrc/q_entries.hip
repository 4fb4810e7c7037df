// The entries of the C ABI (include/hqpkkt.h) on the sparse Q of the program where it lies on the device, 23 of them:
// hqpkkt_q_values .. hqpkkt_q_dscale_report (kernels: q_values.hip.h), hqpkkt_q_blocks, hqpkkt_q_bfgs_update and its report
// (q_bfgs.hip.h), hqpkkt_q_components, hqpkkt_q_sparse_bfgs_update and its report (q_sparse_bfgs.hip.h),
// hqpkkt_q_eigen_control and its report (q_eigen.hip.h), hqpkkt_q_eigen_control_short (q_eigen_short.hip.h),
// hqpkkt_q_eigen_control_exact (q_eigen_mid.hip.h beside it), hqpkkt_q_eigen_control_long (q_eigen_long.hip.h beside both),
// hqpkkt_q_eigen_control_blocked (q_eigen_blocked.hip.h beside all three), hqpkkt_q_eigen_control_wide (q_eigen_wide.hip.h
// beside all four) and hqpkkt_lagrangian_gradient.  Their state is TreeDev::QVal; everything else they use of the handle is declared in hqpkkt_handle.hpp.
// The damped updates - Hqp_HL_DScale::update on the diagonal, Hqp_HL_BFGS on the blocks - are ONE pipeline over the plan of
// a partition (qb_plan): the sums of the units, the decision per block, v and s'v, the outcome per block, and then the
// update's own write (k_qv_ds_apply per variable, k_qb_apply per stored entry).  The eigenvalue control runs over the
// same plans.
#include <mutex>
#include <numeric>

#include "hqpkkt_handle.hpp"
#include "q_values.hip.h"
#include "q_bfgs.hip.h"
#include "q_sparse_bfgs.hip.h"
#include "q_eigen.hip.h"
#include "q_eigen_short.hip.h"
#include "q_eigen_mid.hip.h"
#include "q_eigen_long.hip.h"
#include "q_eigen_blocked.hip.h"
#include "q_eigen_wide.hip.h"

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

// The connected components of the graph of Q's analysed pattern (the blocks Hqp_HL_SparseBFGS finds behind its
// permutation), from the entries with col > row alone: numbered by their smallest variable, `member` their variables block
// after block and ascending inside one, `first` the blocks' first POSITIONS in it with n behind them; and per block whether
// every (i, j), i <= j, of it is stored.  Union by the smaller root, so a root is its component's smallest variable.
static void qsb_partition(const hqpkkt_t *h, std::vector<int> &first, std::vector<int> &member, std::vector<unsigned char> &full) {
  const int n = h->an.n;
  const int *Qp = h->pQp.data(), *Qi = h->pQi.data();
  first.clear(), member.clear(), full.clear();
  if (n <= 0) return;
  std::vector<int> root((size_t)n), blk((size_t)n);
  std::iota(root.begin(), root.end(), 0);
  const auto find = [&](int i) {
    while (root[i] != i) i = root[i] = root[root[i]];
    return i;
  };
  for (int i = 0; i < n; i++)
    for (int k = Qp[i]; k < Qp[i + 1]; k++)
      if (Qi[k] > i) {
        const int a = find(i), b = find(Qi[k]);
        root[std::max(a, b)] = std::min(a, b);
      }
  int nb = 0;
  for (int i = 0; i < n; i++) {  // (a root comes before its members: it has its number when they ask)
    const int r = find(i);
    if (r == i) first.push_back(0), nb++;
    blk[i] = r == i ? nb - 1 : blk[r];
    first[blk[i]]++;
  }
  first.push_back(0);
  for (int b = 0, at = 0; b <= nb; b++) {  // lengths -> first positions
    const int len = first[b];
    first[b] = at, at += len;
  }
  member.resize((size_t)n);
  std::vector<int> fill(first.begin(), first.end() - 1);
  std::vector<long long> stored((size_t)nb, 0);
  for (int i = 0; i < n; i++) {
    member[fill[blk[i]]++] = i;
    for (int k = Qp[i]; k < Qp[i + 1]; k++) stored[blk[i]] += Qi[k] >= i;  // (the rows are strictly ascending: a count decides)
  }
  for (int b = 0; b < nb; b++) {
    const long long len = first[b + 1] - first[b];
    full.push_back(stored[b] == len * (len + 1) / 2);
  }
}

int hqpkkt_q_components(hqpkkt_t *h, int *first, int *member, int *full, long long cap, long long *n_blocks) {
  return guarded([&]() -> int {
    if (!h || !n_blocks || (first && !member)) return HQPKKT_E_NULL;
    if (!h->analyzed) return HQPKKT_E_INTERN;
    std::vector<int> f, m;
    std::vector<unsigned char> fl;
    qsb_partition(h, f, m, fl);
    *n_blocks = (long long)fl.size();
    if (!first) return 0;
    if (cap < *n_blocks) return HQPKKT_E_RANGE;
    std::copy(f.begin(), f.end(), first), std::copy(m.begin(), m.end(), member);
    if (full) std::copy(fl.begin(), fl.end(), full);
    return 0;
  });
}

// the plan of one key - a bsize's (qb_key) or QB_COMPONENTS -: the host's partition, then (with_device) its tables, partial
// sums and the BFGS update's report on the device; the components' plan has its member list, the positions and the packed
// vectors besides
static int qb_plan_of(hqpkkt_t *h, int key, bool with_device, int *index) {
  TreeDev::QVal &q = h->td.qv;
  const int n = h->an.n;
  int at = -1;
  for (size_t k = 0; k < q.bfgs_plans.size(); k++)
    if (q.bfgs_plans[k].bsize == key) at = (int)k;
  if (at < 0) {
    QPlan p;
    p.bsize = key;
    if (key == TreeDev::QVal::QB_COMPONENTS)
      qsb_partition(h, p.first, p.member, p.full);
    else
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
    for (int j = p.first[b]; j < p.first[b + 1]; j++) blk_of[p.member.empty() ? j : p.member[j]] = b;
    bunit[b] = u;
    for (int j = 0; j < (len + qv::QV_CHUNK - 1) / qv::QV_CHUNK; j++) ublk[u++] = b;
    bunit[b + 1] = u;
  }
  int e;
  if ((e = p.boff.upload(p.first)) || (e = p.bunit.upload(bunit)) || (e = p.ublk.upload(ublk)) || (e = p.part.alloc(3 * (size_t)p.nunits)) ||
      (e = p.rep.alloc((size_t)qv::QV_REPORT * p.nblocks)))
    return e;
  if (!p.member.empty()) {
    std::vector<int> pos_of((size_t)n);
    for (int j = 0; j < n; j++) pos_of[p.member[j]] = j;
    if ((e = p.d_member.upload(p.member)) || (e = p.pos_of.upload(pos_of)) || (e = p.pk.alloc(2 * (size_t)n))) return e;
  }
  return p.blk_of.upload(blk_of);  // (last: it says the plan is complete)
}
static int qb_plan(hqpkkt_t *h, int bsize, bool with_device, int *index) { return qb_plan_of(h, qb_key(h, bsize), with_device, index); }

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
// `member` (the components' plan, its vectors in block order): the decision with Hqp_HL_SparseBFGS's clamp.
template <bool DIAG>
static void qb_passes(hqpkkt_t *h, const QPlan &p, const QShape &L, const double *s, const double *y, const double *src, const int *didx,
                      double gamma, double *rep, double *v, const int *member = nullptr) {
  const int B = p.max_len;  // (DIAG: the block length of the uniform partition)
  double *part = p.part.p, *part2 = p.part.p + 2 * (size_t)p.nunits;
  hipStream_t st = h->stream;
  pick(L.wave_units, qv::k_qb_sums<4, DIAG>, qv::k_qb_sums<1, DIAG>)<<<L.ugrid, 256, 0, st>>>(L.g, s, y, src, didx, B, part);
  if (member)
    qv::k_qsb_decide<<<nblk(p.nblocks), 256, 0, st>>>(L.g, member, part, gamma, rep);
  else
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

// what every plan's BFGS update shares, made by the first: the entries' rows and columns, Q s and v
static int qb_shared(hqpkkt_t *h) {
  TreeDev::QVal &q = h->td.qv;
  if (q.erow.p) return 0;
  const int n = h->an.n;
  std::vector<int> erow((size_t)h->an.nq);
  for (int i = 0; i < n; i++) std::fill(erow.begin() + h->pQp[i], erow.begin() + h->pQp[i + 1], i);
  int e;
  if ((e = q.ecol.upload(h->pQi)) || (e = q.bfgs_qs.alloc((size_t)n)) || (e = q.bfgs_v.alloc((size_t)n)) || (e = q.erow.upload(erow))) return e;
  return 0;
}

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
    if ((e = qb_shared(h)) || (e = qb_plan(h, u->bsize, true, &at))) return e;
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

// ---- Hqp_HL_SparseBFGS: the update on the connected components, their variables anywhere (q_sparse_bfgs.hip.h)

int hqpkkt_q_sparse_bfgs_update(hqpkkt_t *h, const hqpkkt_q_bfgs_update_args *u) {
  return guarded([&]() -> int {
    if (!h || !u || !u->s || !u->y) return HQPKKT_E_NULL;
    if (!std::isfinite(u->gamma) || u->gamma < 0.0 || u->bsize != 0) return HQPKKT_E_RANGE;  // (the reference's SparseBFGS ignores alpha)
    if (u->fill != HQPKKT_QBFGS_FULL && u->fill != HQPKKT_QBFGS_PATTERN) return HQPKKT_E_RANGE;
    int e = qv_refused(h, true), at = -1;
    if (e || (e = qb_plan_of(h, TreeDev::QVal::QB_COMPONENTS, false, &at))) return e;
    if (u->fill == HQPKKT_QBFGS_FULL && !h->td.qv.bfgs_plans[at].all_full) return HQPKKT_E_FORMAT;
    if ((e = qv_prepare(h, true, false))) return e;
    TreeDev::QVal &q = h->td.qv;
    const int n = h->an.n, nq = h->an.nq;
    if (n <= 0) {
      q.sbfgs_last = at;
      return 0;
    }
    if ((e = qb_shared(h)) || (e = qb_plan_of(h, TreeDev::QVal::QB_COMPONENTS, true, &at))) return e;
    const QPlan &p = q.bfgs_plans[at];
    CallerVecs io{h};
    const double *ds, *dy;
    double *dv, *dQs;
    if ((e = io.in(u->s, (size_t)n, &ds)) || (e = io.in(u->y, (size_t)n, &dy))) return e;
    io.out(u->v, (size_t)n, &dv), io.out(u->Qs, (size_t)n, &dQs);
    double *sp = p.pk.p, *yp = sp + n, *Qsp = q.bfgs_qs.p, *vp = q.bfgs_v.p;  // all four in block order
    hipStream_t s = h->stream;
    const QShape L(h, p);
    qv::k_qsb_pack<<<nblk(n), 256, 0, s>>>(n, p.d_member.p, ds, dy, sp, yp);
    pick(L.short_rows, qv::k_qsb_rows<16>, qv::k_qsb_rows<4>)<<<L.rgrid, 256, 0, s>>>(n, h->td.Qf.dev(), p.pos_of.p, ds, Qsp);
    qb_passes<false>(h, p, L, sp, yp, Qsp, nullptr, u->gamma, p.rep.p, vp, p.d_member.p);
    if (nq) qv::k_qsb_apply<<<nblk(nq), 256, 0, s>>>(nq, q.erow.p, q.ecol.p, q.kind.p, p.blk_of.p, p.pos_of.p, Qsp, vp, p.rep.p, h->td.vals.p);
    if (dv || dQs) qv::k_qsb_unpack<<<nblk(n), 256, 0, s>>>(n, p.d_member.p, vp, Qsp, dv, dQs);
    q.sbfgs_last = at;
    if ((e = qv_written(h))) return e;
    return io.finish();
  });
}

int hqpkkt_q_sparse_bfgs_report(hqpkkt_t *h, double *out, long long cap_blocks, long long *n_blocks) {
  return qv_report(h, &TreeDev::QVal::sbfgs_last, &QPlan::rep, qv::QV_REPORT, out, cap_blocks, n_blocks);
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
  p.eig_cap = p.eig_tcap = steps;
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

// ---- the same control on a plan of short blocks: Householder's T of every block, one launch (q_eigen_short.hip.h)

// what it needs beside the plan's tables - the report, T with stride 2 max_len per block, the floors -, made or grown as
// qe_buffers does; the basis, the partials and the states stay as they are for hqpkkt_q_eigen_control to make or grow
static int qes_buffers(hqpkkt_t *h, QPlan &p) {
  if (p.eig_rep.p && p.eig_tcap >= p.max_len) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));  // (a report or a control still in the stream reads the old ones)
  DBuf<double> T, rep, flr;
  int e;
  if ((e = T.alloc(2 * (size_t)p.max_len * p.nblocks)) || (e = rep.alloc((size_t)qv::QE_REPORT * p.nblocks)) || (e = flr.alloc((size_t)p.nblocks))) return e;
  p.eig_T = std::move(T), p.eig_rep = std::move(rep), p.eig_floor = std::move(flr);
  p.eig_tcap = p.max_len;
  return 0;
}

// ---- and on blocks up to 128 and up to 512: the blocks of 65 .. 128 by a workgroup each, over their list (q_eigen_mid.hip.h);
// the blocks of 129 .. 512 by persistent workgroups over theirs, the images in device memory (q_eigen_long.hip.h)

// one pass over the plan: the list of its blocks of 65 .. 128, of its blocks of 129 .. 512 and of its blocks of 513 .. 2048
// (q_eigen_blocked.hip.h), the longest of each and the longest block of at most 64: made once per plan
static int qem_list(QPlan &p) {
  if (p.mid_count >= 0) return 0;
  std::vector<int> mid, lng, blk;
  int mid_max = 0, short_max = 0, long_max = 0, blk_max = 0;
  for (int b = 0; b < p.nblocks; b++) {
    const int len = p.first[b + 1] - p.first[b];
    if (len >= qv::QEB_MIN && len <= qv::QEB_MAX)
      blk.push_back(b), blk_max = std::max(blk_max, len);
    else if (len >= qv::QEL_MIN && len <= qv::QEL_MAX)
      lng.push_back(b), long_max = std::max(long_max, len);
    else if (len >= qv::QEM_MIN && len <= qv::QEM_MAX)
      mid.push_back(b), mid_max = std::max(mid_max, len);
    else if (len < qv::QEM_MIN)
      short_max = std::max(short_max, len);
  }
  DBuf<int> dm, dl, db;
  int e;
  if ((e = dm.upload(mid)) || (e = dl.upload(lng)) || (e = db.upload(blk))) return e;
  p.mid_list = std::move(dm), p.long_list = std::move(dl), p.blk_list = std::move(db);
  p.long_count = (int)lng.size(), p.long_max = long_max;
  p.blk_count = (int)blk.size(), p.blk_max = blk_max;
  p.mid_count = (int)mid.size(), p.mid_max = mid_max, p.short_max = short_max;
  return 0;
}
// the images of k_qel_block: slots = min(listed blocks, CUs) - capped by the test hook HQPKKT_QEL_SLOTS, read here -, each
// LD x LD doubles, LD the longest listed block rounded up to 16: at most 256 x 2 MB.  All or nothing
static int qel_workspace(hqpkkt_t *h, QPlan &p) {
  if (p.long_ws.p || p.long_count <= 0) return 0;
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->opts.device));
  int slots = std::min(p.long_count, std::max(cus, 1));
  if (const char *cap = getenv("HQPKKT_QEL_SLOTS"))
    if (atoi(cap) > 0) slots = std::min(slots, atoi(cap));
  const int ld = (p.long_max + 15) & ~15;
  DBuf<double> ws;
  if (int e = ws.alloc((size_t)slots * ld * ld)) return e;
  p.long_ws = std::move(ws), p.long_slots = slots, p.long_ld = ld;
  return 0;
}
// the slots of k_qeb_block: slots = min(listed blocks, CUs, what 4 GiB hold) - capped by the test hook HQPKKT_QEB_SLOTS, read
// here -, each an image of LD x LD doubles, LD the longest listed block rounded up to 16, and two panels of LD x 32.  All or
// nothing
static int qeb_workspace(hqpkkt_t *h, QPlan &p) {
  if (p.blk_ws.p || p.blk_count <= 0) return 0;
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->opts.device));
  const int ld = (p.blk_max + 15) & ~15;
  const size_t slot = qv::qeb_slot_doubles(ld) * sizeof(double), most = ((size_t)4 << 30) / slot;
  int slots = (int)std::min<size_t>(std::min(p.blk_count, std::max(cus, 1)), most);
  if (const char *cap = getenv("HQPKKT_QEB_SLOTS"))
    if (atoi(cap) > 0) slots = std::min(slots, atoi(cap));
  DBuf<double> ws;
  if (int e = ws.alloc((size_t)slots * qv::qeb_slot_doubles(ld))) return e;
  p.blk_ws = std::move(ws), p.blk_slots = slots, p.blk_ld = ld;
  return 0;
}
// the dynamic LDS of k_qeb_ritz, 96 KB: set once per device, as qem_raise_lds below does; a device that refuses it is
// HQPKKT_E_DEVICE before any launch
static int qeb_raise_lds(hqpkkt_t *h) {
  static std::mutex attr_mutex;
  static bool done[64];
  if (h->opts.device < 0 || h->opts.device >= 64) return HQPKKT_E_RANGE;
  std::lock_guard<std::mutex> lk(attr_mutex);
  if (done[h->opts.device]) return 0;
  HIPCHK(hipFuncSetAttribute((const void *)qv::k_qeb_ritz, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(eig::RitzLdsT<qv::QEB_MAX>)));
  done[h->opts.device] = true;
  return 0;
}
// columns per panel of k_qeb_block: QEB_NB by the measurement in DESIGN.md; HQPKKT_QEB_NB (16 or 32) is the hook that
// measurement used - the two instances give different bits, each its own from call to call
static const int QEB_NB = 16;
static int qeb_nb() {
  const char *v = getenv("HQPKKT_QEB_NB");  // (read per call: the measurement lets the two take turns)
  return v && (atoi(v) == 16 || atoi(v) == 32) ? atoi(v) : QEB_NB;
}
// the dynamic-LDS limits of k_qem_block: state of the process and of the current device (as raise_lds_limits, tree.hip),
// constants here, so set once per device
static int qem_raise_lds(hqpkkt_t *h) {
  static std::mutex attr_mutex;
  static bool done[64];
  if (h->opts.device < 0 || h->opts.device >= 64) return HQPKKT_E_RANGE;
  std::lock_guard<std::mutex> lk(attr_mutex);
  if (done[h->opts.device]) return 0;
  HIPCHK(hipFuncSetAttribute((const void *)qv::k_qem_block<96>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)qv::qem_lds_bytes<96>()));
  HIPCHK(hipFuncSetAttribute((const void *)qv::k_qem_block<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)qv::qem_lds_bytes<128>()));
  done[h->opts.device] = true;
  return 0;
}

// threads per workgroup of k_qel_block: QEL_THREADS by the measurement in DESIGN.md; HQPKKT_QEL_THREADS (512 or 1024) is the
// hook that measurement used - the two instances give the same bits
static const int QEL_THREADS = 1024;
static int qel_threads() {
  const char *v = getenv("HQPKKT_QEL_THREADS");  // (read per call: the measurement lets the two take turns)
  return v ? atoi(v) : QEL_THREADS;
}

// ---- and on blocks up to 8192: the blocks of HQPKKT_QEW_FROM and more by the whole chip, a few slots in lockstep, one lower
// triangle of the image stored (q_eigen_wide.hip.h); the others by the kernels above, over lists without them

// the test hooks of the wide control, read per call: HQPKKT_QEW_FROM, the smallest block length that takes the k_qew_* kernels
// (1 .. 2049, the default: k_qeb_block serves no more than 2048), and HQPKKT_QEW_GROUPS, the most workgroups per slot of
// k_qew_pass
static int qew_env(const char *name, int lo, int hi, int dflt) {
  const char *v = getenv(name);
  return v && atoi(v) >= lo && atoi(v) <= hi ? atoi(v) : dflt;
}
// one pass over the plan for a threshold `from`: the blocks that long, longest first; the runs of blocks between them for
// k_qes_block; the lists of qem_list without them.  Kept with the plan until a call comes with another threshold
static int qew_lists(hqpkkt_t *h, QPlan &p, int from) {
  if (p.wl.from == from) return 0;
  HIPCHK(hipStreamSynchronize(h->stream));  // (a control still in the stream reads the old lists)
  QPlan::WideLists w;
  std::vector<int> mid, lng, blk;
  for (int b = 0; b < p.nblocks; b++) {
    const int len = p.first[b + 1] - p.first[b];
    if (len >= from) {
      w.wide.push_back(b);
      continue;
    }
    if (!w.runs.empty() && w.runs.back() == b)
      w.runs.back() = b + 1;
    else
      w.runs.push_back(b), w.runs.push_back(b + 1);
    if (len >= qv::QEB_MIN)
      blk.push_back(b);
    else if (len >= qv::QEL_MIN)
      lng.push_back(b);
    else if (len >= qv::QEM_MIN)
      mid.push_back(b), w.mid_max = std::max(w.mid_max, len);
    else
      w.short_max = std::max(w.short_max, len);
  }
  std::stable_sort(w.wide.begin(), w.wide.end(), [&](int a, int b) { return p.first[a + 1] - p.first[a] > p.first[b + 1] - p.first[b]; });
  w.mid_count = (int)mid.size(), w.long_count = (int)lng.size(), w.blk_count = (int)blk.size();
  int e;
  if ((e = w.wide_list.upload(w.wide)) || (e = w.mid_list.upload(mid)) || (e = w.long_list.upload(lng)) || (e = w.blk_list.upload(blk))) return e;
  w.from = from;
  p.wl = std::move(w);
  return 0;
}
// the slots of k_qew_*: slots = min(listed blocks, CUs, what 4 GiB and half the free memory hold) - capped by the test hook
// HQPKKT_QEW_SLOTS, read here -, each qew_slot_doubles(LD), LD the plan's longest block rounded up to 64: made once and kept
// with the plan; six work arrays of max_len per listed block for k_qew_ritz, grown where a call lists more; and the dynamic
// LDS of k_qew_pass, v of a block of 8192 and the parts, set once per device.  All or nothing
static int qew_workspace(hqpkkt_t *h, QPlan &p) {
  const size_t count = p.wl.wide.size();
  if (!count) return 0;
  static std::mutex attr_mutex;
  static bool raised[64];
  if (h->opts.device < 0 || h->opts.device >= 64) return HQPKKT_E_RANGE;
  {
    std::lock_guard<std::mutex> lk(attr_mutex);
    if (!raised[h->opts.device])
      HIPCHK(hipFuncSetAttribute((const void *)qv::k_qew_pass, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * qv::qew_pass_doubles(qv::QEW_MAX))));
    raised[h->opts.device] = true;
  }
  DBuf<double> ws, rz;
  int e, slots = p.wide_slots;
  const int ld = (p.max_len + qv::QEW_M - 1) & ~(qv::QEW_M - 1);
  if (p.wide_rz < count) {
    HIPCHK(hipStreamSynchronize(h->stream));  // (a control still in the stream uses the old arrays)
    if ((e = rz.alloc(6 * (size_t)p.max_len * count))) return e;
  }
  if (!p.wide_ws.p) {
    int cus = 0;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->opts.device));
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const size_t slot = qv::qew_slot_doubles(ld) * sizeof(double), most = std::max<size_t>(std::min<size_t>((size_t)4 << 30, free_b / 2) / slot, 1);
    slots = (int)std::min<size_t>(std::min<size_t>(count, (size_t)std::max(cus, 1)), most);
    if (const char *cap = getenv("HQPKKT_QEW_SLOTS"))
      if (atoi(cap) > 0) slots = std::min(slots, atoi(cap));
    if ((e = ws.alloc((size_t)slots * qv::qew_slot_doubles(ld)))) return e;
  }
  if (rz.p) p.wide_ritz = std::move(rz), p.wide_rz = count;
  if (ws.p) p.wide_ws = std::move(ws), p.wide_slots = slots, p.wide_ld = ld;
  return 0;
}
// The listed blocks in batches of wide_slots, all slots of a batch in lockstep: the gather, the off-diagonal sums and the
// start, then per column k k_qew_column (finish k - 1, form k; behind a whole panel finish, k_qew_update, form) and k_qew_pass;
// then k_qew_ritz over all, and the shift over the rows of each
static void qew_launches(hqpkkt_t *h, const QPlan &p, const double *flr, double eps2, const double *bfgs, int cap) {
  const int nw = (int)p.wl.wide.size(), LD = p.wide_ld, NB = qv::QEW_NB, M = qv::QEW_M;
  const int groups = qew_env("HQPKKT_QEW_GROUPS", 1, qv::QEW_G, qv::QEW_G);
  const int *boff = p.boff.p;
  double *T = p.eig_T.p, *rep = p.eig_rep.p, *ws = p.wide_ws.p;
  hipStream_t s = h->stream;
  for (int b0 = 0; b0 < nw; b0 += p.wide_slots) {
    const unsigned nb = (unsigned)std::min(p.wide_slots, nw - b0);
    const int *wl = p.wl.wide_list.p + b0;
    const int Lb = p.first[p.wl.wide[b0] + 1] - p.first[p.wl.wide[b0]], nT = (Lb + M - 1) / M;
    qv::k_qew_gather<<<dim3((unsigned)nT, nb), 256, 0, s>>>(wl, boff, h->td.Qf.dev(), cap, ws, LD);
    qv::k_qew_offsum<<<dim3((unsigned)nT, nb), 64, 0, s>>>(wl, boff, cap, ws, LD);
    qv::k_qew_start<<<nb, 256, 0, s>>>(wl, boff, flr, eps2, bfgs, cap, T, rep, ws, LD);
    for (int k = 0; k < Lb; k++) {
      if (k > 0 && k % NB == 0) {
        const int left = nT - k / M;
        qv::k_qew_column<<<nb, qv::QEW_NT, 0, s>>>(wl, boff, cap, T, rep, ws, LD, k - 1, -1);
        qv::k_qew_update<<<dim3((unsigned)(left * (left + 1) / 2), nb), 256, 0, s>>>(wl, boff, rep, cap, ws, LD, k);
        qv::k_qew_column<<<nb, qv::QEW_NT, 0, s>>>(wl, boff, cap, T, rep, ws, LD, -1, k);
      } else
        qv::k_qew_column<<<nb, qv::QEW_NT, 0, s>>>(wl, boff, cap, T, rep, ws, LD, k - 1, k);
      if (k + 2 < Lb) {  // (the last two columns form no reflector)
        const int rows = nT - (k + 1) / M;  // the tile rows that hold an index > k
        qv::k_qew_pass<<<dim3((unsigned)std::min(rows, groups), nb), qv::QEW_PNT, sizeof(double) * qv::qew_pass_doubles(M * rows), s>>>(wl, boff, rep, cap, ws, LD, k);
      }
    }
  }
  qv::k_qew_ritz<<<(unsigned)nw, 64, 0, s>>>(p.wl.wide_list.p, boff, cap, T, rep, p.wide_ritz.p);
  for (int b : p.wl.wide) {
    const int first = p.first[b], len = p.first[b + 1] - first;
    qv::k_qe_shift<<<nblk(len), 256, 0, s>>>(len, p.blk_of.p + first, h->td.qv.didx.p + first, rep, h->td.vals.p);
  }
}

// the five entries: `longest` is the block length the entry serves, 64, 128, 512, 2048 or 8192 (the wide entry: the blocks
// of its threshold and more through qew_launches, the lists of the others from qew_lists)
static int qes_control(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec, int longest) {
  return guarded([&]() -> int {
    if (!h || !ec) return HQPKKT_E_NULL;
    if (!std::isfinite(ec->eps) || !(ec->eps > 0.0) || ec->max_steps != 0) return HQPKKT_E_RANGE;
    if (ec->floor_from_bfgs != 0 && ec->floor_from_bfgs != 1) return HQPKKT_E_RANGE;
    int e = qv_refused(h, true), at = -1;
    if (e || (e = qb_plan(h, ec->bsize, false, &at))) return e;
    TreeDev::QVal &q = h->td.qv;
    if (ec->floor_from_bfgs && q.bfgs_last != at) return HQPKKT_E_INTERN;
    for (int b = 0; ec->floor && b < q.bfgs_plans[at].nblocks; b++)
      if (!std::isfinite(ec->floor[b])) return HQPKKT_E_RANGE;
    const int cap = q.bfgs_plans[at].max_len;
    if (cap > longest) return HQPKKT_E_SIZES;
    if ((e = qv_prepare(h, true, true))) return e;
    if (h->an.n <= 0) {
      q.eig_last = at, q.bfgs_plans[at].eig_steps = 0;
      return 0;
    }
    if ((e = qb_plan(h, ec->bsize, true, &at))) return e;
    QPlan &p = q.bfgs_plans[at];
    if ((e = qes_buffers(h, p))) return e;
    const bool wide = longest == qv::QEW_MAX;
    const bool mid = cap > 64 || wide;  // (the plan has blocks for k_qem_block)
    if (mid && (e = qem_list(p))) return e;
    if (wide && ((e = qew_lists(h, p, qew_env("HQPKKT_QEW_FROM", 1, qv::QEW_MIN, qv::QEW_MIN))) || (e = qew_workspace(h, p)))) return e;
    // the lists of this call: the plan's, or the wide entry's without its own blocks (the same where it has none)
    const QPlan::WideLists &w = p.wl;
    const int mid_count = wide ? w.mid_count : mid ? p.mid_count : 0, mid_max = wide ? w.mid_max : p.mid_max;
    const int long_count = wide ? w.long_count : mid ? p.long_count : 0, blk_count = wide ? w.blk_count : mid ? p.blk_count : 0;
    const int *mid_list = wide ? w.mid_list.p : p.mid_list.p, *long_list = wide ? w.long_list.p : p.long_list.p, *blk_list = wide ? w.blk_list.p : p.blk_list.p;
    const bool lng = long_count > 0;  // (blocks for k_qel_block)
    const bool blk = blk_count > 0;   // (and for k_qeb_block)
    if ((lng && (e = qel_workspace(h, p))) || (mid_count > 0 && (e = qem_raise_lds(h)))) return e;
    if (blk && ((e = qeb_workspace(h, p)) || (e = qeb_raise_lds(h)))) return e;
    hipStream_t s = h->stream;
    if (ec->floor) {  // (as hqpkkt_q_eigen_control: the caller's again on return)
      HIPCHK(hipMemcpyAsync(p.eig_floor.p, ec->floor, sizeof(double) * (size_t)p.nblocks, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
    }
    const double *flr = ec->floor ? p.eig_floor.p : nullptr, *bfgs = ec->floor_from_bfgs ? p.rep.p : nullptr;
    const double eps2 = ec->eps * ec->eps;
    // the instance by the LDS of its image: the smallest that holds the longest block of at most 64, which returns at
    // once on a longer one; the wide entry launches it over the runs of blocks between its own
    const int sm = wide ? w.short_max : mid ? p.short_max : cap;
    const auto block = pick(sm > 16, pick(sm > 8, qv::k_qes_block<8>, qv::k_qes_block<16>), pick(sm > 32, qv::k_qes_block<32>, qv::k_qes_block<64>));
    const int whole[2] = {0, p.nblocks};
    const int *runs = wide ? w.runs.data() : whole;
    for (size_t r = 0; r < (wide ? w.runs.size() : 2); r += 2) {
      const long long a = runs[r];
      block<<<(unsigned)(runs[r + 1] - runs[r]), 64, 0, s>>>(p.boff.p + a, h->td.Qf.dev(), q.didx.p, h->td.vals.p, flr ? flr + a : nullptr, eps2,
                                                          bfgs ? bfgs + qv::QV_REPORT * a : nullptr, cap, p.eig_T.p + 2 * (long long)cap * a, p.eig_rep.p + qv::QE_REPORT * a);
    }
    if (mid_count > 0) {
      const bool big = mid_max > 96;
      pick(big, qv::k_qem_block<96>, qv::k_qem_block<128>)<<<(unsigned)mid_count, 256, big ? qv::qem_lds_bytes<128>() : qv::qem_lds_bytes<96>(), s>>>(
          mid_list, p.boff.p, h->td.Qf.dev(), flr, eps2, bfgs, cap, p.eig_T.p, p.eig_rep.p);
      qv::k_qem_ritz<<<(unsigned)mid_count, 64, 0, s>>>(mid_list, p.boff.p, q.didx.p, h->td.vals.p, cap, p.eig_T.p, p.eig_rep.p);
    }
    if (lng) {
      const bool many = qel_threads() > 512;
      pick(many, qv::k_qel_block<512>, qv::k_qel_block<1024>)<<<(unsigned)std::min(p.long_slots, long_count), many ? 1024 : 512, 0, s>>>(
          long_list, long_count, p.boff.p, h->td.Qf.dev(), flr, eps2, bfgs, cap, p.eig_T.p, p.eig_rep.p, p.long_ws.p, p.long_ld);
      qv::k_qel_ritz<<<(unsigned)long_count, 64, 0, s>>>(long_list, p.boff.p, q.didx.p, h->td.vals.p, cap, p.eig_T.p, p.eig_rep.p);
    }
    if (blk) {
      pick(qeb_nb() > 16, qv::k_qeb_block<16>, qv::k_qeb_block<32>)<<<(unsigned)std::min(p.blk_slots, blk_count), qv::QEB_NT, 0, s>>>(
          blk_list, blk_count, p.boff.p, h->td.Qf.dev(), flr, eps2, bfgs, cap, p.eig_T.p, p.eig_rep.p, p.blk_ws.p, p.blk_ld);
      qv::k_qeb_ritz<<<(unsigned)blk_count, 64, sizeof(eig::RitzLdsT<qv::QEB_MAX>), s>>>(blk_list, p.boff.p, q.didx.p, h->td.vals.p, cap, p.eig_T.p, p.eig_rep.p);
    }
    if (wide && !w.wide.empty()) qew_launches(h, p, flr, eps2, bfgs, cap);
    q.eig_last = at, p.eig_steps = cap;
    return qv_written(h);
  });
}

int hqpkkt_q_eigen_control_short(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec) { return qes_control(h, ec, 64); }
int hqpkkt_q_eigen_control_exact(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec) { return qes_control(h, ec, qv::QEM_MAX); }
int hqpkkt_q_eigen_control_long(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec) {
  static_assert(qv::QEL_MAX == HQPKKT_QEIG_LONG_MAX, "the kernels size their LDS by it");
  return qes_control(h, ec, qv::QEL_MAX);
}
int hqpkkt_q_eigen_control_blocked(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec) {
  static_assert(qv::QEB_MAX == HQPKKT_QEIG_BLOCKED_MAX, "the kernels size their LDS by it");
  return qes_control(h, ec, qv::QEB_MAX);
}
int hqpkkt_q_eigen_control_wide(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *ec) {
  static_assert(qv::QEW_MAX == HQPKKT_QEIG_WIDE_MAX, "the kernels size their partial sums by it");
  return qes_control(h, ec, qv::QEW_MAX);
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
