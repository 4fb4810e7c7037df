// Host side of the entries on the dense stage Hessians (hqpkkt_set_stage_hessian .. hqpkkt_eigen_report; kernels:
// staged_hess*.hip.h).  Included by staged_engine.hip alone, behind staged_host.hip.h and the helpers of the dense
// hand-over.  Every entry is a HessCall: the context offers the steps - handle test, arrival, device, geometry, update
// launch - and the entry's body says in which order it takes them, because that order is the header's (include/hqpkkt.h
// documents it per entry) and differs from entry to entry.  A caller's vectors go through CallerVecs (hqpkkt_handle.hpp).
#pragma once

namespace {

// where block k lies and how its launches cover it: offset in the arena, leading dimension, tile rows, order, first
// column, packed flag, and the units of a launch over the whole block (stored tiles, or nt x nt tiles of the dense block)
struct HessGeom {
  long long off;
  int ld, nt, nz, col0, packed, units;
};

struct HessCall {
  hqpkkt_t *h;
  StagedDev &d;
  const kktdev::StagedPlan &P;
  const int K1;
  const size_t n;
  explicit HessCall(hqpkkt_t *h_) : h(h_), d(*h_->sd), P(d.plan), K1(P.K + 1), n((size_t)P.n) {}
  // what the entries ask of the handle before they make a HessCall: the dense form with the dense hand-over; the
  // entries that only read (product, reports, debug views): an uploaded handle of the dense form, either hand-over
  static bool ready(const hqpkkt_t *h) { return staged_dense_ready(h, true); }
  static bool uploaded(const hqpkkt_t *h) { return h->sd && h->uploaded && h->sd->plan.hess_dense; }
  // the hand-over rule: which blocks have arrived since the analysis
  bool arrived(int k) const { return (int)d.hess.set.size() == K1 && d.hess.set[k]; }
  void mark_arrived(int k) {
    if ((int)d.hess.set.size() != K1) d.hess.set.assign(K1, 0);
    d.hess.set[k] = 1;
  }
  // the entries that read the blocks: every block of nonzero order has arrived (need: of the stages it marks alone)
  int all_arrived(const unsigned char *need) const {
    for (int k = 0; k < K1; k++)
      if (P.hess_order(k) > 0 && (!need || need[k]) && !arrived(k)) return HQPKKT_E_INTERN;
    return 0;
  }
  HessGeom geom(int k) const {
    const int nz = P.hess_order(k), nt = (nz + stg::HP_T - 1) / stg::HP_T;
    const bool packed = P.stage_packed(k);
    return HessGeom{P.oQ[k], P.ldQ[k], nt, nz, P.nmk[k], packed ? 1 : 0, packed ? (int)P.hess_tiles(nz) : nt * nt};
  }
  // the upload if it is due and the device; guard: and what the safeguards make at their first call
  int device(bool guard) {
    int e;
    if (!h->uploaded && (e = staged_upload(h))) return e;
    HIPCHK(hipSetDevice(h->opts.device));
    return guard ? prepare_guard() : 0;
  }
  // the four work vectors of n of the entries that need device scratch (BFGS, the safeguards), made by the first of them
  int scratch() { return d.hess.work.p ? 0 : d.hess.work.alloc(4 * n + 1); }
  double *work(int i) const { return d.hess.work.p + (size_t)i * n; }
  // stage k's descriptor of an update launch: beta's mode, no coefficients; run: over the whole block (units)
  stg::HuDesc update_desc(int k, int mode, double beta, bool run) const {
    const HessGeom g = geom(k);
    return stg::HuDesc{g.off, g.ld, g.nt, g.nz, g.col0, g.packed, run ? g.units : 0, mode, 0, beta, {0.0, 0.0, 0.0, 0.0}};
  }
  static int units_max(const std::vector<stg::HuDesc> &hd) {
    int m = 0;
    for (const stg::HuDesc &q : hd) m = std::max(m, q.units);
    return m;
  }
  // the descriptors to the device: through the pinned words, in the handle's stream; buffers and event are made by the
  // first call
  int descriptors(const std::vector<stg::HuDesc> &hd) {
    StagedDev::Hessians::Update &u = d.hess.upd;
    int e;
    if (!u.desc.p) {
      if ((e = u.desc.alloc(hd.size()))) return e;
      HIPCHK(u.hdesc.alloc(hd.size(), hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&u.ev.h, hipEventDisableTiming));
    } else
      HIPCHK(hipEventSynchronize(u.ev));  // (the copy of the last call's descriptors out of the pinned words)
    std::copy(hd.begin(), hd.end(), u.hdesc.p);
    HIPCHK(hipMemcpyAsync(u.desc.p, u.hdesc.p, sizeof(stg::HuDesc) * hd.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(u.ev, h->stream));
    return 0;
  }
  // the update launch over the stages with units (none: no launch); sent: the descriptors are on the device already
  int update(const std::vector<stg::HuDesc> &hd, const stg::HuVecs &V, bool sent = false) {
    const int um = units_max(hd);
    int e;
    if (um > 0 && !sent && (e = descriptors(hd))) return e;
    if (um > 0) KLAUNCH(h, KC_ASSEMBLE, stg::k_hu_update<<<dim3((unsigned)um, (unsigned)K1), 256, 0, h->stream>>>(d.hess.upd.desc.p, d.hess.Q.p, V));
    HIPCHK(hipGetLastError());
    return 0;
  }
  void touched() { h->factored = false; }

  // the safeguards' descriptors and buffers (staged_hess_guard.hip.h), made by the first call of any of them
  int prepare_guard() {
    StagedDev::Hessians::Guard &q = d.hess.guard;
    if (q.desc.p) return 0;
    std::vector<stg::HgDesc> gd(K1);
    q.slots = 0, q.tiles_max = q.nz_max = 0;
    for (int k = 0; k < K1; k++) {
      const HessGeom g = geom(k);
      const bool packed = g.nz > 0 && g.packed;
      gd[k] = stg::HgDesc{g.off, q.slots, g.ld, g.nt, g.nz, g.col0, packed ? 1 : 0, packed ? g.units : 0};
      if (packed) q.slots += (long long)g.nt * g.nt * stg::HP_T;
      q.tiles_max = std::max(q.tiles_max, gd[k].tiles), q.nz_max = std::max(q.nz_max, g.nz);
    }
    int e;
    if ((e = q.scr.alloc((size_t)(2 * q.slots) + 1)) || (e = scratch()) || (e = q.st.alloc((size_t)K1 * stg::HE_STATE)) || (e = q.T.alloc((size_t)K1 * 2 * stg::HE_MAX_STEPS)) ||
        (e = q.rep.alloc((size_t)K1 * stg::HE_REPORT)) || (e = q.floor.alloc(K1)))
      return e;
    HIPCHK(q.hfloor.alloc(K1, hipHostMallocDefault));
    HIPCHK(hipEventCreateWithFlags(&q.ev.h, hipEventDisableTiming));
    return q.desc.upload(gd);
  }
  // ... and their row pass: rowmax and offsum (either may be null) of every stage, device vectors of n
  void rows(double *rowmax, double *offsum) {
    const StagedDev::Hessians &q = d.hess;
    const StagedDev::Hessians::Guard &g = q.guard;
    if (q.hs_nz_max > 0)
      KLAUNCH(h, KC_VECTOR, stg::k_hg_rows<<<dim3((unsigned)std::min((q.hs_nz_max + 3) / 4, 1024), (unsigned)K1), 256, 0, h->stream>>>(g.desc.p, q.Q.p, rowmax, offsum));
    if (g.tiles_max > 0) {
      KLAUNCH(h, KC_VECTOR, stg::k_hg_tiles<<<dim3((unsigned)g.tiles_max, (unsigned)K1), 256, 0, h->stream>>>(g.desc.p, q.Q.p, g.scr.p, g.scr.p + g.slots));
      KLAUNCH(h, KC_VECTOR, stg::k_hg_finish<<<dim3((unsigned)q.hp_nt_max, (unsigned)K1), stg::HP_T, 0, h->stream>>>(g.desc.p, g.scr.p, g.scr.p + g.slots, rowmax, offsum));
    }
  }
  // q_ii lifted by k_hg_diag: Gerschgorin's rule from the off-diagonal sums, or the shifts of a control's report
  void lift_diagonal(const double *offsum, double eps, const double *rep) {
    const StagedDev::Hessians::Guard &g = d.hess.guard;
    if (g.nz_max > 0)
      KLAUNCH(h, KC_ASSEMBLE, stg::k_hg_diag<<<dim3((unsigned)((g.nz_max + 255) / 256), (unsigned)K1), 256, 0, h->stream>>>(g.desc.p, d.hess.Q.p, offsum, eps, rep, rep ? 1 : 0));
  }
};

// y = Q x of the three entries that ask for it: x, y per opts.loc or (as_host, the debug entries) host arrays; complete
// when it returns.  ms: the average device time of `reps` further products, by events on the handle's stream
int hess_symv_call(hqpkkt_t *h, const double *x, double *y, bool as_host, int reps = 0, double *ms = nullptr) {
  if (!HessCall::uploaded(h)) return HQPKKT_E_INTERN;
  HessCall c(h);
  HIPCHK(hipSetDevice(h->opts.device));
  CallerVecs io{h, as_host};
  const double *dx;
  double *dy;
  int e;
  if ((e = io.ready()) || (e = io.in(x, c.n, &dx))) return e;
  io.out(y, c.n, &dy);
  EventOwner t0, t1;
  if (ms) {
    HIPCHK(hipEventCreate(&t0.h));
    HIPCHK(hipEventCreate(&t1.h));
  }
  staged_hess_symv(h, c.d, dx, dy);  // (timed: the one product ahead of the timed ones)
  if (ms) {
    HIPCHK(hipEventRecord(t0, h->stream));
    for (int r = 0; r < reps; r++) staged_hess_symv(h, c.d, dx, dy);
    HIPCHK(hipEventRecord(t1, h->stream));
  }
  if ((e = io.finish())) return e;
  if (!io.host()) HIPCHK(hipStreamSynchronize(h->stream));
  if (ms) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, t0, t1));
    *ms = (double)t / reps;
  }
  return 0;
}

// the words an update or a control has left on the device, read back behind everything in the stream
int hess_read_back(hqpkkt_t *h, double *a, const DBuf<double> &A, double *b = nullptr, const DBuf<double> *B = nullptr) {
  HIPCHK(hipSetDevice(h->opts.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(a, A.p, sizeof(double) * A.count, hipMemcpyDeviceToHost));
  if (b) HIPCHK(hipMemcpy(b, B->p, sizeof(double) * B->count, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int hqpkkt_set_stage_hessian(hqpkkt_t *h, int k, const double *Q, long long ldQ) {
  return guarded([&]() -> int {
    if (!h || !Q) return HQPKKT_E_NULL;
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    const kktdev::StagedPlan &P = c.P;
    StagedDev &d = c.d;
    int e;
    if ((e = c.device(false))) return e;
    if (k < 0 || k > P.K) return HQPKKT_E_RANGE;
    const int nz = P.hess_order(k);
    if (ldQ < nz) return HQPKKT_E_SIZES;
    const hipMemcpyKind kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (nz > 0 && P.stage_packed(k)) {
      // packed lower tiles: k_hp_pack reads a device block where it lies; of a host block the rows come in groups of
      // HESS_COPY_ROWS, every group from its first column on, into the staging block (reused in stream order)
      const double *src = Q;
      long long lds = ldQ;
      if (kind == hipMemcpyHostToDevice) {
        if (d.hess.stage.count < (size_t)P.q_stage_elems && (e = d.hess.stage.alloc((size_t)P.q_stage_elems))) return e;
        lds = P.ldQ[k], src = d.hess.stage.p;
        for (int r = 0; r < nz; r += P.HESS_COPY_ROWS)
          HIPCHK(hipMemcpy2DAsync(d.hess.stage.p + (long long)r * lds + r, sizeof(double) * lds, Q + (long long)r * ldQ + r, sizeof(double) * ldQ,
                                  sizeof(double) * (nz - r), std::min(P.HESS_COPY_ROWS, nz - r), kind, h->stream));
      }
      stg::k_hp_pack<<<dim3((unsigned)P.hess_tiles(nz), 16), 256, 0, h->stream>>>(src, lds, nz, d.hess.Q.p + P.oQ[k]);
    } else if (nz > 0) {  // the caller's nz columns of every row, then the strict lower triangle from the upper one
      double *dst = d.hess.Q.p + P.oQ[k];
      HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * P.ldQ[k], Q, sizeof(double) * ldQ, sizeof(double) * nz, nz, kind, h->stream));
      const unsigned T = (unsigned)((nz + stg::HS_TILE - 1) / stg::HS_TILE);
      stg::k_hs_mirror<<<T * (T + 1) / 2, 256, 0, h->stream>>>(dst, P.ldQ[k], nz, (int)T);
    }
    if ((e = staged_staging_used(h, Q))) return e;
    c.mark_arrived(k);
    c.touched();
    return 0;
  });
}

int hqpkkt_debug_stage_hessian(hqpkkt_t *h, int k, double *out, long long cap, long long *len) {
  return guarded([&]() -> int {
    if (!h || !len) return HQPKKT_E_NULL;
    if (!HessCall::uploaded(h)) return HQPKKT_E_INTERN;
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
      HIPCHK(hipMemcpy(t.data(), h->sd->hess.Q.p + P.oQ[k], sizeof(double) * t.size(), hipMemcpyDeviceToHost));
      std::fill(out, out + elems, 0.0);
      for (int i = 0; i < nz; i++)
        for (int j = 0; j < nz; j++) {
          const int a = std::max(i, j) / T, b = std::min(i, j) / T;
          const size_t tile = ((size_t)a * (a + 1) / 2 + b) * T * T;
          out[(long long)i * P.ldQ[k] + j] = i / T >= j / T ? t[tile + (size_t)(i % T) * T + j % T] : t[tile + (size_t)(j % T) * T + i % T];
        }
      return 0;
    }
    if (elems) HIPCHK(hipMemcpy(out, h->sd->hess.Q.p + P.oQ[k], sizeof(double) * elems, hipMemcpyDeviceToHost));
    return 0;
  });
}

int hqpkkt_debug_hess_symv(hqpkkt_t *h, const double *x, double *y) {
  return guarded([&]() -> int {
    if (!h || !x || !y) return HQPKKT_E_NULL;
    return hess_symv_call(h, x, y, true);
  });
}

int hqpkkt_debug_hess_symv_timed(hqpkkt_t *h, const double *x, double *y, int reps, double *ms) {
  return guarded([&]() -> int {
    if (!h || !x || !y || !ms) return HQPKKT_E_NULL;
    if (reps < 1) return HQPKKT_E_RANGE;
    return hess_symv_call(h, x, y, true, reps, ms);
  });
}

int hqpkkt_hessian_product(hqpkkt_t *h, const double *x, double *y) {
  return guarded([&]() -> int {
    if (!h || !x || !y) return HQPKKT_E_NULL;
    return hess_symv_call(h, x, y, false);
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
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    for (int k = 0; k < c.K1; k++) {
      if (u->beta && !std::isfinite(u->beta[k])) return HQPKKT_E_RANGE;
      for (int j = 0; j < r; j++)
        if (!std::isfinite(u->coef[(size_t)k * r + j])) return HQPKKT_E_RANGE;
    }
    // the launch's descriptors; a stage with beta = 1, every coefficient 0 and no diagonal is left alone (units = 0)
    std::vector<stg::HuDesc> hd(c.K1);
    for (int k = 0; k < c.K1; k++) {
      const double beta = u->beta ? u->beta[k] : 1.0;
      stg::HuDesc &q = hd[k];
      q = c.update_desc(k, beta == 0.0 ? 0 : beta == 1.0 ? 1 : 2, beta, false);
      bool touched = beta != 1.0 || u->diag;
      for (int j = 0; j < r; j++) q.c[j] = u->coef[(size_t)k * r + j], touched = touched || q.c[j] != 0.0;
      if (!touched || q.nz == 0) continue;
      // (the hand-over rule: what is kept of a block must have arrived since the analysis)
      if (beta != 0.0 && !c.arrived(k)) return HQPKKT_E_INTERN;
      q.units = c.geom(k).units;
    }
    CallerVecs io{h};
    int e;
    if ((e = c.device(false)) || (e = io.ready())) return e;
    if (c.units_max(hd) > 0) {
      stg::HuVecs V{};
      V.r = r;
      for (int j = 0; j < r; j++)
        if ((e = io.in(u->U[j], c.n, &V.u[j]))) return e;
      if ((e = io.in(u->diag, c.n, &V.diag)) || (e = c.update(hd, V)) || (e = io.finish())) return e;  // (a host caller's vectors are free again)
    }
    for (int k = 0; k < c.K1; k++)
      if (hd[k].mode == 0) c.mark_arrived(k);  // (beta = 0: the block has been made here)
    c.touched();
    return 0;
  });
}

int hqpkkt_bfgs_update_stage_hessians(hqpkkt_t *h, const hqpkkt_bfgs_update *b) {
  return guarded([&]() -> int {
    if (!h || !b || !b->s || !b->y) return HQPKKT_E_NULL;
    static_assert(stg::HB_REPORT == HQPKKT_BFGS_REPORT, "the kernel writes the report's words");
    if (!std::isfinite(b->gamma) || (b->gamma < 0.0 && !std::isfinite(b->alpha))) return HQPKKT_E_RANGE;
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    // the base descriptors of the update launch: beta = 1, every stage as if touched - k_hb_terms writes the coefficients
    // and takes the stages it leaves alone out (units = 0); every block is kept, so every block must have arrived
    int e;
    if ((e = c.all_arrived(nullptr))) return e;
    std::vector<stg::HuDesc> hd(c.K1);
    for (int k = 0; k < c.K1; k++) hd[k] = c.update_desc(k, 1, 1.0, true);
    const double gamma_eff = bfgs_gamma_eff(b->gamma, b->alpha);
    CallerVecs io{h};
    if ((e = c.device(false)) || (e = io.ready()) || (e = c.scratch())) return e;
    StagedDev::Hessians::Bfgs &q = c.d.hess.bfgs;
    if (!q.rep.p && (e = q.rep.alloc((size_t)c.K1 * stg::HB_REPORT))) return e;
    const double *s, *y;
    double *Qs = c.work(0), *v;
    if ((e = io.in(b->s, c.n, &s)) || (e = io.in(b->y, c.n, &y))) return e;
    io.out(b->v, c.n, &v);
    if (!v) v = c.work(1);
    if ((e = c.descriptors(hd))) return e;
    staged_hess_symv(h, c.d, s, Qs);
    KLAUNCH(h, KC_VECTOR, stg::k_hb_terms<<<(unsigned)c.K1, 256, 0, h->stream>>>(c.d.hess.upd.desc.p, s, y, Qs, v, gamma_eff, q.rep.p));
    stg::HuVecs V{};
    V.r = 2, V.u[0] = v, V.u[1] = Qs;
    if ((e = c.update(hd, V, true))) return e;
    q.done = true;
    c.touched();
    return io.finish();  // (a host caller's vectors are free again, v is complete)
  });
}

int hqpkkt_bfgs_report(hqpkkt_t *h, double *out) {
  return guarded([&]() -> int {
    if (!h || !out) return HQPKKT_E_NULL;
    if (!h->sd || !h->uploaded || !h->sd->hess.bfgs.done) return HQPKKT_E_INTERN;
    return hess_read_back(h, out, h->sd->hess.bfgs.rep);
  });
}

int hqpkkt_hessian_row_stats(hqpkkt_t *h, double *rowmax, double *offsum) {
  return guarded([&]() -> int {
    if (!h || (!rowmax && !offsum)) return HQPKKT_E_NULL;
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    CallerVecs io{h};
    int e;
    if ((e = c.all_arrived(nullptr)) || (e = c.device(true)) || (e = io.ready())) return e;
    double *rm, *os;
    io.out(rowmax, c.n, &rm), io.out(offsum, c.n, &os);
    c.rows(rm, os);
    HIPCHK(hipGetLastError());
    return io.finish();
  });
}

int hqpkkt_restart_stage_hessians(hqpkkt_t *h, double eps, const unsigned char *stages) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (!std::isfinite(eps) || !(eps > 0.0)) return HQPKKT_E_RANGE;
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    int e;
    if ((e = c.all_arrived(stages))) return e;
    // the update launch's descriptors: beta = 0 on the chosen stages, every other stage left alone (units = 0)
    std::vector<stg::HuDesc> hd(c.K1);
    for (int k = 0; k < c.K1; k++) {
      const bool chosen = c.P.hess_order(k) > 0 && (!stages || stages[k]);
      hd[k] = c.update_desc(k, chosen ? 0 : 1, chosen ? 0.0 : 1.0, chosen);
    }
    if ((e = c.device(true))) return e;
    if (c.units_max(hd) > 0) {
      double *rm = c.work(0), *dv = c.work(2);
      c.rows(rm, nullptr);
      KLAUNCH(h, KC_VECTOR, stg::k_hg_clip<<<nblk((long long)c.n), 256, 0, h->stream>>>((long long)c.n, rm, eps, 1.0 / eps, dv));
      stg::HuVecs V{};
      V.r = 0, V.diag = dv;
      if ((e = c.update(hd, V))) return e;
    }
    c.touched();
    return 0;
  });
}

int hqpkkt_gerschgorin_stage_hessians(hqpkkt_t *h, double eps) {
  return guarded([&]() -> int {
    if (!h) return HQPKKT_E_NULL;
    if (!std::isfinite(eps) || !(eps > 0.0)) return HQPKKT_E_RANGE;
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    int e;
    if ((e = c.all_arrived(nullptr)) || (e = c.device(true))) return e;
    if (c.d.hess.guard.nz_max > 0) {
      double *os = c.work(1);
      c.rows(nullptr, os);
      c.lift_diagonal(os, eps, nullptr);
      HIPCHK(hipGetLastError());
    }
    c.touched();
    return 0;
  });
}

int hqpkkt_eigen_control_stage_hessians(hqpkkt_t *h, const hqpkkt_eigen_control *ec) {
  return guarded([&]() -> int {
    if (!h || !ec) return HQPKKT_E_NULL;
    static_assert(stg::HE_MAX_STEPS == HQPKKT_EIG_MAX_STEPS && stg::HE_REPORT == HQPKKT_EIG_REPORT, "the kernels size T and the report");
    if (!std::isfinite(ec->eps) || !(ec->eps > 0.0) || ec->max_steps < 0 || ec->max_steps > HQPKKT_EIG_MAX_STEPS) return HQPKKT_E_RANGE;
    if (!HessCall::ready(h)) return HQPKKT_E_INTERN;
    HessCall c(h);
    const int K1 = c.K1;
    const size_t n = c.n;
    for (int k = 0; k < K1 && ec->floor; k++)
      if (!std::isfinite(ec->floor[k])) return HQPKKT_E_RANGE;
    int e;
    if ((e = c.all_arrived(nullptr))) return e;
    if (ec->floor_from_bfgs && !c.d.hess.bfgs.done) return HQPKKT_E_INTERN;
    if ((e = c.device(true))) return e;
    StagedDev::Hessians::Guard &g = c.d.hess.guard;
    // the floors the caller gave, NaN where theta_k comes from eps: through the pinned words, in the handle's stream
    HIPCHK(hipEventSynchronize(g.ev));  // (the copy of the last call's floors out of the pinned words)
    for (int k = 0; k < K1; k++) g.hfloor.p[k] = ec->floor ? ec->floor[k] : std::numeric_limits<double>::quiet_NaN();
    HIPCHK(hipMemcpyAsync(g.floor.p, g.hfloor.p, sizeof(double) * K1, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipEventRecord(g.ev, h->stream));
    double *os = c.work(1), *w = c.work(3);
    const int steps = std::min(ec->max_steps ? ec->max_steps : 64, g.nz_max);
    // the basis of the recurrence, `steps` vectors of n: grown here, outside every capture, and cleared - a stage that is
    // done keeps v = 0 from there on
    if (g.V.count < (size_t)steps * n + 1 && (e = g.V.alloc((size_t)steps * n + 1))) return e;
    double *V = g.V.p;
    HIPCHK(hipMemsetAsync(V, 0, sizeof(double) * (size_t)steps * n, h->stream));
    c.rows(nullptr, os);
    KLAUNCH(h, KC_VECTOR, stg::k_he_start<<<(unsigned)K1, 256, 0, h->stream>>>(g.desc.p, c.d.hess.Q.p, os, g.floor.p, ec->eps * ec->eps,
                                                                             ec->floor_from_bfgs ? c.d.hess.bfgs.rep.p : nullptr, g.st.p, g.rep.p, g.T.p, V));
    for (int j = 0; j < steps; j++) {  // (nothing is read back: a stage that has ended returns from its workgroup at once)
      staged_hess_symv(h, c.d, V + (size_t)j * n, w);
      KLAUNCH(h, KC_VECTOR, stg::k_he_step<<<(unsigned)K1, stg::HE_STEP_THREADS, 0, h->stream>>>(g.desc.p, g.st.p, g.T.p, V, w, (long long)n, j, j + 1 == steps ? 1 : 0));
    }
    KLAUNCH(h, KC_VECTOR, stg::k_he_ritz<<<(unsigned)K1, 64, 0, h->stream>>>(g.st.p, g.T.p, g.rep.p));
    c.lift_diagonal(nullptr, 0.0, g.rep.p);
    HIPCHK(hipGetLastError());
    g.done = true;
    c.touched();
    return 0;
  });
}

int hqpkkt_eigen_report(hqpkkt_t *h, double *out, double *T) {
  return guarded([&]() -> int {
    if (!h || !out) return HQPKKT_E_NULL;
    if (!h->sd || !h->uploaded || !h->sd->hess.guard.done) return HQPKKT_E_INTERN;
    return hess_read_back(h, out, h->sd->hess.guard.rep, T, &h->sd->hess.guard.T);
  });
}

}  // extern "C"
