// Host side of the STAGED engine: device residency of the stage blocks and the kernel
// sequences of factor (backward recursion over the stages) and step (backward vector sweep,
// initial state, forward sweep).  Included by staged_engine.hip alone, behind hqpkkt_handle.hpp and staged.hip.h; what
// the other units call of it is declared in hqpkkt_handle.hpp.
// Reference counterpart: Hqp_IpLQDOCP::update / factor / step (hqp/Hqp_IpLQDOCP.C:722-976).
#pragma once

// The schedules of a holder's launches of the dense product (stg::gemm_schedule) with what they look up on the device:
// one entry per request whose launch walks a work list or a tile order (GemmSchedule::kept).  get() with `create` makes
// the entry unless it exists - the engine in upload's dry walk of the factor sequence (hqpkkt::listing), so an eager and
// a captured run of a handle take the same schedule and nothing is allocated inside a captured sequence; without it
// get() only finds, as at every launch.  hits: launches that looked the entry up since it was made (hqpkkt_debug_get 38)
struct GemmCache {
  struct Entry {
    stg::GemmRequest rq;
    stg::GemmSchedule s;
    DBuf<stg::SkUnit> units;
    DBuf<int> order;
    int hits = 0;
  };
  std::vector<Entry> entries;
  Entry *find(const stg::GemmRequest &rq) {
    for (Entry &e : entries)
      if (e.rq == rq) return &e;
    return nullptr;
  }
  // the schedule of rq in *out: its entry; `local` where the schedule keeps nothing; a kept one without an entry is made
  // if `create`, and is HQPKKT_E_INTERN otherwise - no reason to take another schedule.  So is a request no form takes
  int get(const stg::GemmCaps &caps, const stg::GemmRequest &rq, bool create, Entry &local, Entry *&out) {
    if ((out = find(rq))) return 0;
    if (stg::gemm_schedule(caps, rq, local.s) != stg::GEMM_SCHED_OK) return HQPKKT_E_INTERN;
    out = &local;
    if (!local.s.kept()) return 0;
    if (!create) return HQPKKT_E_INTERN;
    local.rq = rq;
    if ((!local.s.tab.units.empty() && local.units.upload(local.s.tab.units)) || (!local.s.order.empty() && local.order.upload(local.s.order))) return HQPKKT_E_MEM;
    entries.push_back(std::move(local));
    out = &entries.back();
    return 0;
  }
};

// The device state of one analysis: the plan, the three arenas, the staging buffers of the block-by-block hand-over, and
// one group per form.  Every group is built by its step of staged_upload (upload_* below) unless it says otherwise
struct StagedDev {
  kktdev::StagedPlan plan;
  DBuf<double> F, V, misc;
  PinnedBuf<double> hblk[2];  // pinned staging of one stage block each (hqpkkt_stage_staging, which makes them)
  EventOwner hblk_ev[2];
  std::vector<char> blocks_set;  // dense hand-over block by block: which stages have arrived since the analysis
  // the plan's tables that every sequence reads, and the int arena
  struct Tables {
    DBuf<int> dyn, eq_rows, fix_rows, fix_src, h_tptr, chk_idx, chk_kind;
    DBuf<long long> h_dst, a_dst;
    DBuf<stg::HTerm> h_terms;
  } tab;
  // The wide rows of C (StagedPlan::wr_rows): where k_st_scatter puts C's values, and the rows ...
  // ... and their vector products in step and residual (StagedPlan::rows_vec; staged_rows.hip.h): the table of the blocks
  // E_k, per wide row its block, the narrow copies of C and C' for the CSR walks, C_wide' t (n) and the wide rows' C dx
  // (m; zero in every other row: nothing else writes it)
  struct WideRows {
    DBuf<long long> c_dst;
    DBuf<int> rows;
    DBuf<stg::RowsBlock> blk;
    DBuf<int> blk_of;
    CsrBuf Cn, CTn;
    DBuf<double> xc, cdx;
    int pairs_max = 0;
  } wr;
  // Dense stage Hessians (StagedPlan::hess_dense); the entries' host side is staged_hess_host.hip.h
  struct Hessians {
    // the blocks and their product (upload_hessians; read by the factor, the residual and every entry): the arena of the
    // blocks Q_k, the scatter map of the CSR hand-over, per stage what k_hs_symv needs, y = Q x of the residual (n), which
    // blocks have arrived since the analysis (HessCall::arrived); as packed lower tiles (StagedPlan::hess_packed) per stage
    // what k_hp_symv_tiles needs and the slots of that product; the launches' extents: most chunks of tiles and tile rows
    // of a packed stage, largest order of a stage that keeps its dense block (0: none)
    DBuf<double> Q, y;
    DBuf<long long> q_dst;
    DBuf<stg::HessDesc> desc;
    std::vector<char> set;
    DBuf<stg::HpDesc> hp_desc;
    DBuf<double> scr;
    int hp_chunks_max = 0, hp_nt_max = 0, hs_nz_max = 0;
    // hqpkkt_set_stage_hessian, first host block of a packed stage: its staging block (reused in stream order)
    DBuf<double> stage;
    // HessCall::scratch, first call of BFGS or of a safeguard: four work vectors of n, carved per call (BFGS: Q s, v; the safeguards: row maxima,
    // off-diagonal sums, the restart's diagonal, w of the recurrence) - never y, which the residual reads.  Nothing reads
    // them once the entry has returned
    DBuf<double> work;
    // the update launch (HessCall::update; rank-r update, BFGS, restart), first call: the per-stage descriptors, written to
    // pinned words and copied from there in the handle's stream (ev: that copy is over, the words may be rewritten)
    struct Update {
      PinnedBuf<stg::HuDesc> hdesc;
      DBuf<stg::HuDesc> desc;
      EventOwner ev;
    } upd;
    // the BFGS terms (hqpkkt_bfgs_update_stage_hessians, first call): the report words of k_hb_terms (8 per stage; read by
    // hqpkkt_bfgs_report and by eigenvalue control with floor_from_bfgs), and whether an update has written them since the analysis
    struct Bfgs {
      DBuf<double> rep;
      bool done = false;
    } bfgs;
    // the safeguards (row stats, restart, Gerschgorin, eigenvalue control; HessCall::prepare_guard at the first call of any):
    // per stage what their kernels need, the slots of the packed row pass (`slots` doubles of maxima, then as many of sums
    // - twice what the product's scratch holds, so it is not shared), the recurrence's basis (as many vectors of n as the
    // control with the most steps asked for), its state, T and report per stage (read by hqpkkt_eigen_report), the floors
    // through pinned words (ev: copied), and whether a control has run since the analysis
    struct Guard {
      DBuf<stg::HgDesc> desc;
      DBuf<double> scr, V, st, T, rep, floor;
      PinnedBuf<double> hfloor;
      EventOwner ev;
      long long slots = 0;
      int tiles_max = 0, nz_max = 0;
      bool done = false;
    } guard;
  } hess;
  // The sparse form (StagedPlan::sparse_dyn): the plan's ranges into the CSR arrays of A and A' ...
  // ... its heavy columns (StagedPlan::hv_cols): the ranges without them, the columns per stage, and per column of A its
  // position among its stage's heavy ones or -1
  struct Sparse {
    DBuf<int> arow, tcol;
    DBuf<int> tcol_light, hv_cols, hv_of;
  } sp;
  // Dense dynamics in the residual (staged_dense_products), one GPU: per stage (K+1) what k_st_dyn_both /
  // k_st_dyn_ax_finish need, A_dyn' dy (n), A_dyn dx (ndyn), and the row sums of A_dyn dx per block of 256 columns
  // (k_st_dyn_both): ndyn x part_cols ...
  struct DynResidual {
    DBuf<stg::DynDesc> desc;
    DBuf<double> x1, x2, part;
    int part_cols = 0;
  } dres;
  // ... and over several ranks: the local dynamics blocks and the products' summed results (A_dyn' dy: n, A_dyn dx: ndyn
  // from sum_x2 on)
  struct DynResidualSharded {
    DBuf<stg::DynLoc> loc;
    DBuf<double> sum;
    long long sum_x2 = 0;
  } dres_sh;
  // One system over several ranks (staged_plan.hpp): per stage where the ranks' strips of W / blocks of G_xx lie in the
  // exchange buffers, this rank's tiles of its blocks' products and its blocks to pack
  // The exchanges of a stage in the stream-ordered form (RCCL) go to a stream of their own, so that the gather of the
  // NEXT stage's F blocks travels beside this stage's products: ev_w[i] "the first stream is ready for exchange i",
  // ev_x[i] "exchange i has arrived" (i = 0, 1: the gathered F in buffer i, 2: the blocks of G_xx)
  struct Sharded {
    DBuf<stg::StripTab> wtabs;  // (the strips of the gathered F: offsets inside one of the two buffers)
    DBuf<stg::RectTab> rtabs;
    DBuf<int> gtile;
    DBuf<unsigned> gowned;              // per stage: bitmap of the 128 x 128 tiles of G this rank computes (k_st_add_h_owned)
    std::vector<long long> gowned_off;  // stage k's words start at gowned_off[k]
    DBuf<stg::PackRect> prects;
    std::vector<int> prect_ptr;
    StreamOwner stream;
    EventOwner ev_x1, ev_w[3], ev_x[3];
  } sh;
  // The profile form (StagedPlan::profile_dyn): the panels' k-slab ranges on the device and the partial sums of the
  // solve's columns product (stg::pf_chunks x columns of the widest stage)
  // packed panels (StagedPlan::packed): per panel of every stage its block for the kernels (offset from the stage's F
  // less 16 lo ld, leading dimension; indexed like rng's pairs), and the partial sums of the carried rows (k_pk_carried)
  struct Profile {
    DBuf<int> rng;
    DBuf<double> part;
    DBuf<stg::PackPanel> pk_tab;
    DBuf<double> pk_part;
    const int *ranges(const kktdev::StagedPlan &P, int k) const { return rng.p + 2 * (size_t)P.pf_ptr[k]; }
    const stg::PackPanel *panels(const kktdev::StagedPlan &P, int k) const { return P.pk_stage(k) ? pk_tab.p + P.pf_ptr[k] : nullptr; }
  } pf;
  // The second stream: the control-sized chain of a stage (G_u strip, H's control part, carried rows, K^-1, Y, Rm)
  // runs beside the large product G_xx = fx'W_x instead of behind it (fork / join by events; inside a
  // captured sequence these are parallel branches of the graph).  Made where a stage can take it (upload_second_stream)
  struct SecondStream {
    StreamOwner stream;
    EventOwner fork, join;
  } s2;
  // The launches of the dense product (st_gemm): what the handle offers them (upload_product_caps) and their schedules
  // with the work lists and tile orders on the device, made in upload's dry walk of the factor sequence
  struct Product {
    stg::GemmCaps caps;
    GemmCache gemms;
    DBuf<double> zeros;    // 256 zero doubles: the operand rows k >= K of the LDS-DMA staging (GemmArgs::zeros)
    DBuf<double> ks_ws2;   // the pieces of a thin product cut in k (k_dgemm_tn_ks) launched on the SECOND stream
    DBuf<double> sk_ws;    // the cut forms of the dgemm: parked partial tiles (SkUnit::slot0)
    DBuf<unsigned> sk_cnt;
    // What staged_run_factor and staged_run_step branch on, per stage k < K, chosen at upload (upload_sequences): the
    // plan's answer (StagedPlan::stage_seq) with the dense stages that form V_k in the G_xx launch (SEQ_FUSED:
    // GemmArgs::K2; `fused` says the same per stage) or run the chain on the second stream (SEQ_DENSE_CHAIN2) told apart
    std::vector<kktdev::StageSeq> seq;
    std::vector<char> fused;
    DBuf<double> fv_nrm;  // -Rm (k_st_rm) of the fused stage in work
    // words of the control-row segment (GemmArgs::ctl), and per stage whether its W launch takes the segment
    DBuf<unsigned> ctl;
    std::vector<char> ctrl_rows;
  } prod;
  // The solve's products with V that stand outside its two chains, many stages per launch (k_st_symv_*_batch; not
  // sharded): [0] g_k = V_{k+1} f_k ahead of the backward sweep, [1] the dynamics rows' multipliers behind the forward
  // sweep.  A launch holds the stages whose partial sums fit StagedPlan::symb_elems; stages that do not take the
  // triangle form (st_symv) go through k_st_gemv_rows one by one.
  struct Symv {
    struct Group {
      int first, count, tiles, fins;
      int kfirst, klast;  // the stages k (products with V_{k+1}) of the launch
    };
    DBuf<stg::SymvItem> items[2];
    std::vector<Group> groups[2];
    std::vector<int> rows_stage[2];
  } symv;
  // dynamic LDS of the one-workgroup kernels, as this handle's stages need it (upload_lds_limits)
  struct Lds {
    size_t small = 0, small_big = 0, init = 0, x0 = 0;
  } lds;
};

namespace {

// the unit's environment switches that are read once per process, each at its first use (HQPKKT_NO_LDSDMA,
// HQPKKT_DGEMM_WAVES and HQPKKT_SK_TABLE are read at every upload: stg::gemm_variant_from_env, gemm_sk_table_from_env)
bool env_no_symv() { static const bool v = getenv("HQPKKT_NO_SYMV") != nullptr; return v; }  // the rows form of the solve's products with V
int env_symv_from() { static const int v = getenv("HQPKKT_SYMV_FROM") ? atoi(getenv("HQPKKT_SYMV_FROM")) : 2048; return v; }
double env_block_gj_tol() { static const double v = getenv("HQPKKT_BLOCK_GJ_TOL") ? atof(getenv("HQPKKT_BLOCK_GJ_TOL")) : 1e-6; return v; }
bool env_spd_test_fail() { static const bool v = getenv("HQPKKT_SPD_TEST_FAIL") != nullptr; return v; }  // tests: k_st_small<1024, false> refuses
// launches go to h->stream: back to the first stream on every way out
struct StreamGuard {
  hqpkkt_t *h;
  hipStream_t s;
  ~StreamGuard() { h->stream = s; }
};
// stream `to` goes on when `from` has come as far as it is now (nothing to do on one stream, and in upload's dry walk)
int stream_after(hqpkkt_t *h, hipEvent_t ev, hipStream_t from, hipStream_t to) {
  if (h->listing || from == to) return 0;
  HIPCHK(hipEventRecord(ev, from));
  HIPCHK(hipStreamWaitEvent(to, ev, 0));
  return 0;
}
// stream b works beside a between fork and join; an error in between must not leave it forked
struct StreamFork {
  hqpkkt_t *h;
  hipStream_t a, b;
  hipEvent_t ev_fork, ev_join;
  bool forked = false;
  int fork() {
    if (int e = stream_after(h, ev_fork, a, b)) return e;
    forked = true;
    return 0;
  }
  int join() {
    forked = false;
    return stream_after(h, ev_join, b, a);
  }
  ~StreamFork() {
    if (forked) (void)join();
  }
};

// per-stage pointers into the arenas
struct StagePtr {
  double *F, *V, *Y, *Rm, *Kinv, *Kmat, *N, *BT, *T, *v, *beta, *eta, *rho;
  int *dyn;
  double *Vs;  // sharded: this rank's row strip of V_k (V: the transient full block; F: the local block [F_p | F_u])
};
inline StagePtr stage_ptr(StagedDev &d, int k) {
  const kktdev::StagedPlan &P = d.plan;
  StagePtr s{};
  double *M = d.misc.p;
  s.V = P.sharded ? M + P.oVf[k & 1] : d.V.p + P.oV[k];
  s.Vs = P.sharded ? d.V.p + P.oVs[k] : nullptr;
  s.BT = M + P.oBT[k], s.N = M + P.oN[k];
  const int capx = std::max(P.cap[k], 1);
  s.v = M + P.oVec[k], s.beta = s.v + P.nk[k], s.eta = s.beta + capx, s.rho = s.eta + capx;
  s.dyn = d.tab.dyn.p + P.dyn_off[k];
  if (k < P.K) {
    s.F = d.F.p + (P.sharded ? P.oFl[k] : P.oF[k]);
    s.Y = M + P.oY[k], s.Rm = M + P.oR[k], s.Kinv = M + P.oK[k], s.Kmat = M + P.oKm[k], s.T = M + P.oT[k];
  }
  return s;
}

// W = V+ F of stage k as a launch; seg: with the control-row segment - the control rows of G = W_u'F out of the free rows
// of W's ragged last tile row (GemmArgs::Au: W's control columns, which the last tile column of the same launch writes)
inline stg::GemmArgs staged_w_args(StagedDev &d, int k, bool seg) {
  const kktdev::StagedPlan &P = d.plan;
  StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1];
  const long long ldf = P.ldf[k], ldg = P.ldg[k];
  double *G = d.misc.p + P.oG, *W = d.misc.p + P.oW;
  stg::GemmArgs g{sn.V, P.ldv[k + 1], sp.F, ldf, nullptr, 0, W, ldf, np, nn + mm, np, 1.0, 0.0, 0, 0};
  if (seg) g.Au = W + nn, g.ldau = ldf, g.mu = mm, g.Cu = G + nn * ldg, g.ldcu = ldg, g.ctl = d.prod.ctl.p;
  return g;
}

// V_k = F_x'W_x - Y'Rm of a fused stage k as one launch (lower tiles, mirrored): the rank-q update as a second k segment
inline stg::GemmArgs staged_v_args(StagedDev &d, int k) {
  const kktdev::StagedPlan &P = d.plan;
  StagePtr sp = stage_ptr(d, k);
  const int nn = P.nk[k];
  const long long ldf = P.ldf[k], ldy = P.ldy[k];
  stg::GemmArgs g{sp.F, ldf, d.misc.p + P.oW, ldf, nullptr, 0, sp.V, P.ldv[k], nn, nn, P.nk[k + 1], 1.0, 0.0, 1, 1};
  g.A2 = sp.Y, g.lda2 = ldy, g.B2 = d.prod.fv_nrm.p, g.ldb2 = ldy, g.K2 = P.qmax[k];
  return g;
}

// C = alpha A'B + beta Cin on the handle's stream by the schedule of its request (gemm_schedule.hpp): made in upload's dry
// walk, where nothing is launched, and only found at a launch.  allow_sk false: launches of the second stream.
// ntiles > 0: the tiles g.tile_map[0 .. ntiles) of the product only (128 x 128 tiles; the blocks of G_xx one rank owns).
// by 1 / 2: the profile form (GEMM_FORM_PROFILE) - every tile over the k-slabs of its panel of the ranged operand alone,
// `panel`: the stage's ranges (host) of B's column panels (W = V+ F) / of A's (G = F'W), `pack`: that operand's packed
// panels or null
int st_gemm(hqpkkt_t *h, stg::GemmArgs g, int cls = KC_ST_GEMM, bool allow_sk = true, int ntiles = 0, int by = 0, const int *panel = nullptr,
            const stg::PackPanel *pack = nullptr) {
  if (g.M <= 0 || g.N <= 0) return 0;
  if (g.apack || g.bpack) return HQPKKT_E_INTERN;  // (packed panels: the profile form's launches alone)
  StagedDev &d = *h->sd;
  const stg::GemmRequest rq = stg::gemm_request(g, !allow_sk, ntiles, by, panel);
  GemmCache::Entry local, *e;
  if (int err = d.prod.gemms.get(d.prod.caps, rq, h->listing, local, e)) return err;
  // (the control-row segment: only where the upload found the launch a list, StagedDev::Product::ctrl_rows)
  if (g.Au && !e->s.seg) return HQPKKT_E_INTERN;
  if (h->listing) return 0;
  e->hits++;
  (by == 2 ? g.apack : g.bpack) = pack;
  const stg::GemmBufs bufs{e->units.p, e->order.p, d.prod.sk_ws.p, d.prod.sk_cnt.p, allow_sk ? d.prod.sk_ws.p : d.prod.ks_ws2.p, d.prod.zeros.p};
  stg::gemm_run(e->s, d.prod.caps, bufs, h->stream, g, [&](auto &&launch) { KLAUNCH(h, cls, launch()); });
  return 0;
}
// ... of stage k in the profile form
int st_gemm_profile(hqpkkt_t *h, const stg::GemmArgs &g, int k, int by, int cls = KC_ST_GEMM) {
  const kktdev::StagedPlan &P = h->sd->plan;
  if (g.M <= 0 || g.N <= 0) return 0;
  if (P.panels(k) != ((by == 2 ? g.M : g.N) + 127) / 128) return HQPKKT_E_INTERN;
  return st_gemm(h, g, cls, true, 0, by, P.stage_ranges(k), h->sd->pf.panels(P, k));
}

int st_gemv_rows(hqpkkt_t *h, stg::GemvRows g) {
  stg::gemv_launch_rows(g, h->stream, [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
  return 0;
}
// y = scale (add + V x + A2 x2) with the symmetric V of a stage: from 2048 states on only the tiles on and below the
// diagonal are read (k_st_symv_tiles + k_st_symv_finish; HQPKKT_NO_SYMV: the rows form throughout)
bool symv_tiles_form(const stg::GemvRows &g) {
  return !(env_no_symv() || g.M != g.N || g.N < env_symv_from() || (g.lda & 1) || (((size_t)g.A) & 15));
}
int st_symv(hqpkkt_t *h, StagedDev &d, stg::GemvRows g) {
  if (!symv_tiles_form(g)) return st_gemv_rows(h, g);
  stg::symv_launch(g, d.misc.p + d.plan.oSym, h->stream, [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
  return 0;
}
// y = add + alpha A'x over a K x N row-major block
// (add2, y2: a second result y2 = y + add2)
int st_gemv_cols(hqpkkt_t *h, StagedDev &d, const double *A, long long lda, int K, int N, const double *x,
                 const double *add, double alpha, double *y, const double *add2 = nullptr, double *y2 = nullptr) {
  if (N <= 0) return 0;
  const kktdev::StagedPlan &P = d.plan;
  const stg::GemvCols g{A, lda, K, N, x, add, alpha, y, d.misc.p + P.oPart, 0, add2, y2};
  stg::gemv_launch_cols(g, P.part_chunks, h->stream, [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
  return 0;
}

// the two tables of StagedDev::Symv::items (at upload time: the arenas' addresses are final)
int staged_build_symv_tables(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  for (int dir = 0; dir < 2; dir++) d.symv.items[dir].release(), d.symv.groups[dir].clear(), d.symv.rows_stage[dir].clear();
  if (P.sharded) return 0;
  double *M = d.misc.p, *S = M + P.oS, *gv = M + P.oGv;
  auto up16 = [](long long x) { return (x + 15) / 16 * 16; };
  for (int dir = 0; dir < 2; dir++) {
    std::vector<stg::SymvItem> items;
    StagedDev::Symv::Group g{0, 0, 0, 0, 0, 0};
    long long used = 0;
    for (int k = 0; k < P.K; k++) {
      const StagePtr sn = stage_ptr(d, k + 1);
      const int np = P.nk[k + 1];
      if (np <= 0) continue;
      const stg::GemvRows gr{sn.V, P.ldv[k + 1], np, np, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1.0};
      if (!symv_tiles_form(gr)) {
        d.symv.rows_stage[dir].push_back(k);
        continue;
      }
      const long long need = up16(kktdev::StagedPlan::symv_need(np));
      if (g.count > 0 && used + need > P.symb_elems) {
        d.symv.groups[dir].push_back(g);
        g = StagedDev::Symv::Group{(int)items.size(), 0, 0, 0, k, k}, used = 0;
      }
      if (g.count == 0) g.kfirst = k;
      g.klast = k;
      double *rowpart, *colpart;
      stg::symv_parts(M + P.oSymB + used, np, rowpart, colpart);
      stg::SymvItem it{};
      it.a = stg::SymvArgs{sn.V, P.ldv[k + 1], np, dir == 0 ? nullptr : S + P.nmk[k + 1], rowpart, colpart};
      if (dir == 0)
        it.f = stg::SymvFinish{np, rowpart, colpart, nullptr, nullptr, 0, nullptr, nullptr, gv + P.nks[k], 1.0};
      else
        it.f = stg::SymvFinish{np, rowpart, colpart, sn.v, P.cap[k + 1] > 0 ? sn.BT : nullptr, P.ldb[k + 1], sn.dyn + 1, sn.eta, nullptr, 1.0};
      it.tile0 = g.tiles, it.fin0 = g.fins;
      it.xrel = dir == 0, it.yrel = dir == 1, it.xoff = it.yoff = P.nks[k];
      items.push_back(it);
      g.tiles += (int)stg::symv_tiles(np), g.fins += (np + 63) / 64, g.count++, used += need;
    }
    if (g.count > 0) d.symv.groups[dir].push_back(g);
    if (!items.empty())
      if (int e = d.symv.items[dir].upload(items)) return e;
  }
  return 0;
}
// one launch pair of StagedDev::Symv::groups[dir] on h->stream.  dir 0: g_k = V_{k+1} f_k (f: the dynamics rows of r2) into
// the plan's oGv; dir 1: the dynamics rows of dy = V+ x+ + v+ + B+' eta+
int staged_symv_group(hqpkkt_t *h, StagedDev &d, int dir, int gi, const double *r2, double *dy) {
  const StagedDev::Symv::Group &g = d.symv.groups[dir][gi];
  stg::symv_launch_batch(d.symv.items[dir].p + g.first, g.count, g.tiles, g.fins, 0, 0, r2, dy, h->stream, [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
  return 0;
}
// ... and the stages outside the groups (no triangle form: few states), one launch each
int staged_symv_rows(hqpkkt_t *h, StagedDev &d, int dir, const double *r2, double *dy) {
  const kktdev::StagedPlan &P = d.plan;
  double *M = d.misc.p, *S = M + P.oS, *gv = M + P.oGv;
  for (int k : d.symv.rows_stage[dir]) {
    const StagePtr sn = stage_ptr(d, k + 1);
    const int np = P.nk[k + 1];
    int e;
    if (dir == 0)
      e = st_gemv_rows(h, stg::GemvRows{sn.V, P.ldv[k + 1], np, np, r2 + P.nks[k], nullptr, nullptr, 0, nullptr, nullptr, gv + P.nks[k], 1.0});
    else
      e = st_gemv_rows(h, stg::GemvRows{sn.V, P.ldv[k + 1], np, np, S + P.nmk[k + 1], sn.v, P.cap[k + 1] > 0 ? sn.BT : nullptr, P.ldb[k + 1],
                                        sn.dyn + 1, sn.eta, dy + P.nks[k], 1.0});
    if (e) return e;
  }
  return 0;
}

}  // namespace

// The control-sized elimination of a stage whose matrices live in global memory: phase (A) and the scaled K by the
// one-workgroup kernel, the inverse by the blocked sweep on the whole chip (k_blk_*, staged.hip.h), its check against
// K, and the one-workgroup inverse behind it in case the blocked one gave up (decided on the device: flags[0]).
// the sweep over the pivot blocks of 64 down the diagonal of the scaled matrix in `scratch` (layout: stg::big_scratch)
static int st_blk_sweep(hqpkkt_t *h, double *scratch, int q, bool allow_sk) {
  const stg::BigScratch bs = stg::big_scratch(scratch, q);
  const int nb = (q + 63) / 64;
  int e;
  for (int j = 0; j < nb; j++) {
    const stg::BlkArgs ba{scratch, q, j};
    KLAUNCH(h, KC_ST_SMALL, stg::k_blk_pivot<<<1, 256, 0, h->stream>>>(ba));
    if ((e = st_gemm(h, stg::GemmArgs{bs.Pb, 64, bs.T0, bs.ldk, nullptr, 0, bs.R, bs.ldk, 64, q, 64, 1.0, 0.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk)) ||
        (e = st_gemm(h, stg::GemmArgs{bs.T0, bs.ldk, bs.R, bs.ldk, bs.Ks, bs.ldk, bs.Ks, bs.ldk, q, q, 64, -1.0, 1.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk)))
      return e;
    KLAUNCH(h, KC_ST_SMALL, stg::k_blk_fixup<<<nblk(64LL * q), 256, 0, h->stream>>>(ba));
  }
  return 0;
}
static int st_small_big(hqpkkt_t *h, StagedDev &d, stg::SmallArgs sa, bool allow_sk) {
  int e;
  sa.mode = 1;
  KLAUNCH(h, KC_ST_SMALL, stg::k_st_small<1024><<<1, 1024, d.lds.small_big, h->stream>>>(sa));
  const stg::BigScratch bs = stg::big_scratch(sa.scratch, sa.qmax);
  const int q = sa.qmax;
  if ((e = st_blk_sweep(h, sa.scratch, q, allow_sk))) return e;
  KLAUNCH(h, KC_ST_SMALL, stg::k_blk_final<<<nblk((long long)q * q), 256, 0, h->stream>>>(sa));
  if ((e = st_gemm(h, stg::GemmArgs{sa.Kmat, sa.ldq, sa.Kinv, sa.ldq, nullptr, 0, bs.Ks, bs.ldk, q, q, q, 1.0, 0.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk)))
    return e;
  KLAUNCH(h, KC_ST_SMALL, stg::k_blk_check<<<1, 1024, 0, h->stream>>>(sa, env_block_gj_tol()));
  sa.mode = 2;
  KLAUNCH(h, KC_ST_SMALL, stg::k_st_small<1024><<<1, 1024, d.lds.small_big, h->stream>>>(sa));
  return 0;
}

// ---- the steps of a stage that the single-GPU and the sharded sequence share; all on h->stream

// H's entries first .. first + count of the plan's list added into the work block G
static void st_add_h(hqpkkt_t *h, StagedDev &d, int first, int count, double *G, int add = 1) {
  if (count)
    KLAUNCH(h, KC_ASSEMBLE, stg::k_st_add_h<<<nblk(count), 256, 0, h->stream>>>(count, d.tab.h_dst.p + first, d.tab.h_tptr.p + first, d.tab.h_terms.p,
                                                                               h->td.vals.p, h->td.wt.p, G, add));
}
// Q's share with dense stage Hessians (StagedPlan::hess_dense; the lists hold C'(Z/W)C alone and go behind it): the rows
// [r0, r1) and the columns [0, c1) of Q_k added into the block G (k_hs_add; lower: the 128 x 128 tiles on and below the diagonal)
static void st_add_q(hqpkkt_t *h, StagedDev &d, int k, int r0, int r1, int c1, int lower, double *G, long long ldg) {
  const kktdev::StagedPlan &P = d.plan;
  if (!P.hess_dense || r1 <= r0 || c1 <= 0) return;
  if (P.stage_packed(k)) {  // the stored tiles of the tile rows the request or its image reaches (k_hp_add)
    const int T = stg::HP_T, a0 = r0 / T, a1 = lower ? (r1 - 1) / T : std::max(r1 - 1, c1 - 1) / T;
    const unsigned tiles = (unsigned)((a1 + 1) * (a1 + 2) / 2 - a0 * (a0 + 1) / 2);
    KLAUNCH(h, KC_ASSEMBLE, stg::k_hp_add<<<dim3(tiles, 16), 256, 0, h->stream>>>(stg::HpAdd{d.hess.Q.p + P.oQ[k], G, ldg, r0, r1, c1, lower, a0}));
    return;
  }
  const dim3 grid((unsigned)nblk((c1 + 1) / 2), (unsigned)std::min(r1 - r0, 1024));
  KLAUNCH(h, KC_ASSEMBLE, stg::k_hs_add<<<grid, 256, 0, h->stream>>>(
                              stg::HsAdd{d.hess.Q.p + P.oQ[k], P.ldQ[k], G, ldg, r0, r1, c1, lower}));
}
// ... and the share of the stage's wide rows of C (StagedPlan::wr_rows, r of them): G += S'S over the lower tiles with
// S = diag(sqrt(z / w)) E_k (k_st_rows_scale), a product of depth r in place; stage K: into V_K with its mirror image.
// Both operands are S, so entry (i, j) and its image are the same sum of the same products
static int st_add_h_wide(hqpkkt_t *h, StagedDev &d, int k, double *G, long long ldg) {
  const kktdev::StagedPlan &P = d.plan;
  const int r = P.wide_count(k), nz = P.hess_order(k);
  if (r <= 0 || nz <= 0) return 0;
  const long long ld = P.ldE[k];
  double *S = d.misc.p + P.oSr;
  KLAUNCH(h, KC_ASSEMBLE, stg::k_st_rows_scale<<<nblk(r * (ld / 2)), 256, 0, h->stream>>>(
                              stg::RowsScale{d.F.p + P.oE[k], S, d.wr.rows.p + P.wr_ptr[k], h->td.wt.p, r, ld}));
  return st_gemm(h, stg::GemmArgs{S, ld, S, ld, G, ldg, G, ldg, nz, nz, r, 1.0, 1.0, 1, k == P.K ? 1 : 0}, KC_ST_GEMM_UPD);
}
// What every sequence that forms the whole work block G of stage k adds behind the product: Q_k's share, the H lists,
// the wide rows' product (lower: as st_add_q takes it)
static int st_add_block(hqpkkt_t *h, StagedDev &d, int k, int lower, double *G, long long ldg) {
  const kktdev::StagedPlan &P = d.plan;
  const int nz = P.hess_order(k);
  st_add_q(h, d, k, 0, nz, nz, lower, G, ldg);
  st_add_h(h, d, P.h_ptr[k], P.h_ptr[k + 1] - P.h_ptr[k], G);
  return st_add_h_wide(h, d, k, G, ldg);
}
// The vector products of the wide rows of C over all stages, one launch each (staged_rows.hip.h):
// d.wr.xc = C_wide' t (the whole n-vector; t by rows of C) ...
static void st_rows_cols(hqpkkt_t *h, StagedDev &d, const double *t) {
  stg::rows_launch_t(stg::RowsGemvT{d.wr.blk.p, d.F.p, d.wr.rows.p, t, d.wr.xc.p}, d.plan.K + 1, d.wr.pairs_max, h->stream,
                     [&](auto &&launch) { KLAUNCH(h, KC_ST_ROWS_VEC, launch()); });
}
// ... and C_wide x with the epilogue of g (x and the epilogue's vectors: the caller's; the table, E, the rows: filled in here)
static void st_rows_rows(hqpkkt_t *h, StagedDev &d, stg::RowsGemv g) {
  g.blk = d.wr.blk.p, g.blk_of = d.wr.blk_of.p, g.R = (int)d.plan.wr_rows.size(), g.E = d.F.p, g.rows = d.wr.rows.p;
  stg::rows_launch(g, h->stream, [&](auto &&launch) { KLAUNCH(h, KC_ST_ROWS_VEC, launch()); });
}
// the carried rows of stage k: N_k[e..] = B+ F (nothing where stage k + 1 carries none)
static int st_carried_rows(hqpkkt_t *h, StagedDev &d, int k, const StagePtr &sp, const StagePtr &sn, bool allow_sk) {
  const kktdev::StagedPlan &P = d.plan;
  const int ek = P.eq_ptr[k + 1] - P.eq_ptr[k];
  return st_gemm(h, stg::GemmArgs{sn.BT, P.ldb[k + 1], sp.F, P.ldf[k], nullptr, 0, sp.N + (size_t)ek * P.ldn[k], P.ldn[k], P.cap[k + 1], P.hess_order(k),
                                  P.nk[k + 1], 1.0, 0.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk);
}
// the control-sized elimination of stage k on the work block G: rank decision and K^-1 (k_st_small, or the blocked sweep
// for matrices that live in global memory), Y and the carried rows, Rm = K^-1 Y (allow_sk: as in st_gemm)
// (nRm: -Rm as well, K of order 1 .. 64)
static int st_eliminate(hqpkkt_t *h, StagedDev &d, int k, const StagePtr &sp, const StagePtr &sn, double *G, bool allow_sk, double *nRm = nullptr) {
  const kktdev::StagedPlan &P = d.plan;
  const int nn = P.nk[k], mm = P.mk[k], ek = P.eq_ptr[k + 1] - P.eq_ptr[k];
  stg::SmallArgs sa{G, P.ldg[k], nn, mm, sp.N, P.ldn[k], ek, P.cap[k + 1] > 0 ? sn.dyn + 1 : nullptr,
                    P.capn[k], P.cap[k], P.qmax[k], h->ge_tol, sp.Kinv, P.ldq[k], sp.Kmat, sp.T, P.ldt[k], sp.dyn, h->td.flags.p,
                    P.big[k] ? d.misc.p + P.oScr : nullptr};
  if (P.big[k]) {
    if (int e2 = st_small_big(h, d, sa, allow_sk)) return e2;
  } else if (P.qmax[k] > 64) {
    if (env_spd_test_fail()) sa.mode = 100;
    KLAUNCH(h, KC_ST_SMALL, (stg::k_st_small<1024, false><<<1, 1024, d.lds.small, h->stream>>>(sa)));
  } else
    KLAUNCH(h, KC_ST_SMALL, stg::k_st_small<256><<<1, 256, d.lds.small, h->stream>>>(sa));
  // Rm = K^-1 Y, refined against K: one launch for K of order <= 64 (k_st_rm), three products above
  // (wa: the arguments of k_st_wide - Y and the carried rows B_k; with K of order 1 .. 64 they are formed inside k_st_rm)
  const int q = P.qmax[k];
  const long long ldy = P.ldy[k];
  stg::WideArgs wa{G, P.ldg[k], nn, mm, sp.N, P.ldn[k], P.capn[k], P.cap[k], q, sp.T, P.ldt[k], sp.dyn, sp.Y, ldy, sp.BT, P.ldb[k]};
  if (q > 0 && q <= 64) {
    stg::RmArgs ra{sp.Kinv, sp.Kmat, P.ldq[k], sp.Y, sp.Rm, ldy, q, nn, 1, wa, nRm};
    KLAUNCH(h, KC_ST_GEMM_UPD, stg::k_st_rm<<<(nn + stg::RM_COLS - 1) / stg::RM_COLS, 256, stg::st_rm_lds(q), h->stream>>>(ra));
    return 0;
  }
  KLAUNCH(h, KC_ST_SMALL, stg::k_st_wide<<<nblk(nn), 256, 0, h->stream>>>(wa));
  if (q <= 0) return 0;
  // one round of refinement against K: Rm += K^-1 (Y - K Rm).  The product with an explicit inverse alone
  // leaves a residual of cond(K) eps |Y| where the reference's solve by Bunch-Kaufman factors
  // (hqp/Hqp_IpLQDOCP.C:1866-1869, 1911-1924) leaves eps |K| |Rm|; stiff stages need the latter
  double *Res = d.misc.p + P.oRes;
  int e;
  if ((e = st_gemm(h, stg::GemmArgs{sp.Kinv, P.ldq[k], sp.Y, ldy, nullptr, 0, sp.Rm, ldy, q, nn, q, 1.0, 0.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk)) ||
      (e = st_gemm(h, stg::GemmArgs{sp.Kmat, P.ldq[k], sp.Rm, ldy, sp.Y, ldy, Res, ldy, q, nn, q, -1.0, 1.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk)) ||
      (e = st_gemm(h, stg::GemmArgs{sp.Kinv, P.ldq[k], Res, ldy, sp.Rm, ldy, sp.Rm, ldy, q, nn, q, 1.0, 1.0, 0, 0}, KC_ST_GEMM_UPD, allow_sk)))
    return e;
  return 0;
}
// the rank-q update V_k = G_xx - Y'Rm (lower tiles, mirrored)
static int st_update_v(hqpkkt_t *h, StagedDev &d, int k, const StagePtr &sp, double *G) {
  const kktdev::StagedPlan &P = d.plan;
  return st_gemm(h, stg::GemmArgs{sp.Y, P.ldy[k], sp.Rm, P.ldy[k], G, P.ldg[k], sp.V, P.ldv[k], P.nk[k], P.nk[k], P.qmax[k], -1.0, 1.0, 1, 1}, KC_ST_GEMM_UPD);
}
// sharded: this rank's rows of V_k for the solve
static void st_keep_rows(hqpkkt_t *h, StagedDev &d, int k) {
  const kktdev::StagedPlan &P = d.plan;
  const StagePtr sp = stage_ptr(d, k);
  const int c0 = P.strip_first(k), wd = P.strip_width(k);
  if (wd > 0)
    KLAUNCH(h, KC_ST_VEC, stg::k_st_copy2d<<<std::min(wd, 2048), 256, 0, h->stream>>>(sp.V + (long long)c0 * P.ldv[k], P.ldv[k], sp.Vs, P.ldv[k], wd, P.nk[k]));
}
// backward sweep of the solve, stage k: the control-sized part (gam: q_k + F' tt)
static void st_bwd_small(hqpkkt_t *h, StagedDev &d, int k, const StagePtr &sp, const StagePtr &sn, const double *r2, const double *gam) {
  const kktdev::StagedPlan &P = d.plan;
  stg::BwdSmall ba{P.nk[k], P.mk[k], P.nk[k + 1], P.eq_ptr[k + 1] - P.eq_ptr[k], P.capn[k], P.cap[k], P.qmax[k], d.tab.eq_rows.p + P.eq_ptr[k], r2,
                   P.cap[k + 1] > 0 ? sn.dyn + 1 : nullptr, sn.beta, sn.BT, P.ldb[k + 1], r2 + P.nks[k], gam, sp.Kinv, sp.Kmat, P.ldq[k], sp.T, P.ldt[k],
                   sp.dyn, sp.rho, sp.beta};
  KLAUNCH(h, KC_ST_SMALL, stg::k_st_bwd_small<<<1, 256, sizeof(double) * (P.capn[k] + 3 * P.qmax[k] + 4 + 256), h->stream>>>(ba));
}
// the initial state x_0 (into S) and the multipliers of its constraints
static int st_initial_state(hqpkkt_t *h, StagedDev &d, const double *r2) {
  const kktdev::StagedPlan &P = d.plan;
  hipStream_t s = h->stream;
  double *M = d.misc.p, *S = M + P.oS;
  const StagePtr s0 = stage_ptr(d, 0);
  const int n0 = P.nk[0];
  if (P.fixed_x0) {
    KLAUNCH(h, KC_ST_VEC, stg::k_st_x0_fixed<<<nblk(std::max(n0, P.cap[0])), 256, 0, s>>>(n0, d.tab.fix_rows.p, d.tab.fix_src.p, h->td.vals.p, r2, S,
                                                                                       s0.eta, P.cap[0]));
    return 0;
  }
  if (P.big0) {
    // with the inverse of the blocked sweep (K0s[3 q]: which form the area holds; decided on the device): three
    // products over the whole chip; k_st_x0_free behind them works only where the factors are in use
    const int q = P.q0max, l8 = (q + 7) / 8 * 8;
    double *vec = M + P.oK0s + 3 * (long long)q + 8, *nb = vec, *pb = vec + l8, *y = vec + 2 * l8, *r = vec + 3 * l8;
    const stg::X0Vec xv{n0, P.cap[0], q, s0.dyn, M + P.oK0s, s0.v, s0.beta, nb, pb, pb, S, s0.eta};
    int e;
    KLAUNCH(h, KC_ST_VEC, stg::k_x0_rhs<<<nblk(q), 256, 0, s>>>(xv));
    if ((e = st_gemv_rows(h, stg::GemvRows{M + P.oK0, P.ldq0, q, q, nb, nullptr, nullptr, 0, nullptr, nullptr, y, 1.0})) ||
        (e = st_gemv_rows(h, stg::GemvRows{M + P.oK0m, P.ldq0, q, q, y, pb, nullptr, 0, nullptr, nullptr, r, -1.0})) ||
        (e = st_gemv_rows(h, stg::GemvRows{M + P.oK0, P.ldq0, q, q, r, y, nullptr, 0, nullptr, nullptr, pb, 1.0})))
      return e;
    KLAUNCH(h, KC_ST_VEC, stg::k_x0_out<<<nblk(n0 + P.cap[0]), 256, 0, s>>>(xv));
  }
  KLAUNCH(h, KC_ST_SMALL, stg::k_st_x0_free<<<1, 256, d.lds.x0, s>>>(n0, P.cap[0], P.q0max, M + P.oK0, M + P.oK0m, M + P.oK0s, P.ldq0, s0.dyn, s0.v,
                                                            s0.beta, S, s0.eta));
  return 0;
}
// forward sweep, stage k: [u ; yhat] = -(Rm x + rho), then the controls and the stage constraints' multipliers
static void st_fwd_small(hqpkkt_t *h, StagedDev &d, int k, const StagePtr &sp, const StagePtr &sn, double *dy) {
  const kktdev::StagedPlan &P = d.plan;
  hipStream_t s = h->stream;
  const int nn = P.nk[k];
  double *xk = d.misc.p + P.oS + P.nmk[k], *uy = d.misc.p + P.oUy;
  if (P.qmax[k] > 0) {
    const stg::GemvRows gr{sp.Rm, P.ldy[k], P.qmax[k], nn, xk, sp.rho, nullptr, 0, nullptr, nullptr, uy, -1.0};
    stg::gemv_launch_wide(gr, s, [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
  }
  stg::FwdSmall fa{nn, P.mk[k], P.eq_ptr[k + 1] - P.eq_ptr[k], P.capn[k], P.cap[k], P.qmax[k], uy, sp.T, P.ldt[k],
                   sp.dyn, sp.eta, d.tab.eq_rows.p + P.eq_ptr[k], xk + nn, dy, sn.eta, P.cap[k + 1]};
  KLAUNCH(h, KC_ST_SMALL, stg::k_st_fwd_small<<<1, 256, sizeof(double) * (P.capn[k] + 4), s>>>(fa));
}

int staged_analyze(hqpkkt_t *h, int n, int me, int m, bool dense_dyn) {
  if (!h->sd) h->sd.reset(new StagedDev);
  kktdev::StagedPlan &P = h->sd->plan;
  kktdev::StagedRequest &rq = h->staged_rq;
  P = kktdev::StagedPlan();
  rq.dense_dyn = dense_dyn;
  if (h->shard_count > 16) return HQPKKT_E_RANGE;
  rq.shard_rank = h->shard_rank, rq.shard_count = h->shard_count;
  rq.sharded = h->shard_count > 1 || h->xchg_fn || h->xchg_sfn;
  if ((rq.want_sparse || rq.want_profile) && dense_dyn) return HQPKKT_E_INTERN;  // the sparse form walks the row lists of the CSR hand-over, the profile form reads its ranges off them
  if ((rq.want_sparse || rq.want_profile) && rq.sharded) return HQPKKT_E_RANGE;   // one system over several ranks stays dense
  if (rq.want_hess_dense && rq.sharded) return HQPKKT_E_RANGE;                   // ... and keeps its term lists
  h->an.shard_rank = h->shard_rank, h->an.shard_count = 1;  // (the tree engine's exchange plan is not used)
  int e = h->an.setup_blocks(1, n, me, m, h->pQp.data(), h->pQi.data(), h->pAp.data(), h->pAi.data(),
                             h->pCp.data(), h->pCi.data());
  if (e) return e;
  e = P.run(rq, n, me, m, h->pQp.data(), h->pQi.data(), h->pAp.data(), h->pAi.data(), h->pCp.data(), h->pCi.data(), h->an.AT.ptr.data(),
            h->an.AT.col.data());
  if (e) return e;
  P.narrow_copies(h->an.C.ptr.data(), h->an.C.col.data(), h->an.C.src.data(), h->an.CT.ptr.data(), h->an.CT.col.data(), h->an.CT.src.data());
  h->an.sbw = -1;
  h->analyzed = true;
  std::memset(&h->st, 0, sizeof(h->st));
  h->st.dim = n + me, h->st.sbw = -1;
  h->st.n_supernodes = P.K + 1, h->st.n_levels = P.K + 1;
  int mf = 0;
  for (int k = 0; k < P.K; k++) mf = std::max(mf, P.hess_order(k) + P.nk[k + 1]);
  h->st.max_front = mf;
  h->st.nnz_kkt = (long long)P.nq + P.na + P.nc;
  h->st.nnz_factor = P.v_elems + P.misc_elems;
  h->st.flops_factor = P.flops_factor;
  h->st.bytes_panels = (long long)sizeof(double) * (P.f_elems + P.v_elems + P.q_elems);
  h->st.bytes_updates = (long long)sizeof(double) * P.misc_elems;
  h->st.shard_rank = P.shard_rank, h->st.shard_count = P.shard_count;
  if (P.sharded) {
    long long bytes = 0, fl = 0;
    const int NR = P.shard_count;
    for (int k = 0; k < P.K; k++) {
      bytes += (long long)sizeof(double) * (P.fgslot[k] + P.xslot[k]) * NR;  // (the gathered F: static, requested a stage ahead)
      const long long wd = P.strip_width(k);
      const long long np = P.nk[k + 1], mm = P.mk[k], nn = P.nk[k], q = P.qmax[k], cx = P.cap[k + 1];
      // own: the strip of W, its columns of the control rows of G and of the carried rows, the tiles of its blocks of
      // G_xx; by every rank: the control columns, the rank-q update of the whole block
      fl += 2 * np * np * wd + 2 * np * 128LL * 128 * (P.gtile_ptr[k + 1] - P.gtile_ptr[k]);
      fl += 2 * np * np * mm + 2 * np * (mm + cx) * (nn + mm) + q * nn * nn;
    }
    h->st.bytes_exchange_factor = bytes, h->st.flops_local = fl, h->st.n_exchange_blocks = 2 * P.K;
    // per solve: a state-sized vector per stage and direction, the partial sums of x+, the dynamics rows' multipliers
    long long sb = 0;
    for (int k = 0; k < P.K; k++) sb += (long long)sizeof(double) * (2LL * P.nk[k + 1] + (long long)NR * P.nk[k + 1]);
    h->st.bytes_exchange_step = sb + (long long)sizeof(double) * P.ndyn;
  }
  return 0;
}

// ---- the steps of staged_upload, in its order: each builds one group of StagedDev from the plan

// what both engines keep in the handle: the CSR blocks, the values, the vectors and their pinned staging
static int upload_handle_vectors(hqpkkt_t *h) {
  Analysis &an = h->an;
  const int n = an.n, me = an.me, m = an.m;
  int e;
  if ((e = h->td.Qf.upload(an.Qfull)) || (e = h->td.A.upload(an.A)) || (e = h->td.AT.upload(an.AT)) ||
      (e = h->td.C.upload(an.C)) || (e = h->td.CT.upload(an.CT)))
    return e;
  const size_t nv = (size_t)an.nq + an.na + an.nc + 1;
  if ((e = h->td.vals.alloc(nv)) || (e = h->td.wt.alloc(m + 1)) || (e = h->td.flags.alloc(128)) ||
      (e = h->td.vin.alloc(2 * (size_t)m + n + me + 2 * (size_t)m)) ||
      (e = h->td.vout.alloc((size_t)n + me + 2 * (size_t)m)) || (e = h->td.vres.alloc((size_t)n + me + 2 * (size_t)m)) ||
      (e = h->td.vcor.alloc((size_t)n + me + 2 * (size_t)m)) || (e = h->td.tz.alloc(m)))
    return e;
  h->td.bits.p = (unsigned long long *)(h->td.flags.p + 120);
  if ((e = alloc_hpin(h))) return e;
  h->td.hstage.release();
  h->td.hstage_in = h->td.hstage_out = 0;
  const size_t nin = 4 * (size_t)m + n + me, nout = (size_t)n + me + 2 * (size_t)m;
  if ((nin + nout) * sizeof(double) <= (size_t)512 * 1024 && nin + nout > 0) {
    HIPCHK(h->td.hstage.alloc(nin + nout, hipHostMallocDefault));
    h->td.hstage_in = nin, h->td.hstage_out = nout;
  }
  const double one = 1.0;
  HIPCHK(hipMemcpy(h->td.vals.p + (nv - 1), &one, sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->td.wt.p + m, &one, sizeof(double), hipMemcpyHostToDevice));
  const double rows = 2.0 * n + me + m;
  const double nnz = (double)an.Qfull.col.size() + 2.0 * an.A.col.size() + 2.0 * an.C.col.size();
  h->short_rows = rows > 0 && nnz / rows < 8.0;
  return 0;
}
// the arenas (slack: 16-byte operand loads of column slices may read a tile's width past a block's last row) and the
// plan's tables; the arenas are cleared by upload_clear_arenas, behind the forms' allocations
static int upload_arenas_tables(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Tables &t = d.tab;
  int e;
  if ((e = d.F.alloc(P.f_elems + 8192)) || (e = d.V.alloc(P.v_elems + 8192)) || (e = d.misc.alloc(P.misc_elems + 8192)) ||
      (e = t.dyn.alloc(P.dyn_ints)) || (e = t.eq_rows.upload(P.eq_rows)) || (e = t.fix_rows.upload(P.fix_rows)) ||
      (e = t.fix_src.upload(P.fix_src)) || (e = t.h_tptr.upload(P.h_tptr)) || (e = t.chk_idx.upload(P.chk_idx)) ||
      (e = t.chk_kind.upload(P.chk_kind)) || (e = t.h_dst.upload(P.h_dst)) || (e = t.a_dst.upload(P.a_dst)))
    return e;
  std::vector<stg::HTerm> ht(P.h_terms.size());
  for (size_t k = 0; k < ht.size(); k++) ht[k] = stg::HTerm{P.h_terms[k].s1, P.h_terms[k].s2, P.h_terms[k].wi};
  return t.h_terms.upload(ht);
}
static int upload_clear_arenas(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  HIPCHK(hipMemset(d.F.p, 0, sizeof(double) * std::max<long long>(P.f_elems, 1)));
  HIPCHK(hipMemset(d.V.p, 0, sizeof(double) * std::max<long long>(P.v_elems, 1)));
  HIPCHK(hipMemset(d.misc.p, 0, sizeof(double) * std::max<long long>(P.misc_elems, 1)));
  HIPCHK(hipMemset(d.tab.dyn.p, 0, sizeof(int) * std::max(P.dyn_ints, 1)));
  return 0;
}
static int upload_wide_rows(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::WideRows &w = d.wr;
  int e;
  if (!P.wr_rows.empty() && ((e = w.c_dst.upload(P.c_dst)) || (e = w.rows.upload(P.wr_rows)))) return e;
  if (!P.rows_vec()) return 0;
  std::vector<stg::RowsBlock> rb(P.K + 1);
  std::vector<int> of(P.wr_rows.size());
  w.pairs_max = 0;
  for (int k = 0; k <= P.K; k++) {
    rb[k] = stg::RowsBlock{P.oE[k], P.ldE[k], P.hess_order(k), P.nmk[k], P.wr_ptr[k], P.wide_count(k)};
    for (int q = P.wr_ptr[k]; q < P.wr_ptr[k + 1]; q++) of[q] = k;
    w.pairs_max = std::max(w.pairs_max, (P.hess_order(k) + 1) / 2);
  }
  Analysis::Csr cn, ctn;
  cn.rows = P.m, cn.ptr = P.cn.ptr, cn.col = P.cn.col, cn.src = P.cn.src;
  ctn.rows = P.n, ctn.ptr = P.ctn.ptr, ctn.col = P.ctn.col, ctn.src = P.ctn.src;
  if ((e = w.blk.upload(rb)) || (e = w.blk_of.upload(of)) || (e = w.Cn.upload(cn)) || (e = w.CTn.upload(ctn)) || (e = w.xc.alloc((size_t)P.n + 1)) ||
      (e = w.cdx.alloc((size_t)P.m + 1)))
    return e;
  HIPCHK(hipMemset(w.cdx.p, 0, sizeof(double) * ((size_t)P.m + 1)));
  return 0;
}
// (the blocks Q_k, cleared once: the scatter and the store write the entries alone)
static int upload_hessians(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Hessians &q = d.hess;
  if (!P.hess_dense) return 0;
  int e;
  std::vector<stg::HessDesc> hd(P.K + 1);
  for (int k = 0; k <= P.K; k++) hd[k] = stg::HessDesc{P.oQ[k], P.ldQ[k], P.stage_packed(k) ? 0 : P.hess_order(k), P.nmk[k], 0};
  q.hp_chunks_max = q.hp_nt_max = q.hs_nz_max = 0;
  for (int k = 0; k <= P.K; k++)
    if (!P.stage_packed(k)) q.hs_nz_max = std::max(q.hs_nz_max, P.hess_order(k));
  if (P.hess_packed) {  // (packed stages: nz = 0 in k_hs_symv's list; the others: no tiles in k_hp_symv_tiles')
    std::vector<stg::HpDesc> pd(P.K + 1);
    for (int k = 0; k <= P.K; k++) {
      const int nt = P.stage_packed(k) ? (P.hess_order(k) + stg::HP_T - 1) / stg::HP_T : 0;
      int nchunks = 0;
      for (int a = 0; a < nt; a++) nchunks += stg::hp_chunks(a);
      pd[k] = stg::HpDesc{P.oQ[k], P.oQs[k], nt, P.hess_order(k), P.nmk[k], nchunks};
      q.hp_nt_max = std::max(q.hp_nt_max, nt), q.hp_chunks_max = std::max(q.hp_chunks_max, nchunks);
    }
    static_assert(stg::HP_T == kktdev::StagedPlan::HESS_T && stg::HP_CHUNK == kktdev::StagedPlan::HESS_CHUNK, "the plan sizes the tiles and the scratch");
    if ((e = q.hp_desc.upload(pd)) || (e = q.scr.alloc((size_t)P.qs_elems + 16))) return e;
  }
  if ((e = q.Q.alloc((size_t)P.q_elems + 16)) || (e = q.desc.upload(hd)) || (e = q.y.alloc((size_t)P.n + 1)) ||
      (!P.q_dst.empty() && (e = q.q_dst.upload(P.q_dst))))
    return e;
  HIPCHK(hipMemset(q.Q.p, 0, sizeof(double) * ((size_t)P.q_elems + 16)));
  return 0;
}
static int upload_sparse(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Sparse &s = d.sp;
  if (!P.sparse_dyn) return 0;
  int e;
  if ((e = s.arow.upload(P.sp_arow)) || (e = s.tcol.upload(P.sp_tcol))) return e;
  if (P.hv_cols.empty()) return 0;
  std::vector<int> of(P.nmk[P.K], -1);
  for (int k = 0; k < P.K; k++)
    for (int q = P.hv_ptr[k]; q < P.hv_ptr[k + 1]; q++) of[P.nmk[k] + P.hv_cols[q]] = q - P.hv_ptr[k];
  if ((e = s.tcol_light.upload(P.sp_tcol_light)) || (e = s.hv_cols.upload(P.hv_cols)) || (e = s.hv_of.upload(of))) return e;
  return 0;
}
// the dense dynamics' tables of the residual products: over several ranks ...
static int upload_dyn_residual_sharded(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  // the local blocks: own state columns [c0, c0 + wd) and the control columns; rank 0 adds what belongs to nobody's strip
  std::vector<stg::DynLoc> dl(P.K + 1);
  for (int k = 0; k <= P.K; k++) {
    stg::DynLoc &x = dl[k];
    x.oF = k < P.K ? P.oFl[k] : 0, x.ldf = k < P.K ? P.ldfl[k] : 0;
    x.np = k < P.K ? P.nk[k + 1] : 0, x.nz = P.hess_order(k);
    x.col0 = P.nmk[k], x.row0 = k < P.K ? P.nks[k] : P.ndyn, x.ncur = P.nk[k];
    x.c0 = P.strip_first(k), x.wd = P.strip_width(k);
    x.m = k < P.K ? P.mk[k] : 0, x.with_controls = P.shard_rank == 0;
  }
  d.dres_sh.sum_x2 = ((long long)P.n + 15) / 16 * 16;
  int e;
  if ((e = d.dres_sh.loc.upload(dl)) || (e = d.dres_sh.sum.alloc((size_t)(d.dres_sh.sum_x2 + P.ndyn + 16)))) return e;
  return 0;
}
// ... and on one GPU
static int upload_dyn_residual(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::DynResidual &r = d.dres;
  std::vector<stg::DynDesc> dd(P.K + 1);
  int nzmax = 1;
  for (int k = 0; k <= P.K; k++) {
    dd[k].oF = k < P.K ? P.oF[k] : 0, dd[k].ldf = k < P.K ? P.ldf[k] : 0;
    dd[k].np = k < P.K ? P.nk[k + 1] : 0, dd[k].nz = P.hess_order(k);
    dd[k].col0 = P.nmk[k], dd[k].row0 = k < P.K ? P.nks[k] : P.ndyn, dd[k].ncur = P.nk[k];
    nzmax = std::max(nzmax, P.hess_order(k));
  }
  int e;
  if ((e = r.desc.upload(dd)) || (e = r.x1.alloc(P.n)) || (e = r.x2.alloc(P.ndyn))) return e;
  r.part_cols = (nzmax + 255) / 256;
  return r.part.alloc((size_t)std::max(P.ndyn, 1) * r.part_cols);
}

// The control-sized chain of a stage on a second stream beside its large product G_xx.  Measured on one MI355X (same
// box, tools/c4_bench.py): stages of 1500 / 2000 / 2500 / 3000 states + 2.7 / 2.5 / 3.5 / 2.7 %, 5000 states - 1.1 % (the
// separate skinny product for the control rows of G and the contention cost more than the hidden chain), 1000 states
// - 13 %.  So: on for stages of 1280 .. 4096 states - the one place that says so.  When sharded the separate product
// exists anyway (staged_stage_sharded).
static bool chain_beside_gxx(int nn) { return nn >= 1280 && nn <= 4096; }
static int upload_second_stream(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  bool any = P.sharded;
  if (!P.sparse_dyn)  // (the sparse form has no large product to run the chain beside)
    for (int k = 0; k < P.K; k++) any = any || chain_beside_gxx(P.nk[k]);
  if (d.s2.stream || !any) return 0;
  // (the control-sized chain ahead of the large products' waiting workgroups: a chain of a few small kernels behind
  // a launch that fills every CU otherwise waits a whole tile time for each of its launches)
  int lo = 0, hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  HIPCHK(hipStreamCreateWithPriority(&d.s2.stream.h, hipStreamNonBlocking, hi));
  HIPCHK(hipEventCreateWithFlags(&d.s2.fork.h, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&d.s2.join.h, hipEventDisableTiming));
  return 0;
}
// What the handle offers the launches of the dense product (stg::GemmCaps) - all of it here
static int upload_product_caps(hqpkkt_t *h) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Product &pr = d.prod;
  int e;
  stg::GemmCaps &c = pr.caps;
  c = stg::GemmCaps{};
  c.variant = stg::gemm_variant_from_env();
  if (c.variant != stg::GEMM_REG4) {  // (the register-staged loop stays selectable for comparisons)
    if ((e = pr.zeros.alloc(256))) return e;
    HIPCHK(hipMemset(pr.zeros.p, 0, sizeof(double) * 256));
  } else
    pr.zeros.release();
  c.unequal = stg::gemm_sk_table_from_env() && !P.sharded;
  c.flags = P.sharded ? stg::GEMM_SHARDED : 0;
  // stream-K grid: two workgroups per CU, if some product of the recursion has more tiles than that
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->opts.device));
  c.cus = cus;
  long long tmax = 0, pmax = 0;  // most tiles / most cut pieces of a product of this handle (column slices have fewer)
  for (int k = 0; k < P.K; k++) {
    const long long t1 = (P.nk[k + 1] + 127) / 128, t2 = (P.hess_order(k) + 127) / 128;
    tmax = std::max(tmax, t1 * t2);
    if (cus > 0)
      for (long long t : {t1 * t2, t2 * (t2 + 1) / 2, t1 * (t1 + 1) / 2})
        for (int grid : {2 * cus, cus})
          pmax = std::max(pmax, stg::gemm_split_plan_pieces(stg::gemm_split_plan(t, (std::max(P.nk[k + 1], P.nk[k]) + stg::GEMM_BK - 1) / stg::GEMM_BK, grid)));
  }
  if (P.sharded)
    for (int k = 0; k < P.K; k++) tmax = std::max<long long>(tmax, P.gtile_ptr[k + 1] - P.gtile_ptr[k]);
  // (a plan has at most two cut phases of at most one unit per workgroup of the grid each: gemm_split_plan; every list
  // is checked against the workspace when it is made, gemm_choose_list.  Until round 5 the workspace was sized 16
  // pieces per tile of the largest product - 3.4 GB at the headline width, per handle, sharded or not)
  pmax = std::max(pmax * 5 / 4 + 64, 4LL * cus + 64);
  c.sk_tiles = (int)tmax;
  if (cus <= 0) return 0;
  c.grid = stg::gemm_wgs_per_cu(c.variant) * cus;
  // (the cut form of the 64 x 64 tiles: at most two phases of one unit per workgroup, up to 3/4 of its grid in tiles)
  c.ws_elems = std::max<long long>(pmax, 1) * 128 * 128;
  c.cnt_elems = c.sk_tiles + 4;
  // (the profile form's lists: a counter per tile of W and of the whole lower block G, at most two parked tiles per
  // workgroup - 2 x grid slots, which the workspace above holds: pmax >= 4 cus + 64)
  for (int k = 0; k < P.K; k++)
    if (P.stage_seq(k) == kktdev::SEQ_PROFILE) {
      const long long t2 = (P.hess_order(k) + 127) / 128;
      c.cnt_elems = std::max(c.cnt_elems, t2 * (t2 + 1) / 2 + 4);
    }
  if ((e = pr.sk_ws.alloc((size_t)c.ws_elems)) || (e = pr.sk_cnt.alloc((size_t)c.cnt_elems))) return e;
  HIPCHK(hipMemset(pr.sk_cnt.p, 0, sizeof(unsigned) * (size_t)c.cnt_elems));
  if (d.s2.stream) {  // (the second stream's products cut in k)
    c.ws2_elems = 8LL << 20;
    if ((e = pr.ks_ws2.alloc((size_t)c.ws2_elems))) return e;
  }
  return 0;
}
// Which sequence every stage runs (StagedDev::Product::seq): the plan's answer, and of its dense stages
// - which form V_k in the G_xx launch (staged_stage_fused).  HQPKKT_FUSED_V=0: none, 1: every stage that can (the
//   tests), unset: those whose W launch also delivers the control rows of G (Product::ctrl_rows: the control-row
//   segment, staged_w_args) and whose width is not one of those that run the chain beside G_xx - with the thin product
//   for the control rows the sequence only takes as long as the one with the separate update
//   (profiles/r08_stage_order.txt).  A stage can when its K has order 1 .. 64 (k_st_rm writes -Rm), its control
//   columns start at an even column and the launch gets 128 x 128 tiles staged by LDS-DMA;
// - which of the others run the control-sized chain on the second stream (staged_stage_dense): the widths that gain by
//   it, with controls that start at an even column (16-byte loads of W + n), and no wide rows of C, whose product adds
//   into the whole lower block of G.
static int upload_sequences(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Product &pr = d.prod;
  int e;
  pr.ctl.release();
  if ((e = pr.ctl.alloc(8))) return e;
  HIPCHK(hipMemset(pr.ctl.p, 0, sizeof(unsigned) * 8));
  pr.ctrl_rows.assign(P.K + 1, 0);
  const char *fv = getenv("HQPKKT_FUSED_V");
  const int mode = fv ? atoi(fv) : 2;
  pr.fused.assign(P.K + 1, 0);
  pr.seq.resize(P.K);
  long long nrm = 0;
  // the schedule of a stage's launch, asked of the launches' own rule (form NONE: refused); equal requests - the stages
  // of a time-invariant system - are answered once.  Nothing is kept: the dry walk makes what the launches look up
  std::vector<std::pair<stg::GemmRequest, stg::GemmSchedule>> asked;
  auto ask = [&](const stg::GemmRequest &rq) -> const stg::GemmSchedule & {
    for (const auto &a : asked)
      if (a.first == rq) return a.second;
    asked.emplace_back(rq, stg::GemmSchedule{});
    if (stg::gemm_schedule(pr.caps, rq, asked.back().second)) asked.back().second = stg::GemmSchedule{};
    return asked.back().second;
  };
  auto can_fuse = [&](int k) -> bool {
    const int nn = P.nk[k], q = P.qmax[k], np = P.nk[k + 1];
    if (mode == 0 || !pr.zeros.p) return false;
    if (P.wide_count(k)) return false;  // (the wide rows' product goes into the work block G)
    if (P.big[k] || q <= 0 || q > 64 || (nn & 1) || np <= 0) return false;
    stg::GemmRequest rt;  // the thin product for the control rows of G behind the W launch
    rt.M = P.mk[k], rt.N = nn + P.mk[k], rt.K = np;
    if (ask(stg::gemm_request(staged_v_args(d, k))).f.kind == stg::GEMM_FORM_NONE) return false;
    // the control rows of G out of the W launch: a cut form with a list in the segment's order, and the guarded
    // product behind it one cut in k (the kernels that know the guard)
    pr.ctrl_rows[k] = ask(rt).f.kind == stg::GEMM_FORM_KS && ask(stg::gemm_request(staged_w_args(d, k, true))).seg;
    if (mode == 1 || (pr.ctrl_rows[k] && !chain_beside_gxx(nn))) return true;
    pr.ctrl_rows[k] = 0;
    return false;
  };
  const bool chain2 = d.s2.stream != nullptr;
  for (int k = 0; k < P.K; k++) {
    pr.seq[k] = P.stage_seq(k);
    if (pr.seq[k] != kktdev::SEQ_DENSE) continue;  // (sharded, sparse, profile: the sequence forms V_k by the separate update)
    if (can_fuse(k)) {
      pr.seq[k] = kktdev::SEQ_FUSED, pr.fused[k] = 1;
      nrm = std::max(nrm, (long long)P.qmax[k] * P.ldy[k]);
    } else if (chain2 && P.mk[k] > 0 && P.nk[k] % 2 == 0 && chain_beside_gxx(P.nk[k]) && !P.wide_count(k))
      pr.seq[k] = kktdev::SEQ_DENSE_CHAIN2;
  }
  pr.fv_nrm.release();
  if (nrm > 0) {  // (slack: the operand loads of the last tile column read a tile's width past a row)
    if ((e = pr.fv_nrm.alloc((size_t)nrm + 8192))) return e;
    HIPCHK(hipMemset(pr.fv_nrm.p, 0, sizeof(double) * ((size_t)nrm + 8192)));
  }
  return 0;
}
static int upload_sharded(hqpkkt_t *h) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Sharded &sh = d.sh;
  if (!P.sharded) return 0;
  int e;
  const int NR = P.shard_count, RK = P.shard_rank;
  std::vector<stg::StripTab> wt(P.K + 1);
  std::vector<stg::RectTab> rt(P.K + 1);
  std::vector<stg::PackRect> pr;
  sh.prect_ptr.assign(P.K + 1, 0);
  for (int k = 0; k < P.K; k++) {
    const int *cut = &P.xcut[(size_t)k * (NR + 1)];
    stg::StripTab &t = wt[k];
    stg::RectTab &r = rt[k];
    t.nranks = r.nranks = NR;
    for (int p = 0; p <= NR; p++) {
      t.cut[p] = r.cut[p] = cut[p];
      if (p < NR) t.off[p] = (long long)p * P.fgslot[k], t.ld[p] = (cut[p + 1] - cut[p] + P.mk[k] + 7) / 8 * 8;
    }
    for (auto &b : r.blk) b.off[0] = b.off[1] = 0, b.rsplit = 1 << 30, b.pad = 0;
    sh.prect_ptr[k] = (int)pr.size();
    for (int q = P.xrect_ptr[k]; q < P.xrect_ptr[k + 1]; q++) {
      const kktdev::StagedPlan::XRect &x = P.xrects[q];
      stg::RectTab::Block &b = r.blk[x.a * 16 + x.b];
      const long long off = (long long)x.owner * P.xslot[k] + x.off;
      if (x.r0 == cut[x.a])
        b.off[0] = off;
      else
        b.off[1] = off, b.rsplit = x.r0;
      if (x.owner == RK) {
        stg::PackRect pk{};
        if (x.mine_rows)
          pk.r0 = x.r0, pk.c0 = x.c0, pk.rows = x.r1 - x.r0, pk.cols = x.c1 - x.c0, pk.transpose = 0;
        else  // computed for the partner's rows in the own row strip of G: rows = own columns
          pk.r0 = x.c0, pk.c0 = x.r0, pk.rows = x.c1 - x.c0, pk.cols = x.r1 - x.r0, pk.transpose = 1;
        pk.off = x.off;
        pr.push_back(pk);
      }
    }
  }
  sh.prect_ptr[P.K] = (int)pr.size();
  if (pr.empty()) pr.push_back(stg::PackRect{});
  std::vector<int> gt = P.gtile;
  if (gt.empty()) gt.push_back(0);
  // which tiles of the work block G of a stage this rank computes (rows: its strip from c0 on)
  std::vector<unsigned> ow;
  sh.gowned_off.assign(P.K + 1, 0);
  for (int k = 0; k < P.K; k++) {
    sh.gowned_off[k] = (long long)ow.size();
    const int ntc = (P.nk[k] + 127) / 128, r0 = P.strip_first(k) / 128;
    ow.resize(ow.size() + ((size_t)ntc * ntc + 31) / 32, 0u);
    for (int t = P.gtile_ptr[k]; t < P.gtile_ptr[k + 1]; t++) {
      const int tr = r0 + (P.gtile[t] >> 16), tc = P.gtile[t] & 0xffff;
      if (tr < ntc && tc < ntc) {
        const size_t bit = (size_t)tr * ntc + tc;
        ow[sh.gowned_off[k] + bit / 32] |= 1u << (bit % 32);
      }
    }
  }
  sh.gowned_off[P.K] = (long long)ow.size();
  if (ow.empty()) ow.push_back(0u);
  if ((e = sh.wtabs.upload(wt)) || (e = sh.rtabs.upload(rt)) || (e = sh.prects.upload(pr)) || (e = sh.gtile.upload(gt)) ||
      (e = sh.gowned.upload(ow)))
    return e;
  if (!sh.ev_x1) HIPCHK(hipEventCreateWithFlags(&sh.ev_x1.h, hipEventDisableTiming));
  if (h->xchg_sfn && !sh.stream) {
    HIPCHK(hipStreamCreateWithFlags(&sh.stream.h, hipStreamNonBlocking));
    for (EventOwner *ev : {&sh.ev_w[0], &sh.ev_w[1], &sh.ev_w[2], &sh.ev_x[0], &sh.ev_x[1], &sh.ev_x[2]})
      HIPCHK(hipEventCreateWithFlags(&ev->h, hipEventDisableTiming));
  }
  return 0;
}
static int upload_profile(StagedDev &d) {
  const kktdev::StagedPlan &P = d.plan;
  StagedDev::Profile &pf = d.pf;
  int e;
  pf.rng.release(), pf.part.release(), pf.pk_tab.release(), pf.pk_part.release();
  if (!P.profile_dyn || P.pf_rng.empty()) return 0;
  long long part = 1;
  for (int k = 0; k < P.K; k++)
    if (P.pf_stage[k]) part = std::max(part, (long long)stg::pf_chunks(P.stage_ranges(k), P.panels(k), P.nk[k + 1]) * P.hess_order(k));
  if ((e = pf.rng.upload(P.pf_rng)) || (e = pf.part.alloc((size_t)part))) return e;
  if (!P.packed) return 0;
  std::vector<stg::PackPanel> tab(P.pk_off.size(), stg::PackPanel{0, 0});
  long long cpart = 1;
  for (int k = 0; k < P.K; k++) {
    if (!P.pk_stage(k)) continue;
    for (int q = P.pf_ptr[k]; q < P.pf_ptr[k + 1]; q++) tab[q] = stg::PackPanel{P.pk_off[q] - 16LL * P.pf_rng[2 * q] * P.pk_ld[q], P.pk_ld[q]};
    cpart = std::max(cpart, (long long)stg::pk_chunks(P.stage_ranges(k), P.panels(k), P.nk[k + 1]) * P.cap[k + 1] * P.hess_order(k));
  }
  if ((e = pf.pk_tab.upload(tab)) || (e = pf.pk_part.alloc((size_t)cpart))) return e;
  return 0;
}
// The work lists of the recursion's cut products and the tile orders of its triangular ones (G, V): a dry walk of the
// factor sequence, in which st_gemm makes what it will look up and nothing is launched (hqpkkt::listing)
static int staged_run_factor(hqpkkt_t *h, const double *z, const double *w);
static int upload_dry_walk(hqpkkt_t *h) {
  StagedDev &d = *h->sd;
  d.prod.gemms.entries.clear();
  struct Listing {
    hqpkkt_t *h;
    ~Listing() { h->listing = false; }
  } walk{h};
  const auto t0 = std::chrono::steady_clock::now();
  h->listing = true;
  if (int e = staged_run_factor(h, nullptr, nullptr)) return e;
  if (getenv("HQPKKT_TIMING"))
    fprintf(stderr, "staged_upload: listing walk over %d stages %.3f ms (%zu schedules with a work list or a tile order)\n", d.plan.K,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), d.prod.gemms.entries.size());
  return 0;
}
// the dynamic LDS this handle's one-workgroup kernels ask for, and the kernels' limits raised to it
static int upload_lds_limits(hqpkkt_t *h) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  d.lds.small = 0, d.lds.small_big = 0;
  for (int k = 0; k < P.K; k++) {
    if (P.big[k])
      d.lds.small_big = std::max(d.lds.small_big, stg::st_small_lds(P.mk[k], P.capn[k], true));
    else
      d.lds.small = std::max(d.lds.small, stg::st_small_lds(P.mk[k], P.capn[k]));
  }
  const size_t q = (size_t)P.q0max;
  d.lds.init = (size_t)kktdev::gj_lds_bytes((long long)q) - (P.big0 ? q * (q | 1) * 8 : 0);
  d.lds.x0 = sizeof(double) * (3 * q + 64 * 65 + 8);
  static std::mutex attr_mutex;  // function attributes are process state, shared by all handles - per DEVICE
  struct PerDev { size_t small = 0, small_big = 0, init = 0, init_big = 0, x0 = 0; bool gemm = false; };
  static PerDev per_dev[64];
  if (h->opts.device < 0 || h->opts.device >= 64) return HQPKKT_E_RANGE;
  std::lock_guard<std::mutex> lk(attr_mutex);
  PerDev &pd = per_dev[h->opts.device];
  if (!pd.gemm) {
    HIPCHK(stg::gemm_set_attributes());
    HIPCHK(hipFuncSetAttribute((const void *)stg::k_st_rm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)stg::st_rm_lds(64)));
    pd.gemm = true;
  }
  // the LDS limit of a kernel goes up when a handle needs more than any before it on the device
  auto raise = [](size_t &have, size_t want, std::initializer_list<const void *> kernels) -> hipError_t {
    if (want <= have) return hipSuccess;
    for (const void *k : kernels)
      if (hipError_t r = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want)) return r;
    have = want;
    return hipSuccess;
  };
  HIPCHK(raise(pd.small, d.lds.small, {(const void *)stg::k_st_small<256>, (const void *)stg::k_st_small<1024, false>}));
  HIPCHK(raise(pd.small_big, d.lds.small_big, {(const void *)stg::k_st_small<1024>}));
  if (!P.big0) HIPCHK(raise(pd.init, d.lds.init, {(const void *)stg::k_st_init_factor<256>}));
  HIPCHK(raise(pd.x0, d.lds.x0, {(const void *)stg::k_st_x0_free}));
  if (P.big0) HIPCHK(raise(pd.init_big, d.lds.init, {(const void *)stg::k_st_init_factor<1024>}));
  return 0;
}

static int staged_upload(hqpkkt_t *h) {
  int e = ensure_device(h);
  if (e) return e;
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  if ((e = upload_handle_vectors(h)) || (e = upload_arenas_tables(d)) || (e = upload_wide_rows(d)) || (e = upload_hessians(d)) || (e = upload_sparse(d))) return e;
  if (P.dense_dyn && (e = P.sharded ? upload_dyn_residual_sharded(d) : upload_dyn_residual(d))) return e;
  if ((e = upload_clear_arenas(d)) || (e = upload_second_stream(d)) || (e = upload_product_caps(h)) || (e = upload_sequences(d)) ||
      (e = upload_sharded(h)) || (e = upload_profile(d)) || (e = upload_dry_walk(h)) || (e = upload_lds_limits(h)) ||
      (e = staged_build_symv_tables(d)))
    return e;
  h->uploaded = true;
  return 0;
}


// the dynamics block of stage k from the caller's F (n+ rows of n_k + m_k values) into the F arena: the whole block,
// or - one system over several ranks - this rank's state columns and the control columns
static int staged_copy_block(hqpkkt_t *h, int k, const double *F, long long ldF, hipMemcpyKind kind) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1];
  if (np <= 0) return 0;
  if (!P.sharded) {
    if (nn + mm > 0)
      HIPCHK(hipMemcpy2DAsync(d.F.p + P.oF[k], sizeof(double) * P.ldf[k], F, sizeof(double) * ldF, sizeof(double) * (nn + mm), np, kind, h->stream));
    return 0;
  }
  const int c0 = P.strip_first(k), wd = P.strip_width(k);
  double *dst = d.F.p + P.oFl[k];
  if (wd > 0) HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * P.ldfl[k], F + c0, sizeof(double) * ldF, sizeof(double) * wd, np, kind, h->stream));
  if (mm > 0) HIPCHK(hipMemcpy2DAsync(dst + wd, sizeof(double) * P.ldfl[k], F + nn, sizeof(double) * ldF, sizeof(double) * mm, np, kind, h->stream));
  return 0;
}

int staged_set_values(hqpkkt_t *h, const double *Qx, const double *Ax, const double *Cx, const double *const *Fblk,
                      const long long *ldF, bool dense) {
  Analysis &an = h->an;
  int e;
  if (!h->uploaded && (e = staged_upload(h))) return e;
  StagedDev &d = *h->sd;
  kktdev::StagedPlan &P = d.plan;
  if (P.dense_dyn != (dense || Fblk != nullptr)) return HQPKKT_E_INTERN;  // analysed for the other hand-over
  HIPCHK(hipSetDevice(h->opts.device));
  hipStream_t s = h->stream;
  hipMemcpyKind kind = h->opts.loc == HQPKKT_LOC_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (Fblk)
    for (int k = 0; k < P.K; k++) {
      if (!Fblk[k] || ldF[k] < P.hess_order(k)) return HQPKKT_E_SIZES;
      if ((e = staged_copy_block(h, k, Fblk[k], ldF[k], kind))) return e;
    }
  if (an.nq) HIPCHK(hipMemcpyAsync(h->td.vals.p, Qx, sizeof(double) * an.nq, kind, s));
  if (an.na) HIPCHK(hipMemcpyAsync(h->td.vals.p + an.nq, Ax, sizeof(double) * an.na, kind, s));
  if (an.nc) HIPCHK(hipMemcpyAsync(h->td.vals.p + an.nq + an.na, Cx, sizeof(double) * an.nc, kind, s));
  return staged_values_changed(h, false);
}

// The values Qx | Ax | Cx are in the handle: the CSR copies, the blocks the values scatter into, the staircase check.
// q_only (the hqpkkt_q_* entries that write Q): A and C are as they were - of the copies Qf alone is gathered again and
// nothing is scattered (Q's entries are read where they lie: st_add_h; with dense stage Hessians those entries refuse).
int staged_values_changed(hqpkkt_t *h, bool q_only) {
  Analysis &an = h->an;
  StagedDev &d = *h->sd;
  kktdev::StagedPlan &P = d.plan;
  hipStream_t s = h->stream;
  for (CsrBuf *c : {&h->td.Qf, &h->td.A, &h->td.AT, &h->td.C, &h->td.CT, &d.wr.Cn, &d.wr.CTn})
    if (c->src.count && (!q_only || c == &h->td.Qf))
      k_gather_values<<<nblk((long long)c->src.count), 256, 0, s>>>((int)c->src.count, c->src.p, h->td.vals.p, c->val.p);
  HIPCHK(hipMemsetAsync(h->td.flags.p, 0, sizeof(int) * 128, s));
  if (an.na && !q_only)
    stg::k_st_scatter<<<nblk(an.na), 256, 0, s>>>(an.na, d.tab.a_dst.p, h->td.vals.p + an.nq, d.F.p, d.misc.p);
  if (P.hess_dense && an.nq && !q_only)  // Q's values into the blocks Q_k (CSR hand-over)
    stg::k_hs_scatter<<<nblk(an.nq), 256, 0, s>>>(an.nq, d.hess.q_dst.p, h->td.vals.p, d.hess.Q.p);
  if (!P.wr_rows.empty() && !q_only)  // the wide rows of C into their blocks E_k
    stg::k_st_scatter<<<nblk(an.nc), 256, 0, s>>>(an.nc, d.wr.c_dst.p, h->td.vals.p + an.nq + an.na, d.F.p, d.misc.p);
  const int nchk = (int)P.chk_idx.size();
  if (nchk) stg::k_st_check<<<nblk(nchk), 256, 0, s>>>(nchk, d.tab.chk_idx.p, d.tab.chk_kind.p, h->td.vals.p, h->td.flags.p);
  int *hs = (int *)h->kept.hpin.p;
  HIPCHK(hipMemcpyAsync(hs, h->td.flags.p, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hs[0]) return HQPKKT_E_FORMAT;  // not the -1.0 staircase (hqp/Hqp_IpLQDOCP.C:214-215) / a zero that fixes x_0
  h->have_values = true;
  h->factored = false;
  return 0;
}

// One stage of the backward recursion when ONE system is sharded over several ranks (DESIGN.md section 7,
// staged_plan.hpp).  Rank p owns the state columns [c0, c1) of the stage: its memory holds those columns of F_k (and the
// control columns), its products are the strip W_p = V+ F_p and the blocks of G_xx the plan gives it - as W_p' F_q, with
// the other rank's F_q out of the GATHERED local blocks, which are static data and were requested a stage ago; W is not
// exchanged.  Everything control-sized is computed by every rank on identical data by launches of identical shape.
//   sA (the handle's): request the gather of stage k - 1's F  ->  W_p = V+ F_p  ->  its blocks of G_xx = W_p' F_q in ONE
//       launch (B from the gathered strips, the tiles of the plan's list), + H_xx  ->  pack (lower orientation)  ->
//       the GATHER OF THE BLOCKS: the one exchange on the critical path
//   sB: W_u = V+ f_u, the control rows of G = W_u' [F_x | F_u] and the carried rows B+ F (thin, deep products over the
//       gathered strips, cut in k), rank decision, K^-1 (k_st_small), Y (k_st_wide), Rm = K^-1 Y - beside the large products
// and, joined: V_k = G_xx - Y' Rm over the WHOLE lower triangle, mirrored, with G_xx read straight from the blocks in
// the exchange buffer (GemmArgs::rects) into the transient full block; the rank keeps its row strip for the solve.
// the gather of the ranks' local blocks of stage k into buffer k & 1: stream-ordered transport: on the exchanges' own
// stream behind `after` (the first stream's position when the buffer's last readers are done); otherwise here and now
static int staged_gather_f(hqpkkt_t *h, int k) {
  StagedDev &d = *h->sd;
  kktdev::StagedPlan &P = d.plan;
  const int NR = P.shard_count, RK = P.shard_rank, i = k & 1;
  const int wd = P.strip_width(k), nloc = wd + P.mk[k], np = P.nk[k + 1];
  double *fg = d.misc.p + P.oFg[i], *mine = fg + (long long)RK * P.fgslot[k];
  hipStream_t sA = h->stream, sX = (h->xchg_sfn && d.sh.stream && !h->listing) ? d.sh.stream : nullptr;
  hipStream_t on = sX ? sX : sA;
  int e;
  if (sX && (e = stream_after(h, d.sh.ev_w[i], sA, sX))) return e;
  if (nloc > 0 && np > 0)
    KLAUNCH(h, KC_ST_VEC, stg::k_st_copy2d<<<std::min(np, 2048), 256, 0, on>>>(stage_ptr(d, k).F, P.ldfl[k], mine, P.ldfl[k], np, nloc));
  if (P.fgslot[k] > 0 && (e = exchange(h, HQPKKT_XCHG_ALLGATHER, fg, P.fgslot[k], NR, sX))) return e;
  if (sX) HIPCHK(hipEventRecord(d.sh.ev_x[i], sX));
  return 0;
}
static int staged_stage_sharded(hqpkkt_t *h, int k) {
  StagedDev &d = *h->sd;
  kktdev::StagedPlan &P = d.plan;
  const int NR = P.shard_count, RK = P.shard_rank;
  StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1];
  const int ek = P.eq_ptr[k + 1] - P.eq_ptr[k], q = P.qmax[k], cx = P.cap[k + 1];
  const int *cut = &P.xcut[(size_t)k * (NR + 1)];
  const int c0 = cut[RK], c1 = cut[RK + 1], wd = c1 - c0;
  const long long ldfl = P.ldfl[k], ldg = P.ldg[k], ldvn = P.ldv[k + 1], ldy = P.ldy[k], ldv = P.ldv[k], ldwl = P.ldwl[k], ldwu = P.ldwu;
  double *G = d.misc.p + P.oG, *Wl = d.misc.p + P.oWl, *Wu = d.misc.p + P.oWu, *xb = d.misc.p + P.oX;
  double *fg = d.misc.p + P.oFg[k & 1];  // the gathered local blocks of THIS stage (requested a stage ago)
  hipStream_t sA = h->stream, sB = d.s2.stream ? d.s2.stream : h->stream;
  // the exchanges' own stream (stream-ordered transport; none in upload's dry walk, which enqueues nothing)
  hipStream_t sX = (h->xchg_sfn && d.sh.stream && !h->listing) ? d.sh.stream : nullptr;
  StreamGuard guard{h, sA};
  StreamFork chain{h, sA, sB, d.s2.fork, d.s2.join};
  const bool two = sB != sA;
  int e;
  const int ne_x = P.h_mid[k] - P.h_ptr[k], ne_u = P.h_ptr[k + 1] - P.h_mid[k];
  // the next stage's F blocks travel while this stage is computed (its buffer's last readers, the stage before this one,
  // are behind us in the first stream)
  if (k > 0 && (e = staged_gather_f(h, k - 1))) return e;
  if ((e = chain.fork())) return e;
  // ---- the control-sized chain, from the gathered F (identical on all ranks: the control columns out of rank 0's slot).
  // Its thin products are launches of hundreds of small workgroups: beside a product that fills every workgroup slot of
  // the chip (the cut form: strips of >= 1024 columns, up to four ranks at the headline width) each of them waits for
  // slots - measured: 1.6 ms for a 20 us kernel, the chain became the critical path - so they go FIRST on the first
  // stream there (0.2 ms), and beside the strip's product only where that one leaves CUs idle (one round of <= 256 tiles).
  const bool thin_first = wd >= 1024;
  h->stream = thin_first ? sA : sB;
  if (sX) HIPCHK(hipStreamWaitEvent(h->stream, d.sh.ev_x[k & 1], 0));
  {
    const stg::StripTab *tab = d.sh.wtabs.p + k;
    const long long ld0 = (cut[1] - cut[0] + mm + 7) / 8 * 8;  // rank 0's local block: [F_0 | F_u]
    const double *Fu = fg + (cut[1] - cut[0]);
    auto thin = [&](const double *A, long long lda, int M, double *C, long long ldc, int cls) -> int {  // C = A' [F_x | F_u]
      int e2;
      stg::GemmArgs gx{A, lda, fg, 0, nullptr, 0, C, ldc, M, nn, np, 1.0, 0.0, 0, 0};
      gx.bstrips = tab;
      if (nn > 0 && (e2 = st_gemm(h, gx, cls, !two || thin_first))) return e2;
      return mm > 0 ? st_gemm(h, stg::GemmArgs{A, lda, Fu, ld0, nullptr, 0, C + nn, ldc, M, mm, np, 1.0, 0.0, 0, 0}, cls, !two || thin_first) : 0;
    };
    if (mm > 0) {
      if ((e = st_gemm(h, stg::GemmArgs{sn.V, ldvn, Fu, ld0, nullptr, 0, Wu, ldwu, np, mm, np, 1.0, 0.0, 0, 0}, KC_ST_GEMM, !two || thin_first))) return e;
      if ((e = thin(Wu, ldwu, mm, G + (long long)nn * ldg, ldg, KC_ST_GEMM))) return e;
    }
    if (cx > 0 && (e = thin(sn.BT, P.ldb[k + 1], cx, sp.N + (size_t)ek * P.ldn[k], P.ldn[k], KC_ST_GEMM_UPD))) return e;
  }
  if (thin_first && (e = stream_after(h, d.sh.ev_x1, sA, sB))) return e;  // the rest of the chain beside the large products
  h->stream = sB;
  st_add_h(h, d, P.h_mid[k], ne_u, G);
  if ((e = st_eliminate(h, d, k, sp, sn, G, !two))) return e;
  // ---- sA: the strip of W, the rank's blocks of G_xx (rows = its strip) in one launch, H_xx, pack, the gather of the blocks
  h->stream = sA;
  if (wd > 0 && (e = st_gemm(h, stg::GemmArgs{sn.V, ldvn, sp.F, ldfl, nullptr, 0, Wl, ldwl, np, wd, np, 1.0, 0.0, 0, 0}))) return e;
  if (sX) HIPCHK(hipStreamWaitEvent(sA, d.sh.ev_x[k & 1], 0));
  const int ntile = P.gtile_ptr[k + 1] - P.gtile_ptr[k];
  if (wd > 0 && ntile > 0) {
    stg::GemmArgs gg{Wl, ldwl, fg, 0, nullptr, 0, G + (long long)c0 * ldg, ldg, wd, nn, np, 1.0, 0.0, 0, 0};
    gg.tile_map = d.sh.gtile.p + P.gtile_ptr[k], gg.bstrips = d.sh.wtabs.p + k;
    if ((e = st_gemm(h, gg, KC_ST_GEMM, true, ntile))) return e;
  }
  if (ne_x)  // H_xx into the rank's own tiles only (everything else in G is left over from earlier stages and read by nobody)
    KLAUNCH(h, KC_ASSEMBLE, stg::k_st_add_h_owned<<<nblk(ne_x), 256, 0, h->stream>>>(ne_x, d.tab.h_dst.p + P.h_ptr[k], d.tab.h_tptr.p + P.h_ptr[k], d.tab.h_terms.p,
                                                                                  h->td.vals.p, h->td.wt.p, G, ldg, d.sh.gowned.p + d.sh.gowned_off[k], (nn + 127) / 128));
  const int npk = d.sh.prect_ptr[k + 1] - d.sh.prect_ptr[k];
  if (npk > 0)
    KLAUNCH(h, KC_ST_VEC, stg::k_st_pack_rects<<<dim3(512, npk), 256, 0, sA>>>(d.sh.prects.p + d.sh.prect_ptr[k], G, ldg, xb + (long long)RK * P.xslot[k]));
  if (P.xslot[k] > 0) {
    if (sX && (e = stream_after(h, d.sh.ev_w[2], sA, sX))) return e;
    if ((e = exchange(h, HQPKKT_XCHG_ALLGATHER, xb, P.xslot[k], NR, sX))) return e;
    if (sX && (e = stream_after(h, d.sh.ev_x[2], sX, sA))) return e;
  }
  if ((e = chain.join())) return e;  // (the chain ended with st_eliminate: nothing has gone to sB since)
  // V_k = G_xx - Y' Rm: lower tiles, mirrored; G_xx from the blocks
  stg::GemmArgs gu{sp.Y, ldy, sp.Rm, ldy, xb, 0, sp.V, ldv, nn, nn, q, -1.0, 1.0, 1, 1};
  gu.rects = d.sh.rtabs.p + k;
  if ((e = st_gemm(h, gu, KC_ST_GEMM_UPD))) return e;  // (q = 0, a stage without controls: V_k = G_xx, the k loop is empty)
  st_keep_rows(h, d, k);
  return 0;
}


// One stage of the backward recursion with V_k formed in the G_xx launch.  The rank-q update V = G_xx - Y'Rm is nothing
// but memory traffic as a launch of its own (G_xx written, read back, V written with its image: 300 MB for 0.25 GFlop);
// as gemm_slabs(q) more k-slabs of the product G_xx = F_x'W_x (GemmArgs::K2: A2 = Y, B2 = -Rm) G_xx never goes to memory.
// That needs Y and Rm BEFORE the large product, and the control-sized chain that makes them needs only the control rows
// of G: G_u = W_u'F, a thin product (k_dgemm_tn_ks) with W's control columns.  All on the first stream: with the chain
// on a second stream beside W (W_u = V+ f_u as a thin product of its own) the stage was slower in every placement that
// was measured - profiles/r08_stage_order.txt.  Where the W launch takes the control-row segment (StagedDev::Product::ctrl_rows) it
// delivers G_u itself, and the thin product behind it is guarded: it runs only if an augmented tile of that launch found
// W's control columns unfinished (GemmArgs::ctl, counted: hqpkkt_debug_get 44), and returns at once otherwise.
static int staged_stage_fused(hqpkkt_t *h, int k) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1], nz = nn + mm;
  const long long ldf = P.ldf[k], ldg = P.ldg[k];
  double *G = d.misc.p + P.oG, *W = d.misc.p + P.oW, *nRm = d.prod.fv_nrm.p;
  const int ne_x = P.h_mid[k] - P.h_ptr[k], ne_u = P.h_ptr[k + 1] - P.h_mid[k];
  int e;
  // W = V+ F; the control rows of G = W_u'F with H's control part; the carried rows N_k[e..] = B+ F
  const bool seg = d.prod.ctrl_rows[k];
  if ((e = st_gemm(h, staged_w_args(d, k, seg)))) return e;
  stg::GemmArgs gu{W + nn, ldf, sp.F, ldf, nullptr, 0, G + nn * ldg, ldg, mm, nz, np, 1.0, 0.0, 0, 0};
  if (seg) gu.guard = d.prod.ctl.p + 2;
  if (mm > 0 && (e = st_gemm(h, gu, KC_ST_GEMM_UPD))) return e;
  if (seg && !h->listing) KLAUNCH(h, KC_ST_SMALL, stg::k_ctrl_rows_end<<<1, 64, 0, h->stream>>>(d.prod.ctl.p));
  st_add_q(h, d, k, nn, nz, nz, 0, G, ldg);
  st_add_h(h, d, P.h_mid[k], ne_u, G);
  if ((e = st_carried_rows(h, d, k, sp, sn, true)) || (e = st_eliminate(h, d, k, sp, sn, G, true, nRm))) return e;
  // V = F_x'W_x - Y'Rm (lower tiles, mirrored), then H_xx into the entry and its image
  if ((e = st_gemm(h, staged_v_args(d, k)))) return e;
  st_add_q(h, d, k, 0, nn, nn, 0, sp.V, P.ldv[k]);  // (the whole of Q_xx, which is its own image bit for bit)
  if (ne_x)
    KLAUNCH(h, KC_ASSEMBLE, stg::k_st_add_h_sym<<<nblk(ne_x), 256, 0, h->stream>>>(ne_x, d.tab.h_dst.p + P.h_ptr[k], d.tab.h_tptr.p + P.h_ptr[k], d.tab.h_terms.p,
                                                                                 h->td.vals.p, h->td.wt.p, sp.V, ldg, P.ldv[k]));
  return 0;
}

// One stage of the backward recursion in the dense form on one GPU: W = V+ F, G = F'W with H, the carried rows, the
// control-sized elimination, the rank-q update V = G_xx - Y'Rm.  ovl (SEQ_DENSE_CHAIN2, upload_sequences): the stage
// runs the control-sized chain on the second stream, beside the large product G_xx.
static int staged_stage_dense(hqpkkt_t *h, int k, bool ovl) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1], nz = nn + mm;
  const long long ldf = P.ldf[k], ldg = P.ldg[k], ldvn = P.ldv[k + 1];
  double *G = d.misc.p + P.oG, *W = d.misc.p + P.oW;
  hipStream_t sA = h->stream, sB = ovl ? d.s2.stream : h->stream;
  StreamGuard guard{h, sA};
  StreamFork chain{h, sA, sB, d.s2.fork, d.s2.join};
  const int ne_x = P.h_mid[k] - P.h_ptr[k], ne_u = P.h_ptr[k + 1] - P.h_mid[k];
  int e;
  // ---- W
  if ((e = st_gemm(h, stg::GemmArgs{sn.V, ldvn, sp.F, ldf, nullptr, 0, W, ldf, np, nz, np, 1.0, 0.0, 0, 0})) || (e = chain.fork())) return e;
  // ---- G: the state part (large) on the first stream ...
  if (!ovl) {
    // G = F'W (lower tiles of the whole (n+m) x (n+m) block)
    if ((e = st_gemm(h, stg::GemmArgs{sp.F, ldf, W, ldf, nullptr, 0, G, ldg, nz, nz, np, 1.0, 0.0, 1, 0}))) return e;
    if ((e = st_add_block(h, d, k, 1, G, ldg))) return e;
  } else {
    if ((e = st_gemm(h, stg::GemmArgs{sp.F, ldf, W, ldf, nullptr, 0, G, ldg, nn, nn, np, 1.0, 0.0, 1, 0}))) return e;
    st_add_q(h, d, k, 0, nn, nn, 1, G, ldg);
    st_add_h(h, d, P.h_ptr[k], ne_x, G);
    // ... the control rows of G (Gux, Guu) = W_u' F and H's control part on the second
    h->stream = sB;
    if ((e = st_gemm(h, stg::GemmArgs{W + nn, ldf, sp.F, ldf, nullptr, 0, G + nn * ldg, ldg, mm, nz, np, 1.0, 0.0, 0, 0}, KC_ST_GEMM, false))) return e;
    st_add_q(h, d, k, nn, nz, nz, 0, G, ldg);
    st_add_h(h, d, P.h_mid[k], ne_u, G);
  }
  h->stream = sB;
  if ((e = st_carried_rows(h, d, k, sp, sn, !ovl)) || (e = st_eliminate(h, d, k, sp, sn, G, !ovl))) return e;
  h->stream = sA;
  if ((e = chain.join())) return e;
  return st_update_v(h, d, k, sp, G);
}

// One stage of the backward recursion in the profile form (StagedPlan::pf_stage): the dense sequence on one stream with
// its two large products by lists in which a tile takes only the k-slabs that hold its panel's stored entries of F_k -
// W = V+ F (tile (tm, tn): the range of panel tn) and the whole lower block G = F'W (the range of panel tm) - and no V
// formed in the G_xx launch.  The thin products (carried rows, the elimination's) stay full-depth dense products: they
// read the arena's zeros.  A stage with packed panels (StagedPlan::pk_stage) runs the same launches by the same lists
// with F_k's panels addressed through StagedDev::Profile::pk_tab, and its carried rows by k_pk_carried over the ranges alone.
static int staged_stage_profile(hqpkkt_t *h, int k) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1], nz = nn + mm;
  const long long ldf = P.ldf[k], ldg = P.ldg[k], ldvn = P.ldv[k + 1];
  double *G = d.misc.p + P.oG, *W = d.misc.p + P.oW;
  int e;
  if ((e = st_gemm_profile(h, stg::GemmArgs{sn.V, ldvn, sp.F, ldf, nullptr, 0, W, ldf, np, nz, np, 1.0, 0.0, 0, 0}, k, 1)) ||
      (e = st_gemm_profile(h, stg::GemmArgs{sp.F, ldf, W, ldf, nullptr, 0, G, ldg, nz, nz, np, 1.0, 0.0, 1, 0}, k, 2)))
    return e;
  if ((e = st_add_block(h, d, k, 1, G, ldg))) return e;
  if (P.pk_stage(k)) {
    const int ek = P.eq_ptr[k + 1] - P.eq_ptr[k];
    stg::pk_launch_carried(stg::PkCarried{sn.BT, P.ldb[k + 1], sp.F, d.pf.panels(P, k), d.pf.ranges(P, k), np, nz, P.cap[k + 1], 0,
                                          sp.N + (size_t)ek * P.ldn[k], P.ldn[k], d.pf.pk_part.p},
                           P.stage_ranges(k), h->stream, [&](auto &&launch) { KLAUNCH(h, KC_ST_GEMM_UPD, launch()); });
  } else if ((e = st_carried_rows(h, d, k, sp, sn, true)))
    return e;
  if ((e = st_eliminate(h, d, k, sp, sn, G, true))) return e;
  return st_update_v(h, d, k, sp, G);
}

// the entries of the columns [c0, c0 + ncols) of F_k out of the CSR arrays of A' (staged_sparse.hip.h)
// (light: the ranges in which the stage's heavy columns are empty, where it has some)
static stg::SpCols sp_cols(hqpkkt_t *h, StagedDev &d, int k, int c0, int ncols, bool light = false) {
  const kktdev::StagedPlan &P = d.plan;
  const int *ent = light && P.heavy_count(k) ? d.sp.tcol_light.p : d.sp.tcol.p;
  return stg::SpCols{ent + 2 * ((long long)P.nmk[k] + c0), h->td.AT.col.p, h->td.AT.val.p, P.nks[k], ncols};
}
// One stage of the backward recursion in the sparse form (StagedPlan::sparse_dyn; Hqp_IpLQDOCP's FormGxxSp,
// hqp/Hqp_IpLQDOCP.C:1119-1220): T = F'V+ in W's place and G = T F with its mirror image by k_sp_gather, the carried
// rows by k_sp_carried; everything behind them is the dense sequence's - H, the control-sized elimination, the rank-q
// update V = G_xx - Y'Rm (still an MFMA product).  One stream: nothing large is left to run the chain beside.
// A stage with heavy columns (hqpkkt_set_dense_columns; D = D_k, nd columns) runs the same walks over the light ranges,
// which leave zeros in the heavy columns' rows and columns of T, G and N, and beside them
//   W_h = V+ D (thin product)  ->  T_h = W_h' (k_sp_heavy_transpose)  ->  G_h = T_h F over the light ranges (k_sp_gather,
//   not lower: the heavy rows of G against every light column)  ->  G_hh = D'W_h  ->  N_h = B+ D
// and k_sp_heavy_place writes row and column h of G from one register and the heavy columns of N, before H is added.
// Every sum has a fixed order: a second factorisation gives the same bits.  A stage without heavy columns runs the
// launches it always has.
static int staged_stage_sparse(hqpkkt_t *h, int k) {
  StagedDev &d = *h->sd;
  const kktdev::StagedPlan &P = d.plan;
  StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
  const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1], nz = nn + mm;
  const int ek = P.eq_ptr[k + 1] - P.eq_ptr[k], cx = P.cap[k + 1];
  const long long ldt = P.ldv[k + 1], ldg = P.ldg[k];
  double *G = d.misc.p + P.oG, *T = d.misc.p + P.oW;
  const stg::SpCols f = sp_cols(h, d, k, 0, nz, true);
  const unsigned cb = (unsigned)((nz + 255) / 256);
  const int nd = np > 0 ? P.heavy_count(k) : 0;
  const long long ldd = P.ldd[k];
  const double *D = d.F.p + P.oD[k];
  double *Wh = d.misc.p + P.oWh, *Th = d.misc.p + P.oTh, *Gh = d.misc.p + P.oGh, *Ghh = d.misc.p + P.oGhh, *Nh = d.misc.p + P.oNh;
  int e;
  if (nd > 0) {
    if ((e = st_gemm(h, stg::GemmArgs{sn.V, ldt, D, ldd, nullptr, 0, Wh, ldd, np, nd, np, 1.0, 0.0, 0, 0}))) return e;
    KLAUNCH(h, KC_ST_SPARSE, stg::k_sp_heavy_transpose<<<nblk(np), 256, 0, h->stream>>>(np, nd, Wh, ldd, Th, ldt));
  }
  if (np > 0 && nz > 0) {
    KLAUNCH(h, KC_ST_SPARSE, stg::k_sp_gather<<<dim3(cb, (np + stg::SP_RB - 1) / stg::SP_RB), 256, 0, h->stream>>>(
                                 stg::SpGather{f, sn.V, P.ldv[k + 1], np, nullptr, 0, T, ldt, 0}));
    KLAUNCH(h, KC_ST_SPARSE, stg::k_sp_gather<<<dim3(cb, (nz + stg::SP_RB - 1) / stg::SP_RB), 256, 0, h->stream>>>(
                                 stg::SpGather{f, T, ldt, nz, G, ldg, G, ldg, 1}));
  }
  if (cx > 0 && nz > 0)  // carried rows: N_k[e..] = B+ F
    KLAUNCH(h, KC_ST_SPARSE, stg::k_sp_carried<<<dim3(cb, (cx + 7) / 8), 256, 0, h->stream>>>(
                                 stg::SpCarried{f, sn.BT, P.ldb[k + 1], cx, sp.N + (size_t)ek * P.ldn[k], P.ldn[k]}));
  if (nd > 0) {
    KLAUNCH(h, KC_ST_SPARSE, stg::k_sp_gather<<<dim3(cb, (nd + stg::SP_RB - 1) / stg::SP_RB), 256, 0, h->stream>>>(
                                 stg::SpGather{f, Th, ldt, nd, Gh, ldg, nullptr, 0, 0}));
    if ((e = st_gemm(h, stg::GemmArgs{D, ldd, Wh, ldd, nullptr, 0, Ghh, ldd, nd, nd, np, 1.0, 0.0, 0, 0}))) return e;
    if (cx > 0 && (e = st_gemm(h, stg::GemmArgs{sn.BT, P.ldb[k + 1], D, ldd, nullptr, 0, Nh, ldd, cx, nd, np, 1.0, 0.0, 0, 0}, KC_ST_GEMM_UPD))) return e;
    KLAUNCH(h, KC_ST_SPARSE, stg::k_sp_heavy_place<<<dim3((unsigned)((std::max(nz, cx) + 255) / 256), nd), 256, 0, h->stream>>>(stg::SpHeavyPlace{
                                 nz, nd, cx, d.sp.hv_cols.p + P.hv_ptr[k], d.sp.hv_of.p + P.nmk[k], Gh, ldg, Ghh, ldd, G, ldg, Nh, sp.N + (size_t)ek * P.ldn[k], P.ldn[k]}));
  }
  // (not lower: k_sp_gather writes the block with its mirror image)
  if ((e = st_add_block(h, d, k, 0, G, ldg)) || (e = st_eliminate(h, d, k, sp, sn, G, true))) return e;
  return st_update_v(h, d, k, sp, G);
}

// Hqp_IpLQDOCP::factor (hqp/Hqp_IpLQDOCP.C:796-862): W^-1 Z, C'(W^-1 Z)C, then the backward
// recursion over the stages (ExRiccatiFactorSc, :1794-1999)
static int staged_run_factor(hqpkkt_t *h, const double *z, const double *w) {
  Analysis &an = h->an;
  StagedDev &d = *h->sd;
  kktdev::StagedPlan &P = d.plan;
  hipStream_t s = h->stream;
  const int m = an.m, K = P.K;
  const bool timed = !h->capturing && !h->listing;  // (listing: upload's dry walk of this sequence, staged_upload)
  int e;
  if (!h->listing) {  // the status words and V_K cleared by one kernel (no memset nodes in the captured sequence: kernels.hip.h, k_clear)
    const long long vk = (long long)P.nk[K] * P.ldv[K];
    kktdev::k_clear<<<(int)std::max<long long>(1, std::min<long long>(4096, (vk / 2 + 1023) / 1024)), 256, 0, s>>>(stage_ptr(d, K).V, vk, h->td.flags.p);
  }
  if (timed) HIPCHK(hipEventRecord(h->ev0, s));
  if (m > 0) KLAUNCH(h, KC_ASSEMBLE, k_weights<<<nblk(m), 256, 0, s>>>(1, m, an.n + an.me, z, w, h->td.wt.p, nullptr, h->td.flags.p));
  if (timed) HIPCHK(hipEventRecord(h->ev1, s));
  {  // last stage: V_K = H_K, all its equality rows are carried
    StagePtr sp = stage_ptr(d, K);
    const int nK = P.nk[K], eK = P.eq_ptr[K + 1] - P.eq_ptr[K];
    st_add_q(h, d, K, 0, nK, nK, 0, sp.V, P.ldv[K]);  // (into the cleared block: V_K = Q_K with its image, then the lists add)
    st_add_h(h, d, P.h_ptr[K], P.h_ptr[K + 1] - P.h_ptr[K], sp.V, P.hess_dense ? 1 : 0);
    if (!P.sharded && (e = st_add_h_wide(h, d, K, sp.V, P.ldv[K]))) return e;
    KLAUNCH(h, KC_ST_SMALL, stg::k_st_last<<<nblk(std::max(nK, 1)), 256, 0, s>>>(nK, eK, P.cap[K], sp.N, P.ldn[K], sp.BT, P.ldb[K], sp.dyn));
    if (P.sharded) st_keep_rows(h, d, K);
  }
  if (P.sharded && K > 0 && (e = staged_gather_f(h, K - 1))) return e;  // (stage k requests stage k - 1's)
  for (int k = K - 1; k >= 0; k--) {
    e = 0;
    switch (d.prod.seq[k]) {
      case kktdev::SEQ_SHARDED: e = staged_stage_sharded(h, k); break;
      case kktdev::SEQ_SPARSE: e = staged_stage_sparse(h, k); break;
      case kktdev::SEQ_PROFILE: e = staged_stage_profile(h, k); break;
      case kktdev::SEQ_FUSED: e = staged_stage_fused(h, k); break;
      case kktdev::SEQ_DENSE: e = staged_stage_dense(h, k, false); break;
      case kktdev::SEQ_DENSE_CHAIN2: e = staged_stage_dense(h, k, true); break;
    }
    if (e) return e;
  }
  {
    StagePtr s0 = stage_ptr(d, 0);
    if (P.fixed_x0)
      KLAUNCH(h, KC_ST_SMALL, stg::k_st_check_fixed<<<1, 64, 0, s>>>(s0.dyn, h->td.flags.p));
    else if (P.big0) {
      // the inverse by the blocked sweep on the whole chip, checked against K0; the LU factorisation by one workgroup
      // behind it runs only where the sweep gave up (decided on the device)
      double *scr = d.misc.p + P.oScr;
      const int q = P.q0max;
      const stg::X0Args xa{P.nk[0], q, s0.V, P.ldv[0], s0.BT, P.ldb[0], s0.dyn, d.misc.p + P.oK0, d.misc.p + P.oK0m, d.misc.p + P.oK0s,
                           P.ldq0, scr, h->td.flags.p};
      KLAUNCH(h, KC_ST_SMALL, stg::k_x0_prepare<<<nblk((long long)q * q), 256, 0, s>>>(xa));
      if ((e = st_blk_sweep(h, scr, q, true))) return e;
      KLAUNCH(h, KC_ST_SMALL, stg::k_x0_final<<<nblk((long long)q * q), 256, 0, s>>>(xa));
      const stg::BigScratch bs = stg::big_scratch(scr, q);
      if ((e = st_gemm(h, stg::GemmArgs{xa.K0mat, P.ldq0, xa.K0inv, P.ldq0, nullptr, 0, bs.Ks, bs.ldk, q, q, q, 1.0, 0.0, 0, 0}, KC_ST_GEMM_UPD, true)))
        return e;
      KLAUNCH(h, KC_ST_SMALL, stg::k_x0_check<<<1, 1024, 0, s>>>(xa, env_block_gj_tol()));
      KLAUNCH(h, KC_ST_SMALL, stg::k_st_init_factor<1024><<<1, 1024, d.lds.init, s>>>(P.nk[0], P.cap[0], s0.V, P.ldv[0], s0.BT, P.ldb[0], s0.dyn,
                                                                                    d.misc.p + P.oK0, d.misc.p + P.oK0m, d.misc.p + P.oK0s, P.ldq0, P.q0max, h->td.flags.p,
                                                                                    scr, bs.flags));
    } else
      KLAUNCH(h, KC_ST_SMALL, stg::k_st_init_factor<256><<<1, 256, d.lds.init, s>>>(P.nk[0], P.cap[0], s0.V, P.ldv[0], s0.BT, P.ldb[0], s0.dyn,
                                                                                  d.misc.p + P.oK0, d.misc.p + P.oK0m, d.misc.p + P.oK0s, P.ldq0, P.q0max, h->td.flags.p, nullptr, nullptr));
  }
  if (timed) HIPCHK(hipEventRecord(h->evs1, s));
  if (!h->listing) HIPCHK(hipGetLastError());
  return 0;
}

// Hqp_IpLQDOCP::step (hqp/Hqp_IpLQDOCP.C:869-976) with ExRiccatiSolveSc (:2007-2182).
// When ONE system is sharded over several ranks (staged_plan.hpp) the products with V_k run on the
// rank's ROW strip, those with F_k on its COLUMN strip (and the control columns); everything control-sized is computed
// by every rank.  Per stage one gather of a state-sized vector in the backward sweep (tt = v+ + V+ f, by rows) and one
// of the ranks' partial sums in the forward sweep (x+ = F s + f, by columns); the multipliers of the dynamics rows
// (V+ x+ + v+ + B+' eta+, by rows) are summed over the ranks once, at the end.  Not captured: the exchanges are calls.
static int staged_run_step(hqpkkt_t *h, const Vecs &v) {
  Analysis &an = h->an;
  StagedDev &d = *h->sd;
  kktdev::StagedPlan &P = d.plan;
  hipStream_t s = h->stream;
  const bool sh = P.sharded;
  const int n = an.n, m = an.m, K = P.K, NR = P.shard_count, RK = P.shard_rank;
  double *M = d.misc.p;
  double *S = M + P.oS, *qv = M + P.oQv, *gam = M + P.oGam, *tt = M + P.oTT, *tmp = M + P.oTmp, *gv = M + P.oGv;
  double *xv = M + P.oXV, *xp = M + P.oXP, *dyx = M + P.oDyx;  // (sharded)
  auto cut0 = [&](int k) { return sh ? P.strip_first(k) : 0; };
  auto width = [&](int k) { return sh ? P.strip_width(k) : 0; };
  int e;
  const long long ndx = (long long)P.ndyn + (P.fixed_x0 ? P.nk[0] : 0);
  if (sh) KLAUNCH(h, KC_ST_VEC, stg::k_st_zero<<<nblk(std::max<long long>(ndx, 1)), 256, 0, s>>>(ndx, dyx));
  if (m > 0) KLAUNCH(h, KC_VECTOR, k_red_t<<<nblk(m), 256, 0, s>>>(m, v.w, h->td.wt.p, v.r3, v.r4, h->td.tz.p));
  // q = C'tz - r1; with wide rows of C (StagedPlan::rows_vec) their share out of the blocks E_k, the walk over the narrow C'
  const bool wide = P.rows_vec();
  const CsrBuf &CT = wide ? d.wr.CTn : h->td.CT, &C = wide ? d.wr.Cn : h->td.C;
  if (wide) st_rows_cols(h, d, h->td.tz.p);
  KLAUNCH(h, KC_VECTOR, stg::k_st_q<<<nblk(n), 256, 0, s>>>(n, CT.ptr.p, CT.col.p, CT.src.p, h->td.vals.p, h->td.tz.p, v.r1, qv, wide ? d.wr.xc.p : nullptr));
  // One GPU: the products with V are not part of the sweeps' chains: V+ f (f: the dynamics' right-hand side) is known before the
  // backward sweep starts, the dynamics rows' multipliers are wanted by nobody before the forward sweep is over - both
  // for many stages per launch (staged_symv_group), which leaves the F products and the control-sized kernels in the
  // chains.
  // (on a stream of their own beside the chains - lowest priority, or a few workgroups that take the tiles in a stride -
  // the launches gained nothing: 35.8 - 37.4 ms per solve against 35.5; what the chains leave idle of HBM they lose again
  // when they share it)
  if (!sh) {
    for (int gi = (int)d.symv.groups[0].size() - 1; gi >= 0; gi--)
      if ((e = staged_symv_group(h, d, 0, gi, v.r2, nullptr))) return e;
    if ((e = staged_symv_rows(h, d, 0, v.r2, nullptr))) return e;
  }
  {  // last stage: v_K, and (one GPU) tt = v_K + V_K f_{K-1} for the stage before
    StagePtr sp = stage_ptr(d, K);
    const int nK = P.nk[K], eK = P.eq_ptr[K + 1] - P.eq_ptr[K];
    if (!sh && K > 0)
      KLAUNCH(h, KC_ST_VEC, stg::k_st_copy_add<<<nblk(nK), 256, 0, s>>>(nK, qv + P.nmk[K], sp.v, gv + P.nks[K - 1], tt));
    else
      KLAUNCH(h, KC_ST_VEC, stg::k_st_copy<<<nblk(nK), 256, 0, s>>>(nK, qv + P.nmk[K], sp.v));
    if (eK) KLAUNCH(h, KC_ST_VEC, stg::k_st_gather<<<nblk(eK), 256, 0, s>>>(eK, d.tab.eq_rows.p + P.eq_ptr[K], v.r2, sp.beta));
  }
  for (int k = K - 1; k >= 0; k--) {
    StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
    const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1];
    const int c0 = cut0(k), wd = width(k), c0n = cut0(k + 1), wdn = width(k + 1);
    const kktdev::StageSeq seq = d.prod.seq[k];
    if (sh) {
      // tt = v+ + V+ f by rows: the ranks' strips side by side (strip p starts at p xw), gathered
      if (wdn > 0 && (e = st_gemv_rows(h, stg::GemvRows{sn.Vs, P.ldv[k + 1], wdn, np, v.r2 + P.nks[k], sn.v + c0n, nullptr, 0, nullptr, nullptr,
                                                          xv + (long long)RK * P.xw[k + 1], 1.0})))
        return e;
      if ((e = exchange(h, HQPKKT_XCHG_ALLGATHER, xv, P.xw[k + 1], NR, nullptr))) return e;
      // gam = q_k + F' tt: the own state columns and the control columns
      if (wd > 0 && (e = st_gemv_cols(h, d, sp.F, P.ldfl[k], np, wd, xv, qv + P.nmk[k] + c0, 1.0, gam + c0))) return e;
      if (mm > 0 && (e = st_gemv_cols(h, d, sp.F + wd, P.ldfl[k], np, mm, xv, qv + P.nmk[k] + nn, 1.0, gam + nn))) return e;
    } else if (seq == kktdev::SEQ_SPARSE) {  // gam = q_k + F' tt over the columns' entries
      if (nn + mm > 0)
        KLAUNCH(h, KC_ST_SPARSE_VEC, stg::k_sp_gemv_cols<<<nblk(nn + mm), 256, 0, s>>>(
                                         stg::SpGemvCols{sp_cols(h, d, k, 0, nn + mm, true), tt, qv + P.nmk[k], 1.0, gam, nullptr, nullptr}));
      if (const int nd = P.heavy_count(k))  // (the heavy columns: a wavefront each)
        KLAUNCH(h, KC_ST_SPARSE_VEC, stg::k_sp_gemv_heavy<<<(nd + 3) / 4, 256, 0, s>>>(stg::SpGemvHeavy{
                                         sp_cols(h, d, k, 0, nn + mm), d.sp.hv_cols.p + P.hv_ptr[k], nd, tt, qv + P.nmk[k], 1.0, gam, nullptr, nullptr}));
    } else if (seq == kktdev::SEQ_PROFILE) {  // gam = q_k + F' tt over the panels' slab ranges
      stg::pf_launch_cols(stg::PfGemv{sp.F, P.ldf[k], np, nn + mm, d.pf.ranges(P, k), tt, qv + P.nmk[k], 1.0, gam, d.pf.part.p, d.pf.panels(P, k)},
                          P.stage_ranges(k), s, [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
    } else if ((e = st_gemv_cols(h, d, sp.F, P.ldf[k], np, nn + mm, tt, qv + P.nmk[k], 1.0, gam)))  // gam = q_k + F' tt with tt = v+ + V+ f (from the stage behind)
      return e;
    st_bwd_small(h, d, k, sp, sn, v.r2, gam);
    // v_k = gam_x - Y' rho: sharded the own entries (all a later product needs); one GPU with tt = v_k + V_k f_{k-1} for the next stage of the sweep
    if (sh ? wd > 0 && (e = st_gemv_cols(h, d, sp.Y + c0, P.ldy[k], P.qmax[k], wd, sp.rho, gam + c0, -1.0, sp.v + c0))
           : (e = st_gemv_cols(h, d, sp.Y, P.ldy[k], P.qmax[k], nn, sp.rho, gam, -1.0, sp.v, k > 0 ? gv + P.nks[k - 1] : nullptr, k > 0 ? tt : nullptr)))
      return e;
  }
  if (sh && !P.fixed_x0) {  // the free initial state needs v_0 in full: gathered
    StagePtr s0 = stage_ptr(d, 0);
    const int n0 = P.nk[0], c0 = cut0(0), wd = width(0);
    if (wd > 0) KLAUNCH(h, KC_ST_VEC, stg::k_st_copy<<<nblk(wd), 256, 0, s>>>(wd, s0.v + c0, xv + (long long)RK * P.xw[0]));
    if ((e = exchange(h, HQPKKT_XCHG_ALLGATHER, xv, P.xw[0], NR, nullptr))) return e;
    KLAUNCH(h, KC_ST_VEC, stg::k_st_copy<<<nblk(n0), 256, 0, s>>>(n0, xv, s0.v));
  }
  if ((e = st_initial_state(h, d, v.r2))) return e;
  for (int k = 0; k < K; k++) {
    StagePtr sp = stage_ptr(d, k), sn = stage_ptr(d, k + 1);
    const int nn = P.nk[k], mm = P.mk[k], np = P.nk[k + 1];
    const int c0 = cut0(k), wd = width(k), c0n = cut0(k + 1), wdn = width(k + 1);
    const kktdev::StageSeq seq = d.prod.seq[k];
    double *xk = S + P.nmk[k];
    st_fwd_small(h, d, k, sp, sn, v.dy);
    if (seq == kktdev::SEQ_SPARSE) {  // x+ = F s + f over the rows' entries
      if (np > 0)
        KLAUNCH(h, KC_ST_SPARSE_VEC, stg::k_sp_gemv_rows<<<(np + 15) / 16, 256, 0, s>>>(stg::SpGemvRows{
                                         d.sp.arow.p + 2 * (long long)P.nks[k], h->td.A.col.p, h->td.A.val.p, P.nmk[k], np, xk, v.r2 + P.nks[k], S + P.nmk[k + 1], 1.0}));
      continue;
    }
    if (seq == kktdev::SEQ_PROFILE) {  // x+ = F s + f over the panels whose range holds the row
      stg::pf_launch_rows(stg::PfGemv{sp.F, P.ldf[k], np, nn + mm, d.pf.ranges(P, k), xk, v.r2 + P.nks[k], 1.0, S + P.nmk[k + 1], nullptr, d.pf.panels(P, k)}, s,
                          [&](auto &&launch) { KLAUNCH(h, KC_ST_VEC, launch()); });
      continue;
    }
    if (!sh) {  // x+ = F s + f (the multipliers p = V+ x+ + v+ + B+' eta+ behind the sweep)
      if ((e = st_gemv_rows(h, stg::GemvRows{sp.F, P.ldf[k], np, nn + mm, xk, v.r2 + P.nks[k], nullptr, 0, nullptr, nullptr, S + P.nmk[k + 1], 1.0})))
        return e;
      continue;
    }
    // x+ = F s + f: the own columns' share of every row, gathered, and added in the order of the ranks to f_u u + f
    if ((e = st_gemv_rows(h, stg::GemvRows{sp.F, P.ldfl[k], np, wd, xk + c0, nullptr, nullptr, 0, nullptr, nullptr, xp + (long long)RK * P.xpslot, 1.0})))
      return e;
    if ((e = exchange(h, HQPKKT_XCHG_ALLGATHER, xp, P.xpslot, NR, nullptr))) return e;
    if ((e = st_gemv_rows(h, stg::GemvRows{sp.F + wd, P.ldfl[k], np, mm, xk + nn, v.r2 + P.nks[k], nullptr, 0, nullptr, nullptr, tt, 1.0}))) return e;
    KLAUNCH(h, KC_ST_VEC, stg::k_st_sum_slots<<<nblk(np), 256, 0, s>>>(np, NR, xp, P.xpslot, tt, S + P.nmk[k + 1]));
    // p = V+ x+ + v+ + B+' eta+: the own rows
    if (wdn > 0 &&
        (e = st_gemv_rows(h, stg::GemvRows{sn.Vs, P.ldv[k + 1], wdn, np, S + P.nmk[k + 1], sn.v + c0n,
                                           P.cap[k + 1] > 0 ? sn.BT + (long long)c0n * P.ldb[k + 1] : nullptr, P.ldb[k + 1], sn.dyn + 1, sn.eta,
                                           dyx + P.nks[k] + c0n, 1.0})))
      return e;
  }
  if (!sh) {
    for (int gi = 0; gi < (int)d.symv.groups[1].size(); gi++)
      if ((e = staged_symv_group(h, d, 1, gi, nullptr, v.dy))) return e;
    if ((e = staged_symv_rows(h, d, 1, nullptr, v.dy))) return e;
  }
  StagePtr sK = stage_ptr(d, K), s0 = stage_ptr(d, 0);
  const int eK = P.eq_ptr[K + 1] - P.eq_ptr[K], n0 = P.nk[0];
  if (eK) KLAUNCH(h, KC_ST_VEC, stg::k_st_y_last<<<nblk(eK), 256, 0, s>>>(eK, d.tab.eq_rows.p + P.eq_ptr[K], sK.eta, v.dy));
  if (sh) {
    if (P.fixed_x0 && width(0) > 0 &&
        (e = st_gemv_rows(h, stg::GemvRows{s0.Vs, P.ldv[0], width(0), n0, S, s0.v + cut0(0), nullptr, 0, nullptr, nullptr, dyx + P.ndyn + cut0(0), 1.0})))
      return e;
    if (ndx > 0 && (e = exchange(h, HQPKKT_XCHG_ALLREDUCE_SUM, dyx, ndx, 1, nullptr))) return e;
    if (P.ndyn > 0) KLAUNCH(h, KC_ST_VEC, stg::k_st_copy<<<nblk(P.ndyn), 256, 0, s>>>(P.ndyn, dyx, v.dy));
  } else if (P.fixed_x0 && (e = st_symv(h, d, stg::GemvRows{s0.V, P.ldv[0], n0, n0, S, s0.v, nullptr, 0, nullptr, nullptr, tmp, 1.0})))
    return e;
  if (P.fixed_x0) KLAUNCH(h, KC_ST_VEC, stg::k_st_y_fixed<<<nblk(n0), 256, 0, s>>>(n0, d.tab.fix_rows.p, d.tab.fix_src.p, h->td.vals.p, sh ? dyx + P.ndyn : tmp, v.dy));
  KLAUNCH(h, KC_VECTOR, stg::k_st_negate<<<nblk(n), 256, 0, s>>>(n, S, v.dx));
  if (m > 0)
    KLAUNCH(h, KC_VECTOR, k_red_dzdw<<<nblk(m), 256, 0, s>>>(m, C.ptr.p, C.col.p, C.src.p, h->td.vals.p, v.dx, h->td.wt.p, h->td.tz.p, v.r3, v.dz, v.dw));
  // (the wide rows are empty in the narrow C: k_red_dzdw has left tz and -r3 there, and the rows form writes dz and dw)
  if (wide) st_rows_rows(h, d, stg::RowsGemv{nullptr, nullptr, 0, nullptr, nullptr, v.dx, h->td.tz.p, h->td.wt.p, v.r3, v.dz, v.dw, nullptr});
  HIPCHK(hipGetLastError());
  return 0;
}
