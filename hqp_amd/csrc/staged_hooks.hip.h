// The debug and test entry points of the STAGED engine that stand outside a handle's sequences: the micro-benchmark and
// self-check of the dense fp64 product, one launch of a product or a vector product on the caller's operands, and the
// host-only views of the launch rule and its work lists (include/hqpkkt.h, hqpkkt_debug_*).  Included by
// staged_engine.hip alone, behind staged_host.hip.h: the same translation unit, the same kernels instantiated once.
#pragma once

extern "C" {

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
