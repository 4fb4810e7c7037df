// Internal header of the C-ABI library (include/hqpkkt.h): the handle and what the units share - device buffers,
// per-class timing, graph capture, and the functions one unit calls in another.  The units:
//   tree.hip           device residency and kernel sequencing of the tree engine (kernels.hip.h, factor_blk.hip.h,
//                      solve_top.hip.h; launch rule: tree_plan.hpp), the vector staging of a call, the residual and the
//                      posted read-backs
//   staged_engine.hip  the STAGED engine (staged.hip.h, staged_gemm.hip.h, staged_host.hip.h; launch rule of its product: gemm_form.hpp)
//   ip_loops.hip       the device-resident interior-point loops (ipdriver.hip.h)
//   q_entries.hip      the entries on the sparse Q where it lies (q_values.hip.h, q_bfgs.hip.h, q_eigen.hip.h)
//   hqpkkt.hip         the rest of the C ABI: handle management, factor / solve and their refinement, getters
#pragma once
#include "../../include/hqpkkt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <atomic>
#include <mutex>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "analysis.hpp"
#include "staged_plan.hpp"
#include "tree_plan.hpp"
#include "device_common.hip.h"

// The kernels that more than one unit launches: defined once (kernels.hip.h, compiled into tree.hip)
namespace kktdev {
__global__ void k_weights(int mode, int m, int nme, const double *z, const double *w, double *wt, double *sc, int *status);
__global__ void k_red_t(int m, const double *w, const double *zw, const double *r3, const double *r4, double *t);
__global__ void k_red_dzdw(int m, const int *Cp, const int *Cc, const int *Cs, const double *vals, const double *dx,
                           const double *zw, const double *t, const double *r3, double *dz, double *dw);
__global__ void k_gather_values(int nnz, const int *src, const double *vals, double *out);
__global__ void k_zd_weak(int n, CsrDev Q, CsrDev AT, int *flag);
__global__ void k_clear(double *p, long long n, int *words);
__global__ void k_copy_vectors(CopyList L, int nvec);
__global__ void k_axpy4(int n, int me, int m, double alpha, const double *e1, const double *e2, const double *e3,
                        const double *e4, double *d1, double *d2, double *d3, double *d4);
}  // namespace kktdev
using namespace kktdev;  // (the units are written against kktdev's names)

// (everything below is internal to the library: not exported)
#pragma GCC visibility push(hidden)

extern char g_last_hip_error[512];  // the text of the last HIP error (hqpkkt_strerror)

#define HIPCHK(call)                                                              \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess) {                                                       \
      std::snprintf(g_last_hip_error, sizeof(g_last_hip_error), "%s:%d %s: %s", __FILE__, \
                    __LINE__, #call, hipGetErrorString(e_));                      \
      return HQPKKT_E_DEVICE;                                                     \
    }                                                                             \
  } while (0)

// ---- owners of HIP resources: move-only, freed by their destructors.  An empty owner makes no HIP call (a handle that
// never touched the device is created and destroyed without HIP).
extern std::atomic<long long> g_live_bufs[2];  // live allocations of DBuf / PinnedBuf in the process (hqpkkt_debug_get 40)

template <class T>
struct DBuf {
  T *p = nullptr;
  size_t count = 0;
  DBuf() = default;
  DBuf(DBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), count(std::exchange(o.count, 0)) {}
  DBuf &operator=(DBuf &&o) noexcept {
    if (this != &o) release(), p = std::exchange(o.p, nullptr), count = std::exchange(o.count, 0);
    return *this;
  }
  ~DBuf() { release(); }
  int alloc(size_t k) {
    release();
    if (hipMalloc((void **)&p, sizeof(T) * (k ? k : 1)) != hipSuccess) {
      p = nullptr;
      return HQPKKT_E_MEM;
    }
    count = k;
    g_live_bufs[0]++;
    return 0;
  }
  int upload(const std::vector<T> &v) {
    int e = alloc(v.size());
    if (e) return e;
    if (!v.empty() &&
        hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess)
      return HQPKKT_E_DEVICE;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p), g_live_bufs[0]--;
    p = nullptr;
    count = 0;
  }
};

// pinned host memory (hipHostMalloc); dev: the device's address of mapped memory (map)
template <class T>
struct PinnedBuf {
  T *p = nullptr, *dev = nullptr;
  size_t count = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept
      : p(std::exchange(o.p, nullptr)), dev(std::exchange(o.dev, nullptr)), count(std::exchange(o.count, 0)) {}
  PinnedBuf &operator=(PinnedBuf &&o) noexcept {
    if (this != &o)
      release(), p = std::exchange(o.p, nullptr), dev = std::exchange(o.dev, nullptr), count = std::exchange(o.count, 0);
    return *this;
  }
  ~PinnedBuf() { release(); }
  hipError_t alloc(size_t k, unsigned flags) {
    release();
    const hipError_t e = hipHostMalloc((void **)&p, sizeof(T) * k, flags);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    count = k;
    g_live_bufs[1]++;
    return hipSuccess;
  }
  hipError_t map() {
    const hipError_t e = hipHostGetDevicePointer((void **)&dev, p, 0);
    if (e != hipSuccess) dev = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p), g_live_bufs[1]--;
    p = dev = nullptr;
    count = 0;
  }
};

// a stream, event or graph and the call that destroys it; create into &x.h
template <class H, hipError_t (*Destroy)(H)>
struct HipOwner {
  H h = nullptr;
  HipOwner() = default;
  HipOwner(HipOwner &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
  HipOwner &operator=(HipOwner &&o) noexcept {
    if (this != &o) reset(), h = std::exchange(o.h, nullptr);
    return *this;
  }
  ~HipOwner() { reset(); }
  void reset() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
  operator H() const { return h; }
};
using StreamOwner = HipOwner<hipStream_t, hipStreamDestroy>;
using EventOwner = HipOwner<hipEvent_t, hipEventDestroy>;

struct CsrBuf {
  DBuf<int> ptr, col, src;
  DBuf<double> val;  // values in CSR order, refreshed by hqpkkt_set_values
  int upload(const Analysis::Csr &c) {
    int e;
    if ((e = ptr.upload(c.ptr)) || (e = col.upload(c.col)) || (e = src.upload(c.src)) || (e = val.alloc(c.src.size())))
      return e;
    return 0;
  }
  CsrDev dev() const { return CsrDev{ptr.p, col.p, src.p, val.p}; }
};

// per-kernel-class device timing (hqpkkt_set_profile): HIP events on the
// handle's stream around every launch, summed per class after the call
enum { KC_ASSEMBLE = 0, KC_FACTOR_DIAG, KC_PANEL_SOLVE, KC_SCHUR_UPDATE,
       KC_SOLVE_FWD, KC_SOLVE_BWD, KC_VECTOR, KC_RESIDUAL, KC_ST_GEMM, KC_ST_SMALL, KC_ST_VEC, KC_ST_GEMM_UPD, KC_XCHG, KC_SOLVE_TOP,
       KC_ST_SPARSE, KC_ST_SPARSE_VEC,  // (the sparse form of the stage products: the factorisation's passes, the solve's)
       KC_ST_ROWS_VEC,                  // (the wide rows of C in step and residual: staged_rows.hip.h)
       KC_COUNT };
static const char *const kc_names[KC_COUNT] = {"assemble", "factor_diag", "panel_solve",
                                               "schur_update", "solve_fwd", "solve_bwd", "vector",
                                               "residual", "staged_gemm", "staged_small", "staged_gemv", "staged_gemm_upd",
                                               "exchange", "solve_top", "staged_sparse", "staged_sparse_gemv", "staged_rows_gemv"};
struct Prof {
  bool on = false;
  std::vector<EventOwner> pool;
  std::vector<int> cls;
  size_t used = 0;
  double ms[KC_COUNT] = {0};
  long long launches[KC_COUNT] = {0};
  hipEvent_t get() {
    if (used == pool.size()) {
      EventOwner e;
      if (hipEventCreate(&e.h) != hipSuccess) return nullptr;
      pool.push_back(std::move(e));
    }
    return pool[used++];
  }
  void begin(int c, hipStream_t s) {
    if (!on) return;
    hipEvent_t e = get();
    cls.push_back(c);
    if (e) (void)hipEventRecord(e, s);
  }
  void end(hipStream_t s) {
    if (!on) return;
    hipEvent_t e = get();
    if (e) (void)hipEventRecord(e, s);
  }
  // call after the stream has been synchronised
  void collect() {
    for (size_t k = 0; k + 1 < used && k / 2 < cls.size(); k += 2) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, pool[k], pool[k + 1]) == hipSuccess) {
        ms[cls[k / 2]] += t;
        launches[cls[k / 2]]++;
      }
    }
    used = 0;
    cls.clear();
  }
  void reset() {
    for (int c = 0; c < KC_COUNT; c++) ms[c] = 0, launches[c] = 0;
  }
};
#define KLAUNCH(h, c, ...)        \
  do {                            \
    if ((h)->listing) break;      \
    (h)->prof.begin(c, (h)->stream); \
    __VA_ARGS__;                  \
    (h)->prof.end((h)->stream);   \
  } while (0)

struct StagedDev;  // (staged_host.hip.h)
struct StagedDevDelete {
  void operator()(StagedDev *d) const;  // (staged_engine.hip, where StagedDev is complete)
};
void staged_reset(StagedDev &d);  // frees what the stage blocks hold on the device; the plan stays

// What release_device frees: the device state of one analysis - the tree engine's structure and numeric arrays, and
// the vectors, status words and pinned staging that both engines use
struct TreeDev {
  // symbolic structure on the device
  DBuf<int> piv_start, npiv, nbor, parent, bidx, rel, child_ptr, child_idx, ent_a, ent_b,
      term_ptr, diag_ent, q2e, pinv;
  struct DevSched {  // device copy of an Analysis::Sched
    DBuf<int> level_nodes, upd_tiles, slabs, gslabs, cblks;
  } ds[2];
  DBuf<long long> zero_panel;  // (offset, length) pairs, sharded mode
  DBuf<int> simple_src, simple_wi;  // FULL: compact single-term records of the entries (k_assemble_simple)
  DBuf<signed char> keep_e;
  DBuf<long long> bptr, panel_off, upd_off, x_off, cb_off, ent_dst, linv_off, pinv_off;
  DBuf<TermDev> terms;
  DBuf<signed char> esign;
  CsrBuf Qf, A, AT, C, CT;
  // numeric state
  DBuf<double> vals, wt, sc, ent_val, panel, upd, xar, dinv, rhs, xsol, cb, ytmp, vtmp, linv;
  DBuf<int> ptype, lperm, flags;  // flags: [0] status, [1] n_2x2, [2] n_perturbed
  // [0] kmax, [1] residual max: inside the flags buffer (ints 120..123) so that status and
  // maxima come back in ONE copy; hqpkkt::Kept::hpin: pinned host memory those copies land in
  struct {
    unsigned long long *p = nullptr;
  } bits;
  // host vectors of a small system: packed into / out of pinned memory by the CPU, ONE transfer each way instead of
  // six + four staged copies from pageable memory; the tree engine maps it (dev: kernels copy in and out of it)
  PinnedBuf<double> hstage;
  size_t hstage_in = 0, hstage_out = 0;  // doubles; 0 = system too large, copy vector by vector
  // vectors: staging for host pointers + refinement work vectors
  DBuf<double> vin;   // z w r1 r2 r3 r4
  DBuf<double> vout;  // dx dy dz dw
  DBuf<double> vres;  // residual vectors _r1.._r4
  DBuf<double> vcor;  // corrections _dx.._dw
  DBuf<double> tz;    // REDUCED temporary (m)
  DBuf<int> top_nodes, top_idx, top_bpos, top_up;  // the fused top of the solve (TreePlan::top); top_up: the fronts leaves first (its split form)
  // trees of small fronts only (TreePlan::small_tree): the exchange arrays (2 x cb_elems, then 2 x dim)
  DBuf<double> tree_x, tree_u;   // tree_u: the exchange copies of the update arena (2 x upd_elems)
  DBuf<int> tree_words, tree_down;  // [0] solves so far, [1] factorisations so far; the fronts root first
  DBuf<double> top_x;  // the exchange arrays of the launch: 2 x top_n x ST_CS contributions, then 2 x top_n x ST_XS solution
  // the entries on the sparse Q where it lies (hqpkkt_q_product .. hqpkkt_lagrangian_gradient; q_entries.hip), both engines
  struct QVal {
    bool mapped = false, bad_diag = false;  // the host tables are made / a row without exactly one stored diagonal
    std::vector<int> h_didx, h_kind;        // per row the index of its diagonal in Qx (-1: none); per entry its row, QV_UPPER or QV_LOWER
    DBuf<int> didx, kind;
    DBuf<double> offsum;                    // Gerschgorin's row pass
    // hqpkkt_q_blocks / hqpkkt_q_bfgs_update / hqpkkt_q_dscale_update (q_bfgs.hip.h): the partition of 0 .. n-1 for one bsize
    // (< 0 detected, 0 one block, > 0 blocks of bsize) with its device tables, partial sums and reports - made by the first
    // update or eigenvalue control with that bsize (qb_plan), never regrown.  Both fills and DScale share a plan: the fills
    // differ in the host's test of `all_full` alone, and DScale's bsize <= 0 is the one block of key 0.
    struct BfgsPlan {
      int bsize = 0, nblocks = 0, nunits = 0, max_len = 0;
      bool all_full = false;
      std::vector<int> first;            // nblocks + 1: the blocks' first indices, n behind them
      std::vector<unsigned char> full;   // per block: every (i, j), i <= j, is stored
      DBuf<int> blk_of, boff, bunit, ublk;  // block of a variable; first index / first unit of a block (+ 1); block of a unit
      DBuf<double> part;                    // 3 per unit: scratch of whichever update runs (the stream orders them)
      DBuf<double> rep, ds_rep;             // QV_REPORT per block: the last BFGS update's words; the last DScale update's,
                                            // made by the first DScale update on this plan
      // hqpkkt_q_eigen_control (q_eigen.hip.h), made or grown by the control that needs them: the basis (eig_cap vectors of
      // n), the units' partial sums, T (stride 2 eig_steps per block), the report, the state's two copies and the floors
      int eig_cap = 0, eig_steps = 0;       // steps the buffers hold; the step cap of the plan's last control
      DBuf<double> eig_V, eig_part, eig_T, eig_rep, eig_st, eig_floor;
    };
    std::vector<BfgsPlan> bfgs_plans;
    int bfgs_last = -1, ds_last = -1; // plan of the last BFGS update / the last DScale update since the analysis
    DBuf<int> erow, ecol;             // row and column of every stored entry of Qx
    DBuf<double> bfgs_qs, bfgs_v;     // Q s restricted to the blocks, v as applied
    int eig_last = -1;                // plan of the last eigenvalue control since the analysis
    DBuf<double> eig_w;               // its product w = Q v (n) and the block-restricted row pass (n)
  } qv;
  // a host caller's vectors of those entries and of the entries on the dense stage Hessians (CallerVecs, which makes them)
  struct CallerBufs {
    DBuf<double> in, out;
  } cv;

  DevTree tree() const {
    return DevTree{piv_start.p, npiv.p,     nbor.p,  parent.p, bptr.p,      bidx.p,     rel.p,
                   panel_off.p, upd_off.p, x_off.p, cb_off.p, child_ptr.p, child_idx.p, pinv.p, pinv_off.p};
  }
};

struct hqpkkt {
  // the handle's own stream and its timing events: destroyed last (members go in reverse order)
  StreamOwner own_stream;
  hipStream_t stream = nullptr;
  EventOwner ev0, ev1, evs0, evs1;
  EventOwner evt0, evt1;  // total time of an interior-point run (hqpkkt_mehrotra / _franke)
  hqpkkt_opts opts;
  Prof prof;
  Analysis an;
  std::unique_ptr<StagedDev, StagedDevDelete> sd;  // HQPKKT_MODE_STAGED: the stage blocks (staged_host.hip.h)
  kktdev::StagedRequest staged_rq;                 // ... and what its setters ask of the next analysis (staged_plan.hpp)
  double ge_tol = 1.0e-6;   // rank decision of the stage constraints (_ge_tol, hqp/Hqp_IpLQDOCP.C:113)
  bool analyzed = false, uploaded = false, have_values = false, factored = false;
  hqpkkt_stats st;
  TreeDev td;
  // What survives release_device(true) (the re-analysis inside hqpkkt_solve, switch_to_policy0): the pattern and with
  // it the sizes stay, and a host may hold the pointers of hqpkkt_values_staging
  struct Kept {
    DBuf<double> ipv;  // interior-point driver: x y z w | r1..r4 | dxa..dwa | dx..dw | c b d | partials | scalars
    // Read-backs without a copy and without hipStreamSynchronize (round 6): hpin is mapped, coherent host memory
    // (hpin.dev: the device's address of it); a one-wavefront kernel at the point of the stream where the words are
    // final stores them there and a sequence number behind them (k_post_words, kernels.hip.h), the host spins on that
    // number (post_wait).  Measured (tools/post_probe.hip): 6 us per read-back behind a queue of small kernels against
    // 16 for hipMemcpyAsync + hipStreamSynchronize - the device-resident interior-point loops read back three times per
    // iteration.  128 doubles: 0..63 status words (as ints), 64.. the IP loop's scalars
    PinnedBuf<double> hpin;
    DBuf<unsigned> post_seq_dev;  // the sequence number of the posted read-backs, counted by k_post_words
    // pinned host staging of Qx | Ax | Cx (hqpkkt_values_staging), nq + na + nc doubles; a new analysis with another
    // pattern allocates again
    PinnedBuf<double> hvals;
  } kept;
  unsigned post_seq = 0;       // the number the last posting kernel in the stream will store (hpin word HPIN_SEQ)
  // one system over several ranks: collectives are delegated to the caller
  int shard_rank = 0, shard_count = 1;
  hqpkkt_exchange_fn xchg_fn = nullptr;
  hqpkkt_exchange_stream_fn xchg_sfn = nullptr;  // stream-ordered form (RCCL): nothing is drained
  void *xchg_ctx = nullptr;
  const double *out_pending = nullptr;   // results wait in hstage + hstage_in for unstage()
  bool out_by_kernel = false;            // ... written there by a kernel in front of the posting kernel (no stream synchronisation needed)
  bool host_graph_call = false;          // inside a solve whose first part ran as hqpkkt::ghost_step (no timing events in the stream)
  kktdev::TreePlan plan;  // what run_factor and run_step launch, level by level (tree_plan.hpp; built by upload)
  // the device-resident interior-point loops: cancelled multiplier pivots are replaced (kernels.hip.h, TINY_REPLACE_WORD)
  // only in the SECOND attempt of a run whose first attempt - without the replacement, i.e. with the factors the
  // reference's own loop gets from this plugin through the shim - ended "degenerate" or singular
  bool tiny_replace_in_loop = false;
  unsigned long long *top_stamps = nullptr;  // (hqpkkt_debug_solve_top_stamps)
  // captured kernel sequences (factor; step on the caller's vectors; step on the
  // refinement's residual vectors): replayed with hipGraphLaunch
  struct GraphSlot {
    HipOwner<hipGraph_t, hipGraphDestroy> g;
    HipOwner<hipGraphExec_t, hipGraphExecDestroy> ge;  // (destroyed before g)
    unsigned n_posts = 0;  // posted read-backs inside (k_post_words counts on the device; the host counts along at every replay)
    void drop() { ge.reset(), g.reset(), n_posts = 0; }
  } gfactor[2], gstep[2][3];  // [phase], [caller's / refinement's vectors][phase]
  // A caller with HOST vectors (the reference's solvers through the shim): the packed vectors are read out of the pinned
  // staging buffer by a kernel, the results written into it by a kernel, and the status words posted - a whole call is
  // one graph on the compute queue (no copy engine between the launches: 9 - 13 us at each change of engine,
  // profiles/r06_shim_timeline.txt) and ends with the posted words, not a stream synchronisation
  GraphSlot ghost_factor, ghost_step;
  // The device-resident interior-point loops hand over the same device vectors in every iteration: their sequences are
  // captured ON those vectors (no copies into and out of the handle's staging buffers), one graph per set of pointers.
  struct DirectGraph {
    const void *key[10];
    GraphSlot g;
  };
  std::vector<DirectGraph> gdirect_step, gdirect_factor;
  // ... and whole SEGMENTS of an iteration of the device-resident loops - everything between two read-backs: the
  // factorisation, a solve, its residual and the posting kernel - as one graph (ip_segment)
  std::vector<DirectGraph> gdirect_seg;
  // ... and a caller's own factor / solve call on its device vectors with its residual and the posted words
  std::vector<DirectGraph> gdirect_call;
  GraphSlot &direct_slot(std::vector<DirectGraph> &cache, const void *const (&key)[10]) {
    for (auto &d : cache)
      if (std::memcmp(d.key, key, sizeof(key)) == 0) return d.g;
    if (cache.size() >= 6)  // (Mehrotra's loop has two sets + the refinement's, Franke's one + the refinement's)
      cache.erase(cache.begin());  // (the oldest graph is dropped)
    cache.emplace_back();
    std::memcpy(cache.back().key, key, sizeof(key));
    return cache.back().g;
  }
  bool use_graphs = true, capturing = false;
  // staged_upload's dry walk of the factor sequence: st_gemm makes the work lists and tile orders its launches will look
  // up; KLAUNCH, the stream pairs, the timing records and exchange() do nothing
  bool listing = false;
  unsigned cap_posts = 0;  // posted read-backs of the capture in progress
  // inside hqpkkt_mehrotra: factor() returns without waiting for its status (read with the
  // residual of the solve that follows), solve() leaves its result in the stream
  bool lazy = false, factor_unchecked = false;
  // hqpkkt_factor / hqpkkt_solve of a caller with DEVICE vectors: the second call in a row with the same pointers works
  // on the caller's vectors themselves (no staging copies; the sequences are captured on them, DirectGraph) - set for
  // the duration of that call.  last_f / last_s: the pointers of the previous call of either kind
  bool direct_now = false;
  const void *last_f[2] = {nullptr, nullptr}, *last_s[10] = {};
  // hqpkkt_franke: the first residual of a solve is not waited for - it comes back with the scalars of the iteration
  // (one read-back per iteration); residual_pending: such a residual is in the stream, collect_residual() reads it
  bool defer_residual = false, residual_pending = false;
  int res_read = 122;  // the word of the flags buffer the residual kernels leave their maximum in (cleared by k_post_words)
  bool no_polled = false;      // a polled launch gave up once: per-level launches for the rest of the handle's life (poll_fallback)
  bool soft_singular = false;  // the factorisation perturbed an exactly zero pivot (counters[3])
  bool soft_tiny = false;      // ... or met a pivot below 1e-13 max|K| on a multiplier-type row (counters[4])
  double refine_target = 0.0;  // > 0: the refinement of hqpkkt_solve aims below mat_eps (set by hqpkkt_franke)
  // hqpkkt_mehrotra left x, y and the hot-start candidates of z, w in ipv (same dimensions)
  bool ip_hot_valid = false;
  bool fr_hot_valid = false;  // hqpkkt_franke left x, y, z, w in ipv (same dimensions)
  double fr_rhomin = 0.0;     // ... and its qp_rhomin, which hot_start keeps (hqp/Hqp_IpsFranke.C:222-266)
  // the caller's pattern (hqpkkt_analyze), kept for the one repetition of the symbolic phase
  // that zd_policy -1 may ask for when the first values arrive; zd_used: policy of h->an
  std::vector<int> pQp, pQi, pAp, pAi, pCp, pCi;
  int zd_used = 2;
  bool zd_decided = true;
  // zd_policy -1 on a QP with weak Hessian diagonals: the values on the host, so that a solve
  // whose refinement fails can switch the handle to policy 0 (symbolic phase, upload, values,
  // factorisation again) and repeat itself
  bool zd_weak = false;
  std::vector<double> hQ, hA, hC;
  bool short_rows = false;  // CSR rows of a handful of entries: 4 lanes per row in the SpMV kernels
  void drop_graphs() {
    for (auto &g : gfactor) g.drop();
    ghost_factor.drop(), ghost_step.drop();
    for (auto &gs : gstep)
      for (auto &g : gs) g.drop();
    gdirect_step.clear(), gdirect_factor.clear(), gdirect_seg.clear(), gdirect_call.clear();
  }
  void release_device(bool keep_ip = false) {  // keep_ip: hqpkkt_mehrotra's vectors and the pinned words stay (Kept)
    td = TreeDev();
    if (!keep_ip) kept = Kept();
    if (sd) staged_reset(*sd);
    drop_graphs();
    uploaded = have_values = factored = false;
  }
};

static inline int nblk(long long work, int bs = 256) { return (int)((work + bs - 1) / bs); }
// grid of k_copy_vectors: enough workgroups for the longest vector, at most 1024
static inline int copy_blocks(const CopyList &L) {
  int mx = 1;
  for (int v = 0; v < 6; v++) mx = std::max(mx, L.len[v]);
  return std::min(1024, std::max(1, nblk(mx)));
}

// pointers of the six input vectors / four outputs for the current call
struct Vecs {
  const double *z, *w, *r1, *r2, *r3, *r4;
  double *dx, *dy, *dz, *dw;
};

struct OutPtrs {
  double *dx, *dy, *dz, *dw;
};

// The caller's vectors of one call of an entry on the sparse Q (q_entries.hip), on the dense stage Hessians
// (staged_hess_host.hip.h) or of hqpkkt_lagrangian_gradient_staged (staged_engine.hip): device vectors are handed through where they lie and finish() does nothing; host vectors are
// copied through the handle's two buffers (TreeDev::CallerBufs) in the handle's stream, and finish() copies the outputs
// back and waits - a host caller has its results, and its vectors back, when it returns.  At most 5 inputs and 2 outputs,
// a null vector takes no room.  ready() makes the buffers at the first host call, for the largest need of any entry, so
// they are never regrown under work still in the stream; it is called outside every capture.
// as_host: the vectors are host arrays whatever opts.loc says (the debug entries)
struct CallerVecs {
  hqpkkt_t *h;
  bool as_host = false;
  size_t in_used = 0, out_used = 0;
  int nout = 0;
  struct { double *host, *dev; size_t k; } outs[2];
  bool host() const { return as_host || h->opts.loc != HQPKKT_LOC_DEVICE; }
  int ready() {
    TreeDev::CallerBufs &b = h->td.cv;
    if (!host() || b.in.p) return 0;
    const size_t n = (size_t)h->an.n;
    int e;
    if ((e = b.in.alloc(std::max((size_t)(HQPKKT_HESS_UPDATE_RANK + 1) * n, 2 * n + h->an.me + h->an.m) + 1)) || (e = b.out.alloc(2 * n + 1))) return e;
    return 0;
  }
  int in(const double *p, size_t k, const double **dev) {
    *dev = p;
    if (!p || !host()) return 0;
    double *b = h->td.cv.in.p + in_used;
    in_used += k;
    if (k) HIPCHK(hipMemcpyAsync(b, p, sizeof(double) * k, hipMemcpyHostToDevice, h->stream));
    *dev = b;
    return 0;
  }
  void out(double *p, size_t k, double **dev) {
    *dev = p;
    if (!p || !host()) return;
    *dev = h->td.cv.out.p + out_used;
    out_used += k;
    outs[nout].host = p, outs[nout].dev = *dev, outs[nout].k = k, nout++;
  }
  int finish() {
    if (!host()) return 0;
    for (int i = 0; i < nout; i++)
      if (outs[i].k) HIPCHK(hipMemcpyAsync(outs[i].host, outs[i].dev, sizeof(double) * outs[i].k, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
  }
};

// replay (or first capture) of a kernel sequence as a hipGraph; falls back to
// eager launches while per-kernel profiling is on
template <class F>
static int graphed(hqpkkt_t *h, hqpkkt::GraphSlot &slot, F body) {
  if (!h->use_graphs || h->prof.on || h->capturing) return body();  // (capturing: a sequence inside a segment's capture)
  if (!slot.ge) {
    HIPCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    h->capturing = true, h->cap_posts = 0;
    int e = body();
    h->capturing = false;
    const hipError_t ce = hipStreamEndCapture(h->stream, &slot.g.h);
    if (e) {
      slot.drop();
      h->post_seq -= h->cap_posts;  // (nothing was posted)
      return e;
    }
    if (ce != hipSuccess || !slot.g || hipGraphInstantiate(&slot.ge.h, slot.g, nullptr, nullptr, 0) != hipSuccess) {
      slot.drop();  // capture not possible: run eagerly from now on
      h->use_graphs = false;
      (void)hipGetLastError();
      h->post_seq -= h->cap_posts;
      return body();
    }
    slot.n_posts = h->cap_posts;  // (the host has counted them during the capture)
  } else
    h->post_seq += slot.n_posts;
  HIPCHK(hipGraphLaunch(slot.ge, h->stream));
  return 0;
}

// The C ABI promises that nothing is thrown across it (the shim's callers longjmp through Meschach
// frames): every entry point that allocates with the standard library runs inside this guard.
template <class F>
static int guarded(F body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return HQPKKT_E_MEM;
  } catch (...) {
    return HQPKKT_E_INTERN;
  }
}

static const int HQPKKT_E_POLL = -7001;  // internal: a polled launch gave up (poll_fallback); never leaves the library

static inline float elapsed(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, a, b) != hipSuccess) ms = -1.f;
  return ms;
}

// the damping factor of the BFGS updates (of the dense stage Hessians, of the sparse Q) as hessian_update.bfgs_terms forms
// it, operation by operation (no contraction)
static inline double bfgs_gamma_eff(double gamma, double alpha) {
#pragma clang fp contract(off)
  if (gamma >= 0.0) return gamma;
  const double g = -gamma, omg = 1.0 + gamma, oma = 1.0 - alpha;
  const double t = omg * oma;
  return g + t;
}

// ---- what one unit calls in another
// tree.hip
int exchange(hqpkkt_t *h, int op, double *buf, long long slot, int nslots, hipStream_t on = nullptr);
int ensure_device(hqpkkt_t *h);
int alloc_hpin(hqpkkt_t *h);
int upload(hqpkkt_t *h);
bool poll_fallback(hqpkkt_t *h, const int *hs);
TreeSwitches tree_switches(const hqpkkt_t *h);  // the environment as it stands, and h->no_polled
bool host_graphs_ok(const hqpkkt_t *h);
size_t stage_pack(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3, const double *r4);
int stage_in(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3, const double *r4,
             Vecs &v);
void stage_out_ptrs(hqpkkt_t *h, Vecs &v);
int stage_out(hqpkkt_t *h, const Vecs &v, double *dx, double *dy, double *dz, double *dw);
void unstage(hqpkkt_t *h, double *dx, double *dy, double *dz, double *dw);
int do_factor(hqpkkt_t *h, const Vecs &v);
int do_step(hqpkkt_t *h, const Vecs &v, int which);
int post_words(hqpkkt_t *h, const double *out, int n_out, bool residual = false);
int post_wait(hqpkkt_t *h);
int residual_launch(hqpkkt_t *h, const Vecs &v);
int run_residual(hqpkkt_t *h, const Vecs &v, double *res, const OutPtrs *out = nullptr);
int collect_residual(hqpkkt_t *h, double *res);
// staged_engine.hip
int staged_analyze(hqpkkt_t *h, int n, int me, int m, bool dense_dyn = false);
int staged_set_values(hqpkkt_t *h, const double *Qx, const double *Ax, const double *Cx, const double *const *Fblk = nullptr,
                      const long long *ldF = nullptr, bool dense = false);  // (Fblk / dense: the dense hand-over of the dynamics)
int staged_factor(hqpkkt_t *h, const Vecs &v);
int staged_step(hqpkkt_t *h, const Vecs &v, int which);
// (xq: Q dx with dense stage Hessians, hqpkkt_set_hessian_form; left alone otherwise)
int staged_dense_products(hqpkkt_t *h, const Vecs &v, const double **x1, const double **x2, int *ndyn, const double **xq);
// the residual's share of the wide rows of C (hqpkkt_set_dense_rows): *xcw = C_wide' dz, *cw = the wide rows' C dx, and the
// narrow copies of C' and C in *CT, *C; leaves all four as they are on a handle without wide rows
void staged_rows_products(hqpkkt_t *h, const Vecs &v, const double **xcw, const double **cw, CsrDev *CT, CsrDev *C);
int staged_debug_get(const hqpkkt_t *h, int what, std::vector<int> &out);
// what staged_set_values does behind its copies into the handle's values; q_only: Q's values alone have changed
int staged_values_changed(hqpkkt_t *h, bool q_only);
// ... and what hqpkkt_set_values does behind its copies on the tree engine (hqpkkt.hip); Qx, Ax, Cx: the caller's arrays the
// values came from, null with q_only
int values_changed(hqpkkt_t *h, bool q_only, const double *Qx, const double *Ax, const double *Cx);
enum { STAGED_FORM_HESS_DENSE = 1, STAGED_FORM_DENSE_DYN = 2, STAGED_FORM_SHARDED = 4 };
int staged_form(const hqpkkt_t *h);  // of an analysed STAGED handle
// hqpkkt.hip
int solve_vecs(hqpkkt_t *h, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
               const double *r4, double *dx, double *dy, double *dz, double *dw, Vecs &v);
int solve_tail(hqpkkt_t *h, Vecs &v, const double *z, const double *w, const double *r1, const double *r2, const double *r3,
               const double *r4, double *dx, double *dy, double *dz, double *dw, double res, double *res_out);

#pragma GCC visibility pop
