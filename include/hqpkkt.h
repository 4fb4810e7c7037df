/*
 * hqpkkt.h -- C ABI of the MI355X-native interior-point KKT linear-system path.
 *
 * This is the drop-in boundary for the reference's Hqp_IpMatrix plugin point
 * (hqp/Hqp_IpMatrix.h:63-88).  A thin C++ subclass of Hqp_IpMatrix (see
 * shim/Hqp_IpSpBKPHip.C and INTEGRATION.md) forwards its virtual methods to
 * these entry points exactly like the reference's own Hqp_IpPARDISO forwards to
 * a dlopen'ed C function (hqp/pardiso_wrapper.h:33-48,
 * hqp/Hqp_IpPARDISO.C:156-222).
 *
 * Conventions
 *  - plain pointers and sizes only; int32 indices, fp64 values; 0-based CSR
 *    with column indices sorted inside each row (as Meschach's SPROW keeps
 *    them, meschach/sparse.h:44-63);
 *  - every function returns a status: 0 = ok, HQPKKT_E_SING (= Meschach's
 *    E_SING, meschach/err.h:88) for a numerically singular system or a zero
 *    z/w component (meschach/vecop.c:346-348), other HQPKKT_E_* otherwise.
 *    Nothing throws, longjmps or aborts across this boundary; the shim turns a
 *    non-zero status into m_error(...) (meschach/err.h:63);
 *  - calls are synchronous from the caller's point of view; a handle is not
 *    re-entrant (the reference drives the plugin from one thread);
 *  - there is NO CPU fallback: numeric entry points need a gfx950 device and
 *    fail with HQPKKT_E_DEVICE without one.  hqpkkt_analyze is host-only.
 */
#ifndef HQPKKT_H
#define HQPKKT_H

#ifdef __cplusplus
extern "C" {
#endif

#define HQPKKT_VERSION 1

/* status codes (values 1..17 mirror meschach/err.h:84-110 where they exist) */
#define HQPKKT_OK 0
#define HQPKKT_E_SIZES 1   /* E_SIZES  */
#define HQPKKT_E_MEM 3     /* E_MEM    */
#define HQPKKT_E_SING 4    /* E_SING   */
#define HQPKKT_E_FORMAT 6  /* E_FORMAT: unsorted / out-of-range CSR */
#define HQPKKT_E_NULL 8    /* E_NULL   */
#define HQPKKT_E_RANGE 10  /* E_RANGE  */
#define HQPKKT_E_INTERN 17 /* E_INTERN: call order (e.g. factor before analyze) */
#define HQPKKT_E_DEVICE 100 /* HIP runtime error / no gfx950 device */

/* which reference plugin's semantics the handle reproduces */
#define HQPKKT_MODE_FULL 0    /* Hqp_IpSpBKP    (hqp/Hqp_IpSpBKP.C:76-218)    */
#define HQPKKT_MODE_REDUCED 1 /* Hqp_IpRedSpBKP (hqp/Hqp_IpRedSpBKP.C:184-368) */
#define HQPKKT_MODE_STAGED 2  /* Hqp_IpLQDOCP    (hqp/Hqp_IpLQDOCP.C:693-976): multistage (DOCP)
                                 structure, dense per-stage blocks - or, for sparse dynamics, the
                                 row lists of A (hqpkkt_set_dynamics_form) -, see hqpkkt_set_stages */

/* where the vectors z,w,r1..r4,dx..dw (and Qx,Ax,Cx) live */
#define HQPKKT_LOC_HOST 0   /* Meschach VEC::ve pointers; copied H2D / D2H per call */
#define HQPKKT_LOC_DEVICE 1 /* device pointers on opts.device, used in place */
/* Device vectors are read and written by the handle's own (non-blocking) stream: whatever the caller has queued on
 * other streams for these vectors - producers of the inputs, but also writes to the OUTPUT vectors such as clearing
 * them - must be complete before a call; every call returns with its results complete.  hqpkkt_factor / hqpkkt_solve
 * stage the vectors through buffers of the handle on the first call; from the second call in a row with the same
 * pointers (none of them overlapping another) they work on the caller's vectors themselves. */

typedef struct hqpkkt hqpkkt_t;

typedef struct hqpkkt_opts {
  int mode;          /* HQPKKT_MODE_*                                         */
  int device;        /* HIP device ordinal                                    */
  int loc;           /* HQPKKT_LOC_*                                          */
  double tol;        /* mat_tol of the reference (hqp/Hqp_IpSpBKP.C:46,59):
                        Bunch-Kaufman alpha = tol*(1+sqrt 17)/8, 0 < tol <= 1  */
  double eps;        /* mat_eps (hqp/Hqp_IpMatrix.C:45-47): refinement target */
  double pivot_eps;  /* static pivot perturbation, relative to max|K_ij|      */
  int leaf_size;     /* nested-dissection leaf size in rows (0 = default)     */
  int max_pivots;    /* max pivots per supernode, <= 192 (0 = default: 160, and 192 in
                        the chains of separators of >= 768 vertices)            */
  int zd_policy;     /* placement of variables with a structurally zero diagonal
                        (equality multipliers): 2 = behind all their neighbours - the
                        pivot is the complete Schur complement A H^-1 A', all pivots 1x1
                        when the Hessian diagonal is strong (fast); 0 = right behind one
                        matched neighbour, so that a 2x2 pivot with it is available inside
                        the pivot block - what QPs with weak Hessian diagonals need (a
                        state with Q_ii = 1e-4 coupled by 1.0 to a multiplier in an
                        ancestor supernode is otherwise eliminated with a multiplier of
                        1e4: in the last iterations of Prg_DID the residual of a solve is
                        1e-1 instead of 1e-15).  -1 (default) = 2, and where the values say
                        that 0 may be needed (some x with |Q_ii| < 0.01 max_r |A_ri|) the
                        first hqpkkt_solve whose refinement does not reach mat_eps switches
                        the handle to 0 (symbolic phase, upload, values and factorisation
                        once more; mat_sbw does not change) and repeats itself             */
  int slack_policy;  /* FULL mode, order of the slack rows inside a supernode:
                        2 = a slack row in front of one of its own x variables is
                        moved right behind it (default: avoids the run-time
                        interchange the Bunch-Kaufman test makes when w/z is small;
                        ~3 % more fill), 0 = band order as it comes (better when
                        the x variables carry weak diagonals, e.g. DOCP states),
                        1 = behind all x variables of the node (~10 % more fill)  */
  int no_small_fronts; /* 1 = do not use the fused one-wavefront kernels for fronts with
                        <= 32 pivots and <= 16 border rows (tests: both paths must agree) */
  int upd_pingpong_mb; /* update blocks (b x b per supernode) beyond this many MB are not kept for
                        the whole factorisation: tree levels are re-assigned as late as possible
                        and the blocks of even / odd levels alternate between two half-arenas
                        (0 = default 16384, < 0 = never)                                      */
  int amalgamation;  /* 1 = a separator of the nested dissection absorbs its child separators while
                        the merged pivot set still fits a small front (<= 32 pivots, elimination
                        order unchanged).  For narrow bands (a handful of rows per separator) the
                        tree levels above the leaves shrink to a third, and a level costs launch
                        latency there, not arithmetic: +7..10 % interior-point iterations/s on
                        the Prg_DID structure, same iteration counts.  Default 0 (DESIGN.md
                        section 4)                                                              */
  int ordering;      /* elimination tree: 0 = nested dissection of the RCM band (default: banded and
                        multistage systems, mat_sbw wide separators on every level), 1 = nested
                        dissection of the graph itself by breadth-first level structures, for
                        irregular sparsity (discretised / CUTE-style programs, hqp_cute/hqp_cute.tcl:
                        22-46 selects RedSpBKP for them): separators shrink with the piece.  mat_sbw
                        and the RCM permutation are reported as before either way; 2 = as 1 without the
                        reference-faithful RCM pass (hqp/sprcm.C:226-384 re-sorts a level after every
                        parent: quadratic in the level width, seconds for a 10^6-node mesh): mat_sbw
                        and hqpkkt_get_perm then describe a plain reverse Cuthill-McKee numbering       */
} hqpkkt_opts;

typedef struct hqpkkt_stats {
  /* structure (valid after analyze) */
  int dim;               /* order of the factored matrix                       */
  int sbw;               /* mat_sbw: semi-bandwidth under the RCM order        */
  int n_supernodes;
  int n_levels;          /* height of the assembly tree                        */
  int max_front;         /* largest front order (pivots + border)              */
  long long nnz_kkt;     /* stored entries of the permuted upper KKT matrix    */
  long long nnz_factor;  /* entries of L kept (panels), incl. diagonal blocks  */
  long long flops_factor;/* flops of one numeric factorisation as implemented  */
  long long bytes_panels, bytes_updates; /* device arena sizes                 */
  /* last numeric calls (valid after factor / solve) */
  int n_2x2;             /* 2x2 pivots chosen in the last factor               */
  int n_perturbed;       /* pivots replaced by +-pivot_eps*max|K| in last factor */
  int refine_rounds;     /* refinement rounds of the last solve                */
  double kmax;           /* max |scaled K_ij| of the last factor               */
  /* device time of the last call of each phase, HIP events on the handle's
     stream, milliseconds */
  float ms_assemble, ms_factor, ms_step, ms_residual, ms_solve;
  /* one system sharded over several ranks (valid after analyze; hqpkkt_set_shard) */
  int shard_rank, shard_count;
  int n_top;              /* supernodes of the replicated top of the tree          */
  int n_exchange_blocks;  /* subtree roots whose update blocks are all-gathered    */
  long long flops_local, flops_top; /* factor flops of this rank's subtrees / top  */
  long long bytes_exchange_factor;  /* all-gather volume per factor (all slots)    */
  long long bytes_exchange_step;    /* all-gather + all-reduce volume per step     */
  int n_slow_pivots;      /* pivots of the last factor that failed the cheap test
                             |a_kk| >= alpha max|column| and took the complete
                             Bunch-Kaufman decision (k_factor_diag's slow path)   */
  int n_poll_fallbacks;   /* times a launch that spans tree levels gave up waiting for
                             another workgroup's words since the handle was created; it
                             has run on per-level launches from the first one on        */
} hqpkkt_stats;

/* Fill *opts with the defaults (mode FULL, device 0, host pointers, tol 1.0,
 * eps 1e-10 as the reference's constructors set them). */
int hqpkkt_default_opts(hqpkkt_opts *opts);

/* ctor / dtor of the plugin object (Hqp_IpSpBKP::Hqp_IpSpBKP, ~Hqp_IpSpBKP,
 * hqp/Hqp_IpSpBKP.C:43-73).  Host-only; no device is touched yet. */
int hqpkkt_create(const hqpkkt_opts *opts, hqpkkt_t **out);
int hqpkkt_destroy(hqpkkt_t *h);

/* Hqp_IpSpBKP::init / Hqp_IpRedSpBKP::init, structure part
 * (hqp/Hqp_IpSpBKP.C:76-114, hqp/Hqp_IpRedSpBKP.C:184-265): RCM ordering of the
 * KKT graph (hqp/sprcm.C:62-420), semi-bandwidth, supernode partition and
 * symbolic factorisation.  Q is n x n (only entries with col >= row are read,
 * meschach/addon2_hqp.c:1078-1086), A is me x n, C is m x n.  Host pointers
 * always.  Host-only: runs without a GPU.  *sbw receives mat_sbw. */
int hqpkkt_analyze(hqpkkt_t *h, int n, int me, int m,
                   const int *Qp, const int *Qi, const int *Ap, const int *Ai,
                   const int *Cp, const int *Ci, int *sbw);

/* Hqp_IpSpBKP::update / Hqp_IpRedSpBKP::update (hqp/Hqp_IpSpBKP.C:117-136,
 * hqp/Hqp_IpRedSpBKP.C:268-278): new values on the analysed pattern.  Pointers
 * per opts.loc.  First call uploads the symbolic structure to the device. */
int hqpkkt_set_values(hqpkkt_t *h, const double *Qx, const double *Ax,
                      const double *Cx);

/* Pinned host buffers of the handle for the three value arrays (after hqpkkt_analyze; nnz(Q), nnz(A),
 * nnz(C) doubles; they live until the next hqpkkt_analyze / hqpkkt_destroy).  A host whose matrices are
 * row lists (Meschach SPMAT: one heap array per row) writes the values of an update() straight into
 * them - several threads, no intermediate copy - and passes the same pointers to hqpkkt_set_values:
 * the transfer is then ONE DMA per block from page-locked memory (opts.loc = HQPKKT_LOC_HOST).  The
 * shim does this when the pattern is unchanged (the reference's PARDISO plugin re-walks its matrices per
 * update as well, hqp/Hqp_IpPARDISO.C:240-330). */
int hqpkkt_values_staging(hqpkkt_t *h, double **Qx, double **Ax, double **Cx);

/* Hqp_IpSpBKP::factor / Hqp_IpRedSpBKP::factor (hqp/Hqp_IpSpBKP.C:139-180,
 * hqp/Hqp_IpRedSpBKP.C:281-320) including spBKPfactor (hqp/spBKP.C:369-645):
 * insert w/z (resp. C'ZW^-1C), symmetric scaling, LDL' with 1x1/2x2 pivots.
 * HQPKKT_E_SING: an exactly zero pivot (hqp/spBKP.C:699-700, 731-732) in a root
 * front or on a variable without a diagonal of its own (equality multiplier, x
 * without Q_ii).  An exactly zero pivot elsewhere is perturbed (the pivot search
 * ends at the supernode, the rest of the column is still to come); hqpkkt_solve
 * then returns HQPKKT_E_SING if its refinement does not reach opts.eps. */
int hqpkkt_factor(hqpkkt_t *h, const double *z, const double *w);

/* Hqp_IpSpBKP::step / Hqp_IpRedSpBKP::step (hqp/Hqp_IpSpBKP.C:183-218,
 * hqp/Hqp_IpRedSpBKP.C:323-368) including spBKPsolve (hqp/spBKP.C:647-797):
 * one solve of  [-Q A' C' 0; A 0 0 0; C 0 0 -I; 0 0 W Z] d = r  with the
 * current factors, no refinement.  FULL mode: dw = C dx - r3 as the reference
 * computes it, except for active constraints (w_j < z_j), whose dw_j comes from
 * z_j dw_j + w_j dz_j = r4_j - the same number, to a relative accuracy. */
int hqpkkt_step(hqpkkt_t *h, const double *z, const double *w,
                const double *r1, const double *r2, const double *r3,
                const double *r4, double *dx, double *dy, double *dz,
                double *dw);

/* Hqp_IpMatrix::residuum (hqp/Hqp_IpMatrix.C:131-178): max inf-norm of the
 * four block residuals of the unreduced system; the residual vectors stay on
 * the device for the next refinement round. */
int hqpkkt_residual(hqpkkt_t *h, const double *z, const double *w,
                    const double *r1, const double *r2, const double *r3,
                    const double *r4, const double *dx, const double *dy,
                    const double *dz, const double *dw, double *res);

/* Hqp_IpMatrix::solve (hqp/Hqp_IpMatrix.C:65-128): step, then at most five
 * rounds of iterative refinement with the reference's back-off
 * (alpha = 1, .7, .4, .1) while the residual exceeds opts.eps.  *res is the
 * value the reference's solve() returns. */
int hqpkkt_solve(hqpkkt_t *h, const double *z, const double *w,
                 const double *r1, const double *r2, const double *r3,
                 const double *r4, double *dx, double *dy, double *dz,
                 double *dw, double *res);

/* mat_sbw (hqp/Hqp_IpSpBKP.C:58) and _QP2J (hqp/Hqp_IpSpBKP.C:91-93):
 * perm[qp_index] = position in the RCM order; dim entries. */
int hqpkkt_get_sbw(const hqpkkt_t *h, int *sbw);
int hqpkkt_get_perm(const hqpkkt_t *h, int *perm);

/* mat_tol / mat_eps setters (Tcl-visible members of the reference plugin,
 * hqp/Hqp_IpSpBKP.C:58-59, hqp/Hqp_IpMatrix.C:47) */
int hqpkkt_set_tol(hqpkkt_t *h, double tol);
int hqpkkt_set_eps(hqpkkt_t *h, double eps);

/* Run the handle's kernels on a caller-provided hipStream_t (NULL = the
 * handle's own stream). */
int hqpkkt_set_stream(hqpkkt_t *h, void *hip_stream);

int hqpkkt_get_stats(const hqpkkt_t *h, hqpkkt_stats *out);

/* ---- one system over several GPUs (nested-dissection / SPIKE cut
 * of the RCM band; the reference's spBKPfactor, hqp/spBKP.C:369-645, is
 * sequential and has no counterpart) ------------------------------------------
 * Every rank holds one handle on its own device and makes the same calls with
 * the same (replicated) arguments.  The symbolic phase splits the assembly tree:
 * the top (the outermost separators) is replicated, the subtrees below it are
 * dealt to the ranks.  Each factor needs ONE all-gather (the update blocks of the
 * subtree roots), each step one all-gather (their contribution vectors) and one
 * all-reduce (the solution in elimination order).  The library does not link a
 * communication library: it calls back into the host, after draining the
 * handle's stream, and continues when the callback returns -- the callback must
 * not return before the result is complete in `buf` (device memory on the
 * handle's device).  With torch.distributed (backend "nccl" = RCCL over xGMI)
 * this is hqp_amd.dist.make_exchange(); a C++ host passes a function that calls
 * ncclAllGather / ncclAllReduce on its communicator.
 *   op HQPKKT_XCHG_ALLGATHER:     buf holds nslots slots of slot_elems doubles,
 *                                 slot `rank` is filled; fill all of them.
 *   op HQPKKT_XCHG_ALLREDUCE_SUM: buf holds slot_elems doubles (nslots = 1);
 *                                 replace them by the sum over the ranks.
 * Returns 0 on success.  Call hqpkkt_set_shard before hqpkkt_analyze. */
#define HQPKKT_XCHG_ALLGATHER 0
#define HQPKKT_XCHG_ALLREDUCE_SUM 1
/* op HQPKKT_XCHG_BCAST_BASE + r (r = 0 .. nranks-1): buf holds slot_elems doubles that rank r has
 * filled (nslots = 1); bring them to every rank.  The STAGED engine gathers the strips of V_k this way
 * when their sizes differ much (one broadcast per rank, issued back to back: hqpkkt_rccl_exchange
 * puts them into one ncclGroup) instead of padding every strip to the largest. */
#define HQPKKT_XCHG_BCAST_BASE 16
typedef int (*hqpkkt_exchange_fn)(void *ctx, int op, double *buf, long long slot_elems, int nslots);
int hqpkkt_set_shard(hqpkkt_t *h, int rank, int count, hqpkkt_exchange_fn fn, void *ctx);
/* The stream-ordered form of the same hook: the callback puts the collective into `hip_stream` (the
 * handle's stream, behind the kernels that fill `buf`) and returns at once; nothing is drained, the
 * kernels that follow wait in the stream.  hqpkkt_rccl_exchange of libhqpkkt_rccl.so
 * (include/hqpkkt_rccl.h: ncclAllGather / ncclAllReduce of RCCL over xGMI) has this signature.
 * STAGED mode over several ranks: the state columns of every stage are cut into one range per rank
 * and the memory goes with them - a rank keeps its columns of every F_k (every rank is handed the
 * same blocks and copies its share) and its rows of every V_k: bytes_panels per rank <= 1 / P of the
 * single-rank figure + 10 %.  Per stage of a factorisation: W_p = V+ F_p (local), the gather of the
 * ranks' F blocks (static data, requested a stage ahead), the blocks of G_xx = F'V+F dealt out in a
 * ring and computed as W_p' F_q, ONE gather of those blocks (n^2/2 doubles in all) on the critical
 * path, V_k = G_xx - Y'Rm by every rank; the control-sized work is done by every rank on identical
 * data.  The solve gathers one state-sized vector per stage and direction.  Needs an even number of
 * states per stage. */
typedef int (*hqpkkt_exchange_stream_fn)(void *ctx, int op, double *buf, long long slot_elems, int nslots,
                                         void *hip_stream);
int hqpkkt_set_shard_stream(hqpkkt_t *h, int rank, int count, hqpkkt_exchange_stream_fn fn, void *ctx);

/* ---- STAGED mode (Hqp_IpLQDOCP, hqp/Hqp_IpLQDOCP.C) ---------------------------------
 * The QP of a discrete-time optimal control problem as Hqp_Docp::setup_qp lays it out
 * (hqp/Hqp_Docp.C:585-755): x = [x_0, u_0, x_1, u_1, ..., x_K]; the first rows of A are the
 * dynamics  fx_k x_k + fu_k u_k - x_{k+1}  (the -1.0 is the last entry of each row), the
 * other equality rows, all rows of C and all rows of Q stay inside one stage.  The engine
 * keeps fx, fu and the cost-to-go Hessians as dense blocks and runs the reference's extended
 * Riccati recursion (ExRiccatiFactorSc / ExRiccatiSolveSc, :1794-2182) as fp64 MFMA matrix
 * products over them; the equality constraints of a stage are eliminated with the controls
 * they determine and carried back to the previous stage otherwise (GE_QP's job,
 * meschach/addon_hqp.c:399-475), a fixed initial state is recognised as in
 * Check_Structure (:343-351).  hqpkkt_analyze finds the stage sizes from the staircase
 * of A exactly as Hqp_IpLQDOCP::Get_Dim does (:201-287) unless hqpkkt_set_stages has given
 * them (K stages, nx[K+1] states, nu[K] controls; K <= 0 returns to the detection);
 * HQPKKT_E_FORMAT: the pattern / the values are not such a staircase (the reference
 * asserts), HQPKKT_E_SIZES: a stage with more than 512 controls, more than 256 constraint rows
 * carried from one stage to the one before it, or a FREE initial state with more than 4096 components
 * + carried rows (a fixed x_0 has no limit).  Up to ~64 controls and ~130 for the order of a stage's
 * [G_uu N_u'; N_u 0] the control-sized work of a stage runs in the LDS of one CU; beyond that the same
 * elimination runs out of global memory (one workgroup: correct and slow, ~20 ms per stage at 300
 * controls).  mat_sbw is -1. */
int hqpkkt_set_stages(hqpkkt_t *h, int K, const int *nx, const int *nu);
/* The form of the stage products with the dynamics F_k = [fx_k fu_k] - Hqp_IpLQDOCP's interface variable mat_a_sparse
 * (hqp/Hqp_IpLQDOCP.C:178; FormGxxSp / FormGxSp, :1119-1273).  HQPKKT_DYN_DENSE (default): the dynamics rows of A are
 * scattered into dense blocks and every stage runs W = V+ F, G = F'W as fp64 MFMA products.  HQPKKT_DYN_SPARSE: F_k stays
 * the row lists of A and A' the handle holds anyway; T = F'V+ and G = T F walk them (two flops per stored entry and row
 * element, no F arena: hqpkkt_stats.bytes_panels shrinks by it), as do the solve's two products with F_k; everything
 * control-sized and the rank-q update of V_k are unchanged.  Host-only; call it before hqpkkt_analyze, like
 * hqpkkt_set_stages: the form holds until it is set again and the next hqpkkt_analyze picks it up.  HQPKKT_E_RANGE: unknown
 * form; HQPKKT_E_INTERN: the handle's mode is not STAGED.  With HQPKKT_DYN_SPARSE set hqpkkt_analyze_staged (the dense
 * hand-over) returns HQPKKT_E_INTERN, and hqpkkt_analyze on a handle with hqpkkt_set_shard / hqpkkt_set_shard_stream
 * returns HQPKKT_E_RANGE: one system over several ranks stays dense.  There is no automatic choice between the two forms;
 * the sparse form pays while a column of F_k holds few entries against the number of states (DESIGN.md section 3 has the
 * measured times), and a few full columns among them can be taken out of the walks (hqpkkt_set_dense_columns).
 * HQPKKT_DYN_PROFILE: for banded and block-banded dynamics.  F_k is stored as in the dense form (same arena, same
 * hqpkkt_stats.bytes_panels); the analysis records per stage and per 128-column panel of F_k the range of 16-row k-slabs
 * that holds the panel's stored entries, and a stage with at least two panels and a range shorter than all slabs runs
 * its two large MFMA products W = V+ F and G = F'W, and the solve's two products with F_k, over those slabs alone; every
 * other stage runs the dense sequence and gives the dense form's bits.  The rules of HQPKKT_DYN_SPARSE hold:
 * hqpkkt_analyze_staged returns HQPKKT_E_INTERN, a sharded handle HQPKKT_E_RANGE at hqpkkt_analyze;
 * hqpkkt_set_dense_columns is accepted and ignored.  No form is chosen automatically.
 * Where the arena of dense blocks does not fit the device (hqpkkt_stats.bytes_panels; a band of 50 under 5000 states
 * is almost all zeros), set the sparse form for dynamics of a few entries per column, and HQPKKT_DYN_PROFILE with
 * hqpkkt_set_packed_panels for banded and block-banded ones. */
#define HQPKKT_DYN_DENSE 0   /* default: dense blocks F_k, MFMA products           */
#define HQPKKT_DYN_SPARSE 1  /* Hqp_IpLQDOCP's mat_a_sparse: F_k stays row lists   */
#define HQPKKT_DYN_PROFILE 3 /* dense blocks F_k, products over the panels' k-slabs (2 is not a form: HQPKKT_E_RANGE) */
int hqpkkt_set_dynamics_form(hqpkkt_t *h, int form);
/* Packed panels of the profile form.  With on = 1 a stage that runs the profile sequence stores F_k panel by panel
 * instead of as a dense block: panel p holds the rows [16 lo_p, min(16 hi_p, n_{k+1})) of its 128 columns, row-major with
 * leading dimension 128 (the last panel: its columns rounded up to 8), the panels back to back, an empty one taking no
 * room, the stage's total rounded up to 16 doubles.  hqpkkt_stats.bytes_panels shrinks accordingly - never grows - and
 * the stage runs the same launches by the same work lists with the panels addressed through a table, the carried rows
 * N = B+ F over the ranges alone (k_pk_carried).  Every other stage keeps its dense block.  Host only; call it before
 * hqpkkt_analyze; it holds until set again.  It has an effect only together with HQPKKT_DYN_PROFILE and is accepted and
 * ignored on any other form; the profile form's rules stand (no dense hand-over, no sharded handle).  0 (default): the
 * arena, launches and bits of a handle that never asked.  HQPKKT_E_NULL; HQPKKT_E_INTERN: not a STAGED handle;
 * HQPKKT_E_RANGE: on is neither 0 nor 1.  hqpkkt_debug_get 42 reports the layout. */
int hqpkkt_set_packed_panels(hqpkkt_t *h, int on);
/* Heavy columns of the sparse form.  Its column walks give one lane one column of F_k, so a stage takes as long as its
 * longest column: a dense control column or a global state among banded ones costs a serial loop over every state.  With
 * min_entries = n > 0 a column of F_k that holds at least n stored entries in its stage's dynamics rows is "heavy": the
 * heavy columns of a stage are kept as a small dense block D_k (n_{k+1} rows of up8(columns) doubles in the F arena,
 * hqpkkt_stats.bytes_panels counts it) and go through the fp64 MFMA product as thin products (V+ D_k, D_k'V+ D_k, B+ D_k),
 * all other columns stay on the walks; in the solve a wavefront takes each heavy column.  0 (default): none, the sparse
 * form as it was.  -1: the library's threshold (32 entries; DESIGN.md section 3 has the measurements).  Heaviness is a
 * property of the pattern, decided per stage at the analysis; a stage without heavy columns runs the launches it always has.
 * The choice between the dense and the sparse form stays the caller's.  Host-only; call it before hqpkkt_analyze, like
 * hqpkkt_set_dynamics_form: it holds until set again and the next hqpkkt_analyze picks it up.  It has an effect only
 * together with HQPKKT_DYN_SPARSE: on a dense-form handle it is accepted and ignored.  HQPKKT_E_INTERN: the handle's mode
 * is not STAGED; HQPKKT_E_RANGE: min_entries < -1. */
int hqpkkt_set_dense_columns(hqpkkt_t *h, int min_entries);
/* Wide rows of the inequality block C.  H_k = Q_k + C_k'(Z/W)C_k is assembled from term lists in which a row of C with L
 * stored entries holds L^2 terms (24 bytes each at the analysis, 12 on the device): right for bound rows, out of reach for
 * an output constraint over every state, a sum over the states of a discretised PDE or a polytopic terminal set.  With
 * min_entries = n > 0 a row of C with at least n stored entries is "wide" (rows of C stay inside one stage; the terminal
 * stage K counts): the r_k wide rows of stage k leave the term lists and are kept as a dense block E_k - r_k rows of
 * up8(n_k + m_k) doubles in the F arena (stage K: up8(n_K)), hqpkkt_stats.bytes_panels counts it - and every factorisation
 * adds S'S with S = diag(sqrt(z / w)) E_k into the stage's work block as ONE fp64 MFMA product of depth r_k: one pass over
 * the block, whatever r_k L^2 is.  The square root goes into both operands, so V_k stays bit-for-bit symmetric; it asks for
 * z / w > 0, which an interior-point iterate gives.  The vector work of the wide rows goes through the blocks too:
 * hqpkkt_step / hqpkkt_solve form q = C'tz - r1, dz and dw, and hqpkkt_residual (with the solve's refinement) forms C dx
 * and C'dz, with the wide rows' share from two streaming kernels over E_k - a wavefront per wide row with 16-byte loads,
 * and a thread per pair of columns for the transposed product; one launch over all stages each, sums in a fixed order -,
 * while the CSR walks of these products take narrow copies of C and C' that do not hold the wide rows.  The
 * interior-point loops' own right-hand-side kernels walk the whole of C as before; the solves they call take the
 * blocks.  hqpkkt_debug_get 46 reports the split.  A stage with wide rows runs its control-sized chain on the
 * first stream and forms V_k by the separate update; every other stage runs exactly the launches it always has.
 * 0 (default): none - the plan, arenas, launches and bits of a handle that never asked.  -1, the library's threshold: no
 * threshold has been measured yet, HQPKKT_E_RANGE.  Host only; call it before hqpkkt_analyze or
 * hqpkkt_analyze_staged; it holds until it is set again.  It works with every form of the dynamics.  On a handle with
 * hqpkkt_set_shard / hqpkkt_set_shard_stream it is accepted and ignored: such a handle keeps its term lists.
 * Whatever the setting, an analysis whose term lists would hold more than 2^31 - 1 terms returns HQPKKT_E_SIZES (the lists
 * are indexed by ints; one row of 46 341 entries is enough).  HQPKKT_E_NULL; HQPKKT_E_INTERN: the handle's mode is not
 * STAGED; HQPKKT_E_RANGE: min_entries < -1.  hqpkkt_debug_get 43 reports the rows and the term counts. */
int hqpkkt_set_dense_rows(hqpkkt_t *h, int min_entries);
/* The stage Hessians Q_k as dense blocks.  With HQPKKT_HESS_CSR every stored entry of Q becomes entries of the H term
 * lists: right for a diagonal or banded Q, out of reach for the dense (n_k + m_k)^2 block per stage that a block-BFGS
 * update hands over (hqp/Hqp_HL_BFGS.C:150-248; Hqp_IpLQDOCP extracts exactly these blocks, hqp/Hqp_IpLQDOCP.C:1084-1105).
 * With HQPKKT_HESS_DENSE block k = 0 .. K of order nz_k = n_k + m_k (stage K: n_K) is kept row-major with leading
 * dimension up8(nz_k), in full, exactly symmetric, zero padded, in an arena of its own that hqpkkt_stats.bytes_panels
 * counts (+ sum of nz_k up8(nz_k) 8 bytes).  Q's terms leave the H lists (those of C'(Z/W)C stay); every factorisation adds
 * the block into the stage's work block by a streaming kernel, Q first, then the lists; the products Q x of
 * hqpkkt_residual, of hqpkkt_solve's refinement and of the interior-point loops run over the blocks in one launch with a
 * fixed order of the sums.
 *   CSR hand-over (hqpkkt_analyze + hqpkkt_set_values): Q is given as always - only col >= row is read, rows stay inside
 *   their stage - and every hqpkkt_set_values scatters its values into the blocks, an off-diagonal entry to both of its
 *   places; what the pattern does not hold stays zero.
 *   Dense hand-over (hqpkkt_analyze_staged): Qp / Qi are ignored and may be NULL; block k comes through
 *   hqpkkt_set_stage_hessian - nz_k rows of ldQ >= nz_k doubles, pointer per opts.loc, of which only the entries j >= i are
 *   read (the strict lower triangle and the columns behind nz_k are the caller's) -, asynchronously in the handle's
 *   stream; a host block may come out of the hqpkkt_stage_staging buffers.  hqpkkt_set_values_staged with Qx = NULL ends the
 *   hand-over: HQPKKT_E_INTERN unless every Hessian block has been set since the analysis.  On the CSR hand-over
 *   hqpkkt_set_stage_hessian returns HQPKKT_E_INTERN.
 * Host only; call hqpkkt_set_hessian_form before the analysis; it holds until it is set again.  It works with every form
 * of the dynamics and with hqpkkt_set_dense_rows.  On a handle with hqpkkt_set_shard / hqpkkt_set_shard_stream the analysis
 * returns HQPKKT_E_RANGE, as for the sparse form.  HQPKKT_HESS_CSR (default) is the plan, arenas, launches and bits of a
 * handle that never asked.  HQPKKT_E_NULL; HQPKKT_E_INTERN: the handle's mode is not STAGED; HQPKKT_E_RANGE: unknown form.
 * hqpkkt_debug_get 45 reports the layout. */
#define HQPKKT_HESS_CSR 0   /* default: term lists */
#define HQPKKT_HESS_DENSE 1 /* Q_k kept as a dense block per stage 0 .. K */
int hqpkkt_set_hessian_form(hqpkkt_t *h, int form);
int hqpkkt_set_stage_hessian(hqpkkt_t *h, int k, const double *Q, long long ldQ);
/* tests: block k of the dense Hessians as it lies in the arena (nz_k rows of up8(nz_k) doubles; of a stage stored as packed
 * tiles the same view, unpacked); out null: *len alone */
int hqpkkt_debug_stage_hessian(hqpkkt_t *h, int k, double *out, long long cap, long long *len);
/* tests: y = Q x over all stage blocks by the kernels of the handle's residual; x, y host arrays of n */
int hqpkkt_debug_hess_symv(hqpkkt_t *h, const double *x, double *y);
/* tests and measurement: the average device time in ms, by HIP events on the handle's stream, of `reps` (>= 1:
 * HQPKKT_E_RANGE otherwise) products Q x as the residual launches them, one untimed product ahead; x, y host arrays of n,
 * y the product; on packed and unpacked handles alike */
int hqpkkt_debug_hess_symv_timed(hqpkkt_t *h, const double *x, double *y, int reps, double *ms);
/* The dense stage Hessians stored as packed lower tiles.  hqpkkt_set_hessian_form(HQPKKT_HESS_DENSE) keeps both triangles of
 * every Q_k although the caller hands over the entries j >= i alone; with on = 1 a stage keeps of its block the tiles (a, b),
 * b <= a < nt = ceil(nz_k / 128), of edge T = 128 - the tile of the stage products -, each T rows of T doubles, row-major,
 * zero padded past nz_k, back to back in the order a (a + 1) / 2 + b; a diagonal tile holds both of its triangles, bit for
 * bit symmetric.  A stage is packed only where that is smaller, nt (nt + 1) / 2 T^2 < nz_k up8(nz_k); every other stage
 * keeps its dense block exactly as without the call, so hqpkkt_stats.bytes_panels never grows.  The rule is not monotone in
 * nz_k: the orders 220 .. 256 pack (three tiles), 257 .. 312 do not, 313 is the first order of three tile rows that packs,
 * 384 packs, 385 does not, 402 does; a block of order 5050 takes 0.526 of its dense arena, large ones tend to one
 * half.  Every user of the blocks works from the tiles: the dense hand-over packs the
 * caller's block (of a host block only the rows' columns from the first column of their group of 64 rows on are moved,
 * about nz_k (nz_k + 64) / 2 doubles, through one device staging block of the largest packed stage's size;
 * hqpkkt_stage_staging keeps its size and meaning), the CSR hand-over scatters to the packed places, the factorisation
 * adds the tiles and, where the dense form adds an upper tile, their transposes - every entry of the work block receives
 * the one add of the value the dense form adds, so factor and step are bit-identical to the unpacked dense form -, and
 * the products Q x load every stored element once for its row's and its column's sum, with a scratch of a little over nt^2 / 2
 * slots of T doubles per packed stage and a fixed order of the sums (not the order of the unpacked form: the products agree to rounding).
 * Host only; call it before the analysis; it holds until it is set again.  It has an effect together with
 * HQPKKT_HESS_DENSE alone: with HQPKKT_HESS_CSR it is accepted and ignored.  0 (default) is the plan, arenas, launches and
 * bits of a handle that never asked.  HQPKKT_E_NULL; HQPKKT_E_INTERN: the handle's mode is not STAGED; HQPKKT_E_RANGE: on is
 * neither 0 nor 1.  hqpkkt_debug_get 47 reports the layout; 45 keeps reporting the order and up8(order), and
 * hqpkkt_debug_stage_hessian returns the unpacked view of a packed stage. */
int hqpkkt_set_packed_hessians(hqpkkt_t *h, int on);
/* The dense stage Hessians updated in place on the device.  A block-BFGS caller changes every Q_k a little in every SQP
 * iteration (hqp/Hqp_HL_BFGS.C:150-248: Q - Qs (Qs)'/s'Qs + v v'/s'v, block by block); without this entry the change reaches
 * the engine only as a new hand-over of every block.  hqpkkt_update_stage_hessians applies to every stage k = 0 .. K
 *     Q_k <- beta_k Q_k + diag(d_k) + sum_{j < r} c_kj u_jk u_jk'
 * where u_jk and d_k are the entries of U[j] and diag that belong to the variables of stage k - the contiguous range the
 * block covers, [x_k, u_k], x_K for stage K.  U[j] and diag hold n doubles, pointers per opts.loc; coef ((K + 1) r doubles,
 * coef[k r + j] = c_kj), beta (K + 1 doubles, or NULL: all 1.0) and the array U itself are HOST arrays; diag NULL: none.
 * It works on both layouts of the blocks, the dense block (both triangles) and the packed lower tiles (the stored tiles), in
 * one launch over all stages (staged_hess_update.hip.h): one read and one write of the arena.
 *   Values.  The value written to (i, j) is a function of Q_ij, beta_k, d_i (i = j only), the c_kj and the ROUNDED products
 *   fl(u_i u_j), evaluated in the fixed order scale, diagonal, terms 0 .. r - 1, every step rounded once (a term is one
 *   fused multiply-add of c_kj and the rounded product).  fl(u_i u_j) does not depend on the order of its factors: a dense
 *   block and a diagonal tile stay symmetric bit for bit, and a packed and an unpacked handle given the same update hold
 *   bit-identical blocks (hqpkkt_debug_stage_hessian).
 *   Skips.  beta_k == 1 exactly: no scaling.  beta_k == 0 exactly: the block is not read - what it held, NaN included, does
 *   not enter.  A term with c_kj == 0 exactly is skipped for that stage: its vector's entries, NaN or Inf included, do not
 *   enter.  A stage with beta_k == 1, every c_kj == 0 and diag == NULL is not touched at all (the reference leaves a block
 *   alone when s'v or s'Qs is zero).
 *   Padding stays +0.0: the columns [nz_k, up8(nz_k)) of a dense block, the rows and columns past nz_k of a packed tile.
 *   Vector entries past the stage's order belong to the next stage: they count as 0 and are never read as values.
 *   Hand-over.  beta_k == 0 counts as the arrival of block k for hqpkkt_set_values_staged's rule, so a caller can create
 *   every Hessian on the device - diag alone for a scaled identity or a restart - and never hand over a block.  beta_k != 0
 *   on a stage the call touches whose block has not arrived since the analysis returns HQPKKT_E_INTERN.
 *   Checks, all before anything is launched (a call applies to every stage or to none): HQPKKT_E_NULL - h or u null, r > 0
 *   with U, U[j] or coef null; HQPKKT_E_RANGE - r outside 0 .. HQPKKT_HESS_UPDATE_RANK, a beta or a coefficient that is not
 *   finite; HQPKKT_E_INTERN - the handle is not STAGED, not analysed, not HQPKKT_HESS_DENSE, or analysed for the CSR hand-over
 *   (whose hqpkkt_set_values rewrites the blocks anyway: the rule of hqpkkt_set_stage_hessian), or the hand-over rule above;
 *   then, without a gfx950 device, HQPKKT_E_DEVICE.
 *   After the call h is not factored (as after hqpkkt_set_stage_hessian); the dynamics and their hand-over state are left
 *   alone, and a later hqpkkt_set_values_staged(Qx = NULL, ..) keeps the updated blocks.
 *   Host vectors are copied through buffers the handle owns (made by the first call, outside any capture), and the call
 *   returns when the stream has read them.  Device vectors are read asynchronously in the handle's stream: the caller keeps
 *   them alive and unchanged until the stream has passed the update.  coef and beta are read before the call returns.
 * The reference's eigenvalue control and the row maxima of restart_Q, which read the blocks, are the entries behind
 * hqpkkt_bfgs_report: hqpkkt_eigen_control_stage_hessians and hqpkkt_restart_stage_hessians.
 * hqpkkt_hessian_product: y = Q x over all stage blocks, x and y of n doubles, pointers per opts.loc, by the launches of
 * the handle's residual - the public form of hqpkkt_debug_hess_symv and the same bits; on any uploaded HQPKKT_HESS_DENSE
 * handle, either hand-over (HQPKKT_E_INTERN otherwise); the result is complete when it returns.  It gives a BFGS caller
 * Q s without a host copy of Q. */
#define HQPKKT_HESS_UPDATE_RANK 4
typedef struct hqpkkt_hess_update {
  int r;                  /* 0 .. HQPKKT_HESS_UPDATE_RANK terms */
  const double *const *U; /* host array of r pointers; U[j]: n doubles, pointer per opts.loc */
  const double *coef;     /* HOST array, (K + 1) * r doubles: coef[k * r + j] = c_kj */
  const double *beta;     /* HOST array of K + 1 doubles, or NULL = all 1.0 */
  const double *diag;     /* n doubles, pointer per opts.loc, or NULL = none */
} hqpkkt_hess_update;
int hqpkkt_update_stage_hessians(hqpkkt_t *h, const hqpkkt_hess_update *u);
int hqpkkt_hessian_product(hqpkkt_t *h, const double *x, double *y);
/* The reference's damped BFGS update of every dense stage Hessian (Hqp_HL_BFGS::update_b_Q, hqp/Hqp_HL_BFGS.C:150-248,
 * without its eigenvalue control) with nothing of it on the host: the step between hqpkkt_hessian_product and
 * hqpkkt_update_stage_hessians - the scalars s'y and s'Qs, Powell's test, the vector v, the two coefficients - runs on the
 * device too, so a caller whose s and y live there never leaves it.  Per stage k = 0 .. K, over the stage's variables:
 *     sy = s'y,  sQs = s'(Q s);  damped where sy < gamma_eff sQs:
 *         theta = (1 - gamma_eff) sQs / (sQs - sy),  v = theta y + (1 - theta) Q s,  sv = s'v;   otherwise v = y, sv = sy
 *     Q_k <- Q_k + v v' / sv - (Q s)(Q s)' / sQs
 * s, y and v (optional: v as applied, y where a stage is not damped) hold n doubles, pointers per opts.loc.  gamma is the
 * reference's sqp_hela_gamma: gamma >= 0 is the damping factor gamma_eff itself, gamma < 0 adapts it to the step length,
 * gamma_eff = g + (1 - g)(1 - alpha) with g = -gamma; alpha is read only then.  gamma_eff is formed on the host.
 *   Launches, all in the handle's stream, on both layouts of the blocks: Q s by the launches of hqpkkt_hessian_product
 *   into a buffer of this entry (not the residual's); k_hb_terms (staged_hess_bfgs.hip.h), one workgroup per stage, which
 *   writes v, the coefficients c0 = 1 / sv, c1 = -1 / sQs and the skips into the device descriptors of the update launch;
 *   then the launch of hqpkkt_update_stage_hessians, unchanged, with U = [v, Q s], r = 2, beta = 1, no diagonal: the bits of
 *   Q+ are those that entry gives for the same v, Q s, c0 and c1.
 *   Values.  The sums run in an order fixed by the stage's order alone (a thread's entries t, t + 256, .. by fused
 *   multiply-adds, the 64 lanes of a wavefront by a butterfly, the four wavefronts in their order): the same bits from run to
 *   run and on a packed and an unpacked handle given the same Q s.  The test, theta, 1 - theta, every v_i = fl(fl(theta y_i)
 *   + fl((1 - theta) (Qs)_i)) and the reciprocals are single operations, each rounded once: hessian_update.bfgs_replay
 *   repeats them in numpy from the reported sums.
 *   Skips.  A stage whose sv or sQs is zero is left alone, as in the reference (a stage of order 0 counts as such).  A stage
 *   whose sv or sQs is not finite is left alone too: that follows hessian_update.bfgs_terms, NOT the reference, which
 *   would write NaN into the block.  Entries past a stage's order belong to the next stage and are never read as values:
 *   a NaN in one stage's y reaches no other stage.
 *   Checks, all before anything is launched (a call applies to every stage or to none): HQPKKT_E_NULL - h, b, b->s or b->y
 *   null; HQPKKT_E_RANGE - gamma not finite, or gamma < 0 with an alpha that is not finite; HQPKKT_E_INTERN - the handle is
 *   not STAGED, not analysed, not HQPKKT_HESS_DENSE or analysed for the CSR hand-over, or a block of nonzero order has not
 *   arrived since the analysis (the hand-over rule of hqpkkt_update_stage_hessians with beta = 1 on every stage); then,
 *   without a gfx950 device, HQPKKT_E_DEVICE.
 *   Host vectors are copied through buffers the handle owns, v is copied back, and the call returns when the stream is
 *   done.  Device vectors: nothing is read back, the call waits for nothing but the descriptor words of the call before
 *   it, and returns with the work enqueued; the caller keeps s, y and v alive and unchanged until the stream has passed,
 *   and v overlaps neither s nor y.  All buffers are made by the first call, outside any capture.
 *   After the call h is not factored; the dynamics and the hand-over state are left alone.
 * hqpkkt_bfgs_report waits for the stream and copies out what k_hb_terms left of the last update, HQPKKT_BFGS_REPORT doubles
 * per stage: 0 sy; 1 sQs; 2 gamma_eff; 3 theta (1.0 where not damped); 4 sv as used (s'v after damping, else sy); 5 c0;
 * 6 c1 (both 0.0 where the stage was left alone); 7 the outcome - 0 updated without damping, 1 updated with damping, 2 left
 * alone because sv or sQs is zero, 3 left alone because sv or sQs is not finite.  HQPKKT_E_NULL; HQPKKT_E_INTERN before
 * the first update since the analysis.
 * The reference's eigenvalue control and restart_Q follow as entries of their own (hqpkkt_eigen_control_stage_hessians,
 * hqpkkt_restart_stage_hessians); a caller runs the control behind this update in the same stream. */
typedef struct hqpkkt_bfgs_update {
  const double *s; /* n doubles, pointer per opts.loc: the step */
  const double *y; /* n doubles, pointer per opts.loc: change of the Lagrangian's gradient */
  double gamma;    /* the reference's sqp_hela_gamma: >= 0 standard damping, < 0 adapted to alpha */
  double alpha;    /* step length; read only when gamma < 0 */
  double *v;       /* optional, n doubles per opts.loc: the vector v as applied (y where no damping) */
} hqpkkt_bfgs_update;
int hqpkkt_bfgs_update_stage_hessians(hqpkkt_t *h, const hqpkkt_bfgs_update *b);
#define HQPKKT_BFGS_REPORT 8
int hqpkkt_bfgs_report(hqpkkt_t *h, double *out /* HOST, (K + 1) * 8 doubles */);
/* The safeguards of a block-BFGS caller on the device: the parts of the reference that READ a block Q_k - restart_Q
 * (hqp/Hqp_HL_BFGS.C:125-146), Hqp_HL_Gerschgorin::update (hqp/Hqp_HL_Gerschgorin.C:66-106) and the eigenvalue control of
 * Hqp_HL_BFGS::update_b_Q (:203-212, on by default there) - so that such a caller never reads a block back.  All of them
 * work on HQPKKT_HESS_DENSE handles with the dense hand-over, on both layouts of the blocks, in the handle's stream, by plain
 * loads and stores (staged_hess_guard.hip.h), and end in a change of the diagonal.
 * The common rules are those of hqpkkt_update_stage_hessians and hqpkkt_bfgs_update_stage_hessians:
 *   Checks, all before anything is launched (a call applies to every stage or to none), in this order: HQPKKT_E_NULL;
 *   HQPKKT_E_RANGE - eps not finite or <= 0, max_steps outside 0 .. HQPKKT_EIG_MAX_STEPS; HQPKKT_E_INTERN - the handle is not
 *   STAGED, not analysed, not HQPKKT_HESS_DENSE or analysed for the CSR hand-over; HQPKKT_E_RANGE - a floor that is not finite
 *   (the floors are K + 1 values: the analysis says how many); HQPKKT_E_INTERN - a block of nonzero order that the call reads
 *   has not arrived since the analysis, floor_from_bfgs without a hqpkkt_bfgs_update_stage_hessians since the analysis;
 *   then, without a gfx950 device, HQPKKT_E_DEVICE.
 *   After hqpkkt_restart_, hqpkkt_gerschgorin_ and hqpkkt_eigen_control_stage_hessians h is not factored; the dynamics and
 *   the hand-over state are left alone.  Host vectors go through buffers the handle owns, made by the first call of any of
 *   these entries, outside any capture; device vectors are read and written asynchronously in the handle's stream.
 *   Entries past a stage's order belong to the next stage and padding is never read as a value.
 * hqpkkt_hessian_row_stats: for variable i of stage k, rowmax[i] = max_j |Q_k(i,j)| and offsum[i] = sum_{j != i} |Q_k(i,j)|
 * over the stage's order; n doubles each, pointers per opts.loc, either may be NULL but not both.  A NaN in a row gives NaN
 * for that row and reaches no other row (with an entry off the diagonal its image's row as well: the blocks are symmetric).
 *   Dense block: a wavefront per row, a lane the column pairs lane, lane + 64, .. in ascending order, then the wavefront's
 *   butterfly.  Packed tiles: every stored element is loaded once and counts for its row and, off the diagonal tile, for its
 *   column (the scheme of the packed product); per-tile partials over 128 columns go to slots of a scratch of this entry (two
 *   statistics: twice the product's, so that one is not shared) and a second launch combines a row's slots in ascending
 *   column order.  The order is fixed by the stage's order alone: the same bits from run to run.  The maxima are exact, so a
 *   packed and an unpacked handle return the same bits; the sums agree to rounding, and exactly on integer operands.
 * hqpkkt_restart_stage_hessians: Q_k <- diag(min(max(eps, rowmax_i), 1 / eps)) on the stages with stages[k] != 0 (HOST, K + 1
 * bytes; NULL: all) - restart_Q's operations in their order (a row maximum that is NaN ends as 1 / eps).  The row pass, a
 * kernel that forms the diagonal vector, then the launch of hqpkkt_update_stage_hessians, unchanged, with beta = 0 on the
 * chosen stages and every other stage left alone: the bits are those of that entry with beta = 0 and diag = that vector.
 * Unlike a beta = 0 update by the caller this READS the block: a chosen block must have arrived.
 * hqpkkt_gerschgorin_stage_hessians: q_ii <- max(q_ii, fl(offsum_i + eps)) on every stage - the row pass and one kernel,
 * k_hg_diag, that touches the diagonal entries alone (on a packed handle: in diagonal tile (a, a)); no pass over the arena.
 * hqpkkt_eigen_control_stage_hessians: per stage, with lambda the smallest eigenvalue of Q_k and theta_k the floor, the
 * reference's effect: where lambda - theta_k < 0, q_ii -= lambda - theta_k.  theta_k = eps eps; with floor_from_bfgs lowered
 * to sQs_k where 0 <= sQs_k < eps eps, sQs_k read ON THE DEVICE from the words of the last hqpkkt_bfgs_update_stage_hessians
 * (the reference's rule); floor, where given, overrides both per stage.  lambda is estimated, not computed (the reference
 * calls symmeig per block): a Lanczos recurrence runs on all stages in lockstep.
 *   Start.  The row pass gives Gerschgorin's bound g_k = min_i (q_ii - offsum_i).  A stage with g_k >= theta_k needs no
 *   shift and is done (outcome 0), as is a stage of order 0 (outcome 5).  Every other stage starts from v = f / |f|,
 *   f_i = 1 + ((37 i + 11) mod 64) / 64 for the index i inside the stage.
 *   Steps.  min(max_steps, largest order) steps (max_steps 0: 64), each one product w = Q v over all stages by the launches of
 *   hqpkkt_hessian_product into a buffer of this entry and one launch k_he_step, a workgroup per stage: alpha_j = v'w,
 *   w <- w - alpha_j v - beta_{j-1} v_prev, then w made orthogonal to the whole basis v_0 .. v_j once more (the entry keeps
 *   the basis, `steps` vectors of n, made or grown by the call that needs it; without that pass the recurrence grows second
 *   copies of a converged eigenvalue and the residual bound below means nothing while one is on its way), beta_j = |w|,
 *   v_{j+1} = w / beta_j; the sums in a fixed order (a thread's entries t, t + 1024, .. by fused multiply-adds, a wavefront's
 *   butterfly, the sixteen wavefronts of the stage's workgroup in their order).  A stage
 *   ends itself where j + 1 equals its order or where beta_j > HQPKKT_EIG_END_REL max(|alpha_0 .. alpha_j|, beta_0 ..
 *   beta_{j-1}) does not hold (an invariant subspace; the value is a condition, not critical): its v becomes 0 and it
 *   records its step count.  Nothing is read back inside the loop.
 *   Ritz value.  k_he_ritz, a wavefront per stage, on the tridiagonal T of the recurrence: |T| its infinity norm; the
 *   smallest eigenvalue bracketed by the Sturm count from T's Gerschgorin interval down to hi - lo <= 2^-50 |T|, 64 points
 *   per round; rho = beta_m |last component of the unit eigenvector of T|, by one step of inverse iteration through the
 *   twisted factorisation of T - lo I - Lanczos' residual bound.
 *   The estimate is conservative, lambda_est = lo - rho (a Ritz value lies above the smallest eigenvalue), and the shift is
 *   d_k = theta_k - lambda_est where lambda_est < theta_k, else 0.  Where T or lambda_est is not finite the stage is left alone
 *   (outcome 4) - NOT the reference, which would write NaN into the block.
 *   Shift.  k_hg_diag adds d_k to the stage's diagonal entries, fl(q_ii + d_k); stages with d_k == 0 are not touched: the
 *   bits are those of hqpkkt_update_stage_hessians(r = 0, beta = 1, diag = d) on the touched stages.
 * hqpkkt_eigen_report waits for the stream and copies out HQPKKT_EIG_REPORT doubles per stage: 0 g_k; 1 theta_k as used;
 * 2 steps; 3 lo; 4 hi; 5 rho; 6 lambda_est; 7 d_k; 8 |T|; 9 the outcome - 0 no shift, by Gerschgorin; 1 no shift, by Lanczos;
 * 2 shifted, converged (rho <= 2^-40 |T|); 3 shifted, not converged; 4 left alone, not finite; 5 order 0 - and, where T is
 * given, per stage alpha_0 .. (HQPKKT_EIG_MAX_STEPS doubles), then beta_0 .. (as many); words past the steps are 0.
 * hessian_update.eigen_replay repeats k_he_ritz in numpy from the reported T.  HQPKKT_E_INTERN before the first control
 * since the analysis.
 * Not built: sharded handles and the CSR hand-over.  (The reference's Hqp_HL_DScale works on the sparse Q: the hqpkkt_q_*
 * entries below.) */
#define HQPKKT_EIG_MAX_STEPS 128
#define HQPKKT_EIG_REPORT 10
#define HQPKKT_EIG_END_REL 9.094947017729282e-13 /* 2^-40 */
typedef struct hqpkkt_eigen_control {
  double eps;          /* the reference's _eps: floor theta_k = eps * eps ... */
  int floor_from_bfgs; /* 1: ... lowered to sQs_k where 0 <= sQs_k < eps * eps, read on the device from the last BFGS update */
  const double *floor; /* HOST, K + 1 doubles or NULL: overrides both of the above per stage */
  int max_steps;       /* 1 .. HQPKKT_EIG_MAX_STEPS; 0 = default 64 */
} hqpkkt_eigen_control;
int hqpkkt_hessian_row_stats(hqpkkt_t *h, double *rowmax, double *offsum);
int hqpkkt_restart_stage_hessians(hqpkkt_t *h, double eps, const unsigned char *stages /* HOST, K + 1, or NULL = all */);
int hqpkkt_gerschgorin_stage_hessians(hqpkkt_t *h, double eps);
int hqpkkt_eigen_control_stage_hessians(hqpkkt_t *h, const hqpkkt_eigen_control *e);
int hqpkkt_eigen_report(hqpkkt_t *h, double *out /* HOST, (K + 1) * HQPKKT_EIG_REPORT */, double *T /* HOST or NULL: (K + 1) * 2 * HQPKKT_EIG_MAX_STEPS */);
/* ---- The sparse Q where it lies on the device: the reference's Hessian approximations that work on Hqp_Program::Q itself
 * (Hqp_HL::init, Hqp_HL_Gerschgorin, Hqp_HL_DScale - what hqp_cute.tcl selects next to RedSpBKP) and grd_L of
 * Hqp_SqpSolver, without a round trip of Qx | Ax | Cx through hqpkkt_set_values.  Kernels: csrc/q_values.hip.h; host code: csrc/q_entries.hip.
 * Handles: FULL, REDUCED and STAGED ones that have had values.  HQPKKT_E_INTERN otherwise, on a sharded handle, for every
 * hqpkkt_q_* entry on a STAGED handle with HQPKKT_HESS_DENSE (its Hessians are the blocks: the stage-Hessian entries
 * above), and for hqpkkt_lagrangian_gradient on a STAGED handle analysed by hqpkkt_analyze_staged (the dynamics are
 * not in A then: hqpkkt_lagrangian_gradient_staged, below, is the entry for such a handle).  hqpkkt_lagrangian_gradient
 * does not touch Q and is accepted with dense stage Hessians.
 * Vectors hold n doubles (y: me, z: m), pointers per opts.loc.  Host vectors go through buffers the handle owns (made
 * by the first call) and the call returns when the stream has read or written them; device vectors are read and written
 * asynchronously in the handle's stream.  Plain loads and stores, no atomics.
 * Entries of Q: only the stored entries with col >= row exist, as for the whole library; entries with col < row are never
 * read and never written.  The diagonal of row i is its stored (i, i).  The entries that write the diagonal
 * (hqpkkt_q_set_diagonal, hqpkkt_q_gerschgorin, hqpkkt_q_dscale_setup, hqpkkt_q_dscale_update, hqpkkt_q_eigen_control) return HQPKKT_E_FORMAT where a
 * row has no stored diagonal or more than one - the reference inserts one; the pattern here is fixed - decided on the host
 * from the analysed pattern, before any launch; the map row -> index of its diagonal is built once.
 * Checks, before anything is launched, in this order: HQPKKT_E_NULL; HQPKKT_E_RANGE (eps not finite or <= 0, gamma not
 * finite or < 0 - hqpkkt_q_bfgs_update has its own, below); HQPKKT_E_INTERN (not analysed, no values yet, a refused handle; hqpkkt_q_dscale_report: no update since the
 * analysis - and its HQPKKT_E_RANGE for cap_blocks comes behind that, with *n_blocks set); HQPKKT_E_FORMAT; HQPKKT_E_DEVICE.
 * Values: every operation named here is rounded once (kernels without contraction); max(a, b) is the reference's macro,
 * a > b ? a : b.
 *   hqpkkt_q_values     Qx out: nnz(Q) doubles as they lie in the handle; waits for the stream.
 *   hqpkkt_q_product    y_i = sum_j q_ij x_j over row i of the symmetric image of the stored upper entries (sp_mv_symmlt);
 *                       4 or 16 lanes a row by the mean row length, lane l takes the row's entries l, l + lanes, .. by
 *                       fused multiply-adds, the lanes add up in a fixed tree: the order depends on the row alone.
 *   hqpkkt_q_row_stats  diag_i = the stored q_ii (0.0 without one), offsum_i = sum |q_ij|, j != i, over the same row walk;
 *                       either may be NULL, not both.  A NaN stays in its row and in its image's row.
 *   hqpkkt_q_set_diagonal   every stored upper off-diagonal entry <- +0.0, q_ii <- d_i (Hqp_HL::init, sp_ident, a restart).
 *   hqpkkt_q_gerschgorin    the row pass, then q_ii <- max(q_ii, fl(offsum_i + eps)): one kernel, a thread per variable, the
 *                       diagonal entries alone (Hqp_HL_Gerschgorin::update = Hqp_HL::posdef).
 *   hqpkkt_q_dscale_setup   off-diagonals <- +0.0, q_ii <- max(q_ii, eps) (Hqp_HL_DScale::setup).
 *   hqpkkt_q_dscale_update  Hqp_HL_DScale::update / update_b_Q.  Block b: the variables [b B, min((b + 1) B, n)), B = bsize > 0 ?
 *                       bsize : n.  Per block, q the diagonal: sq_i = fl(s_i q_i), sy = sum s_i y_i, sqs = sum sq_i s_i; damped
 *                       where sy < fl(gamma sqs): theta = fl(fl((1 - gamma) sqs) / fl(sqs - sy)), v_i = fl(fl(theta y_i) +
 *                       fl((1 - theta) sq_i)), sv = sum s_i v_i; otherwise v = y, sv = sy; then q_i <- fl(q_i - fl(fl(sq_i sq_i)
 *                       / sqs)) and q_i <- fl(q_i + fl(fl(v_i v_i) / sv)) - divisions, as in the reference.  Off-diagonal
 *                       entries are neither read nor written.  A block with sv or sqs zero is left alone (the reference),
 *                       and so is one with sv or sqs not finite (the rule of hqpkkt_bfgs_update_stage_hessians; the reference
 *                       writes NaN); a NaN in one block's y reaches no other block.  The sums: chunks of 4096 entries from
 *                       the block's first index, a chunk by 256 threads - thread t takes t, t + 256, .. by fused
 *                       multiply-adds, a wavefront's butterfly, the four wavefronts in order -, a block's chunks added in
 *                       ascending order by one thread: fixed by the block's length alone, not by bsize, the number of
 *                       blocks or the grid; the same bits from run to run and in all three modes.  v (optional): the
 *                       vector as applied, y where a block is not damped.
 *   hqpkkt_q_dscale_report  waits for the stream; HQPKKT_DSCALE_REPORT doubles per block of the last update: 0 sy, 1 sqs,
 *                       2 gamma, 3 theta (1.0 undamped), 4 sv as used, 5 first index, 6 length, 7 outcome - 0 updated,
 *                       1 updated with damping, 2 left alone (zero), 3 left alone (not finite).  out is a HOST array.
 *                       hessian_update.dscale_replay repeats the decision and the update in numpy from the reported sums.
 *   hqpkkt_q_blocks     Hqp_HL_BFGS::next_block on the analysed pattern of Q: the partition of 0 .. n-1 into contiguous blocks.
 *                       bsize < 0 (sqp_hela_bsize's default): a block grows while the last stored column of any of its rows
 *                       reaches past its end (a row without entries, or whose last column is below the diagonal, reaches
 *                       itself); bsize == 0: one block; bsize > 0: blocks of bsize, the last one shorter.  Host only: works
 *                       after hqpkkt_analyze alone (HQPKKT_E_INTERN before it) and touches no device.  first: n_blocks + 1
 *                       ints, the blocks' first indices and n behind the last; full (optional, n_blocks ints): 1 where
 *                       every (i, j), i <= j, of the block is stored.  first == NULL: *n_blocks alone is set; cap (in
 *                       blocks) too small: HQPKKT_E_RANGE with *n_blocks set.  n == 0: no blocks.
 *   hqpkkt_q_bfgs_update    Hqp_HL_BFGS::update (the reference's default approximation) on the blocks of hqpkkt_q_blocks(bsize),
 *                       in place in Qx.  Per block B: Qs_i = sum over j in B of q_ij s_j over row i of the symmetric image -
 *                       the walk and the bits of hqpkkt_q_product where no stored entry crosses a block (always so for
 *                       bsize <= 0); entries whose column lies in another block are skipped, as symsp_extract_mat leaves
 *                       them out -, sy = s'y, sQs = s'(Qs).  gamma_eff = gamma for gamma >= 0, else fl(g + fl(fl(1 - g) fl(1 -
 *                       alpha))), g = -gamma, formed on the host (as hqpkkt_bfgs_update_stage_hessians).  Damped where
 *                       sy < fl(gamma_eff sQs): theta = fl(fl((1 - gamma_eff) sQs) / fl(sQs - sy)) - not clamped, unlike
 *                       Hqp_HL_SparseBFGS -, v_i = fl(fl(theta y_i) + fl(fl(1 - theta) Qs_i)), sv = s'v; otherwise v = y,
 *                       sv = sy.  Every stored entry (i, j), j >= i, with both indices in B: q <- fl(q - fl(fl(Qs_i Qs_j) /
 *                       sQs)), then q <- fl(q + fl(fl(v_i v_j) / sv)) - divisions, as in the reference.  Entries with col < row
 *                       and entries whose indices lie in different blocks are never read or written.  A block with sv or
 *                       sQs zero is left alone (the reference), and so is one with either not finite (the rule of the
 *                       other BFGS / DScale entries; the reference writes NaN); a NaN in one block's y reaches no other
 *                       block.  The sums are made as hqpkkt_q_dscale_update makes them (chunks of 4096 from the block's
 *                       first index): a block's bits depend on its length alone.
 *                       fill = HQPKKT_QBFGS_FULL: Hqp_HL_BFGS proper, every block's upper triangle must be stored - a block
 *                       that is not makes the call return HQPKKT_E_FORMAT, decided on the host from the pattern before
 *                       any launch: a call applies to every block or to none (the reference allocates the entries; the
 *                       pattern here is fixed).  fill = HQPKKT_QBFGS_PATTERN: any pattern, the update on the stored entries
 *                       alone; with bsize = 0 that is the update of Hqp_HL_Gangster on the symmetric image.  (The
 *                       reference's Hqp_HL_Gangster multiplies with the stored triangle alone - sp_mv_mlt on an upper-stored
 *                       Q; the two coincide for a diagonal Q.  This entry follows hqpkkt_q_product.)
 *                       Checks: HQPKKT_E_NULL (h, the arguments, s or y); HQPKKT_E_RANGE (gamma not finite; gamma < 0 with
 *                       alpha not finite; fill neither value - a negative gamma is valid here); HQPKKT_E_INTERN;
 *                       HQPKKT_E_FORMAT; HQPKKT_E_DEVICE.  v, Qs (optional, n doubles each, overlapping neither input): v as
 *                       applied (y where a block is not damped) and the block-restricted Q s the update used.  The
 *                       device tables of a bsize are made by the first update with it; later ones allocate nothing.
 *                       The eigenvalue control of Hqp_HL_BFGS (on by default there) is the entry behind it,
 *                       hqpkkt_q_eigen_control.
 *   hqpkkt_q_bfgs_report    as hqpkkt_q_dscale_report, per block of the last hqpkkt_q_bfgs_update: 0 sy, 1 sQs, 2 gamma_eff,
 *                       3 theta (1.0 undamped), 4 sv as used, 5 first index, 6 length, 7 outcome - 0 updated, 1 updated
 *                       with damping, 2 left alone (zero), 3 left alone (not finite).  hessian_update.q_bfgs_replay repeats
 *                       the decision and the update in numpy from the reported sums and the returned Qs.
 *   hqpkkt_q_eigen_control  the eigenvalue control at the end of Hqp_HL_BFGS::update_b_Q (hqp/Hqp_HL_BFGS.C:203-212, which
 *                       sqp_hela_eigen_control turns on by default) on the blocks of hqpkkt_q_blocks(bsize), in place in Qx.
 *                       The block of the variable set B is the symmetric image of the stored upper entries with both
 *                       indices in B - the operator of hqpkkt_q_bfgs_update, what symsp_extract_mat extracts; a block that is
 *                       not fully stored is the matrix with zeros in the missing places (any pattern is accepted).  Entries
 *                       across blocks and entries with col < row are never read or written.  Per block, with lambda its
 *                       smallest eigenvalue and theta_b the floor, the reference's effect: where lambda - theta_b < 0,
 *                       q_ii -= lambda - theta_b.  theta_b = fl(eps eps); with floor_from_bfgs lowered to sQs_b where
 *                       0 <= sQs_b < eps eps, sQs_b read ON THE DEVICE from the report words of the last
 *                       hqpkkt_q_bfgs_update (the reference's rule), and a block that update left alone (its outcome 2, 3)
 *                       is skipped (outcome 6: the reference's early return); floor, where given, overrides both per
 *                       block.  lambda is estimated, not computed (the reference calls symmeig per block): a Lanczos
 *                       recurrence runs on all blocks in lockstep, with the rules of hqpkkt_eigen_control_stage_hessians -
 *                         Start.  A block-restricted row pass (hqpkkt_q_row_stats counts the entries across blocks) gives
 *                         Gerschgorin's bound g_b = min_i (q_ii - offsum_i), a NaN kept.  A block with g_b >= theta_b needs no
 *                         shift and is done (outcome 0).  Every other block starts from v = f / |f|, f_i = 1 + ((37 i + 11)
 *                         mod 64) / 64 for the index i inside the block.
 *                         Steps.  min(max_steps, longest block) steps (max_steps 0: 64), each one product w = Q v over all
 *                         blocks by the launch of hqpkkt_q_bfgs_update's Q s, unchanged, and four launches: alpha_j = v'w;
 *                         w <- fl(fl(w - fl(alpha_j v)) - fl(beta_{j-1} v_prev)) and the products v_i'w against the whole
 *                         basis; their removal in ascending i, each product and difference rounded on its own (one full
 *                         re-orthogonalisation per step), and w'w; beta_j = |w|, the end test, T and v_{j+1} = w / beta_j.
 *                         A block ends itself where j + 1 equals its length or where beta_j > HQPKKT_EIG_END_REL
 *                         max(|alpha_0 .. alpha_j|, beta_0 .. beta_{j-1}) does not hold (an invariant subspace; the value
 *                         is a condition, not critical): its v becomes 0 and it records its step count.  Every sum is made
 *                         as hqpkkt_q_dscale_update makes its sums (chunks of 4096 from the block's first index, a block's
 *                         chunks in ascending order): a block's bits depend on its length and its values alone, not on
 *                         where it lies, on the other blocks or on the mode.  Nothing is read back inside the loop.
 *                         Ritz value, estimate and shift.  As for the stage entry and by the same device function: the
 *                         Sturm bracket of T's smallest eigenvalue down to hi - lo <= 2^-50 |T|, rho by the twisted
 *                         factorisation, lambda_est = lo - rho, d_b = theta_b - lambda_est where lambda_est < theta_b, else 0.
 *                         Where T or lambda_est is not finite the block is left alone (outcome 4) - NOT the reference,
 *                         which would write NaN into the block; a NaN in one block reaches no other block.  A thread per
 *                         variable adds d_b to the stored diagonals, fl(q_ii + d_b); blocks with d_b == 0 are not touched.
 *                       Checks, before any launch (a call applies to every block or to none), in this order: HQPKKT_E_NULL
 *                       (h, the arguments); HQPKKT_E_RANGE (eps not finite or <= 0, max_steps outside 0 ..
 *                       HQPKKT_EIG_MAX_STEPS, floor_from_bfgs neither 0 nor 1); HQPKKT_E_INTERN (not analysed, no values, a
 *                       refused handle; floor_from_bfgs where the last hqpkkt_q_bfgs_update since the analysis was not
 *                       with this bsize, or there was none); HQPKKT_E_RANGE (a floor that is not finite: the block count is
 *                       known only here); HQPKKT_E_FORMAT (a row without exactly one stored diagonal, as for the other
 *                       entries that write the diagonal); HQPKKT_E_DEVICE; HQPKKT_E_MEM.  The device state belongs to the
 *                       plan of the bsize, which both this entry and hqpkkt_q_bfgs_update make: the basis (step cap x n
 *                       doubles - one block of 10^6 at 64 steps is 512 MB), the units' partial sums, T and the report are
 *                       made or grown by the call that needs them; later calls with the same bsize and a step cap no
 *                       higher allocate nothing; a failed allocation is HQPKKT_E_MEM with the handle unchanged.
 *                       Not built: sharded handles; dense stage Hessians (hqpkkt_eigen_control_stage_hessians);
 *                       Hqp_HL_SparseBFGS's RCM re-blocking; Hqp_HL_AugBFGS; the reference's _logging print.
 *   hqpkkt_q_eigen_report   as hqpkkt_q_bfgs_report (HQPKKT_E_INTERN before a control since the analysis; cap_blocks too small:
 *                       HQPKKT_E_RANGE with *n_blocks and *t_steps set); waits for the stream.  Per block of the last
 *                       hqpkkt_q_eigen_control HQPKKT_EIG_REPORT doubles with the meanings of hqpkkt_eigen_report: 0 g_b;
 *                       1 theta_b as used; 2 steps; 3 lo; 4 hi; 5 rho; 6 lambda_est; 7 d_b; 8 |T|; 9 the outcome - 0 no shift,
 *                       by Gerschgorin; 1 no shift, by Lanczos; 2 shifted, converged (rho <= 2^-40 |T|); 3 shifted, not
 *                       converged; 4 left alone, not finite; 5 never (order 0: reserved, so that hessian_update.eigen_replay
 *                       serves both entries); 6 skipped, the block's last BFGS update left it alone.  T (optional): per
 *                       block alpha_0 .. (*t_steps doubles), then beta_0 .. (as many), words past a block's steps 0;
 *                       *t_steps is the step cap of that call, min(max_steps or 64, longest block) - not
 *                       HQPKKT_EIG_MAX_STEPS: 125 000 blocks at stride 128 would be 256 MB of zeros.
 *   hqpkkt_lagrangian_gradient  Hqp_SqpSolver::grd_L: t_i = sum over row i of A' of a y, then over row i of C' of c z (one
 *                       accumulator per lane, fused multiply-adds, fixed order), out_i = fl(c_i - t_i), then fl(out_i -
 *                       minus_i) where minus is given (u = grad L+ - grad L from the second call).  One kernel.  y / z may
 *                       be NULL where me / m is 0.
 * After an entry that writes Q the handle is in the state hqpkkt_set_values would leave with these values of Q and the A,
 * C it has: not factored; of the CSR copies the image of Q alone is gathered again; with zd_policy < 0 the weak-diagonal
 * test runs again, and the host copies kept for the switch of placement are refreshed from the device where it says weak. */
int hqpkkt_q_values(hqpkkt_t *h, double *Qx);
int hqpkkt_q_product(hqpkkt_t *h, const double *x, double *y);
int hqpkkt_q_row_stats(hqpkkt_t *h, double *diag, double *offsum);
int hqpkkt_q_set_diagonal(hqpkkt_t *h, const double *d);
int hqpkkt_q_gerschgorin(hqpkkt_t *h, double eps);
int hqpkkt_q_dscale_setup(hqpkkt_t *h, double eps);
typedef struct hqpkkt_dscale_update {
  const double *s, *y; /* the step and the change of the Lagrangian's gradient, n doubles each */
  double gamma;        /* Powell's damping (the reference's _gamma, 0.2) */
  int bsize;           /* the reference's _bsize; <= 0: one block of everything */
  double *v;           /* optional, n doubles: the vector as applied */
} hqpkkt_dscale_update;
int hqpkkt_q_dscale_update(hqpkkt_t *h, const hqpkkt_dscale_update *u);
#define HQPKKT_DSCALE_REPORT 8
int hqpkkt_q_dscale_report(hqpkkt_t *h, double *out /* HOST */, long long cap_blocks, long long *n_blocks);
#define HQPKKT_QBFGS_FULL 0    /* Hqp_HL_BFGS: every block's upper triangle must be stored */
#define HQPKKT_QBFGS_PATTERN 1 /* the update on the stored entries of a block alone (the operator of Hqp_HL_Gangster) */
#define HQPKKT_QBFGS_REPORT 8
typedef struct hqpkkt_q_bfgs_update_args {
  const double *s, *y; /* the step and the change of the Lagrangian's gradient, n doubles each */
  double gamma;        /* sqp_hela_gamma: >= 0 the damping factor, < 0 adapted to alpha (as hqpkkt_bfgs_update) */
  double alpha;        /* the step length; read only when gamma < 0 */
  int bsize;           /* sqp_hela_bsize: < 0 detect the blocks, 0 one block of everything, > 0 blocks of bsize */
  int fill;            /* HQPKKT_QBFGS_FULL or HQPKKT_QBFGS_PATTERN */
  double *v;           /* optional, n doubles: the vector as applied */
  double *Qs;          /* optional, n doubles: the block-restricted product Q s the update used */
} hqpkkt_q_bfgs_update_args;
int hqpkkt_q_blocks(hqpkkt_t *h, int bsize, int *first /* HOST */, int *full /* HOST */, long long cap, long long *n_blocks);
int hqpkkt_q_bfgs_update(hqpkkt_t *h, const hqpkkt_q_bfgs_update_args *u);
int hqpkkt_q_bfgs_report(hqpkkt_t *h, double *out /* HOST */, long long cap_blocks, long long *n_blocks);
typedef struct hqpkkt_q_eigen_control_args {
  double eps;          /* the reference's _eps: floor theta_b = fl(eps eps) ... */
  int bsize;           /* the partition: hqpkkt_q_blocks(bsize) */
  int floor_from_bfgs; /* 1: ... lowered to sQs_b where 0 <= sQs_b < eps eps, read ON THE DEVICE from the report words of
                          the last hqpkkt_q_bfgs_update; a block that update left alone (outcome 2, 3) is skipped */
  const double *floor; /* HOST, n_blocks doubles or NULL: overrides both per block */
  int max_steps;       /* 1 .. HQPKKT_EIG_MAX_STEPS; 0 = 64 */
} hqpkkt_q_eigen_control_args;
int hqpkkt_q_eigen_control(hqpkkt_t *h, const hqpkkt_q_eigen_control_args *e);
int hqpkkt_q_eigen_report(hqpkkt_t *h, double *out /* HOST, cap_blocks * HQPKKT_EIG_REPORT */,
                          double *T /* HOST or NULL: cap_blocks * 2 * *t_steps */, long long cap_blocks,
                          long long *n_blocks, int *t_steps);
int hqpkkt_lagrangian_gradient(hqpkkt_t *h, const double *c, const double *y, const double *z,
                               const double *minus /* or NULL */, double *out);
/* The same with the dynamics handed over as DENSE blocks instead of CSR rows - what a DOCP of
 * 10^6 variables needs (K = 200 stages of 5000 states: the CSR form of fx alone would hold
 * 5*10^9 entries, beyond int32 row pointers; Hqp_IpLQDOCP::update extracts exactly these dense
 * blocks fx[k], fu[k] from A, hqp/Hqp_IpLQDOCP.C:748-755).  hqpkkt_analyze_staged replaces
 * hqpkkt_analyze: stage sizes as in hqpkkt_set_stages; n_total = number of variables the blocks Q, E,
 * C are built for (must equal nx[K] + sum of nx[k] + nu[k]: HQPKKT_E_SIZES otherwise); E (me_rest x n)
 * holds the equality rows other than the dynamics.  The vectors r2 / dy of factor / step / solve keep the reference's
 * row order: the sum of nx[1..K] dynamics rows first, then the me_rest rows of E.
 * hqpkkt_set_values_staged replaces hqpkkt_set_values: F[k] points to the row-major
 * nx[k+1] x (nx[k] + nu[k]) block [fx_k fu_k] with leading dimension ldF[k] (the -1.0 of the
 * staircase is implied); pointers per opts.loc (the array F itself is a host array).  The
 * blocks are copied: the caller may release them afterwards.  hqpkkt_mehrotra / _franke run on this
 * form too (their products with the dynamics rows go through the dense blocks; b / y in the same row
 * order as r2 / dy). */
/* Stage sizes from the staircase of the dynamics rows, for hosts that keep A as row lists and must never make a CSR
 * copy of the dynamics (the reference-side binding, shim/Hqp_IpSpBKPHip.C: 5*10^9 entries at K = 200, nx = 5000):
 * per row of A its length, the column of its last entry and of the one before it (three ints per row).  What
 * Hqp_IpLQDOCP::Get_Dim reads off the same rows (hqp/Hqp_IpLQDOCP.C:201-287).  nx holds cap + 1, nu cap entries;
 * returns K, nx[0..K], nu[0..K-1] and the number of dynamics rows (the first rows of A); HQPKKT_E_FORMAT: not a
 * staircase, HQPKKT_E_SIZES: more than cap stages.  Host-only, no handle, no device. */
int hqpkkt_detect_stages(int n, int rows, const int *row_len, const int *last_col, const int *prev_col, int cap, int *K,
                         int *nx, int *nu, int *dyn_rows);
int hqpkkt_analyze_staged(hqpkkt_t *h, int K, const int *nx, const int *nu, int n_total, int me_rest, int m, const int *Qp,
                          const int *Qi, const int *Ep, const int *Ei, const int *Cp, const int *Ci);
/* The dense blocks one at a time, for hosts that extract them from row lists stage by stage (two stage-sized pinned
 * buffers instead of K of them): hqpkkt_stage_staging returns pinned buffer `which` (0 / 1; large enough for the
 * largest block - with HQPKKT_HESS_DENSE for the largest Q_k too, nz_k * nz_k doubles; it waits until the copy that last read the buffer is over), hqpkkt_set_stage_block copies block k =
 * [fx_k fu_k] (nx[k+1] x (nx[k] + nu[k]), row-major, leading dimension ldF; any pointer per opts.loc) into the engine's
 * arena, asynchronously in the handle's stream.  hqpkkt_set_values_staged with F = NULL then takes the other values
 * and ends the hand-over (HQPKKT_E_INTERN unless every block has been set since the analysis). */
int hqpkkt_stage_staging(hqpkkt_t *h, int which, double **buf, long long *elems);
int hqpkkt_set_stage_block(hqpkkt_t *h, int k, const double *F, long long ldF);
int hqpkkt_set_values_staged(hqpkkt_t *h, const double *Qx, const double *const *F, const long long *ldF,
                             const double *Ex, const double *Cx);
/* ---- grad L on a handle of the dense hand-over: Hqp_SqpSolver::grd_L, c - A'y - C'z, where the dynamics rows of A are the
 * blocks F_k in the engine's arena - the y = grad L(x+) - grad L(x) that hqpkkt_bfgs_update_stage_hessians and the other
 * Hessian approximations consume, formed without a copy of F on the host.  Kernel: csrc/staged_gradl.hip.h.
 * Handles: STAGED ones analysed by hqpkkt_analyze_staged whose hand-over has ended (hqpkkt_set_values_staged), with the
 * Hessians in CSR form or as dense blocks, packed or not (Q is not read).  Nothing in the handle is written: a
 * factorisation stays valid.
 * Vectors: c, minus and out hold n doubles, z m doubles, y me doubles in the reference's row order - the sum of nx[1..K]
 * dynamics rows first (stage k's rows start at row0_k = sum of nx[1..k]), then the me_rest rows of E.  Pointers per opts.loc,
 * host vectors through the buffers of the hqpkkt_q_* entries, with their rule of completion.  y / z may be NULL where
 * me / m is 0; minus may be NULL.
 * Checks, before anything is launched, in this order: HQPKKT_E_NULL (h, c, out; y or z of an analysed handle with rows);
 * HQPKKT_E_INTERN (not analysed; the hand-over has not ended; a handle of the CSR hand-over - hqpkkt_lagrangian_gradient
 * serves it; a sharded handle: not built, it needs the ranks' sum); HQPKKT_E_DEVICE.
 * Values, for variable i = column lc of stage k (states of the stage first, then its controls; stage K: its states):
 *   t_i = sum over the rows li = 0 .. nx[k+1] - 1 of F_k[li][lc] y[row0_k + li]   (k < K; 0 for stage K, which has no block):
 *         four partial sums, partial w over the rows li = w, w + 4, .. in ascending order from +0.0 by fused multiply-adds,
 *         added as (p0 + p1) + (p2 + p3)
 *   t_i = fl(t_i - y[row0_k - nx[k] + lc])   where k > 0 and lc is a state column: the -1.0 of the dynamics row that
 *         produces that component of x_k
 *   then t_i = fma(e, y_r, t_i) over the stored entries of column i of E in ascending row order, then t_i = fma(c, z_r, t_i)
 *         over those of column i of C in ascending row order
 *   out_i = fl(c_i - t_i), then fl(out_i - minus_i) where minus is given: the two-call protocol of
 *         hqpkkt_lagrangian_gradient - the gradient with the old blocks first, then, the new blocks handed over, with
 *         minus = the first result.
 * One launch, no atomics, no scratch, nothing read back: the same bits from run to run, and a column's bits depend on its
 * stage's sizes and values alone - not on K, not on the other stages.  The order differs from hqpkkt_lagrangian_gradient's
 * (lanes share a row there): the two hand-overs of one program agree to rounding, and exactly on integer operands.
 * The launch is (column blocks of 256 of the widest stage) x (K + 1) workgroups, each sweeping all rows of its columns: a
 * handle of very few, very wide stages underfills the device, as the residual's pass over F does. */
int hqpkkt_lagrangian_gradient_staged(hqpkkt_t *h, const double *c, const double *y, const double *z,
                                      const double *minus /* or NULL */, double *out);
/* tests: rank and number of carried rows per stage (2 ints each, K+1 stages) of the last factor */
int hqpkkt_debug_stage_ranks(hqpkkt_t *h, int *out, int cap);
/* tests: V_k of the last factor (n_k x n_k, row-major); one GPU.  out null: *len alone */
int hqpkkt_debug_stage_block(hqpkkt_t *h, int k, double *out, long long cap, long long *len);

/* Micro-benchmark and self-check of the dense fp64 MFMA product the STAGED engine is made of:
 * C (M x N) = A'B for pseudo-random k-major operands (K x M, K x N), `reps` timed launches
 * (lower: only the tiles of the lower triangle, mirror: the upper one written from them).
 * *ms: average device time of a launch; *max_err: largest |C_ij - exact| / sum_k |a_ki b_kj|
 * over 4096 sampled entries. */
int hqpkkt_debug_dgemm(int device, int M, int N, int K, int lower, int mirror, int reps, double *ms, double *max_err);
/* The same with a second k segment: C = A'B - A2'B2 (A2: K2 x M, B2: K2 x N) out of ONE launch of the 128 x 128 LDS-DMA
 * kernels (HQPKKT_E_RANGE for a shape or a variant that does not take them); asym: entries of a lower + mirror result
 * that are not bit-identical to their mirror image. */
int hqpkkt_debug_dgemm2(int device, int M, int N, int K, int K2, int lower, int mirror, int reps, double *ms, double *max_err, long long *asym);

/* Test hook: ONE launch of that product on the caller's operands, in the form the engine's launch rule gives the shape and
 * through the engine's own launch code, and the whole of the C buffer back.  Nothing is compared in the library: it
 * copies, launches and copies.  C (M x N) = alpha (A'B + A2'B2) + beta Cin.
 * An operand is a host buffer of rows x ld doubles, row-major; the kernel's pointer is p + col0 and its leading dimension
 * ld (both may be odd: such operands are staged through registers instead of by LDS-DMA).  A, A2: K, K2 rows of M
 * columns; B, B2: K, K2 rows of N columns; rows must be at least K + 1 (K2 + 1): the caller may fill the rows behind K,
 * which no result may depend on, and a 16-byte load may reach one element past row K - 1.  Cin: M rows of N columns, read
 * when beta != 0; cin_is_c != 0: the product is in place, Cin is the C block itself.
 * C: c_rows x ldc doubles, the block starts at row c_row0, column c_col0.  The whole buffer goes to the device before the
 * launch and comes back after it, so the caller sees every element the launch wrote, inside the block or not.
 * flags: as hqpkkt_debug_gemm_form's 1, 8, 16, 32; 0 is the engine's rule on one GPU.  HQPKKT_NO_LDSDMA, HQPKKT_DGEMM_WAVES and
 * HQPKKT_SK_TABLE are honoured as by hqpkkt_debug_dgemm.
 * Out: form (hqpkkt_debug_gemm_form's numbering), tiles, nsplit (pieces of the k range of the thin-deep form), tile_map
 * (the launch walked the tile order of a large triangle), ldsdma (the operands were staged by LDS-DMA).
 * krange, krange_by (the profile form): krange_by 0: as above.  1 / 2: krange holds two ints (lo, hi) per 128-wide column
 * panel of B (1: tile (tm, tn) takes the k-slabs [lo, hi) of panel tn, as W = V+ F) or of A (2: panel tm, as G = F'W); the
 * launch is k_dgemm_tn_sk by a profile list and reports form 6.  No entry of the ranged operand outside its panels' ranges
 * is read as a value that counts.  K2 must be 0, 0 <= lo <= hi <= ceil(K / 16).
 * HQPKKT_E_RANGE: a shape, an operand layout or a form the kernels do not take; HQPKKT_E_MEM: an allocation failed. */
typedef struct hqpkkt_dgemm_operand {
  const double *p;
  long long rows, ld, col0;
} hqpkkt_dgemm_operand;
typedef struct hqpkkt_dgemm_case {
  int M, N, K, K2;
  int lower, mirror, flags, cin_is_c;
  double alpha, beta;
  hqpkkt_dgemm_operand A, B, A2, B2, Cin;
  double *C;
  long long c_rows, ldc, c_row0, c_col0;
  int form, tile_map, ldsdma, nsplit; /* out */
  long long tiles;                    /* out */
  const int *krange;                  /* in: the profile form's ranges, or NULL */
  int krange_by;                      /* in: 0 none, 1 B's column panels, 2 A's */
} hqpkkt_dgemm_case;
int hqpkkt_debug_dgemm_full(int device, hqpkkt_dgemm_case *c);

/* Test hook: ONE launch of the product C (M x N) = A'B, K = M, with the control-row segment for the last mu columns of
 * C - Cu (mu x N) = C[:, N - mu : N]'B out of the free rows of the ragged last tile row - followed, as in the engine's
 * fused stage, by the guarded thin product for Cu and the end of the segment's use.  The launch is the cut form on 128 x
 * 128 tiles whatever the rule says, by the chooser's list for tiles + 1 units on `grid` workgroups (0: two per CU) in the
 * segment's order.  taken: 1 where the launch took the segment (M mod 128 even and > 0, M mod 128 + mu <= 128, the
 * operands staged by LDS-DMA, a list with that order); 0: the thin product alone formed Cu.  fallbacks: launches whose
 * augmented tiles found C's last columns unfinished (the guarded product ran).  A, B as in hqpkkt_dgemm_case; C: c_rows
 * (> M) x ldc (> N), the block at row 0, column 0; Cu: cu_rows (>= mu) x ldcu (>= N); both whole buffers go to the device
 * and come back.  mu = 0: no segment, no thin product. */
typedef struct hqpkkt_ctrl_rows_case {
  int M, N, mu, grid;
  hqpkkt_dgemm_operand A, B;
  double *C;
  long long c_rows, ldc;
  double *Cu;
  long long cu_rows, ldcu;
  int taken, fallbacks, form; /* out */
  long long tiles;            /* out */
} hqpkkt_ctrl_rows_case;
int hqpkkt_debug_dgemm_ctrl_rows(int device, hqpkkt_ctrl_rows_case *c);

/* Test hook, host only: the work list and tile order of a launch with the control-row segment (gemm_ctrl_rows_order,
 * sk_table.hpp) for tiles_m x tiles_n tiles of nslab k-slabs on `grid` workgroups: a list for tiles_m tiles_n + 1 logical
 * tiles (kind as hqpkkt_debug_sk_table; -1: the list the engine's chooser gives), units as there, and tile_map (or NULL;
 * tiles_m tiles_n + 1 ints): logical tile -> tile row << 16 | tile column, bit 31: the augmented form.  Returns the
 * stride, or 0: no list, or none with that order. */
int hqpkkt_debug_sk_ctrl_rows(int tiles_m, int tiles_n, int nslab, int grid, int kind, int *units, long long cap_ints, int *tile_map, long long *pieces);

/* Test hook, host only (no device needed): a work list of the cut forms of that product (k_dgemm_tn_sk walks one list
 * per workgroup, whatever the schedule) for `tiles` tiles of `nslab` k-slabs on `grid` workgroups, sk_table.hpp.
 * kind 0: unequal shares for the two workgroups of a CU; 1: equal shares, whole rounds and cut phases; 2: the fractional
 * cut, the k-slabs of all tiles as one sequence.
 * units (or NULL): six ints per unit, (b * stride + i) * 6 for unit i of workgroup b (blockIdx.x): tile (-1: end of the
 * list), first and one-past-last k-slab, first parking slot of the tile, pieces of the tile, number of this piece.
 * Returns the stride (units per workgroup incl. the end mark), or 0 (no list for these sizes; cap_ints too small).
 * *pieces: parking slots; *whole_a / *whole_b (kind 0; else 0): whole tiles per workgroup of the first / second half of
 * the launch. */
int hqpkkt_debug_sk_table(long long tiles, int nslab, int grid, int kind, int *units, long long cap_ints, long long *pieces, int *whole_a, int *whole_b);

/* Test hook, host only: the work list of the profile form (gemm_profile_table, sk_table.hpp) for `tiles` tiles of which
 * tile t takes the k-slabs [ranges[2 t], ranges[2 t + 1]), on `grid` workgroups.  units, cap_ints, *pieces and the
 * returned stride as in hqpkkt_debug_sk_table. */
int hqpkkt_debug_sk_profile(const int *ranges, long long tiles, int grid, int *units, long long cap_ints, long long *pieces);

/* Test hook: one launch of either product of the profile form's solve on the caller's host arrays.  A: a_rows >= K rows
 * of ld doubles (ld >= N, a multiple of 8), ranges: two ints (lo, hi) per 128-column panel, 0 <= lo <= hi <= ceil(K / 16).
 * rows_form 0: y (N) = add + alpha A'x (x: K entries), panel p summed over the rows [16 lo_p, min(K, 16 hi_p));
 * rows_form 1: y (K) = add + alpha A x (x: N entries), row r over the panels with lo_p <= r / 16 < hi_p.  add may be NULL.
 * HQPKKT_E_INTERN: the launch wrote behind y. */
int hqpkkt_debug_gemv_profile(int device, int rows_form, int K, int N, const double *A, long long a_rows, long long ld, const int *ranges,
                              const double *x, const double *add, double alpha, double *y);

/* Test hooks of the packed panels (hqpkkt_set_packed_panels).  The caller packs: `packed` is a host buffer of
 * packed_elems doubles, `panel` holds two long longs per 128-column panel of the K-row operand - the offset of the
 * panel's first element (even) and its leading dimension (a multiple of 8, at least the panel's columns) - and the ranges
 * are (lo, hi) k-slab pairs as in hqpkkt_dgemm_case.  Panel p's rows [16 lo_p, min(16 hi_p, K)) must lie inside the buffer
 * (HQPKKT_E_RANGE otherwise); nothing outside them is read as a value that counts.
 * hqpkkt_debug_dgemm_packed: hqpkkt_debug_dgemm_full with c->krange_by 1 / 2 and c->krange set, in which operand B / A
 * of the case is not read and comes from the packed buffer (K2 must be 0); both staging paths take it.
 * hqpkkt_debug_gemv_packed: hqpkkt_debug_gemv_profile on packed panels.
 * hqpkkt_debug_carried_packed: the carried rows of a packed stage, C[c_row0 + r][c_col0 + c] = sum over the rows k of
 * panel(c)'s range of BT[k][r] F[k][c] for r < R, c < N; BT: bt_rows >= K rows of ldb >= R doubles; C: a host buffer of
 * c_rows x ldc doubles that goes to the device whole and comes back whole after the launch. */
int hqpkkt_debug_dgemm_packed(int device, hqpkkt_dgemm_case *c, const double *packed, long long packed_elems, const long long *panel);
int hqpkkt_debug_gemv_packed(int device, int rows_form, int K, int N, const double *packed, long long packed_elems, const long long *panel,
                             const int *ranges, const double *x, const double *add, double alpha, double *y);
int hqpkkt_debug_carried_packed(int device, int K, int N, int R, const double *BT, long long bt_rows, long long ldb, const double *packed,
                                long long packed_elems, const long long *panel, const int *ranges, double *C, long long c_rows, long long ldc,
                                long long c_row0, long long c_col0);

/* Test hooks of the solve's dense vector products (staged.hip.h: k_st_gemv_rows, k_st_gemv_wide, k_st_gemv_cols with
 * k_st_cols_finish, k_st_symv_tiles with k_st_symv_finish and their _batch forms): ONE launch on the caller's host arrays
 * through the launch functions the engine's sweeps call, host arrays back, nothing compared in the library.
 * A case: A and A2 are operands as hqpkkt_dgemm_case's - a buffer of rows x ld doubles, the kernel's pointer is p + col0:
 * ld and col0 may be odd, which decides between the 16-byte and the scalar loads -; x, x2: host vectors of x_len, x2_len
 * doubles, uploaded whole (the caller may poison what lies behind the entries that count); add, add2: NULL or as long
 * as the result; y, y2: go to the device before the launch and come back after it.  On the device every result vector
 * and every scratch area has 64 marked doubles behind it, and the scratch areas - sized as the plan sizes them,
 * StagedPlan::symv_need(N) and part_chunks (N + 8) doubles - are NaN before the launch: HQPKKT_E_INTERN where a mark, or
 * scratch outside the partial sums in use, has changed.
 * hqpkkt_debug_gemv_dense, form 0 (rows form): y (M) = scale (add + A x + A2 x2), A: M x N, A2 (or p NULL): M rows of which
 *   the first n2 columns count (n2 is read on the device, as the engine's live carried rows), x2: n2 entries.
 *   form 1 (wide form, a workgroup per row): the same without A2.
 *   form 2 (columns form): y (N) = add + scale A'x over the M rows of A (x: M entries), y2 = y + add2 (both or neither);
 *   part_chunks stands for the plan's value: min(part_chunks, M / 64) chunks of rows, at least one.
 *   Out: chunks (launched; forms 0, 1: 1); vec16: forms 0 and 1 the rows whose pointer takes the 16-byte loads, form 2
 *   whether the block takes them (aligned start, even ld).
 * hqpkkt_debug_symv: y (N) = scale (add + V x + A2 x2) with V = A, N x N, by the triangle form whatever HQPKKT_SYMV_FROM /
 *   HQPKKT_NO_SYMV say: no element of V above the diagonal is read as a value that counts.  HQPKKT_E_RANGE: odd ld or
 *   odd col0, which the engine gives to the rows form.  Out: chunks = tiles launched.
 * hqpkkt_debug_symv_batch: `count` such products in one launch pair.  xbase non-NULL: item i reads xbase + xoff (its x is
 *   ignored), else its own x; ybase non-NULL: item i writes ybase + yoff, and the whole of ybase (ybase_len doubles)
 *   travels both ways.  The items' partial sums lie in one area, at steps of symv_need(N) rounded up to 16.  grid_tiles
 *   / grid_fins: workgroups of the two launches, each striding over the tiles / finishing blocks of all items; 0: one
 *   per tile / block, as the engine launches.  Out: cases[0].chunks = tiles of all items.
 * HQPKKT_E_NULL, HQPKKT_E_RANGE (sizes, an operand outside its buffer), HQPKKT_E_DEVICE (no such device), HQPKKT_E_MEM. */
typedef struct hqpkkt_gemv_case {
  int M, N;
  hqpkkt_dgemm_operand A, A2;
  int n2, part_chunks;
  const double *x;
  long long x_len;
  const double *x2;
  long long x2_len;
  const double *add, *add2;
  double scale;
  double *y, *y2;
  long long xoff, yoff; /* hqpkkt_debug_symv_batch */
  int chunks, vec16;    /* out */
} hqpkkt_gemv_case;
int hqpkkt_debug_gemv_dense(int device, int form, hqpkkt_gemv_case *c);
int hqpkkt_debug_symv(int device, hqpkkt_gemv_case *c);
int hqpkkt_debug_symv_batch(int device, int count, hqpkkt_gemv_case *cases, const double *xbase, long long xbase_len, double *ybase, long long ybase_len,
                            int grid_tiles, int grid_fins);
/* Test hook of the wide rows' vector products (hqpkkt_set_dense_rows; staged_rows.hip.h: k_st_rows_gemv, k_st_rows_gemv_t):
 * ONE launch of either kernel on the caller's host arrays through the launch function the engine's step and residual
 * call, host arrays back, nothing compared in the library.
 * A case: nblocks blocks in one buffer E of e_len doubles.  Block b has rows[b] >= 0 rows of ld[b] doubles (a multiple of
 * 8) from E + off[b] (even), of which the first cols[b] >= 1 columns count and meet x[col0[b] .. col0[b] + cols[b]); its
 * rows are the next rows[b] entries of row_index (indices < m into the vectors that go by rows of C, no index twice).
 *   form 0 (rows form, the residual's epilogue): y[row] = sum_c E_b[i][c] x[col0[b] + c] for every row of every block.
 *     x: n doubles; y: m doubles, to the device before the launch and back after it.
 *   form 1 (rows form, the step's epilogue): dz[row] = tz[row] - zw[row] cdx, dw[row] = -1.0 r3[row] + cdx with the same
 *     cdx.  tz, zw, r3: m doubles; dz, dw: m doubles, both ways.
 *   form 2 (columns form): xc[col0[b] + c] = sum_i E_b[i][c] t[row_index of row i], i ascending, for every c < cols[b] of
 *     every block; zero where rows[b] = 0.  t: m doubles; xc: n doubles, both ways.
 * On the device every vector the kernel reads (x, t, tz, zw, r3) has 64 NaN doubles behind its counted entries and every
 * result 64 marked doubles: HQPKKT_E_INTERN where a mark has changed.  HQPKKT_E_NULL; HQPKKT_E_RANGE: an unknown form, a
 * block outside E or x, ld no multiple of 8 or below cols, an odd off, a row index outside m; HQPKKT_E_DEVICE; HQPKKT_E_MEM. */
typedef struct hqpkkt_rows_case {
  int nblocks;
  const int *rows, *cols, *ld, *col0;
  const long long *off;
  const double *E;
  long long e_len;
  const int *row_index;
  int n, m;
  const double *x;             /* forms 0, 1 */
  const double *t;             /* form 2 */
  const double *tz, *zw, *r3;  /* form 1 */
  double *y;                   /* form 0 */
  double *dz, *dw;             /* form 1 */
  double *xc;                  /* form 2 */
} hqpkkt_rows_case;
int hqpkkt_debug_rows_gemv(int device, int form, hqpkkt_rows_case *c);
/* Host only: the (row tile, column tile) of tile t = 0 .. tiles - 1 of the triangle form of order N, by the code the
 * kernel runs (64-row, 512-column tiles on and below the diagonal); pairs (or NULL): 2 ints per tile, written where
 * cap >= 2 tiles.  Returns the number of tiles. */
long long hqpkkt_debug_symv_map(int N, int *pairs, long long cap);

/* Test hook, host only: the form the STAGED engine's launch rule (gemm_form.hpp) gives an M x N x K product on a device
 * of `cus` CUs with a split grid of `grid` workgroups (0: none), arrival counters for sk_tiles tiles and workspaces of
 * ws_elems / ws2_elems doubles (first / second stream).  flags: 1 one system over several ranks, 2 a launch of the
 * second stream, 8 never the product cut in k, 16 never a tile order, 32 the cut form forced (8, 16, 32: what
 * hqpkkt_debug_dgemm sets).  Returns -1 (nothing to launch / lower with M < N), 0 fractional
 * cut, 1 planned or table cut, 2 plain 128 x 128 round, 3 thin-deep cut in k, 4 64 x 32 tiles, 5 64 x 64 tiles;
 * *tiles: tiles of the launch; *table / *tile_map: a work table / a tile order of the triangle is wanted; *nsplit: pieces
 * of the k range of the thin-deep form (1 otherwise). */
int hqpkkt_debug_gemm_form(int M, int N, int K, int lower, int mirror, int cus, int grid, long long sk_tiles, long long ws_elems,
                           long long ws2_elems, int flags, long long *tiles, int *table, int *tile_map, int *nsplit);

/* Test hook, host only: the schedule of ONE launch of that product (gemm_schedule.hpp) - what the engine's launches and
 * the hooks hqpkkt_debug_dgemm* look up and run - for what a holder offers (caps) and a launch described by numbers.
 * caps: the 128 x 128 variant (0 register-staged, 1 / 2 LDS-DMA on 4 / 8 waves), CUs, workgroups of the cut forms,
 * tiles the rule may give a cut form, size of the arrival counters' array, workspaces of the first / second stream in
 * doubles, whether unequal shares are allowed, hqpkkt_debug_gemm_form's flags 1, 8, 16, 32.
 * launch: the shape; second_stream; ntiles > 0: that many 128 x 128 tiles out of the caller's list; the operands'
 * addresses and leading dimensions (a, lda, ...: never read - they decide whether the operands may be staged by
 * LDS-DMA); mu > 0: the control-row segment for the columns [c0, c0 + mu) of C (address c, leading dimension ldc);
 * panel with by 1 / 2: the profile form, (lo, hi) k-slabs per 128-column panel of B / of A.
 * other (or NULL): a second launch; out->same_key says whether the two share a schedule (the cache key's equality).
 * out: form (hqpkkt_debug_gemm_form's numbering, 6 profile), nsplit, the variant launched, list (-1 none - a plain round
 * -, 0 unequal, 1 equal, 2 fractional, 3 profile), its stride and parked pieces, segment taken, tiles, k-slabs per tile,
 * length of the tile order (0: the kernel's own).  units (or NULL; six ints per unit as hqpkkt_debug_sk_table's, grid x
 * stride of them) and order (or NULL; tile row << 16 | tile column, bit 31: the augmented form).
 * Returns 0; 1: no form takes the launch; 2: the profile form's list does not fit the counters or the workspace; -1: a
 * NULL argument, or units / order too small. */
typedef struct hqpkkt_gemm_caps {
  int variant, cus, grid, unequal, flags;
  long long sk_tiles, cnt_elems, ws_elems, ws2_elems;
} hqpkkt_gemm_caps;
typedef struct hqpkkt_gemm_launch {
  int M, N, K, K2, lower, mirror, second_stream, ntiles;
  unsigned long long a, b, a2, b2, c;
  long long lda, ldb, lda2, ldb2, ldc, c0;
  int mu, by;
  const int *panel;
} hqpkkt_gemm_launch;
typedef struct hqpkkt_gemm_schedule_out {
  int form, nsplit, variant, list, stride, seg, same_key;
  long long tiles, nslab, pieces, order_len;
} hqpkkt_gemm_schedule_out;
int hqpkkt_debug_gemm_schedule(const hqpkkt_gemm_caps *caps, const hqpkkt_gemm_launch *launch, const hqpkkt_gemm_launch *other,
                               hqpkkt_gemm_schedule_out *out, int *units, long long cap_ints, int *order, long long cap_order);

/* Per-kernel-class device timing for bench.py's roofline line: with on != 0
 * every kernel launch is bracketed by HIP events on the handle's stream and the
 * elapsed times are summed per class (hqpkkt_profile_class_name(c), c = 0..) at
 * the end of each call.  set_profile also zeroes the sums.  get_profile fills
 * up to n_classes entries and returns the number of classes that exist (as a
 * positive value, not a status). */
int hqpkkt_set_profile(hqpkkt_t *h, int on);
int hqpkkt_get_profile(const hqpkkt_t *h, int n_classes, double *ms, long long *launches);
const char *hqpkkt_profile_class_name(int c);
const char *hqpkkt_strerror(int status);

/* ---- device-resident interior-point loop ------------------
 * The reference's Mehrotra predictor-corrector solver (hqp/Hqp_IpsMehrotra.C:
 * cold_start :209-327, step :355-693, solve :696-735) with all vector work on the
 * device: per iteration one factor and two (rarely three) solves of this library plus
 * a handful of kernels over the CSR blocks; only the scalars that steer the iteration
 * come back to the host.  The handle must hold the QP's matrices (hqpkkt_analyze +
 * hqpkkt_set_values with Q, A, C of the Hqp_Program, hqp/Hqp_Program.h:43-60); c, b, d
 * and the outputs x, y, z, w follow opts.loc of the handle.  Cold start
 * (qp_init_method 0-3) or hot start from the handle's previous solve.  result uses the reference's Hqp_Result numbering
 * (hqp/Hqp_impl.h:37-43): 0 optimal, 3 suboptimal, 4 degenerate. */
typedef struct hqpkkt_ip_opts {
  double eps;       /* qp_eps (hqp/Hqp_Solver.C:53)                                   */
  int max_iters;    /* qp_max_iters (hqp/Hqp_Solver.C:52)                             */
  double gammaf;    /* step damping (hqp/Hqp_IpsMehrotra.C:95)                        */
  double norm_data; /* max inf-norm of Q, A, C, c, b, d (hqp/Hqp_IpsMehrotra.C:462-464);
                       the caller holds the data, 0 = use 1                            */
  int hot_start;    /* 0 = cold start (Hqp_IpsMehrotra::cold_start, :209-327);
                       1 = Hqp_IpsMehrotra::hot_start (:330-352) if the previous call on this handle
                       (same dimensions, hot_start != 0) left its x, y and the (z, w) of its last
                       iteration far from the solution (:475-478); as in Hqp_IpsMehrotra::solve
                       (:696-733) a hot start that does not reduce phi by 1.2 per iteration, takes a
                       step below 1e-5, runs max_warm_iters or does not end optimal is thrown away,
                       the QP is solved again from a cold start and its iterations are added to
                       iters; 2 = cold start, but keep what the next hot start needs           */
  int max_warm_iters; /* qp_max_warm_iters (hqp/Hqp_IpsMehrotra.C:111), 0 = 25                */
  int init_method;  /* qp_init_method of the cold start (hqp/Hqp_IpsMehrotra.C:226-250, 294-297):
                       0 z = w = 1, r4 = 0 (default); 1 w = max(|d|,1e-10) |Q| / |C|; 2 w =
                       |C| / max(|d|,1e-10) / |Q|; 3 as 0 with r4 = -z.*w and dz, dw added to z, w */
  int reserved[1];
  double norm_Q, norm_C, norm_d; /* inf-norms of Q, C (largest absolute row sum) and d: init_method 1, 2 */
  double qp_mu0;    /* hqpkkt_franke: qp_mu0 (hqp/Hqp_IpsFranke.C:77,87): > 0 chooses the cold start's Ltilde
                       from it (:167-173), 0 (default) "according Wright" (:175-182)                    */
} hqpkkt_ip_opts;
typedef struct hqpkkt_ip_result {
  int result, iters;     /* Hqp_Result, iterations                                    */
  int n_factor, n_solve; /* plugin calls made                                         */
  double gap, mu, phi, pcost, alpha; /* of the last iteration                         */
  float ms_total;        /* device time of the whole call                             */
  int attempts;          /* 1; 2: the first run ended degenerate / singular and the loop was run again, from a cold
                          * start, with static pivoting (cancelled multiplier pivots replaced): n_factor, n_solve
                          * and ms_total are then the totals over both runs, iters the count of the second (the
                          * field takes the place of the structure's tail padding: size and offsets are those of
                          * earlier builds) */
} hqpkkt_ip_result;
int hqpkkt_default_ip_opts(hqpkkt_ip_opts *opts);
int hqpkkt_mehrotra(hqpkkt_t *h, const hqpkkt_ip_opts *opts, const double *c, const double *b,
                    const double *d, double *x, double *y, double *z, double *w, hqpkkt_ip_result *res);

/* The reference's other interior-point solver, Hqp_IpsFranke (hqp/Hqp_IpsFranke.C: potential
 * reduction with the infeasibility measure zeta; cold_start :156-216, step :271-378, solve
 * :381-416), the default of Hqp_SqpSolver: per iteration one factor and one solve of this
 * library, whose returned residual is part of its optimality test (:372).  Same conventions as
 * hqpkkt_mehrotra; of hqpkkt_ip_opts it reads eps, max_iters, hot_start (1 = Hqp_IpsFranke::
 * hot_start, :222-266, from the iterate the previous hqpkkt_franke call on this handle ended with;
 * thrown away as in :388-411) and max_warm_iters (0 = 15); qp_beta 0.995 and qp_mu0 0 are the
 * reference's defaults (qp_mu0: hqpkkt_ip_opts.qp_mu0).  res->result: 0 optimal, 3 suboptimal, 4
 * degenerate, 1 feasible / 2 infeasible when max_iters ends the run. */
int hqpkkt_franke(hqpkkt_t *h, const hqpkkt_ip_opts *opts, const double *c, const double *b,
                  const double *d, double *x, double *y, double *z, double *w, hqpkkt_ip_result *res);

/* ---- introspection of the symbolic structure (host arrays; used by the
 * structure tests, not by the reference-side shim) ------------------------ */
/* what: 0 elim (QP index -> elimination index, dim), 1 node_piv_start,
 * 2 node_npiv, 3 node_nborder, 4 node_parent, 5 node_level (n_supernodes
 * each), 6 border_ptr (n_supernodes+1), 7 border_idx (border_ptr[last]),
 * 8 entry_row, 9 entry_col (elimination indices, nnz_kkt each), 10 node_owner
 * (rank per supernode, -1 = replicated top), 11 exchanged subtree roots; STAGED: 20 states
 * per stage, 21 controls, 22 first column, 23 / 24 own equality rows (ptr / rows), 25 rows
 * that fix x_0, 26 capacity of carried rows, 27 column cuts of the ranks ((K+1) x (ranks+1)), 28 two counters of
 * the last factorisation: stages whose K was inverted by the blocked elimination, and those of them that fell back to the
 * one-workgroup elimination (device -> host copy); 32 - 35 further STAGED diagnostics (staged_engine.hip); 36 per stage
 * k < K two ints: the stored entries of F_k and 1 where the stage runs the sparse sequence, 2 the profile sequence
 * (hqpkkt_set_dynamics_form);
 * 37 the sparse form's ranges: per dynamics row [first, end) into A's CSR arrays (the row without its -1), then per column
 * of the stages k < K [first, end) into the CSR arrays of A' (rows ascending) - the column's entries in the dynamics rows
 * of its stage; empty on a dense-form handle; 38 the work lists the upload made for the cut forms of the stage products,
 * five ints each: tiles, k-slabs, form (0 fractional, 1 cut), list (0 unequal shares, 1 equal, 2 fractional, -1 none fits
 * the workspace) and the launches that looked the list up since the upload (a captured sequence looks up once, at its
 * capture); empty before the upload; 39 the sparse form's heavy columns (hqpkkt_set_dense_columns): K + 1 pointers, then the
 * heavy columns of every stage as column indices local to the stage (states first, then controls), ascending; empty
 * unless the sparse form is set; valid after hqpkkt_analyze, without a device; 30 (zero-diagonal policy in use, last
 * values have weak Hessian diagonals), 31 (fronts of the tree's top that the solve handles in one launch, first
 * such level, LDS bytes of that launch); 40 (device buffers and pinned host buffers the library holds in this
 * process, over all handles: answered on any handle, analysed or not); 41 the profile form's ranges: K + 1 pointers, then
 * the (lo, hi) k-slab pairs of the 128-column panels of every stage's F_k; empty unless HQPKKT_DYN_PROFILE is set; valid
 * after hqpkkt_analyze, without a device; 42 the packed panels (hqpkkt_set_packed_panels): the same K + 1 pointers, then
 * per panel two ints, its offset in doubles from the stage's first panel and its leading dimension, (-1, 0) for the
 * panels of a stage that keeps its dense block; empty unless HQPKKT_DYN_PROFILE is set; 43 the wide rows of C
 * (hqpkkt_set_dense_rows): K + 2 pointers, then the wide rows of every stage 0 .. K as row indices of C, ascending, then per
 * stage two 64-bit counts as (low, high) int pairs - the H terms the plan kept and the terms the stage's wide rows would
 * have added; empty unless the analysis had a threshold > 0; valid after the analysis, without a device; 44 the
 * control-row segment of the fused stages: [0] W launches since the upload whose augmented tiles found W's control
 * columns unfinished, so that the guarded thin product formed the control rows of G, then per stage 1 where the W launch
 * takes the segment (decided at the upload); 45 the dense Hessians (hqpkkt_set_hessian_form): per stage 0 .. K four ints -
 * the block's order, its leading dimension, and the H terms left in the lists as a (low, high) pair; empty unless
 * HQPKKT_HESS_DENSE is set; valid after the analysis, without a device; 46 the wide rows' vector products
 * (hqpkkt_set_dense_rows): six ints - 1 where hqpkkt_step and hqpkkt_residual take the wide rows through the blocks E_k
 * (0: they walk C), the number of wide rows, and two 64-bit counts as (low, high) int pairs: the stored entries of C left
 * in the narrow copy the CSR walks take, and the entries taken out; empty unless the analysis found wide rows; valid after
 * the analysis, without a device; 47 the packed lower tiles of the dense Hessians (hqpkkt_set_packed_hessians): per stage
 * 0 .. K eight ints - the tile edge T (0 where the stage keeps its dense block), the tiles stored, and three 64-bit counts
 * as (low, high) int pairs: the arena elements of the stage, the doubles one dense hand-over of the stage moves from the
 * caller's host block, the stage's share of the product's scratch; empty unless packing was analysed together with
 * HQPKKT_HESS_DENSE; valid after the analysis, without a device; 48 what a handle of the tree engine launches
 * (csrc/tree_plan.hpp): the plan in use, or before the upload - without a device - the plan that the environment
 * (HQPKKT_NO_TREE_SWEEPS, HQPKKT_NO_SOLVE_TOP, HQPKKT_SOLVE_TOP_FUSED) gives at the time of the call; 31 is answered from
 * the same plan.  A header of 16 ints: [0..6] the seven ints of 31 (fronts of the fused top, its first level or the
 * number of levels, its LDS bytes, ns of its instance, 1 for whole-tree sweeps of the solve, 1 for a whole-tree
 * factorisation, 1 for the top's split form), [7] [8] ldp and ldb of the whole-tree factorisation, [9..11] dynamic LDS
 * bytes of k_panel_solve, k_solve_bwd_b and the largest k_factor_blk launch, [12] tree levels L, [13] ints per record R
 * (32), [14] [15] the fronts of the two schedules.  Then 2 L records of R ints, schedule 0 (this rank's subtrees) level
 * 0 .. L-1, then schedule 1 (the replicated top); a count or grid of 0 means no launch:
 *   [0] fronts of the level, [1] their offset in the schedule's level_nodes;
 *   [2..5] k_factor_diag_small<true>: fronts, ldp, ldb, LDS bytes;  [6..8] k_factor_diag_small<false>: blocks, ldp, LDS bytes;
 *   [9..12] k_factor_blk: fronts, instance (0 .. 3: up to 128, 160, 176, 192 pivots), threads, LDS bytes;
 *   [13..15] k_panel_solve: grid, XCD chunk, offset (pairs) in slabs;
 *   [16..20] k_schur_update: 64-tiles, variant (1 or 2), grid, XCD chunk as passed, offset (triples) in upd_tiles;
 *   [21] [22] k_schur_update_big: 128-tiles, offset (triples) in upd_tiles;
 *   [23..27] forward sweep: form (0 none, 1 k_solve_fwd, 2 k_solve_fwd_a + _b, 3 the level belongs to the fused top, 4 to
 *   the whole-tree launches), fronts of k_solve_fwd_small, grid of k_solve_fwd or _b, grid of _a, offset (pairs) in gslabs;
 *   [28..31] backward sweep: fronts of k_solve_bwd_small, grid of k_solve_bwd_b, grid of _a, offset (pairs) in cblks.
 * *len receives the element count; out may be NULL to query it. */
int hqpkkt_debug_get(const hqpkkt_t *h, int what, int *out, long long *len);
/* diagnostics of the solve's fused top (k_solve_top): one solve on the vectors of the last one with time stamps inside
 * the launch; out (cap >= 8 x fronts doubles) receives per front its tree level and six times in microseconds: start,
 * static data in, children arrived, forward done, border solution arrived, backward done. */
int hqpkkt_debug_solve_top_stamps(hqpkkt_t *h, double *out, int cap);

/* Numeric blocks of one supernode after factor (device -> host copy, tests only):
 * what 0 = panel ((p+b) x p, column-major: L11 below the diagonal, L21), 1 = the
 * explicit inverse of the unit lower L11 (p x p, column-major, diagonal blocks of
 * 16 complete), 2 = X = A21 P' L11^-T (b x p), 3 = update block (b x b; lower
 * triangle; after a whole-tree factorisation the exchange copy it was posted to),
 * 4 = the inverse pivot data of the supernode (2 p doubles, the layout of dinv in
 * hqpkkt_debug_factor_block: 1/d, 0 for a 1x1 pivot; i11 i21 | i22 i21 for a 2x2),
 * 5 = the pivot types (p values: 0, or 1 followed by 2 for a 2x2), 6 = the pivot
 * order inside the block (p values: local row at every pivot position) - 5 and 6
 * are ints on the device and come back as doubles -, 7 = the scale vector of the
 * last factorisation (dim doubles, QP numbering; `node` must be valid, is not used).
 * *len receives the element count; out may be NULL to query it. */
int hqpkkt_debug_read(hqpkkt_t *h, int what, int node, double *out, long long cap, long long *len);

/* MFMA f64 16x16x4 layout self-test on the device: C = A * B for integer-valued
 * asymmetric 16x16x16 operands; *max_err is max |C - exact|. */
int hqpkkt_selftest_mfma(int device, double *max_err);

/* The pivot-block kernel on ONE dense symmetric p x p block (1 <= p <= 192; A row-major), without a tree:
 * what the tests check P A P' = L D L' and M L = I with, for every pivot count and for blocks that need
 * interchanges and 2x2 pivots (hqp/spBKP.C:392, 431-438, 471, 480 restricted to the block).
 * variant 0: k_factor_blk as the library launches it (8 wavefronts up to 128 pivots, 16 beyond);
 * 1: k_factor_diag of rounds 1-3 (p <= 128); 2: k_factor_blk with 16 wavefronts whatever p.
 * Out (each may be NULL): L (p x p column-major, unit lower factor below the diagonal), dinv (2 p: D^-1, for a
 * 2x2 pivot i11 i21 | i22 i21), ptype (0 / 1 / 2), lperm (row of A at every pivot position), W = L^-1 (p x p
 * column-major), counters (128 ints: status, 2x2 pivots, perturbed, slow steps, ...; instrumented builds: time stamps from [9] on), ms (average of `reps`
 * launches of one workgroup). */
int hqpkkt_debug_factor_block(int device, int p, const double *A, double tol, double pivot_eps, int variant,
                              int reps, double *L, double *dinv, int *ptype, int *lperm, double *W,
                              int *counters, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* HQPKKT_H */
