// Host-side symbolic phase of the STAGED engine: stage dimensions from the staircase of
// A (semantics of Hqp_IpLQDOCP::Get_Dim / Get_Constr_Dim / Check_Structure,
// hqp/Hqp_IpLQDOCP.C:201-287, 368-407, 298-354), static capacities of the carried
// constraint rows, storage plan of the dense stage blocks, term lists of the reduced
// Hessian H = Q + C'(Z/W)C and the scatter maps of the CSR values.  Integer work only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace kktdev {

// LDS bytes of the one-workgroup inverse of an order-q matrix (gj_inverse_any in staged.hip.h):
// the matrix, its scaling, the pivot column (>= 64) and row (>= 128: the register form broadcasts
// the augmented row), three int work arrays
inline long long gj_lds_bytes(long long q) {
  const long long cv = q > 64 ? q : 64, rv = q > 128 ? q : 128;
  return q * (q | 1) * 8 + (q + cv + rv) * 8 + 3 * q * 4 + 64;
}

int stages_from_staircase(int n, int rows, const int *row_len, const int *last_col, const int *prev_col,
                          std::vector<int> &states, std::vector<int> &controls, std::vector<int> &first_col, int &dyn_rows);

// What the caller asks of the next analysis (the setters of the C ABI write it, the handle keeps it from one analysis to
// the next) with the other inputs of StagedPlan::run that are not the pattern.  The plan holds only what came of it
struct StagedRequest {
  bool want_sparse = false, want_profile = false;  // hqpkkt_set_dynamics_form: the sparse / the profile form of the stage products
  int want_heavy = 0;                              // hqpkkt_set_dense_columns (-1: StagedPlan::HEAVY_DEFAULT; read by the sparse form alone)
  int want_rows = 0;                               // hqpkkt_set_dense_rows (-1: StagedPlan::ROWS_DEFAULT; a sharded handle keeps its term lists)
  bool want_packed = false;                        // hqpkkt_set_packed_panels (read by the profile form alone)
  bool want_hess_dense = false, want_hess_packed = false;  // hqpkkt_set_hessian_form, hqpkkt_set_packed_hessians (the second with the first alone)
  std::vector<int> given_nx, given_nu;             // explicit stage sizes (hqpkkt_set_stages): nx[K+1], nu[K]; empty: detect from A
  bool dense_dyn = false;                          // dynamics handed over as dense blocks: their rows of A are empty
  int shard_rank = 0, shard_count = 1;             // one system over several ranks (hqpkkt_set_shard)
  bool sharded = false;                            // several ranks, or one rank with a transport set (tests the exchange path)
};

// The kernel sequence stage k < K of the factorisation runs, one function each in staged_host.hip.h; the solve's sweeps
// branch on it too.  StagedPlan::stage_seq answers with one of the first four, which the plan alone decides; the upload
// tells the dense stages apart by the launches' schedules and the stage's width (StagedDev::Product::seq)
enum StageSeq : char { SEQ_SHARDED, SEQ_SPARSE, SEQ_PROFILE, SEQ_DENSE, SEQ_FUSED, SEQ_DENSE_CHAIN2 };

struct StagedPlan {
  int n = 0, me = 0, m = 0, K = 0;
  StageSeq stage_seq(int k) const { return sharded ? SEQ_SHARDED : sparse_dyn ? SEQ_SPARSE : profile_dyn && pf_stage[k] ? SEQ_PROFILE : SEQ_DENSE; }
  int nq = 0, na = 0, nc = 0;
  std::vector<int> nk, mk, nmk;  // states (K+1), controls (K), first column of a stage (K+1)
  std::vector<int> nks;          // first dynamics row of stage k (K+1 entries, nks[K] = ndyn)
  int ndyn = 0;
  std::vector<int> eq_ptr, eq_rows;  // own equality rows per stage (QP row indices), K+2 / total
  bool fixed_x0 = false;
  std::vector<int> fix_rows, fix_src;  // per x_0 component: its row of A and the index of its value in vals
  bool dense_dyn = false;  // dynamics handed over as dense blocks: their rows of A are empty (StagedRequest::dense_dyn)
  // The sparse form of the stage products (hqpkkt_set_dynamics_form, Hqp_IpLQDOCP's mat_a_sparse,
  // hqp/Hqp_IpLQDOCP.C:1119-1273): F_k stays the row lists of A and A' - no dense block, f_elems = 0.  Per dynamics row
  // i of A the entries sp_arow[2 i] .. sp_arow[2 i + 1] of A's CSR arrays (the row without its trailing -1); per column
  // c < nmk[K] the entries sp_tcol[2 c] .. sp_tcol[2 c + 1] of the CSR arrays of A' that lie in the dynamics rows of c's
  // stage (a row of A' also holds the -1 of the stage before and the other equality rows: skipped, as FormGxxSp skips
  // its first entry).  The values stay in `vals` behind the CSR blocks' src.
  bool sparse_dyn = false;
  std::vector<int> sp_arow, sp_tcol;
  std::vector<int> sp_nnz;  // stored entries of F_k (K)
  std::vector<int> hv_nnz;  // ... those of them in heavy columns (K)
  // Heavy columns of the sparse form (hqpkkt_set_dense_columns): a column of F_k with at least heavy_min stored entries
  // (0: none) leaves the column walks and is kept as a column of the dense block D_k = n_{k+1} rows of ldd[k] = up8(nd_k)
  // doubles at oD[k] in the F arena (k-major: either operand of the MFMA product), filled by the scatter of A's values.
  // hv_cols[hv_ptr[k] .. hv_ptr[k + 1]): the heavy columns of stage k, local to the stage, ascending.  sp_tcol_light:
  // sp_tcol with the heavy columns' ranges empty - what the column walks take where a stage has heavy columns.  The work
  // blocks of the stage in the misc arena, sized for the largest stage: oWh = V+ D (n+ x ldd), oTh its transpose (nd rows of
  // up8(n+)), oGh = the heavy rows of G (nd x ldg), oGhh = D'V+D (nd x ldd), oNh = B+ D (carried rows x ldd).
  // HEAVY_DEFAULT: the smallest count of the sweep from which taking sixteen columns out of the walks won at 2000 and at
  // 5000 states, profiles/r12_dense_columns.txt
  static const int HEAVY_DEFAULT = 32;
  int heavy_min = 0;
  std::vector<int> hv_ptr, hv_cols, sp_tcol_light, ldd;
  std::vector<long long> oD;
  long long oWh = 0, oTh = 0, oGh = 0, oGhh = 0, oNh = 0;
  int heavy_count(int k) const { return hv_ptr.empty() ? 0 : hv_ptr[k + 1] - hv_ptr[k]; }
  // The profile form (HQPKKT_DYN_PROFILE): F_k is stored as in the dense form - same arena, same scatter -, and the
  // analysis records per stage k < K and per 128-column panel p of F_k = [fx_k fu_k] the range of 16-row k-slabs that
  // holds the panel's stored entries: pf_rng[2 (pf_ptr[k] + p)] = lo = (first dynamics row of the stage with an entry in
  // the panel's columns) / 16, pf_rng[2 (pf_ptr[k] + p) + 1] = hi = (last such row) / 16 + 1; lo = hi = 0 for a panel
  // without entries.  A property of the pattern, read off the CSR arrays of A'.  The large products of a stage and the
  // solve's two products with F_k then take only these slabs (staged_stage_profile).  pf_stage[k]: the stage runs that
  // sequence - at least two panels and a range shorter than all slabs of n_{k+1}; every other stage runs the dense
  // sequence.
  bool profile_dyn = false;
  std::vector<int> pf_ptr, pf_rng;
  std::vector<char> pf_stage;
  int panels(int k) const { return pf_ptr.empty() ? 0 : pf_ptr[k + 1] - pf_ptr[k]; }
  // Packed panels (hqpkkt_set_packed_panels, with the profile form only): a stage that runs the profile sequence stores
  // F_k panel by panel, back to back from oF[k] - panel p the rows [16 lo_p, min(16 hi_p, n_{k+1})) of its columns,
  // row-major with leading dimension pk_ld = 128 (the last panel: up8 of its columns); an empty panel takes no room, the
  // stage's total is rounded up to 16 doubles.  pk_off[pf_ptr[k] + p]: the panel's first element, in doubles from oF[k];
  // -1 (pk_ld 0) for the panels of a stage that keeps its dense block.  Never larger than the dense block: with exact
  // row counts sum_p rows_p ld_p <= n_{k+1} up8(n_k + m_k).
  bool packed = false;
  std::vector<long long> pk_off;
  std::vector<int> pk_ld;
  bool pk_stage(int k) const { return packed && pf_stage[k]; }
  // element (row li, column lc) of F_k of a packed stage, from oF[k]
  long long pk_at(int k, int li, int lc) const {
    const size_t q = (size_t)pf_ptr[k] + lc / 128;
    return pk_off[q] + (long long)(li - 16 * pf_rng[2 * q]) * pk_ld[q] + lc % 128;
  }

  // Wide rows of C (hqpkkt_set_dense_rows): a row of the inequality block with at least rows_min stored entries (0: none)
  // leaves the H term lists - L entries are L^2 terms there - and is kept as a row of the dense block E_k of its stage
  // k = 0..K: wide_count(k) rows of ldE[k] = up8(n_k + m_k) doubles (stage K: up8(n_K)) at oE[k] in the F arena, row-major
  // (k-major: either operand of the MFMA product), behind every stage's dynamics blocks.  wr_rows[wr_ptr[k] ..
  // wr_ptr[k + 1]): the wide rows of stage k as row indices of C, ascending.  c_dst: per stored entry of C its place in
  // the F arena or -1 (k_st_scatter runs it as it runs a_dst; the arena is cleared at upload and nothing else writes
  // the blocks: the padding stays zero); empty without wide rows.  oSr: the work block S = diag(sqrt(z / w)) E_k of the
  // stage in work, in the misc arena, sized for the largest stage.
  // The vector products of the wide rows (step and residual; k_st_rows_gemv, k_st_rows_gemv_t) read the blocks too, and
  // the CSR walks of these products take narrow copies of C and C' (cn, ctn: ptr / col / src as Analysis::Csr holds
  // them, the entries in their order) in which the wide rows are empty and the wide rows' entries are missing from the
  // columns; c_kept / c_cut: stored entries of C in cn / taken out.  Built by narrow_copies() behind run(), empty without
  // wide rows.  The interior-point loops' own right-hand-side kernels keep the full arrays.
  // h_kept[k] / h_cut[k]: H terms of stage k in the lists / the terms its wide rows would have added.
  // ROWS_DEFAULT 0: no threshold has been measured and the setter refuses -1; a sharded handle keeps its term lists
  // (rows_min = 0)
  static const int ROWS_DEFAULT = 0;
  int rows_min = 0;
  std::vector<int> wr_ptr, wr_rows, ldE;
  std::vector<long long> oE, c_dst, h_kept, h_cut;
  long long oSr = 0;
  struct Narrow {
    std::vector<int> ptr, col, src;
  };
  Narrow cn, ctn;
  long long c_kept = 0, c_cut = 0;
  bool rows_vec() const { return !wr_rows.empty(); }  // step and residual take the wide rows through the blocks
  void narrow_copies(const int *Cp, const int *Ci, const int *Cs, const int *CTp, const int *CTi, const int *CTs);
  int wide_count(int k) const { return wr_ptr.empty() ? 0 : wr_ptr[k + 1] - wr_ptr[k]; }

  // Dense stage Hessians (hqpkkt_set_hessian_form): Q_k of stage k = 0..K, order n_k + m_k (stage K: n_K), kept in full -
  // exactly symmetric - as rows of ldQ[k] = up8(order) doubles at oQ[k] in an arena of its own (q_elems doubles, blocks back
  // to back: a row is 64 bytes or a multiple); Q's terms are not in the H lists.  q_dst: CSR hand-over - per stored entry p
  // of Q its two places in the arena (2 p: row i, column j; 2 p + 1: the image, -1 on the diagonal; both -1 for an entry
  // with col < row, which nobody reads).
  bool hess_dense = false;
  std::vector<int> ldQ;
  std::vector<long long> oQ, q_dst;
  long long q_elems = 0;
  int hess_order(int k) const { return k < K ? nk[k] + mk[k] : nk[k]; }
  // ... stored as packed lower tiles (hqpkkt_set_packed_hessians; with hess_dense alone): stage k with q_packed[k] keeps, at
  // oQ[k], the tiles (a, b), b <= a < nt = ceil(order / HESS_T), each HESS_T rows of HESS_T doubles, zero padded, tile
  // (a, b) at (a (a + 1) / 2 + b) HESS_T^2; a diagonal tile holds both of its triangles.  A stage packs only where that is
  // fewer doubles than its dense block - not monotone in the order: 220 .. 256 pack, 257 .. 312 do not, 313 .. 384 do, 385 does not, 402 does.
  // q_dst then holds the packed places (the image: inside a diagonal tile alone).  oQs[k]: the stage's hess_slots(nt) HESS_T
  // doubles of the product's scratch (qs_elems in all) - per row tile r one slot per HESS_CHUNK tiles of its own row and one
  // per tile (a, r) below it, a little over nt^2 / 2 slots (staged_hess_packed.hip.h); q_stage_elems: the staging block of the dense hand-over from host
  // memory, order x up8(order) of the largest packed stage.
  static const int HESS_T = 128, HESS_COPY_ROWS = 64, HESS_CHUNK = 8;
  static long long hess_slots(long long nt) {
    long long s = 0;
    for (long long r = 0; r < nt; r++) s += (r + HESS_CHUNK) / HESS_CHUNK + nt - 1 - r;
    return s;
  }
  bool hess_packed = false;
  std::vector<char> q_packed;
  std::vector<long long> oQs;
  long long qs_elems = 0, q_stage_elems = 0;
  bool stage_packed(int k) const { return hess_packed && q_packed[k]; }
  static long long hess_tiles(int order) {
    const long long nt = (order + HESS_T - 1) / HESS_T;
    return nt * (nt + 1) / 2;
  }
  static bool hess_packs(int order) { return hess_tiles(order) * HESS_T * HESS_T < (long long)order * ((order + 7) / 8 * 8); }
  // doubles one dense hand-over of a block moves from host memory: a packed stage's rows in groups of HESS_COPY_ROWS,
  // every group from its first column on (order (order + HESS_COPY_ROWS) / 2, about); order^2 where the block stays dense
  static long long hess_handover(int order, bool packed_) {
    if (!packed_) return (long long)order * order;
    long long c = 0;
    for (int r = 0; r < order; r += HESS_COPY_ROWS) c += (long long)std::min(HESS_COPY_ROWS, order - r) * (order - r);
    return c;
  }

  // static bounds: cap[k] carried rows leaving stage k, capn[k] rows of N_k, qmax[k] order of K_k
  std::vector<int> cap, capn, qmax;
  int q0max = 0, ldq0 = 8;  // free initial state: order of [V_0 B_0'; B_0 0]
  std::vector<char> big;    // per stage: its control-sized matrices do not fit LDS (scratch in the misc arena instead)
  int big0 = 0;             // the same for the free initial state
  long long scratch_elems = 0, oScr = 0;

  // dense storage (element offsets; leading dimensions are multiples of 8)
  std::vector<int> ldf, ldv, ldy, ldn, ldb, ldq, ldt, ldg;
  std::vector<long long> oF, oV;                      // F arena, V arena
  std::vector<long long> oY, oR, oK, oKm, oN, oBT, oT;  // misc arena (oKm: K itself, next to its inverse oK)
  std::vector<long long> oVec;                        // per stage: v(n) beta(cap) rho(qmax) eta(cap)
  long long oW = 0, oG = 0, oK0 = 0, oK0m = 0, oK0s = 0, oRes = 0, oGam = 0, oTT = 0, oPart = 0, oS = 0, oQv = 0, oTmp = 0, oUy = 0, oSym = 0;
  // the solve's products with V that stand outside its two chains, many stages per launch (not sharded): g_k = V_{k+1} f_k
  // for all stages (ndyn doubles) and the partial sums of one launch's stages (symb_elems; symv_need(N) per stage)
  long long oGv = 0, oSymB = 0, symb_elems = 0;
  static long long symv_need(long long N) { return ((N + 63) / 64 + (N + 511) / 512) * (N + 8); }
  long long f_elems = 0, v_elems = 0, misc_elems = 0;
  int part_chunks = 1;
  std::vector<int> dyn_off;  // int arena: per stage [r, nl, R(capn), L(capn)]
  int dyn_ints = 0;

  // H term lists: entries of stage k are h_ptr[k] .. h_ptr[k+1]; dst = li * ld + lj inside the
  // stage's dense block (ld = ldg[k], last stage: ldv[K])
  struct Term {
    int s1, s2, wi;
  };
  std::vector<int> h_ptr, h_tptr;
  std::vector<int> h_mid;  // per stage: first entry that touches a control row / column (the state part comes first)
  std::vector<long long> h_dst;
  std::vector<Term> h_terms;

  // scatter of the A values: >= 0 offset into the F arena, <= -2: -(offset into misc + 2), -1: none
  std::vector<long long> a_dst;
  std::vector<int> chk_idx, chk_kind;  // values to check: kind 0 must be -1.0, kind 1 must be non-zero

  long long flops_factor = 0;  // as implemented (dense products of the recursion)
  long long bytes_step = 0;    // dense bytes one step streams

  // One system over several ranks (hqpkkt_set_shard), DESIGN.md section 7: the STATE COLUMNS of every stage are cut into one
  // contiguous range per rank - the same width for every rank but the last, a multiple of 128 - and the memory goes
  // with them: rank p keeps the columns [cut[p], cut[p+1]) of F_k next to the control columns (Floc_k = [F_p | F_u],
  // n+ x ldfl) and, for the solve, the ROWS [cut[p], cut[p+1]) of V_k.  Per stage of the factorisation:
  //   W_p = V+ F_p                                   local (V+ in full: the transient result of the stage before); W is
  //                                                  NOT exchanged
  //   gather of the ranks' Floc_k                    STATIC data: requested a stage ahead (stage k - 1's while stage k is
  //                                                  computed), into one of two buffers - off the critical path
  //   G_xx block (a, b), a >= b                      by one of the two ranks, as W_p' F_q = (V+ F_p)' F_q in its row strip
  //                                                  of the work block (the owner of the block's columns computes the
  //                                                  transpose): pair {a, b} belongs to b if a - b <= (P - 1) / 2 else to
  //                                                  a; with P even the pairs P / 2 apart are cut in two by rows;
  //                                                  diagonal blocks: lower tiles
  //   gather of the blocks (lower orientation)       n^2 / 2 doubles in all: the one exchange on the critical path
  //   V_k = G_xx - Y' Rm in full (every rank), its row strip kept
  // The control-sized chain (W_u = V+ F_u, the control rows of G = W_u' F, the carried rows B+ F, K^-1, Y, Rm) is
  // computed by every rank from the gathered F - by launches of the same shape everywhere, so that all ranks see
  // identical bits.  The solve's products run on the strips with one gather of a state-sized vector per stage and direction.
  int shard_rank = 0, shard_count = 1;
  bool sharded = false;          // several ranks, or one rank with a transport set (tests the exchange path)
  std::vector<int> xcut;         // (K+1) x (shard_count+1): first state column of rank p in stage k (k = K: rows of V_K)
  std::vector<int> xw;           // per stage (K+1): the common strip width (all ranks but the last)
  std::vector<int> ldfl;         // per stage: leading dimension of Floc_k (own strip + control columns)
  std::vector<long long> oFl, oVs;  // local F blocks (F arena), own row strips of V_k (V arena, ld = ldv[k])
  long long oVf[2] = {0, 0};     // the two full-size transient V blocks (misc arena): V_k lives in oVf[k & 1]
  long long oFg[2] = {0, 0};     // the gathered local F blocks: stage k's in oFg[k & 1], shard_count slots of fgslot[k] doubles (misc)
  std::vector<long long> fgslot;
  long long oWl = 0, oWu = 0;    // W_p = V+ F_p (n+ x ldwl[k]) and W_u = V+ F_u (n+ x ldwu) of the stage in work (misc)
  std::vector<int> ldwl;
  int ldwu = 8;
  long long oX = 0;              // the gather of the blocks of G_xx: shard_count slots of xslot[k] doubles (misc)
  std::vector<long long> xslot;
  long long oXV = 0;             // gathers of the solve: the ranks' strips of a state-sized vector, side by side (misc)
  long long xvslot = 0;
  long long oXP = 0;             // ... and shard_count whole state-sized vectors (the partial sums of x+ = F s + f)
  long long xpslot = 0;
  long long oDyx = 0;            // the dynamics rows' multipliers (+ V_0 x_0 + v_0 with a fixed x_0): summed over the ranks
  // a block (part) of G_xx in the exchange buffer 2, lower orientation: rows [r0, r1) x columns [c0, c1) of G_xx,
  // row-major with leading dimension c1 - c0 at slot `owner`, offset `off`; how the owner computes it: `mine_rows`
  // (A = its own F strip: the block is the rows of its strip) or not (A = W of the row block's owner, B = its own F strip:
  // computed transposed in its row strip of the work block, packed with a transposition)
  struct XRect {
    int a, b;            // block row / column (ranks)
    int r0, r1, c0, c1;
    int owner;
    bool mine_rows;
    long long off;       // inside the owner's slot
  };
  std::vector<XRect> xrects;      // all stages, all ranks: stage k holds xrect_ptr[k] .. xrect_ptr[k+1]
  std::vector<int> xrect_ptr;
  std::vector<int> gtile;         // this rank's tiles of its blocks' products: (tile row in the strip) << 16 | global tile column
  std::vector<int> gtile_ptr;     // per stage

  // the entries of xcut that every sharded step needs: this rank's first state column of stage k and its strip's width
  int strip_first(int k) const { return xcut[(size_t)k * (shard_count + 1) + shard_rank]; }
  int strip_width(int k) const { return xcut[(size_t)k * (shard_count + 1) + shard_rank + 1] - strip_first(k); }
  // the profile form's (lo, hi) k-slab pairs of stage k's panels
  const int *stage_ranges(int k) const { return pf_rng.data() + 2 * (size_t)pf_ptr[k]; }

  // returns 0, or a HQPKKT_E_* code: 6 the pattern is not a staircase / rows leave their stage,
  // 1 a stage exceeds what the one-workgroup kernels hold, or the H term lists would hold more than 2^31 - 1 terms
  // (ATp, ATi: the CSR arrays of A' as Analysis::setup_blocks builds them, rows ascending; read by the sparse form alone)
  int run(const StagedRequest &rq, int n, int me, int m, const int *Qp, const int *Qi, const int *Ap, const int *Ai, const int *Cp,
          const int *Ci, const int *ATp = nullptr, const int *ATi = nullptr);
};

}  // namespace kktdev
