// gfx950 kernels of the dense stage Hessians stored as packed lower tiles (hqpkkt_set_packed_hessians,
// StagedPlan::hess_packed): stage k keeps of its block Q_k the tiles (a, b), b <= a < nt = ceil(nz / HP_T), each HP_T rows
// of HP_T doubles, row-major, zero padded, tile (a, b) at (a (a + 1) / 2 + b) HP_T^2; a diagonal tile holds both of its
// triangles, bit for bit symmetric.
//   store     k_hp_pack: the caller's block (only j >= i read) into the tiles, a tile below the diagonal as the transpose of
//             the caller's rows of tile row b, through LDS; the CSR hand-over keeps k_hs_scatter with the packed map
//   assembly  k_hp_add: the requests of k_hs_add tile by tile - a stored tile added where the request covers it, its
//             transpose to the image tile where the request is not `lower`; every entry of G gets one add of the value the
//             dense form adds
//   products  k_hp_symv_tiles / k_hp_symv_finish: y = Q x over all packed stages; a stored element is loaded once and
//             serves its row's and its column's sum; partial sums through a scratch of about nt^2 / 2 slots of HP_T doubles;
//             the sums' order is fixed by the block's order alone
// Plain loads and stores: no polled words, no waits between workgroups, no atomics.  Included by staged_hess.hip.h.
#pragma once
#include <hip/hip_runtime.h>

namespace stg {

static const int HP_T = 128;  // the tile edge: that of the stage products (StagedPlan::HESS_T)
static const int HP_S = 32;   // pack and add move a tile as 4 x 4 subtiles of HP_S x HP_S through LDS

__device__ __forceinline__ void hp_tile_of(int t, int &a, int &b) {  // t = a (a + 1) / 2 + b, b <= a
  a = 0;
  while ((a + 1) * (a + 2) / 2 <= t) a++;
  b = t - a * (a + 1) / 2;
}

// The caller's block S (row-major, leading dimension lds, order nz) into the tiles at Qt.  Workgroup (t, s): subtile
// s = 4 p + q (rows HP_S p .., columns HP_S q .. of the tile) of stored tile t = (a, b).  Entry (i, j) of Q is S[min][max]:
// a subtile strictly below the diagonal is the transpose of the caller's subtile at rows b HP_T + HP_S q, columns a HP_T +
// HP_S p, a subtile above it (diagonal tiles alone) the caller's own, and one on the diagonal both halves of its upper
// triangle.  Of S only entries with i <= j < nz are loaded; the tile is written whole, zeros past nz.
__global__ void __launch_bounds__(256) k_hp_pack(const double *__restrict__ S, long long lds, int nz, double *__restrict__ Qt) {
  __shared__ double t[HP_S][HP_S + 1];
  int a, b;
  hp_tile_of(blockIdx.x, a, b);
  const int p = blockIdx.y >> 2, q = blockIdx.y & 3;
  const int gi = a * HP_T + p * HP_S, gj = b * HP_T + q * HP_S;  // the subtile's first row and column in Q
  const bool trans = gi > gj, diag = gi == gj;
  const int rs = trans ? gj : gi, cs = trans ? gi : gj;  // ... and in S (rs <= cs)
  for (int u = threadIdx.x; u < HP_S * HP_S; u += 256) {
    const int r = u / HP_S, c = u % HP_S;
    double v = 0.0;
    if (rs + r < nz && cs + c < nz && cs + c >= rs + r) v = S[(long long)(rs + r) * lds + cs + c];
    t[r][c] = v;
  }
  __syncthreads();
  double *dst = Qt + (long long)blockIdx.x * HP_T * HP_T + (long long)(p * HP_S) * HP_T + q * HP_S;
  for (int u = threadIdx.x; u < HP_S * HP_S; u += 256) {
    const int r = u / HP_S, c = u % HP_S;
    dst[(long long)r * HP_T + c] = trans ? t[c][r] : diag ? (r <= c ? t[r][c] : t[c][r]) : t[r][c];
  }
}

// k_hs_add's request on a packed stage: G[i][j] += Q[i][j] for the rows [r0, r1) and the columns [0, c1); lower: of row i only
// the columns up to the end of its HP_T-wide diagonal block - exactly the stored tiles.  Workgroup (t, s): subtile s of stored
// tile t, loaded once; added to G at its own place where the request covers it, and - not lower, tile below the diagonal -
// transposed through LDS to its image.  A diagonal tile holds both triangles: its own place is all of it.
struct HpAdd {
  const double *Qt;
  double *G;
  long long ldg;
  int r0, r1, c1, lower;
  int a0;  // first tile row of the launch (the tiles of the rows before it are not in the request, nor are their images)
};
__global__ void __launch_bounds__(256) k_hp_add(HpAdd g) {
  __shared__ double t[HP_S][HP_S + 1];
  int a, b;
  hp_tile_of(blockIdx.x + g.a0 * (g.a0 + 1) / 2, a, b);
  const int p = blockIdx.y >> 2, q = blockIdx.y & 3;
  const int gi = a * HP_T + p * HP_S, gj = b * HP_T + q * HP_S;
  const bool image = !g.lower && a != b;
  // (uniform over the workgroup: nothing of the subtile or of its image in the request)
  const bool own = gi < g.r1 && gi + HP_S > g.r0 && gj < g.c1;
  const bool img = image && gj < g.r1 && gj + HP_S > g.r0 && gi < g.c1;
  if (!own && !img) return;
  const double *src = g.Qt + ((long long)a * (a + 1) / 2 + b) * HP_T * HP_T + (long long)(p * HP_S) * HP_T + q * HP_S;
  for (int u = threadIdx.x; u < HP_S * HP_S; u += 256) {
    const int r = u / HP_S, c = u % HP_S;
    const double v = src[(long long)r * HP_T + c];
    t[r][c] = v;
    const int i = gi + r, j = gj + c;
    if (own && i >= g.r0 && i < g.r1 && j < g.c1) g.G[(long long)i * g.ldg + j] += v;
  }
  if (!img) return;
  __syncthreads();
  for (int u = threadIdx.x; u < HP_S * HP_S; u += 256) {
    const int r = u / HP_S, c = u % HP_S;  // entry (gj + r, gi + c) of Q = t[c][r]
    const int i = gj + r, j = gi + c;
    if (i >= g.r0 && i < g.r1 && j < g.c1) g.G[(long long)i * g.ldg + j] += t[c][r];
  }
}

// y = Q x over the packed stages.  A workgroup takes up to HP_CHUNK neighbouring tiles (a, b0 ..) of one tile row of a stage
// (stages that keep their dense block have no tiles here: nt = 0).  Wavefront w takes the rows w, w + 4, .. of a tile, a lane
// two columns.  Rows: a row's products are summed over the wavefront (hp_wave_sum8, eight rows at a time) and over the chunk's
// tiles in ascending b, and the 128 sums go to one slot of row tile a.  Columns: a lane's two column sums over the wavefront's rows are
// summed over the four wavefronts in their order and go to a slot of row tile b - the transpose's share; a diagonal tile
// counts once, by its rows.  x past the stage's order counts as 0 (the tiles hold zeros there).
// The slots of row tile r, HP_T doubles each, in ascending order of the columns they cover: its own chunks 0 ..
// hp_chunks(r) - 1, then the tiles (a, r), a = r + 1 .. nt - 1; hp_slot_base(r, nt) slots lie ahead of them.  The sums'
// order is fixed by the block's order alone.  (StagedPlan::hess_slots is the same count on the host.)
// Two workgroups per CU (launch bounds): a stage of order 3000 has 48 chunks, and eight such stages fit the device at once.
static const int HP_CHUNK = 8;
__host__ __device__ inline int hp_chunks(int a) { return (a + HP_CHUNK) / HP_CHUNK; }  // of tile row a: ceil((a + 1) / HP_CHUNK)
__host__ __device__ inline long long hp_slot_base(int r, int nt) {
  long long s = 0;
  for (int q = 0; q < r; q++) s += hp_chunks(q) + nt - 1 - q;
  return s;
}
// The sums over a wavefront of eight values per lane in ten exchanges: the halves of the wavefront trade four values each,
// the quarters two, the eighths one, and the eight lanes that then hold partial sums of the same value finish it.  Lane l
// returns the sum of p[hp_row_of(l)].  A fixed order.
__device__ __forceinline__ int hp_row_of(int lane) { return ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1); }
__device__ __forceinline__ double hp_wave_sum8(const double (&p)[8], int lane) {
  double q[4], r[2];
  bool hi = lane & 32;
#pragma unroll
  for (int i = 0; i < 4; i++) q[i] = (hi ? p[4 + i] : p[i]) + __shfl_xor(hi ? p[i] : p[4 + i], 32);
  hi = lane & 16;
#pragma unroll
  for (int i = 0; i < 2; i++) r[i] = (hi ? q[2 + i] : q[i]) + __shfl_xor(hi ? q[i] : q[2 + i], 16);
  hi = lane & 8;
  double t = (hi ? r[1] : r[0]) + __shfl_xor(hi ? r[0] : r[1], 8);
  t += __shfl_xor(t, 4), t += __shfl_xor(t, 2), t += __shfl_xor(t, 1);
  return t;
}
struct HpDesc {
  long long oQ, oS;  // the stage's tiles in the arena, its slots in the scratch
  int nt, nz, col0, nchunks;  // (nchunks: the sum of hp_chunks over the tile rows)
};
__global__ void __launch_bounds__(256, 2) k_hp_symv_tiles(const HpDesc *__restrict__ desc, const double *__restrict__ Q, const double *__restrict__ x,
                                                       double *__restrict__ scr) {
  const HpDesc d = desc[blockIdx.y];
  if ((int)blockIdx.x >= d.nchunks) return;
  __shared__ double xa[HP_T], part[4][HP_T];
  int a = 0, ch = blockIdx.x;
  while (ch >= hp_chunks(a)) ch -= hp_chunks(a), a++;
  const int b0 = ch * HP_CHUNK, b1 = min(b0 + HP_CHUNK, a + 1);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < HP_T) {
    const int i = a * HP_T + threadIdx.x;
    xa[threadIdx.x] = i < d.nz ? x[d.col0 + i] : 0.0;
  }
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // (of row wave + 4 (8 m + hp_row_of(lane)), m = 0 .. 3)
  for (int b = b0; b < b1; b++) {
    const int j = b * HP_T + 2 * lane;
    const double xb0 = j < d.nz ? x[d.col0 + j] : 0.0, xb1 = j + 1 < d.nz ? x[d.col0 + j + 1] : 0.0;
    const hs_d2 *tile = (const hs_d2 *)(Q + d.oQ + ((long long)a * (a + 1) / 2 + b) * HP_T * HP_T);
    double c0 = 0.0, c1 = 0.0;
#pragma unroll
    for (int m = 0; m < 4; m++) {  // eight rows in flight per wavefront
      hs_d2 v[8];
      double p[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = tile[(wave + 4 * (8 * m + u)) * (HP_T / 2) + lane];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const double xr = xa[wave + 4 * (8 * m + u)];
        c0 += v[u].x * xr, c1 += v[u].y * xr;
        p[u] = v[u].x * xb0 + v[u].y * xb1;
      }
      acc[m] += hp_wave_sum8(p, lane);
    }
    if (b == a) continue;  // (uniform over the workgroup)
    part[wave][2 * lane] = c0, part[wave][2 * lane + 1] = c1;
    __syncthreads();
    if (threadIdx.x < HP_T)
      scr[d.oS + (hp_slot_base(b, d.nt) + hp_chunks(b) + (a - b - 1)) * HP_T + threadIdx.x] =
          ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    __syncthreads();
  }
  if (lane & 7) return;
  double *row_slot = scr + d.oS + (hp_slot_base(a, d.nt) + ch) * HP_T;
#pragma unroll
  for (int m = 0; m < 4; m++) row_slot[wave + 4 * (8 * m + hp_row_of(lane))] = acc[m];
}
// ... and the slots of a row tile summed in their order: workgroup (r, k), a lane per row
__global__ void __launch_bounds__(HP_T) k_hp_symv_finish(const HpDesc *__restrict__ desc, const double *__restrict__ scr, double *__restrict__ y) {
  const HpDesc d = desc[blockIdx.y];
  const int r = blockIdx.x, i = r * HP_T + threadIdx.x;
  if (r >= d.nt || i >= d.nz) return;
  const double *s = scr + d.oS + hp_slot_base(r, d.nt) * HP_T + threadIdx.x;
  const int cnt = hp_chunks(r) + d.nt - 1 - r;
  double sum = 0.0;
  for (int c = 0; c < cnt; c++) sum += s[(long long)c * HP_T];
  y[d.col0 + i] = sum;
}

}  // namespace stg
