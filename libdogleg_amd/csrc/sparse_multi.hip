// sparse_multi.hip -- blocked multi-right-hand-side solves with the resident supernodal factor
// (SURVEY 8f-3): (JtJ + lambda I) U = R for MR = 16 right-hand sides per pass over the factor,
// replacing cholmod_solve / cholmod_spsolve on a dense block of right-hand sides (reference:
// pseudoinverse_J_sparse dogleg.c:1863-1921, cholmod_spsolve 2864-2868).
//
// Layout: the MR right-hand sides are interleaved, element (variable k, rhs c) at [k*MR + c], so
// a supernode's rows are contiguous 128-byte records.  Per supernode and sweep one workgroup:
//   forward   y_t = L_tt^-1 (b_t - gathered updates);  U = L_below y_t  (r x 16) on the matrix
//             cores: A = a 16-row tile of L_below read straight from HBM (each entry of the panel
//             exactly once for all 16 right-hand sides), B = y_t from LDS (v_mfma_f64_16x16x4_f64);
//   backward  x_t = L_tt^-T (y_t - L_below^T x_below): the mat-mat product again on the matrix
//             cores, L_below staged through LDS in chunks of 32 rows (coalesced reads).
// The triangular part keeps L_tt as a packed lower triangle in LDS (w <= 128) and runs one
// barrier per column with thread = (right-hand side, row group).
#include "sparse_internal.h"
#include <algorithm>
#include <cfloat>
#include <cstdint>

namespace {
constexpr int MR = 16;                 // right-hand sides per pass
constexpr int MS_WMAX = 128;           // widest supernode these kernels take
typedef double ms_v4d __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int tri(int i, int j) { return i*(i + 1)/2 + j; }     // packed lower triangle, row-major

// stage the w x w top block of panel L (column-major, ld = nrows) as a packed lower triangle + reciprocal pivots
__device__ __forceinline__ void ms_stage_top(const double* __restrict__ L, int nrows, int w, double* Lt, double* dinv, int tid)
{
  for(int e = tid; e < w*w; e += TPB)
  {
    const int j = e / w, i = e - j*w;
    if(i >= j) { const double v = L[i + (size_t)j*nrows]; Lt[tri(i, j)] = v; if(i == j) dinv[j] = 1.0/v; }
  }
}

__global__ void __launch_bounds__(TPB) k_msolve_fwd_level(const int* __restrict__ lvl_sn,
                                                          const int* __restrict__ sn_c0,
                                                          const int* __restrict__ sn_rowptr,
                                                          const int64_t* __restrict__ sn_lx,
                                                          const int* __restrict__ sn_scr,
                                                          const int* __restrict__ rl_ptr,
                                                          const int* __restrict__ rl_pos,
                                                          const int* __restrict__ perm,
                                                          const double* __restrict__ Lx,
                                                          const double* __restrict__ B,
                                                          double* __restrict__ scr,
                                                          double* __restrict__ Y)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int s = lvl_sn[blockIdx.x];
  const int c0 = sn_c0[s], w = sn_c0[s+1] - c0;
  const int nrows = sn_rowptr[s+1] - sn_rowptr[s];
  const int r = nrows - w - 1;                    // the augmented row is not part of these solves
  const double* L = Lx + sn_lx[s];
  const int tid = threadIdx.x, c = tid & (MR - 1), g = tid >> 4;      // 16 row groups
  double* Lt = lds;                               // packed lower triangle
  double* dinv = Lt + ((w*(w + 1)/2 + 1) & ~1);
  double* Ys = dinv + ((w + 1) & ~1);             // [w][MR] running right-hand sides
  double* Yd = Ys + w*MR;                         // [w][MR] the solution y_t
  ms_stage_top(L, nrows, w, Lt, dinv, tid);
  for(int j = g; j < w; j += TPB/MR)
  {
    const int k = c0 + j;
    double sum = 0.0;
    for(int e = rl_ptr[k]; e < rl_ptr[k+1]; e++) sum += scr[(size_t)rl_pos[e]*MR + c];
    Ys[j*MR + c] = B[(size_t)perm[k]*MR + c] - sum;
  }
  __syncthreads();
  for(int j = 0; j < w; j++)
  {
    const double yj = Ys[j*MR + c]*dinv[j];
    if(g == (j & 15)) Yd[j*MR + c] = yj;
    for(int i = j + 1 + g; i < w; i += TPB/MR) Ys[i*MR + c] -= Lt[tri(i, j)]*yj;
    __syncthreads();
  }
  for(int j = g; j < w; j += TPB/MR) Y[(size_t)(c0 + j)*MR + c] = Yd[j*MR + c];
  // U = L_below y_t on the matrix cores: a wave takes row tiles of 16
  const int lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  double* U = scr + (size_t)sn_scr[s]*MR;
  for(int t = wv; 16*t < r; t += TPB/64)
  {
    const int row = 16*t + mm;
    const double* Lr = L + w + min(row, r - 1);
    ms_v4d acc = {0.0, 0.0, 0.0, 0.0};
    for(int k4 = 0; k4 < w; k4 += 8)
    {
      // two k-steps per round, their loads issued together
      const int ka = k4 + kq, kb = k4 + 4 + kq;
      const double a0 = (ka < w && row < r) ? Lr[(size_t)ka*nrows] : 0.0;
      const double a1 = (kb < w && row < r) ? Lr[(size_t)kb*nrows] : 0.0;
      const double b0 = (ka < w) ? Yd[ka*MR + mm] : 0.0;
      const double b1 = (kb < w) ? Yd[kb*MR + mm] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
    }
#pragma unroll
    for(int q = 0; q < 4; q++) { const int i = 16*t + kq + 4*q; if(i < r) U[(size_t)i*MR + mm] = acc[q]; }
  }
}

constexpr int MS_CH = 32;              // below rows staged per round of the backward product
__global__ void __launch_bounds__(TPB) k_msolve_bwd_level(const int* __restrict__ lvl_sn,
                                                          const int* __restrict__ sn_c0,
                                                          const int* __restrict__ sn_rowptr,
                                                          const int* __restrict__ sn_rows,
                                                          const int64_t* __restrict__ sn_lx,
                                                          const int* __restrict__ perm,
                                                          const double* __restrict__ Lx,
                                                          double* __restrict__ Y,       // in: y (permuted), out: x (permuted)
                                                          double* __restrict__ out)     // x in the original variable order
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int s = lvl_sn[blockIdx.x];
  const int c0 = sn_c0[s], w = sn_c0[s+1] - c0;
  const int nrows = sn_rowptr[s+1] - sn_rowptr[s];
  const int* rows = sn_rows + sn_rowptr[s];
  const int r = nrows - w - 1;
  const double* L = Lx + sn_lx[s];
  const int tid = threadIdx.x, c = tid & (MR - 1), g = tid >> 4;
  const int lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  double* Lt = lds;
  double* dinv = Lt + ((w*(w + 1)/2 + 1) & ~1);
  double* Vs = dinv + ((w + 1) & ~1);             // [w][MR] y_t - L_below^T x_below
  double* Xd = Vs + w*MR;                         // [w][MR] the solution x_t
  double* Ls = Xd + w*MR;                         // [w][MS_CH + 1] a chunk of L_below, column j at Ls + j*(MS_CH + 1)
  double* Xs = Ls + w*(MS_CH + 1);                // [MS_CH][MR] x at the chunk's rows
  ms_stage_top(L, nrows, w, Lt, dinv, tid);
  // V = L_below^T X_below: wave wv owns the column tiles wv, wv + 4 (w <= 128: at most two)
  ms_v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  const int t0 = wv, t1 = wv + TPB/64;
  for(int i0 = 0; i0 < r; i0 += MS_CH)
  {
    const int nr = min(MS_CH, r - i0);
    __syncthreads();
    for(int e = tid; e < MS_CH*w; e += TPB)
    {
      const int j = e / MS_CH, i = e - j*MS_CH;                 // consecutive threads: consecutive rows of one column
      Ls[j*(MS_CH + 1) + i] = (i < nr) ? L[w + i0 + i + (size_t)j*nrows] : 0.0;
    }
    for(int e = tid; e < MS_CH*MR; e += TPB)
    {
      const int i = e / MR, cc = e - i*MR;
      Xs[e] = (i < nr) ? Y[(size_t)rows[w + i0 + i]*MR + cc] : 0.0;
    }
    __syncthreads();
    for(int k4 = 0; k4 < MS_CH; k4 += 4)
    {
      const double b = Xs[(k4 + kq)*MR + mm];
      if(16*t0 < w) acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ls[min(16*t0 + mm, w - 1)*(MS_CH + 1) + k4 + kq], b, acc0, 0, 0, 0);
      if(16*t1 < w) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(Ls[min(16*t1 + mm, w - 1)*(MS_CH + 1) + k4 + kq], b, acc1, 0, 0, 0);
    }
  }
  __syncthreads();
  // D[i][n]: this lane holds rows i = kq + 4q of its tiles, column n = mm
#pragma unroll
  for(int q = 0; q < 4; q++)
  {
    const int j0 = 16*t0 + kq + 4*q, j1 = 16*t1 + kq + 4*q;
    if(j0 < w) Vs[j0*MR + mm] = Y[(size_t)(c0 + j0)*MR + mm] - acc0[q];
    if(j1 < w) Vs[j1*MR + mm] = Y[(size_t)(c0 + j1)*MR + mm] - acc1[q];
  }
  __syncthreads();
  for(int j = w - 1; j >= 0; j--)
  {
    const double xj = Vs[j*MR + c]*dinv[j];
    if(g == (j & 15)) Xd[j*MR + c] = xj;
    for(int i = g; i < j; i += TPB/MR) Vs[i*MR + c] -= Lt[tri(j, i)]*xj;        // (L^T)[i][j] = L[j][i]
    __syncthreads();
  }
  for(int j = g; j < w; j += TPB/MR)
  {
    const double v = Xd[j*MR + c];
    Y[(size_t)(c0 + j)*MR + c] = v;
    out[(size_t)perm[c0 + j]*MR + c] = v;
  }
}

// column-major (ld = N) block of ncols <= MR columns <-> interleaved [N][MR] (unused columns zero)
__global__ void __launch_bounds__(TPB) k_cols_to_interleaved(const double* __restrict__ cols, int N, int ncols, double* __restrict__ il)
{
  const size_t e = (size_t)blockIdx.x*TPB + threadIdx.x;
  if(e >= (size_t)N*MR) return;
  const int k = (int)(e / MR), c = (int)(e % MR);
  il[e] = (c < ncols) ? cols[(size_t)c*N + k] : 0.0;
}
__global__ void __launch_bounds__(TPB) k_interleaved_to_cols(const double* __restrict__ il, int N, int ncols, double* __restrict__ cols)
{
  const size_t e = (size_t)blockIdx.x*TPB + threadIdx.x;
  if(e >= (size_t)N*ncols) return;
  const int c = (int)(e / N), k = (int)(e % N);
  cols[e] = il[(size_t)k*MR + c];
}
// interleaved block of Jt[:, row0 : row0 + ncols] from the rank-local CSC pattern / values (zero elsewhere)
__global__ void __launch_bounds__(TPB) k_jt_chunk_sparse(const int* __restrict__ Jp, const int* __restrict__ Ji,
                                                         const double* __restrict__ Jv, int row0, int ncols,
                                                         double* __restrict__ il)
{
  const int c = blockIdx.x;
  if(c >= ncols) return;
  for(int q = Jp[row0 + c] + threadIdx.x; q < Jp[row0 + c + 1]; q += TPB) il[(size_t)Ji[q]*MR + c] = Jv[q];
}

// ---- leverage blocks A_f = V_f^T V_f, V_f = L^-1 P J_f^T (sparse_leverage_reach) --------------------------------------
// The right-hand side of a chunk (16 rows of J) is non-zero on the columns its rows touch, so V is non-zero only on the
// supernodes that are ancestors of theirs: the chunk's reach, a few paths to the root.  One workgroup per (chunk, supernode)
// pair of a level, many chunks per launch.  The forward kernel above gathers every descendant's update through the
// rl lists; here the sources are the chunk's own pairs in front of this one (sorted by level), each with the rows of its
// update block that fall into this supernode's columns -- a supernode outside the reach is never looked at, so the scratch
// needs no clearing between chunks.  The workgroup sums the Gram products its features need over its own w rows of V into
// a slot of its own; V never leaves LDS.
constexpr int LEV_SRC = TPB;           // sources looked up per round

// Gram partials of the w x MR block Y: 8 row groups of 32 products, added up in a fixed order
__device__ __forceinline__ void lev_gram_block(const double* Y, int w, int fs, double* red, double* __restrict__ out, int tid)
{
  const int p = tid & 31, g = tid >> 5, np = lev_np(fs);
  double acc = 0.0;
  if(p < np) { int a, c; lev_prod(fs, p, a, c); for(int j = g; j < w; j += TPB/32) acc += Y[j*MR + a]*Y[j*MR + c]; }
  red[tid] = acc;
  __syncthreads();
  if(tid < np) { double sum = 0.0; for(int q = 0; q < TPB/32; q++) sum += red[q*32 + tid]; out[tid] = sum; }
}

__device__ __forceinline__ int lev_lower_bound(const int* __restrict__ v, int n, int key)
{
  int lo = 0, hi = n;
  while(lo < hi) { const int mid = (lo + hi) >> 1; if(v[mid] < key) lo = mid + 1; else hi = mid; }
  return lo;
}

// the shared steps of the reach-restricted forward kernels (k_lev_fwd_level, k_cov_fwd_level), one (chunk, supernode) pair
// per workgroup.  The updates of the chunk's pairs in front of pair p (pairs p0 .. p - 1): rows of their update blocks
// inside [c0, c0 + w), subtracted from Ys in pair order.
__device__ __forceinline__ void reach_gather(int p0, int p, int c0, int w, const int* __restrict__ pair_sn,
                                             const int64_t* __restrict__ pair_off, const int* __restrict__ sn_c0,
                                             const int* __restrict__ sn_rowptr, const int* __restrict__ sn_rows,
                                             const double* __restrict__ scr, int* src_i0, int* src_i1, double* Ys, int tid)
{
  for(int b0 = p0; b0 < p; b0 += LEV_SRC)
  {
    const int nb = min(LEV_SRC, p - b0);
    __syncthreads();
    if(tid < nb)
    {
      const int d = pair_sn[b0 + tid], wd = sn_c0[d+1] - sn_c0[d];
      const int rd = sn_rowptr[d+1] - sn_rowptr[d] - wd - 1;
      const int* rows = sn_rows + sn_rowptr[d] + wd;
      src_i0[tid] = lev_lower_bound(rows, rd, c0);
      src_i1[tid] = lev_lower_bound(rows, rd, c0 + w);
    }
    __syncthreads();
    for(int t = 0; t < nb; t++)
    {
      const int i0 = src_i0[t], i1 = src_i1[t];
      if(i0 == i1) continue;                      // (the same for every thread)
      const int d = pair_sn[b0 + t];
      const int* rows = sn_rows + sn_rowptr[d] + (sn_c0[d+1] - sn_c0[d]);
      const double* U = scr + (size_t)pair_off[b0 + t]*MR;
      for(int e = tid; e < (i1 - i0)*MR; e += TPB)
      {
        const int i = i0 + e / MR, cc = e & (MR - 1);
        Ys[(rows[i] - c0)*MR + cc] -= U[(size_t)i*MR + cc];
      }
      __syncthreads();
    }
  }
  __syncthreads();
}
// y_t = L_tt^-1 Ys, column by column (thread = right-hand side c, row group g), into Yd
__device__ __forceinline__ void reach_sweep(const double* Lt, const double* dinv, int w, double* Ys, double* Yd, int c, int g)
{
  for(int j = 0; j < w; j++)
  {
    const double yj = Ys[j*MR + c]*dinv[j];
    if(g == (j & 15)) Yd[j*MR + c] = yj;
    for(int i = j + 1 + g; i < w; i += TPB/MR) Ys[i*MR + c] -= Lt[tri(i, j)]*yj;
    __syncthreads();
  }
}
// U = L_below y_t (r x MR) on the matrix cores: a wave takes row tiles of 16
__device__ __forceinline__ void reach_below(const double* __restrict__ L, int nrows, int w, int r, const double* Yd,
                                            double* __restrict__ U, int tid)
{
  const int lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  for(int t = wv; 16*t < r; t += TPB/64)
  {
    const int row = 16*t + mm;
    const double* Lr = L + w + min(row, r - 1);
    ms_v4d acc = {0.0, 0.0, 0.0, 0.0};
    for(int k4 = 0; k4 < w; k4 += 8)
    {
      const int ka = k4 + kq, kb = k4 + 4 + kq;
      const double a0 = (ka < w && row < r) ? Lr[(size_t)ka*nrows] : 0.0;
      const double a1 = (kb < w && row < r) ? Lr[(size_t)kb*nrows] : 0.0;
      const double b0 = (ka < w) ? Yd[ka*MR + mm] : 0.0;
      const double b1 = (kb < w) ? Yd[kb*MR + mm] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
    }
#pragma unroll
    for(int q = 0; q < 4; q++) { const int i = 16*t + kq + 4*q; if(i < r) U[(size_t)i*MR + mm] = acc[q]; }
  }
}

__global__ void __launch_bounds__(TPB) k_lev_fwd_level(const int* __restrict__ wl,
                                                       const int* __restrict__ pair_sn,
                                                       const int* __restrict__ pair_ch,
                                                       const int64_t* __restrict__ pair_off,
                                                       const int* __restrict__ cp_ptr,
                                                       const int* __restrict__ sn_c0,
                                                       const int* __restrict__ sn_rowptr,
                                                       const int* __restrict__ sn_rows,
                                                       const int64_t* __restrict__ sn_lx,
                                                       const int* __restrict__ iperm,
                                                       const int* __restrict__ Jp,
                                                       const int* __restrict__ Ji,
                                                       const double* __restrict__ Jv,
                                                       const double* __restrict__ Lx,
                                                       int nrow_feat, int fs,
                                                       double* __restrict__ scr,
                                                       double* __restrict__ gram)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int src_i0[LEV_SRC], src_i1[LEV_SRC];
  __shared__ double red[TPB];
  const int p = wl[blockIdx.x], s = pair_sn[p], ch = pair_ch[p];
  const int c0 = sn_c0[s], w = sn_c0[s+1] - c0;
  const int nrows = sn_rowptr[s+1] - sn_rowptr[s];
  const int r = nrows - w - 1;                    // the augmented row is not part of these solves
  const double* L = Lx + sn_lx[s];
  const int tid = threadIdx.x, c = tid & (MR - 1), g = tid >> 4;
  double* Lt = lds;
  double* dinv = Lt + ((w*(w + 1)/2 + 1) & ~1);
  double* Ys = dinv + ((w + 1) & ~1);
  double* Yd = Ys + w*MR;
  ms_stage_top(L, nrows, w, Lt, dinv, tid);
  for(int e = tid; e < w*MR; e += TPB) Ys[e] = 0.0;
  __syncthreads();
  // right-hand side: the chunk's rows of J at this supernode's columns, one thread per row, in the row's order
  if(tid < MR)
  {
    const int row = ch*MR + tid;
    if(row < nrow_feat)
      for(int q = Jp[row]; q < Jp[row+1]; q++) { const int k = iperm[Ji[q]] - c0; if(k >= 0 && k < w) Ys[k*MR + tid] += Jv[q]; }
  }
  reach_gather(cp_ptr[ch], p, c0, w, pair_sn, pair_off, sn_c0, sn_rowptr, sn_rows, scr, src_i0, src_i1, Ys, tid);
  reach_sweep(Lt, dinv, w, Ys, Yd, c, g);
  lev_gram_block(Yd, w, fs, red, gram + (size_t)p*LEV_NP, tid);
  reach_below(L, nrows, w, r, Yd, scr + (size_t)pair_off[p]*MR, tid);   // into this pair's update block
}

// ---- covariance blocks (sparse_covariance_reach): the same forward solves with unit right-hand sides.  Column c of a chunk
// is e at the permuted index pcol[c] (-1: unused), so it is non-zero only on the path from that column's supernode to the
// root.  The pair stores the Gram products Yd^T Yd its chunk needs (prod: a*16 + c, a <= c) in its own slot.
// Query covariance (sparse_query_reach_run) runs the same kernel with right-hand sides from a caller's CSR (RhsCsr).
struct RhsUnit
{
  const int* __restrict__ pcol;
  __device__ __forceinline__ void load(int ch, int c0, int w, double* Ys, int tid) const
  { if(tid < MR) { const int k = pcol[(size_t)ch*MR + tid] - c0; if(k >= 0 && k < w) Ys[k*MR + tid] = 1.0; } }
};
// column c of chunk ch is row crow[ch] + c of the CSR (rp, pv: permuted indices, val), if below crow[ch + 1]; one thread per
// row, in the row's order (duplicates summed, as k_lev_fwd_level loads J)
struct RhsCsr
{
  const int* __restrict__ crow; const int* __restrict__ rp; const int* __restrict__ pv; const double* __restrict__ val;
  __device__ __forceinline__ void load(int ch, int c0, int w, double* Ys, int tid) const
  {
    if(tid < MR)
    {
      const int row = crow[ch] + tid;
      if(row < crow[ch+1])
        for(int q = rp[row]; q < rp[row+1]; q++) { const int k = pv[q] - c0; if(k >= 0 && k < w) Ys[k*MR + tid] += val[q]; }
    }
  }
};
template <class Rhs>
__global__ void __launch_bounds__(TPB) k_cov_fwd_level(const int* __restrict__ wl,
                                                       const int* __restrict__ pair_sn,
                                                       const int* __restrict__ pair_ch,
                                                       const int64_t* __restrict__ pair_off,
                                                       const int* __restrict__ cp_ptr,
                                                       const int* __restrict__ sn_c0,
                                                       const int* __restrict__ sn_rowptr,
                                                       const int* __restrict__ sn_rows,
                                                       const int64_t* __restrict__ sn_lx,
                                                       const double* __restrict__ Lx,
                                                       Rhs rhs,
                                                       const int* __restrict__ pptr,
                                                       const int* __restrict__ prod,
                                                       const int64_t* __restrict__ goff,
                                                       double* __restrict__ scr,
                                                       double* __restrict__ gram)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int src_i0[LEV_SRC], src_i1[LEV_SRC];
  __shared__ double red[MR*MR];
  const int p = wl[blockIdx.x], s = pair_sn[p], ch = pair_ch[p];
  const int c0 = sn_c0[s], w = sn_c0[s+1] - c0;
  const int nrows = sn_rowptr[s+1] - sn_rowptr[s];
  const int r = nrows - w - 1;
  const double* L = Lx + sn_lx[s];
  const int tid = threadIdx.x, c = tid & (MR - 1), g = tid >> 4;
  double* Lt = lds;
  double* dinv = Lt + ((w*(w + 1)/2 + 1) & ~1);
  double* Ys = dinv + ((w + 1) & ~1);
  double* Yd = Ys + w*MR;
  ms_stage_top(L, nrows, w, Lt, dinv, tid);
  for(int e = tid; e < w*MR; e += TPB) Ys[e] = 0.0;
  __syncthreads();
  rhs.load(ch, c0, w, Ys, tid);
  reach_gather(cp_ptr[ch], p, c0, w, pair_sn, pair_off, sn_c0, sn_rowptr, sn_rows, scr, src_i0, src_i1, Ys, tid);
  reach_sweep(Lt, dinv, w, Ys, Yd, c, g);
  // Gram Yd^T Yd (16 x 16) on the matrix cores, one wave, K = w padded to a multiple of 4: A[i][k] = Yd[k][i] and
  // B[k][j] = Yd[k][j] are the same lane value; D[i][j] is register q of lane 16*kq + j with i = kq + 4 q (the f64 map)
  if(tid < 64)
  {
    const int mm = tid & 15, kq = tid >> 4;
    ms_v4d acc = {0.0, 0.0, 0.0, 0.0};
    for(int k4 = 0; k4 < w; k4 += 4)
    {
      const double a = (k4 + kq < w) ? Yd[(k4 + kq)*MR + mm] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
    }
#pragma unroll
    for(int q = 0; q < 4; q++) red[(kq + 4*q)*MR + mm] = acc[q];
  }
  __syncthreads();
  const int q0 = pptr[ch], np = pptr[ch+1] - q0;
  if(tid < np) gram[goff[p] + tid] = red[prod[q0 + tid]];
  reach_below(L, nrows, w, r, Yd, scr + (size_t)pair_off[p]*MR, tid);
}

// the Gram products of a chunk from its solved block U = (JtJ + lambda I)^-1 Jt[:, rows] (interleaved, original order):
// A[a][c] = J[row0 + a] . U[:, c], one thread per product (the full-sweep route)
__global__ void __launch_bounds__(64) k_lev_gram_rows(const int* __restrict__ Jp, const int* __restrict__ Ji,
                                                      const double* __restrict__ Jv, int row0, int nrows, int fs,
                                                      const double* __restrict__ U, double* __restrict__ out)
{
  const int p = threadIdx.x;
  if(p >= lev_np(fs)) return;
  int a, c; lev_prod(fs, p, a, c);
  double acc = 0.0;
  if(a < nrows) for(int q = Jp[row0 + a]; q < Jp[row0 + a + 1]; q++) acc += Jv[q]*U[(size_t)Ji[q]*MR + c];
  out[p] = acc;
}

// per feature: its chunk's slots summed in order; mode 0: the packed block, mode 1: the outlierness factor
__global__ void __launch_bounds__(TPB) k_lev_finish(int nf, int fs, const int* __restrict__ slot_ptr,
                                                    const double* __restrict__ gram, const double* __restrict__ x,
                                                    double scale, int mode, double* __restrict__ out)
{
  const int f = blockIdx.x*TPB + threadIdx.x;
  if(f >= nf) return;
  const int nfc = MR/fs, ch = f / nfc, nt = lev_nt(fs), o = (f - ch*nfc)*nt;
  const int q0 = slot_ptr ? slot_ptr[ch] : ch, q1 = slot_ptr ? slot_ptr[ch+1] : ch + 1;
  double A[3] = {0.0, 0.0, 0.0};
  for(int q = q0; q < q1; q++)
    for(int e = 0; e < nt; e++) A[e] += gram[(size_t)q*LEV_NP + o + e];
  if(mode == 0) { for(int e = 0; e < nt; e++) out[(size_t)f*nt + e] = A[e]; return; }
  const double k = scale/8.0;
  if(fs == 1)
  {
    // x_f^2 / (1 - a)
    const double den = 1.0 - A[0];
    out[f] = (fabs(den) < 1e-8) ? DBL_MAX : x[f]*x[f]/den*k;
    return;
  }
  // B = (A_f - I)^-1 = adj / det; x^T (B + B^2) x = (x^T adj x) / det + |adj x|^2 / det^2
  const double m00 = A[0] - 1.0, m01 = A[1], m11 = A[2] - 1.0;
  const double det = m00*m11 - m01*m01;
  if(fabs(det) < 1e-8) { out[f] = DBL_MAX; return; }
  const double x0 = x[2*f], x1 = x[2*f + 1];
  const double j00 = m11, j01 = -m01, j11 = m00;           // adjugate of A_f - I
  const double xBx = (x0*x0*j00 + 2.0*x0*x1*j01 + x1*x1*j11)/det;
  const double v0 = x0*j00 + x1*j01, v1 = x0*j01 + x1*j11;
  out[f] = (xBx + (v0*v0 + v1*v1)/(det*det))*k;
}

// covariance: per output element e, the product e_p[e] of chunk e_ch[e], its slots summed in order (slot q at goff[q];
// the slots of chunk ch: [slot_ptr[ch], slot_ptr[ch + 1]))
__global__ void __launch_bounds__(TPB) k_cov_finish(long ne, const int* __restrict__ e_ch, const int* __restrict__ e_p,
                                                    const int* __restrict__ slot_ptr, const int64_t* __restrict__ goff,
                                                    const double* __restrict__ gram, double* __restrict__ out)
{
  const long e = (long)blockIdx.x*TPB + threadIdx.x;
  if(e >= ne) return;
  const int ch = e_ch[e], t = e_p[e];
  double acc = 0.0;
  for(int q = slot_ptr[ch]; q < slot_ptr[ch+1]; q++) acc += gram[goff[q] + t];
  out[e] = acc;
}
// the full-sweep route: unit right-hand sides of chunk ch (variables var[c], original order, -1: none), interleaved
__global__ void __launch_bounds__(TPB) k_cov_unit_il(const int* __restrict__ var, int ch, int N, double* __restrict__ il)
{
  const size_t e = (size_t)blockIdx.x*TPB + threadIdx.x;
  if(e >= (size_t)N*MR) return;
  const int k = (int)(e / MR), c = (int)(e % MR);
  il[e] = (var[(size_t)ch*MR + c] == k) ? 1.0 : 0.0;
}
// ... and its products from the solved block X = Sigma[:, var]: product (a, c) is X[var[a]][c]
__global__ void __launch_bounds__(TPB) k_cov_pick(const int* __restrict__ var, const int* __restrict__ pptr,
                                                  const int* __restrict__ prod, const int64_t* __restrict__ goff, int ch,
                                                  const double* __restrict__ X, double* __restrict__ gram)
{
  const int t = threadIdx.x, q0 = pptr[ch];
  if(t >= pptr[ch+1] - q0) return;
  const int a = prod[q0 + t] / MR, c = prod[q0 + t] % MR;
  gram[goff[ch] + t] = X[(size_t)var[(size_t)ch*MR + a]*MR + c];
}

size_t ms_lds_fwd(int w) { return sizeof(double)*(size_t)(((w*(w + 1)/2 + 1) & ~1) + ((w + 1) & ~1) + 2*w*MR); }
size_t ms_lds_bwd(int w) { return ms_lds_fwd(w) + sizeof(double)*(size_t)(w*(MS_CH + 1) + MS_CH*MR); }
} // namespace

int sparse_multi_width_ok(const dlg_backend* b)
{
  const SymHost& H = b->sym->H;
  for(int s = 0; s < H.nsn; s++) if(H.sn_c0[s+1] - H.sn_c0[s] > MS_WMAX) return 0;
  return H.part_nranks <= 1;
}
int sparse_multi_rhs() { return MR; }

// d_il: [N][MR] interleaved right-hand sides in the ORIGINAL variable order; solved in place
int sparse_solve_multi(dlg_backend* b, double* d_il)
{
  SparseSym* Y = b->sym;
  if(!Y) { dlg_set_error("dlg_sparse_set_pattern must be called first"); return DLG_ERR_STATE; }
  const SymHost& H = Y->H;
  hipStream_t st = b->stream;
  if(!Y->ms_scr)
  {
    DLG_HIP(hipMalloc(&Y->ms_scr, sizeof(double)*((size_t)H.scr_size + 1)*MR)); Y->allocs.push_back(Y->ms_scr);
    DLG_HIP(hipMalloc(&Y->ms_y, sizeof(double)*(size_t)H.N*MR)); Y->allocs.push_back(Y->ms_y);
    int wmax = 1;
    for(int s = 0; s < H.nsn; s++) wmax = std::max(wmax, H.sn_c0[s+1] - H.sn_c0[s]);
    Y->ms_lds_f = (int)ms_lds_fwd(wmax); Y->ms_lds_b = (int)ms_lds_bwd(wmax);
    DLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_msolve_fwd_level), hipFuncAttributeMaxDynamicSharedMemorySize, Y->ms_lds_f));
    DLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_msolve_bwd_level), hipFuncAttributeMaxDynamicSharedMemorySize, Y->ms_lds_b));
  }
  for(int l = 0; l < H.nlevels; l++)
  {
    const int n = H.xl_ptr[l+1] - H.xl_ptr[l];
    if(n > 0)
      hipLaunchKernelGGL(k_msolve_fwd_level, dim3(n), dim3(TPB), Y->ms_lds_f, st, Y->xl_sn + H.xl_ptr[l], Y->sn_c0,
                         Y->sn_rowptr, Y->sn_lx, Y->sn_scr, Y->rl_ptr, Y->rl_pos, Y->perm, Y->Lx, d_il, Y->ms_scr, Y->ms_y);
  }
  for(int l = H.nlevels - 1; l >= 0; l--)
  {
    const int n = H.xl_ptr[l+1] - H.xl_ptr[l];
    if(n > 0)
      hipLaunchKernelGGL(k_msolve_bwd_level, dim3(n), dim3(TPB), Y->ms_lds_b, st, Y->xl_sn + H.xl_ptr[l], Y->sn_c0,
                         Y->sn_rowptr, Y->sn_rows, Y->sn_lx, Y->perm, Y->Lx, Y->ms_y, d_il);
  }
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int multi_cols_to_interleaved(dlg_backend* b, const double* d_cols, int ncols, double* d_il)
{
  hipLaunchKernelGGL(k_cols_to_interleaved, dim3(dlg_cdiv((long)b->N*MR, TPB)), dim3(TPB), 0, b->stream, d_cols, b->N, ncols, d_il);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int multi_interleaved_to_cols(dlg_backend* b, const double* d_il, int ncols, double* d_cols)
{
  hipLaunchKernelGGL(k_interleaved_to_cols, dim3(dlg_cdiv((long)b->N*ncols, TPB)), dim3(TPB), 0, b->stream, d_il, b->N, ncols, d_cols);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int sparse_jt_chunk_interleaved(dlg_backend* b, int s, int row0, int ncols, double* d_il)
{
  SparseSym* Y = b->sym;
  DLG_HIP(hipMemsetAsync(d_il, 0, sizeof(double)*(size_t)b->N*MR, b->stream));
  hipLaunchKernelGGL(k_jt_chunk_sparse, dim3(ncols), dim3(TPB), 0, b->stream, Y->Jp, Y->Ji, b->slot[s].Jin(), row0, ncols, d_il);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}

// ---- leverage blocks: the reach of every chunk, launched level by level over many chunks -------------------------------
void reach_plan_release(ReachPlan& P)
{
  for(void* q : {(void*)P.pair_sn, (void*)P.pair_ch, (void*)P.cp_ptr, (void*)P.wl, (void*)P.pair_off, (void*)P.gram, (void*)P.scr})
    if(q) (void)hipFree(q);
  P = ReachPlan();
}
namespace {
constexpr int64_t LEV_BATCH_ROWS = (int64_t)1 << 21;     // update-block rows of the chunks of one batch (256 MB of scratch)

struct ReachHost { std::vector<int> pair_sn, pair_ch, cp_ptr, wl, wl_ptr; std::vector<int64_t> pair_off; int nbatch = 0; int64_t scr_rows = 0; };

// the (chunk, supernode) pairs of nch chunks whose columns start at the supernodes starts(ch, list) lists: every chunk's
// reach (the union of the paths from those to the root) sorted by (level, supernode), chunks cut into batches of at most
// LEV_BATCH_ROWS update-block rows, a batch's pairs listed by level.  Host only.
template <class F> void reach_build(const SymHost& H, int nch, F starts, ReachHost& R)
{
  const int nsn = H.nsn;
  std::vector<int> parent(nsn), rbelow(nsn);
  for(int s = 0; s < nsn; s++)
  {
    const int w = H.sn_c0[s+1] - H.sn_c0[s];
    rbelow[s] = H.sn_rowptr[s+1] - H.sn_rowptr[s] - w - 1;
    parent[s] = rbelow[s] > 0 ? H.col_sn[H.sn_rows[H.sn_rowptr[s] + w]] : -1;   // the supernode of the first row below
  }
  std::vector<int> stamp(nsn, -1), reach, st;
  std::vector<int>& pair_sn = R.pair_sn; std::vector<int>& pair_ch = R.pair_ch; std::vector<int>& cp_ptr = R.cp_ptr;
  cp_ptr.assign(1, 0);
  for(int ch = 0; ch < nch; ch++)
  {
    reach.clear(); st.clear();
    starts(ch, st);
    for(int s0 : st)
      for(int s = s0; s >= 0 && stamp[s] != ch; s = parent[s]) { stamp[s] = ch; reach.push_back(s); }
    std::sort(reach.begin(), reach.end(), [&](int a, int c) { return H.sn_level[a] != H.sn_level[c] ? H.sn_level[a] < H.sn_level[c] : a < c; });
    for(int s : reach) { pair_sn.push_back(s); pair_ch.push_back(ch); }
    cp_ptr.push_back((int)pair_sn.size());
  }
  const int npair = (int)pair_sn.size(), nl = H.nlevels;
  R.pair_off.assign(npair, 0);
  std::vector<int>& wl = R.wl; wl.reserve(npair);
  std::vector<int> cnt(nl);
  R.wl_ptr.assign(1, 0);
  for(int ch0 = 0; ch0 < nch;)
  {
    // a batch: whole chunks while their update blocks fit (at least one chunk)
    int64_t rows = 0; int ch1 = ch0;
    while(ch1 < nch)
    {
      int64_t rc = 0;
      for(int q = cp_ptr[ch1]; q < cp_ptr[ch1+1]; q++) rc += rbelow[pair_sn[q]];
      if(ch1 > ch0 && rows + rc > LEV_BATCH_ROWS) break;
      for(int q = cp_ptr[ch1]; q < cp_ptr[ch1+1]; q++) { R.pair_off[q] = rows; rows += rbelow[pair_sn[q]]; }
      ch1++;
    }
    R.scr_rows = std::max(R.scr_rows, rows);
    std::fill(cnt.begin(), cnt.end(), 0);
    for(int q = cp_ptr[ch0]; q < cp_ptr[ch1]; q++) cnt[H.sn_level[pair_sn[q]]]++;
    const size_t base = wl.size();
    std::vector<size_t> at(nl);
    for(int l = 0, acc = 0; l < nl; l++) { at[l] = base + acc; acc += cnt[l]; R.wl_ptr.push_back((int)(base + acc)); }
    wl.resize(base + (cp_ptr[ch1] - cp_ptr[ch0]));
    for(int q = cp_ptr[ch0]; q < cp_ptr[ch1]; q++) wl[at[H.sn_level[pair_sn[q]]]++] = q;
    R.nbatch++;
    ch0 = ch1;
  }
}
// the device half of a reach plan (its gram is the caller's)
int reach_upload(const ReachHost& R, int nch, ReachPlan& P)
{
  DLG_CHECK(upload(P.pair_sn, R.pair_sn)); DLG_CHECK(upload(P.pair_ch, R.pair_ch)); DLG_CHECK(upload(P.cp_ptr, R.cp_ptr));
  DLG_CHECK(upload(P.wl, R.wl)); DLG_CHECK(upload(P.pair_off, R.pair_off));
  P.wl_ptr = R.wl_ptr; P.nbatch = R.nbatch; P.scr_rows = R.scr_rows;
  DLG_HIP(hipMalloc(&P.scr, sizeof(double)*MR*(size_t)std::max<int64_t>(P.scr_rows, 1)));
  P.nch = nch; P.npair = (int)R.pair_sn.size(); P.visits = P.npair;
  return DLG_OK;
}
// what both reach routes need once per pattern: iperm on the device, the LDS of the widest supernode
int reach_setup(dlg_backend* b)
{
  SparseSym* Y = b->sym;
  const SymHost& H = Y->H;
  if(Y->lev_iperm) return DLG_OK;
  DLG_CHECK(upload(Y->lev_iperm, H.iperm)); Y->allocs.push_back(Y->lev_iperm);
  const int mloc = dlg_mloc(b);
  Y->lev_jp.resize((size_t)mloc + 1);
  DLG_HIP(hipMemcpy(Y->lev_jp.data(), Y->Jp, sizeof(int)*((size_t)mloc + 1), hipMemcpyDeviceToHost));
  Y->lev_ji.resize((size_t)Y->lev_jp[mloc]);
  if(!Y->lev_ji.empty()) DLG_HIP(hipMemcpy(Y->lev_ji.data(), Y->Ji, sizeof(int)*Y->lev_ji.size(), hipMemcpyDeviceToHost));
  int wmax = 1;
  for(int s = 0; s < H.nsn; s++) wmax = std::max(wmax, H.sn_c0[s+1] - H.sn_c0[s]);
  Y->lev_lds = (int)ms_lds_fwd(wmax);
  DLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lev_fwd_level), hipFuncAttributeMaxDynamicSharedMemorySize, Y->lev_lds));
  DLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cov_fwd_level<RhsUnit>), hipFuncAttributeMaxDynamicSharedMemorySize, Y->lev_lds));
  DLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cov_fwd_level<RhsCsr>), hipFuncAttributeMaxDynamicSharedMemorySize, Y->lev_lds));
  return DLG_OK;
}
// the levels of a reach plan that hold pairs, batch after batch: launch(the level's pairs in R.wl, how many)
template <class F> void reach_for_each_level(const ReachPlan& R, int nl, F launch)
{
  for(int bt = 0; bt < R.nbatch; bt++)
    for(int l = 0; l < nl; l++)
    {
      const int w0 = R.wl_ptr[(size_t)bt*nl + l], n = R.wl_ptr[(size_t)bt*nl + l + 1] - w0;
      if(n > 0) launch(R.wl + w0, n);
    }
}
// the supernodes the columns of chunk ch start at: those of its variables (covariance blocks) ...
void cov_starts(const SymHost& H, const CovPack& K, int ch, std::vector<int>& st)
{
  for(int c = 0; c < MR; c++) { const int x = K.var[(size_t)ch*MR + c]; if(x >= 0) st.push_back(H.col_sn[H.iperm[x]]); }
}
// ... those of its rows' variables (query covariance)
void query_starts(const SymHost& H, const CovPack& K, int ch, std::vector<int>& st)
{
  for(int q = K.qrp[K.crow[ch]]; q < K.qrp[K.crow[ch+1]]; q++) st.push_back(H.col_sn[H.iperm[K.qvar[q]]]);
}
// the slots of a packed plan's Gram products.  Reach route: the reach of every chunk from starts(H, K, ch, list), a slot
// of the chunk's products per (chunk, supernode) pair (cov_finish walks R.cp_ptr)
template <class F> int reach_slots(dlg_backend* b, CovPlan& P, F starts)
{
  const SymHost& H = b->sym->H;
  const CovPack& K = P.K;
  DLG_CHECK(reach_setup(b));
  ReachHost R;
  reach_build(H, K.nch, [&](int ch, std::vector<int>& st) { starts(H, K, ch, st); }, R);
  DLG_CHECK(reach_upload(R, K.nch, P.R));
  std::vector<int64_t> goff(R.pair_sn.size() + 1, 0);
  for(size_t q = 0; q < R.pair_sn.size(); q++) { const int ch = R.pair_ch[q]; goff[q+1] = goff[q] + (K.pptr[ch+1] - K.pptr[ch]); }
  DLG_CHECK(upload(P.goff, goff));
  DLG_HIP(hipMalloc(&P.gram, sizeof(double)*(size_t)std::max<int64_t>(goff.back(), 1)));
  return DLG_OK;
}
// ... every other route: one slot per chunk
int chunk_slots(CovPlan& P)
{
  const CovPack& K = P.K;
  std::vector<int> slot_ptr(K.nch + 1);
  std::vector<int64_t> goff(K.nch + 1);
  for(int ch = 0; ch <= K.nch; ch++) { slot_ptr[ch] = ch; goff[ch] = K.pptr[ch]; }
  DLG_CHECK(upload(P.slot_ptr, slot_ptr)); DLG_CHECK(upload(P.goff, goff));
  DLG_HIP(hipMalloc(&P.gram, sizeof(double)*(size_t)std::max(K.pptr.back(), 1)));
  return DLG_OK;
}
// the forward solves of a packed plan's chunks on the supernodes they reach, level by level
template <class Rhs> int reach_run(dlg_backend* b, CovPlan& P, const Rhs& rhs)
{
  SparseSym* Y = b->sym;
  DLG_CHECK(reach_setup(b));                 // (the LDS attribute and size of this pattern's widest supernode)
  const ReachPlan& R = P.R;
  reach_for_each_level(R, Y->H.nlevels, [&](const int* wl, int n) {
    hipLaunchKernelGGL(k_cov_fwd_level<Rhs>, dim3(n), dim3(TPB), Y->lev_lds, b->stream, wl, R.pair_sn, R.pair_ch, R.pair_off,
                       R.cp_ptr, Y->sn_c0, Y->sn_rowptr, Y->sn_rows, Y->sn_lx, Y->Lx, rhs, P.pptr, P.prod, P.goff, R.scr, P.gram);
  });
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}

// the (chunk, supernode) pairs of the chunks of nf features of fs rows
int lev_plan_build(dlg_backend* b, int fs, int nf)
{
  SparseSym* Y = b->sym;
  const SymHost& H = Y->H;
  SparseSym::LevPlan& P = Y->lev[fs - 1];
  if(P.nf == nf) return DLG_OK;
  DLG_HIP(hipStreamSynchronize(b->stream));
  reach_plan_release(P);
  DLG_CHECK(reach_setup(b));
  const int nrow = nf*fs, nch = dlg_cdiv(nrow, MR);
  ReachHost R;
  reach_build(H, nch, [&](int ch, std::vector<int>& st) {
    for(int row = ch*MR; row < std::min(nrow, ch*MR + MR); row++)
      for(int q = Y->lev_jp[row]; q < Y->lev_jp[row+1]; q++) st.push_back(H.col_sn[H.iperm[Y->lev_ji[q]]]);
  }, R);
  DLG_CHECK(reach_upload(R, nch, P));
  DLG_HIP(hipMalloc(&P.gram, sizeof(double)*LEV_NP*(size_t)std::max(P.npair, 1)));
  P.nf = nf;
  return DLG_OK;
}

// ---- covariance blocks: packing requests into chunks (host) ----------------------------------------------------------
// the distinct variables of a request, ascending: one or two ranges
void cov_req_vars(int r0, int nr, int c0, int nc, std::vector<int>& v)
{
  v.clear();
  for(int i = 0; i < nr; i++) v.push_back(r0 + i);
  for(int j = 0; j < nc; j++) v.push_back(c0 + j);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
}
} // namespace

// Requests sorted by the elimination position (permuted column: a postorder of the tree) of their shallowest column, then
// of their deepest (dense: the largest variable, then the smallest), so that requests sharing their shallowest variables
// are neighbours -- in bundle adjustment the points are eliminated first, and a camera's blocks with its points follow
// one another; then packed next-fit into chunks of at most 16 distinct variables, a request whole into one chunk; a
// variable already in the chunk is not repeated.
int cov_pack_requests(int N, const int* iperm, int nreq, const int* r0, const int* nr, const int* c0,
                      const int* nc, CovPack& K, const char* who)
{
  K = CovPack();
  std::vector<int64_t> key_hi(nreq), key_lo(nreq);
  std::vector<int> v;
  for(int q = 0; q < nreq; q++)
  {
    if(nr[q] < 1 || nc[q] < 1 || r0[q] < 0 || c0[q] < 0 || r0[q] > N - nr[q] || c0[q] > N - nc[q])
    { dlg_set_error("%s: request %d (rows %d + %d, columns %d + %d) is empty or outside the %d variables", who, q, r0[q], nr[q], c0[q], nc[q], N); return DLG_ERR_ARG; }
    if(nr[q] > COV_MAXV || nc[q] > COV_MAXV) v.assign(COV_MAXV + 1, 0);
    else cov_req_vars(r0[q], nr[q], c0[q], nc[q], v);
    if((int)v.size() > COV_MAXV)
    { dlg_set_error("%s: request %d spans more than %d distinct variables; take wider blocks of the inverse from dlg_solve_multi with unit columns", who, q, COV_MAXV); return DLG_ERR_ARG; }
    int64_t hi = -1, lo = INT64_MAX;
    for(int x : v) { const int64_t k = iperm ? (int64_t)iperm[x] : (int64_t)x; hi = std::max(hi, k); lo = std::min(lo, k); }
    key_hi[q] = hi; key_lo[q] = lo;
  }
  std::vector<int> ord(nreq);
  for(int q = 0; q < nreq; q++) ord[q] = q;
  std::sort(ord.begin(), ord.end(), [&](int a, int c) { return key_hi[a] != key_hi[c] ? key_hi[a] < key_hi[c] : key_lo[a] != key_lo[c] ? key_lo[a] < key_lo[c] : a < c; });
  K.req_ch.assign(nreq, -1);
  std::vector<int> cur;                      // variables of the open chunk
  std::vector<int> ch_first(1, 0);           // requests of chunk ch: ord[ch_first[ch] .. ch_first[ch + 1])
  for(int i = 0; i < nreq; i++)
  {
    const int q = ord[i];
    cov_req_vars(r0[q], nr[q], c0[q], nc[q], v);
    int add = 0;
    for(int x : v) add += std::find(cur.begin(), cur.end(), x) == cur.end();
    if((int)cur.size() + add > COV_MAXV)
    {
      K.maxvar = std::max(K.maxvar, (int)cur.size());
      for(int c = 0; c < MR; c++) K.var.push_back(c < (int)cur.size() ? cur[c] : -1);
      cur.clear(); ch_first.push_back(i);
    }
    for(int x : v) if(std::find(cur.begin(), cur.end(), x) == cur.end()) cur.push_back(x);
    K.req_ch[q] = (int)ch_first.size() - 1;
  }
  if(nreq > 0)
  {
    K.maxvar = std::max(K.maxvar, (int)cur.size());
    for(int c = 0; c < MR; c++) K.var.push_back(c < (int)cur.size() ? cur[c] : -1);
    ch_first.push_back(nreq);
  }
  K.nch = (int)K.var.size() / MR;
  // products: per chunk in the order its requests first need them; per output value (request order) its product
  std::vector<int> pidx(MR*MR, -1);
  std::vector<int64_t> e0(nreq + 1, 0);
  for(int q = 0; q < nreq; q++) e0[q+1] = e0[q] + (int64_t)nr[q]*nc[q];
  K.e_ch.resize(e0[nreq]); K.e_p.resize(e0[nreq]);
  K.pptr.assign(1, 0);
  for(int ch = 0; ch < K.nch; ch++)
  {
    std::fill(pidx.begin(), pidx.end(), -1);
    const int* vv = K.var.data() + (size_t)ch*MR;
    auto loc = [&](int x) { int c = 0; while(vv[c] != x) c++; return c; };
    for(int i = ch_first[ch]; i < ch_first[ch+1]; i++)
    {
      const int q = ord[i];
      int lr[COV_MAXV], lc[COV_MAXV];
      for(int a = 0; a < nr[q]; a++) lr[a] = loc(r0[q] + a);
      for(int c = 0; c < nc[q]; c++) lc[c] = loc(c0[q] + c);
      for(int a = 0; a < nr[q]; a++)
        for(int c = 0; c < nc[q]; c++)
        {
          const int x = std::min(lr[a], lc[c]), y = std::max(lr[a], lc[c]);
          int& t = pidx[x*MR + y];
          if(t < 0) { t = (int)K.prod.size() - K.pptr[ch]; K.prod.push_back(x*MR + y); }
          const int64_t e = e0[q] + (int64_t)a*nc[q] + c;
          K.e_ch[e] = ch; K.e_p[e] = t;
        }
    }
    K.pptr.push_back((int)K.prod.size());
  }
  return DLG_OK;
}
void cov_pack_marginal(int N, const int* perm, CovPack& K)
{
  K = CovPack();
  K.nch = dlg_cdiv(N, MR);
  K.var.assign((size_t)K.nch*MR, -1);
  K.pptr.assign(1, 0);
  K.e_ch.resize(N); K.e_p.resize(N);
  for(int ch = 0; ch < K.nch; ch++)
  {
    const int n = std::min(MR, N - ch*MR);
    for(int c = 0; c < n; c++)
    {
      const int k = ch*MR + c, x = perm ? perm[k] : k;
      K.var[(size_t)ch*MR + c] = x;
      K.prod.push_back(c*MR + c);
      K.e_ch[x] = ch; K.e_p[x] = c;
    }
    K.pptr.push_back((int)K.prod.size());
    K.maxvar = std::max(K.maxvar, n);
  }
}
void cov_plan_release(CovPlan& P)
{
  for(void* q : {(void*)P.var, (void*)P.kb0, (void*)P.pcol, (void*)P.pptr, (void*)P.prod, (void*)P.e_ch, (void*)P.e_p, (void*)P.slot_ptr,
                 (void*)P.goff, (void*)P.gram, (void*)P.out, (void*)P.crow, (void*)P.qrp, (void*)P.qvar, (void*)P.qval})
    if(q) (void)hipFree(q);
  reach_plan_release(P.R);
  P = CovPlan();
}

// the reach route of a packed plan: the slots, and the chunks' columns in the factor's order
int sparse_cov_reach_plan(dlg_backend* b, CovPlan& P)
{
  const SymHost& H = b->sym->H;
  const CovPack& K = P.K;
  DLG_CHECK(reach_slots(b, P, cov_starts));
  std::vector<int> pcol(K.var.size());
  for(size_t i = 0; i < K.var.size(); i++) pcol[i] = K.var[i] >= 0 ? H.iperm[K.var[i]] : -1;
  return upload(P.pcol, pcol);
}
int sparse_cov_reach_run(dlg_backend* b, CovPlan& P) { return reach_run(b, P, RhsUnit{P.pcol}); }
// build plan P for a route: which 0, the requests; 1, the marginal variances
int cov_plan_build(dlg_backend* b, CovPlan& P, FactorRoute route, int which, int nreq, const int* r0, const int* nr, const int* c0,
                   const int* nc, const char* who)
{
  const SymHost* H = route != ROUTE_DENSE ? &b->sym->H : nullptr;
  if(which == 0) DLG_CHECK(cov_pack_requests(b->N, H ? H->iperm.data() : nullptr, nreq, r0, nr, c0, nc, P.K, who));
  else cov_pack_marginal(b->N, H ? H->perm.data() : nullptr, P.K);
  const CovPack& K = P.K;
  P.ne = (long)K.e_ch.size();
  DLG_CHECK(upload(P.var, K.var)); DLG_CHECK(upload(P.pptr, K.pptr)); DLG_CHECK(upload(P.prod, K.prod));
  DLG_CHECK(upload(P.e_ch, K.e_ch)); DLG_CHECK(upload(P.e_p, K.e_p));
  DLG_HIP(hipMalloc(&P.out, sizeof(double)*(size_t)std::max<long>(P.ne, 1)));
  if(route == ROUTE_REACH) return sparse_cov_reach_plan(b, P);
  if(route == ROUTE_DENSE) DLG_CHECK(dense_cov_setup(b, P));
  return chunk_slots(P);
}
uint64_t sparse_pattern_key(const dlg_backend* b) { return b->sym ? b->sym->pat_key : 0; }
// of a plan that has been run: chunks, supernode visits of all chunks (reach route), supernodes of the pattern
int cov_plan_stats(const dlg_backend* b, const CovPlan& P, long* nchunks, long* visits, int* nsn)
{
  *nchunks = P.K.nch; *visits = P.R.npair > 0 ? P.R.visits : 0; *nsn = b->sym ? b->sym->H.nsn : 0;
  return DLG_OK;
}
int cov_unit_il(dlg_backend* b, const CovPlan& P, int ch, double* d_il)
{
  hipLaunchKernelGGL(k_cov_unit_il, dim3(dlg_cdiv((long)b->N*MR, TPB)), dim3(TPB), 0, b->stream, P.var, ch, b->N, d_il);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int cov_pick(dlg_backend* b, const CovPlan& P, int ch, const double* d_il)
{
  hipLaunchKernelGGL(k_cov_pick, dim3(1), dim3(TPB), 0, b->stream, P.var, P.pptr, P.prod, P.goff, ch, d_il, P.gram);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int cov_finish(dlg_backend* b, const CovPlan& P)
{
  if(P.ne <= 0) return DLG_OK;
  hipLaunchKernelGGL(k_cov_finish, dim3(dlg_cdiv(P.ne, TPB)), dim3(TPB), 0, b->stream, P.ne, P.e_ch, P.e_p,
                     P.R.cp_ptr ? P.R.cp_ptr : P.slot_ptr, P.goff, P.gram, P.out);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}

// host only: the symbolic phase on a pattern and the packing and reach of a request list (the CPU tests check the
// packing without a GPU).  stats: {chunks, pair visits, most distinct variables in a chunk}
extern "C" int dlg_covariance_plan_probe(int N, int M, const int* colptr, const int* rowidx, int nreq, const int* r0,
                                         const int* nr, const int* c0, const int* nc, int* chunk_of_req, long* stats, int nstats)
{
  if(nreq < 0 || (nreq > 0 && (!r0 || !nr || !c0 || !nc))) { dlg_set_error("dlg_covariance_plan_probe: bad argument"); return DLG_ERR_ARG; }
  SymHost H;
  char err[512];
  if(sym_analyze(H, N, M, colptr, rowidx, 0, M, err, sizeof(err))) { dlg_set_error("symbolic analysis: %s", err); return DLG_ERR_ARG; }
  CovPack K;
  DLG_CHECK(cov_pack_requests(N, H.iperm.data(), nreq, r0, nr, c0, nc, K, "dlg_covariance_plan_probe"));
  ReachHost R;
  reach_build(H, K.nch, [&](int ch, std::vector<int>& st) { cov_starts(H, K, ch, st); }, R);
  if(chunk_of_req) for(int q = 0; q < nreq; q++) chunk_of_req[q] = K.req_ch[q];
  const long v[] = { (long)K.nch, (long)R.pair_sn.size(), (long)K.maxvar };
  for(int i = 0; i < nstats && i < 3; i++) stats[i] = v[i];
  return DLG_OK;
}

// ---- query covariance: packing a query batch into chunks (host) -------------------------------------------------------
// Queries whole, greedily in query order, into chunks of at most 16 rows; a query of fs rows keeps the fs (fs + 1) / 2
// products of its own rows; per output value (the queries' full fs x fs blocks, row-major, in query order) its product.
int query_pack(int N, int nq, const int* qrow, const int* rowptr, const int* var, CovPack& K, const char* who)
{
  K = CovPack();
  if(nq < 0 || (nq > 0 && (!qrow || !rowptr || !var))) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  if(nq == 0) return DLG_OK;
  if(qrow[0] < 0) { dlg_set_error("%s: qrow[0] = %d is negative", who, qrow[0]); return DLG_ERR_ARG; }
  for(int k = 0; k < nq; k++)
  {
    const int fs = qrow[k+1] - qrow[k];
    if(fs < 1 || fs > QCOV_MAXROWS)
    { dlg_set_error("%s: query %d has %d rows (1 to %d are taken); take wider queries from dlg_solve_multi on the columns of Jq^T", who, k, fs, QCOV_MAXROWS); return DLG_ERR_ARG; }
  }
  const int r0 = qrow[0], nrow = qrow[nq] - r0, e0 = rowptr[r0];
  K.qrp.resize((size_t)nrow + 1);
  for(int i = 0; i <= nrow; i++)
  {
    K.qrp[i] = rowptr[r0 + i] - e0;
    if(K.qrp[i] < (i ? K.qrp[i-1] : 0)) { dlg_set_error("%s: rowptr decreases at row %d", who, r0 + i); return DLG_ERR_ARG; }
  }
  K.qvar.assign(var + e0, var + e0 + K.qrp[nrow]);
  for(size_t q = 0; q < K.qvar.size(); q++)
    if(K.qvar[q] < 0 || K.qvar[q] >= N) { dlg_set_error("%s: index %d at entry %ld is outside the %d variables", who, K.qvar[q], (long)(e0 + q), N); return DLG_ERR_ARG; }
  K.req_ch.assign(nq, -1);
  K.crow.assign(1, 0);
  for(int k = 0; k < nq; k++)
  {
    const int a0 = qrow[k] - r0, a1 = qrow[k+1] - r0;
    if(a1 - K.crow.back() > MR) K.crow.push_back(a0);
    K.req_ch[k] = (int)K.crow.size() - 1;
  }
  K.crow.push_back(nrow);
  K.nch = (int)K.crow.size() - 1;
  for(int ch = 0; ch < K.nch; ch++) K.maxvar = std::max(K.maxvar, K.crow[ch+1] - K.crow[ch]);
  int64_t ne = 0;
  for(int k = 0; k < nq; k++) ne += (int64_t)(qrow[k+1] - qrow[k])*(qrow[k+1] - qrow[k]);
  K.e_ch.resize(ne); K.e_p.resize(ne);
  K.pptr.assign(1, 0);
  int64_t e = 0;
  for(int k = 0, ch = 0; k < nq; k++)
  {
    for(; ch < K.req_ch[k]; ch++) K.pptr.push_back((int)K.prod.size());
    const int fs = qrow[k+1] - qrow[k], a0 = qrow[k] - r0 - K.crow[ch], p0 = (int)K.prod.size() - K.pptr[ch];
    for(int i = 0; i < fs; i++) for(int j = i; j < fs; j++) K.prod.push_back((a0 + i)*MR + a0 + j);
    // product (i, j), i <= j, of the query at p0 + i fs - i (i - 1) / 2 + (j - i)
    for(int i = 0; i < fs; i++)
      for(int j = 0; j < fs; j++, e++)
      {
        const int x = std::min(i, j), y = std::max(i, j);
        K.e_ch[e] = ch; K.e_p[e] = p0 + x*fs - x*(x - 1)/2 + (y - x);
      }
  }
  while((int)K.pptr.size() <= K.nch) K.pptr.push_back((int)K.prod.size());
  return DLG_OK;
}
// the device half of a query plan: the CSR, per route the slots (route 0: the reach of each chunk, a slot of the chunk's
// products per pair; otherwise a slot per chunk), the values' buffer
int query_plan_build(dlg_backend* b, CovPlan& P, FactorRoute route, int nq, const int* qrow, const int* rowptr, const int* var,
                     const char* who)
{
  DLG_CHECK(query_pack(b->N, nq, qrow, rowptr, var, P.K, who));
  const CovPack& K = P.K;
  P.ne = (long)K.e_ch.size();
  P.qnnz = (long)K.qvar.size();
  DLG_CHECK(upload(P.pptr, K.pptr)); DLG_CHECK(upload(P.prod, K.prod));
  DLG_CHECK(upload(P.e_ch, K.e_ch)); DLG_CHECK(upload(P.e_p, K.e_p));
  DLG_CHECK(upload(P.crow, K.crow)); DLG_CHECK(upload(P.qrp, K.qrp));
  DLG_HIP(hipMalloc(&P.out, sizeof(double)*(size_t)std::max<long>(P.ne, 1)));
  DLG_HIP(hipMalloc(&P.qval, sizeof(double)*(size_t)std::max<long>(P.qnnz, 1)));
  if(route == ROUTE_REACH)
  {
    const SymHost& H = b->sym->H;
    DLG_CHECK(reach_slots(b, P, query_starts));
    std::vector<int> pv(K.qvar.size());
    for(size_t q = 0; q < pv.size(); q++) pv[q] = H.iperm[K.qvar[q]];
    return upload(P.qvar, pv);
  }
  DLG_CHECK(upload(P.qvar, K.qvar));
  if(route == ROUTE_DENSE) DLG_CHECK(dense_cov_setup(b, P));
  return chunk_slots(P);
}
int sparse_query_reach_run(dlg_backend* b, CovPlan& P) { return reach_run(b, P, RhsCsr{P.crow, P.qrp, P.qvar, P.qval}); }
// host only: the symbolic phase on a pattern and the packing and reach of a query batch.  stats: {chunks, pair visits, most
// rows in a chunk}
extern "C" int dlg_query_covariance_plan_probe(int N, int M, const int* colptr, const int* rowidx, int nq, const int* qrow,
                                               const int* rowptr, const int* var, int* chunk_of_query, long* stats, int nstats)
{
  SymHost H;
  char err[512];
  if(sym_analyze(H, N, M, colptr, rowidx, 0, M, err, sizeof(err))) { dlg_set_error("symbolic analysis: %s", err); return DLG_ERR_ARG; }
  CovPack K;
  DLG_CHECK(query_pack(N, nq, qrow, rowptr, var, K, "dlg_query_covariance_plan_probe"));
  ReachHost R;
  reach_build(H, K.nch, [&](int ch, std::vector<int>& st) { query_starts(H, K, ch, st); }, R);
  if(chunk_of_query) for(int k = 0; k < nq; k++) chunk_of_query[k] = K.req_ch[k];
  const long v[] = { (long)K.nch, (long)R.pair_sn.size(), (long)K.maxvar };
  for(int i = 0; i < nstats && i < 3; i++) stats[i] = v[i];
  return DLG_OK;
}

void sparse_leverage_free(SparseSym* Y) { for(auto& P : Y->lev) reach_plan_release(P); }

// Gram products of the first nf features of fs rows through the reach-restricted forward solves; *d_gram / *d_slot_ptr:
// what lev_finish sums
int sparse_leverage_reach(dlg_backend* b, int s, int fs, int nf, double** d_gram, const int** d_slot_ptr, long* visits)
{
  SparseSym* Y = b->sym;
  if(!Y) { dlg_set_error("dlg_sparse_set_pattern must be called first"); return DLG_ERR_STATE; }
  DLG_CHECK(lev_plan_build(b, fs, nf));
  SparseSym::LevPlan& P = Y->lev[fs - 1];
  reach_for_each_level(P, Y->H.nlevels, [&](const int* wl, int n) {
    hipLaunchKernelGGL(k_lev_fwd_level, dim3(n), dim3(TPB), Y->lev_lds, b->stream, wl, P.pair_sn, P.pair_ch, P.pair_off,
                       P.cp_ptr, Y->sn_c0, Y->sn_rowptr, Y->sn_rows, Y->sn_lx, Y->lev_iperm, Y->Jp, Y->Ji, b->slot[s].Jin(),
                       Y->Lx, nf*fs, fs, P.scr, P.gram);
  });
  DLG_LAUNCH_CHECK();
  *d_gram = P.gram; *d_slot_ptr = P.cp_ptr;
  if(visits) *visits = P.visits;
  return DLG_OK;
}
// of the plan held for fs: chunks, supernode visits of all chunks, supernodes of the pattern
int sparse_leverage_stats(const dlg_backend* b, int fs, long* nchunks, long* visits, int* nsn)
{
  const SparseSym* Y = b->sym;
  if(!Y || fs < 1 || fs > 2 || Y->lev[fs - 1].nf < 0) { dlg_set_error("no leverage plan is held for feature size %d", fs); return DLG_ERR_STATE; }
  *nchunks = Y->lev[fs - 1].nch; *visits = Y->lev[fs - 1].visits; *nsn = Y->H.nsn;
  return DLG_OK;
}
int lev_gram_rows(dlg_backend* b, int s, int row0, int nrows, int fs, const double* d_il, double* d_gram)
{
  SparseSym* Y = b->sym;
  hipLaunchKernelGGL(k_lev_gram_rows, dim3(1), dim3(64), 0, b->stream, Y->Jp, Y->Ji, b->slot[s].Jin(), row0, nrows, fs, d_il, d_gram);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int lev_finish(dlg_backend* b, int s, int nf, int fs, const int* d_slot_ptr, const double* d_gram, double scale, int mode, double* d_out)
{
  if(nf <= 0) return DLG_OK;
  hipLaunchKernelGGL(k_lev_finish, dim3(dlg_cdiv(nf, TPB)), dim3(TPB), 0, b->stream, nf, fs, d_slot_ptr, d_gram, b->slot[s].xin(),
                     scale, mode, d_out);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
