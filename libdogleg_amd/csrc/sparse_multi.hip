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
  // the updates of the chunk's pairs in front of this one: rows of their update blocks inside [c0, c0 + w)
  for(int b0 = cp_ptr[ch]; b0 < p; b0 += LEV_SRC)
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
  for(int j = 0; j < w; j++)
  {
    const double yj = Ys[j*MR + c]*dinv[j];
    if(g == (j & 15)) Yd[j*MR + c] = yj;
    for(int i = j + 1 + g; i < w; i += TPB/MR) Ys[i*MR + c] -= Lt[tri(i, j)]*yj;
    __syncthreads();
  }
  lev_gram_block(Yd, w, fs, red, gram + (size_t)p*LEV_NP, tid);
  // U = L_below y_t on the matrix cores, into this pair's update block
  const int lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  double* U = scr + (size_t)pair_off[p]*MR;
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
namespace {
constexpr int64_t LEV_BATCH_ROWS = (int64_t)1 << 21;     // update-block rows of the chunks of one batch (256 MB of scratch)

void lev_plan_release(SparseSym::LevPlan& P)
{
  for(void* q : {(void*)P.pair_sn, (void*)P.pair_ch, (void*)P.cp_ptr, (void*)P.wl, (void*)P.pair_off, (void*)P.gram, (void*)P.scr})
    if(q) (void)hipFree(q);
  P = SparseSym::LevPlan();
}

// the (chunk, supernode) pairs of the chunks of nf features of fs rows: every chunk's reach sorted by (level, supernode),
// chunks cut into batches of at most LEV_BATCH_ROWS update-block rows, a batch's pairs listed by level
int lev_plan_build(dlg_backend* b, int fs, int nf)
{
  SparseSym* Y = b->sym;
  const SymHost& H = Y->H;
  SparseSym::LevPlan& P = Y->lev[fs - 1];
  if(P.nf == nf) return DLG_OK;
  DLG_HIP(hipStreamSynchronize(b->stream));
  lev_plan_release(P);
  if(!Y->lev_iperm)
  {
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
  }
  const int nsn = H.nsn, nrow = nf*fs, nch = dlg_cdiv(nrow, MR);
  std::vector<int> parent(nsn), rbelow(nsn);
  for(int s = 0; s < nsn; s++)
  {
    const int w = H.sn_c0[s+1] - H.sn_c0[s];
    rbelow[s] = H.sn_rowptr[s+1] - H.sn_rowptr[s] - w - 1;
    parent[s] = rbelow[s] > 0 ? H.col_sn[H.sn_rows[H.sn_rowptr[s] + w]] : -1;   // the supernode of the first row below
  }
  std::vector<int> stamp(nsn, -1), pair_sn, pair_ch, cp_ptr(1, 0), reach;
  for(int ch = 0; ch < nch; ch++)
  {
    reach.clear();
    for(int row = ch*MR; row < std::min(nrow, ch*MR + MR); row++)
      for(int q = Y->lev_jp[row]; q < Y->lev_jp[row+1]; q++)
        for(int s = H.col_sn[H.iperm[Y->lev_ji[q]]]; s >= 0 && stamp[s] != ch; s = parent[s]) { stamp[s] = ch; reach.push_back(s); }
    std::sort(reach.begin(), reach.end(), [&](int a, int c) { return H.sn_level[a] != H.sn_level[c] ? H.sn_level[a] < H.sn_level[c] : a < c; });
    for(int s : reach) { pair_sn.push_back(s); pair_ch.push_back(ch); }
    cp_ptr.push_back((int)pair_sn.size());
  }
  const int npair = (int)pair_sn.size(), nl = H.nlevels;
  std::vector<int64_t> pair_off(npair);
  std::vector<int> wl; wl.reserve(npair);
  std::vector<int> cnt(nl);
  P.wl_ptr.assign(1, 0);
  for(int ch0 = 0; ch0 < nch;)
  {
    // a batch: whole chunks while their update blocks fit (at least one chunk)
    int64_t rows = 0; int ch1 = ch0;
    while(ch1 < nch)
    {
      int64_t rc = 0;
      for(int q = cp_ptr[ch1]; q < cp_ptr[ch1+1]; q++) rc += rbelow[pair_sn[q]];
      if(ch1 > ch0 && rows + rc > LEV_BATCH_ROWS) break;
      for(int q = cp_ptr[ch1]; q < cp_ptr[ch1+1]; q++) { pair_off[q] = rows; rows += rbelow[pair_sn[q]]; }
      ch1++;
    }
    P.scr_rows = std::max(P.scr_rows, rows);
    std::fill(cnt.begin(), cnt.end(), 0);
    for(int q = cp_ptr[ch0]; q < cp_ptr[ch1]; q++) cnt[H.sn_level[pair_sn[q]]]++;
    const size_t base = wl.size();
    std::vector<size_t> at(nl);
    for(int l = 0, acc = 0; l < nl; l++) { at[l] = base + acc; acc += cnt[l]; P.wl_ptr.push_back((int)(base + acc)); }
    wl.resize(base + (cp_ptr[ch1] - cp_ptr[ch0]));
    for(int q = cp_ptr[ch0]; q < cp_ptr[ch1]; q++) wl[at[H.sn_level[pair_sn[q]]]++] = q;
    P.nbatch++;
    ch0 = ch1;
  }
  DLG_CHECK(upload(P.pair_sn, pair_sn)); DLG_CHECK(upload(P.pair_ch, pair_ch)); DLG_CHECK(upload(P.cp_ptr, cp_ptr));
  DLG_CHECK(upload(P.wl, wl)); DLG_CHECK(upload(P.pair_off, pair_off));
  DLG_HIP(hipMalloc(&P.gram, sizeof(double)*LEV_NP*(size_t)std::max(npair, 1)));
  DLG_HIP(hipMalloc(&P.scr, sizeof(double)*MR*(size_t)std::max<int64_t>(P.scr_rows, 1)));
  P.nf = nf; P.nch = nch; P.npair = npair; P.visits = npair;
  return DLG_OK;
}
} // namespace

void sparse_leverage_free(SparseSym* Y) { for(auto& P : Y->lev) lev_plan_release(P); }

// Gram products of the first nf features of fs rows through the reach-restricted forward solves; *d_gram / *d_slot_ptr:
// what lev_finish sums
int sparse_leverage_reach(dlg_backend* b, int s, int fs, int nf, double** d_gram, const int** d_slot_ptr, long* visits)
{
  SparseSym* Y = b->sym;
  if(!Y) { dlg_set_error("dlg_sparse_set_pattern must be called first"); return DLG_ERR_STATE; }
  DLG_CHECK(lev_plan_build(b, fs, nf));
  SparseSym::LevPlan& P = Y->lev[fs - 1];
  const int nl = Y->H.nlevels;
  for(int bt = 0; bt < P.nbatch; bt++)
    for(int l = 0; l < nl; l++)
    {
      const int w0 = P.wl_ptr[(size_t)bt*nl + l], n = P.wl_ptr[(size_t)bt*nl + l + 1] - w0;
      if(n > 0)
        hipLaunchKernelGGL(k_lev_fwd_level, dim3(n), dim3(TPB), Y->lev_lds, b->stream, P.wl + w0, P.pair_sn, P.pair_ch, P.pair_off,
                           P.cp_ptr, Y->sn_c0, Y->sn_rowptr, Y->sn_rows, Y->sn_lx, Y->lev_iperm, Y->Jp, Y->Ji, b->slot[s].Jin(),
                           Y->Lx, nf*fs, fs, P.scr, P.gram);
    }
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
