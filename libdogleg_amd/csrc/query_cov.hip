// query_cov.hip -- query covariance Jq Sigma Jq^T (factor_users.hip: dlg_query_covariance), the kernels outside the reach route.
// The reach route (the forward solve of the chunks' rows on the supernodes they reach) is k_cov_fwd_level<RhsCsr> in
// sparse_multi.hip; here:
//   k_query_rhs_il     the rows of a chunk as interleaved right-hand sides Jq^T (the full-solve routes, dense forward)
//   k_query_gram_rows  the products of a chunk from U = Sigma Jq^T: row a of Jq . column c of U (the full-sweep route)
//   k_qobs_gram        the observation form: Y = J[0:nobs] U, 16 columns per chunk, and its Gram Y^T Y on the matrix cores
//   k_qobs_reduce      ... the workgroups' partial Grams of a chunk summed in a fixed order (no atomics)
#include "sparse_internal.h"
#include <algorithm>
#include <cstdint>

namespace {
constexpr int MR = 16;                 // right-hand sides per chunk
typedef double qc_v4d __attribute__((ext_vector_type(4)));

// chunk ch0 + q at il + q N MR (cleared before): column c is row crow[ch] + c of the CSR, in the variables' order;
// duplicates summed in the row's order
__global__ void __launch_bounds__(TPB) k_query_rhs_il(const int* __restrict__ crow, const int* __restrict__ qrp,
                                                      const int* __restrict__ qvar, const double* __restrict__ qval,
                                                      int ch0, int nch, int N, double* __restrict__ il)
{
  const int t = blockIdx.x*TPB + threadIdx.x;
  if(t >= nch*MR) return;
  const int q = t / MR, c = t - q*MR, ch = ch0 + q, row = crow[ch] + c;
  if(row >= crow[ch+1]) return;
  double* col = il + (size_t)q*N*MR + c;
  for(int e = qrp[row]; e < qrp[row+1]; e++) col[(size_t)qvar[e]*MR] += qval[e];
}

// product t = (a, c) of chunk ch: Jq[crow[ch] + a] . U[:, c], one thread per product
__global__ void __launch_bounds__(TPB) k_query_gram_rows(const int* __restrict__ crow, const int* __restrict__ qrp,
                                                         const int* __restrict__ qvar, const double* __restrict__ qval,
                                                         const int* __restrict__ pptr, const int* __restrict__ prod,
                                                         const int64_t* __restrict__ goff, int ch,
                                                         const double* __restrict__ U, double* __restrict__ gram)
{
  const int t = threadIdx.x, p0 = pptr[ch];
  if(t >= pptr[ch+1] - p0) return;
  const int a = prod[p0 + t] / MR, c = prod[p0 + t] % MR, row = crow[ch] + a;
  double acc = 0.0;
  for(int e = qrp[row]; e < qrp[row+1]; e++) acc += qval[e]*U[(size_t)qvar[e]*MR + c];
  gram[goff[ch] + t] = acc;
}

// The observation form.  A wave takes 16-row tiles of J[0:nobs] (grid-strided over the waves of the grid): lane (mm, kq)
// forms Y[r][mm] = J_r . U[:, mm] for the rows r = 16 t + 4 i + kq, i = 0 .. 3, of every chunk of the pass (J is read once
// for all of them), and the tile's Gram Y^T Y goes onto the matrix cores as four K = 4 steps: A[i][k] = Y[k][i] and
// B[k][j] = Y[k][j] are the same lane value.  The four waves' 16 x 16 accumulators are added in a fixed order into one
// partial per (workgroup, chunk).  DENSE: J row-major [M][N]; otherwise the CSR rows of the pattern (Jp, Ji) with values Jv.
// NC: the chunks of the pass (a compile-time count keeps the accumulators in registers).
template <bool DENSE, int NC>
__global__ void __launch_bounds__(TPB) k_qobs_gram(const int* __restrict__ Jp, const int* __restrict__ Ji,
                                                   const double* __restrict__ Jv, int N, int nobs,
                                                   const double* __restrict__ U, double* __restrict__ part)
{
  __shared__ double red[TPB/64][NC][MR*MR];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  const size_t us = (size_t)N*MR;
  qc_v4d acc[NC];
#pragma unroll
  for(int cc = 0; cc < NC; cc++) acc[cc] = (qc_v4d){0.0, 0.0, 0.0, 0.0};
  const int ntile = (nobs + 15) / 16;
  for(int t = blockIdx.x*(TPB/64) + wv; t < ntile; t += gridDim.x*(TPB/64))
  {
#pragma unroll
    for(int i = 0; i < 4; i++)
    {
      const int r = 16*t + 4*i + kq;
      double y[NC];
#pragma unroll
      for(int cc = 0; cc < NC; cc++) y[cc] = 0.0;
      if(r < nobs)
      {
        if(DENSE)
        {
          const double* Jr = Jv + (size_t)r*N;
          for(int k = 0; k < N; k++)
          {
            const double v = Jr[k];
#pragma unroll
            for(int cc = 0; cc < NC; cc++) y[cc] += v*U[cc*us + (size_t)k*MR + mm];
          }
        }
        else
          for(int q = Jp[r]; q < Jp[r+1]; q++)
          {
            const size_t k = (size_t)Ji[q]*MR + mm;
            const double v = Jv[q];
#pragma unroll
            for(int cc = 0; cc < NC; cc++) y[cc] += v*U[cc*us + k];
          }
      }
#pragma unroll
      for(int cc = 0; cc < NC; cc++) acc[cc] = __builtin_amdgcn_mfma_f64_16x16x4f64(y[cc], y[cc], acc[cc], 0, 0, 0);
    }
  }
  // D[i][j]: register q of lane 16 kq + j, i = kq + 4 q
#pragma unroll
  for(int cc = 0; cc < NC; cc++)
#pragma unroll
    for(int q = 0; q < 4; q++) red[wv][cc][(kq + 4*q)*MR + mm] = acc[cc][q];
  __syncthreads();
  for(int cc = 0; cc < NC; cc++)
    part[((size_t)blockIdx.x*QOBS_NC + cc)*MR*MR + tid] = ((red[0][cc][tid] + red[1][cc][tid]) + red[2][cc][tid]) + red[3][cc][tid];
}
// chunk ch0 + blockIdx.x: each of its products summed over the nwg partials in workgroup order
__global__ void __launch_bounds__(TPB) k_qobs_reduce(const double* __restrict__ part, int nwg, int ch0,
                                                     const int* __restrict__ pptr, const int* __restrict__ prod,
                                                     const int64_t* __restrict__ goff, double* __restrict__ gram)
{
  const int cc = blockIdx.x, ch = ch0 + cc, p0 = pptr[ch], np = pptr[ch+1] - p0;
  for(int t = threadIdx.x; t < np; t += TPB)
  {
    const int e = prod[p0 + t];
    double acc = 0.0;
    for(int w = 0; w < nwg; w++) acc += part[((size_t)w*QOBS_NC + cc)*MR*MR + e];
    gram[goff[ch] + t] = acc;
  }
}
} // namespace

int query_rhs_il(dlg_backend* b, const CovPlan& P, int ch0, int nch, double* d_il)
{
  DLG_HIP(hipMemsetAsync(d_il, 0, sizeof(double)*(size_t)nch*b->N*MR, b->stream));
  hipLaunchKernelGGL(k_query_rhs_il, dim3(dlg_cdiv((long)nch*MR, TPB)), dim3(TPB), 0, b->stream, P.crow, P.qrp, P.qvar, P.qval,
                     ch0, nch, b->N, d_il);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int query_gram_rows(dlg_backend* b, const CovPlan& P, int ch, const double* d_il)
{
  hipLaunchKernelGGL(k_query_gram_rows, dim3(1), dim3(TPB), 0, b->stream, P.crow, P.qrp, P.qvar, P.qval, P.pptr, P.prod, P.goff,
                     ch, d_il, P.gram);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
int query_obs_gram(dlg_backend* b, int s, const CovPlan& P, int ch0, int nch, int nobs, const double* d_U, double* d_part)
{
  if(nch < 1 || nch > QOBS_NC) { dlg_set_error("query_obs_gram: %d chunks in one pass", nch); return DLG_ERR_ARG; }
  const int ntile = (nobs + 15) / 16;
  const int nwg = std::max(1, std::min(QOBS_WG, dlg_cdiv(ntile, TPB/64)));
  const double* Jv = b->slot[s].Jin();
  const bool dense = b->type != DLG_SPARSE;
  const int* Jp = dense ? nullptr : b->sym->Jp;
  const int* Ji = dense ? nullptr : b->sym->Ji;
  typedef void (*kfn)(const int*, const int*, const double*, int, int, const double*, double*);
  static const kfn kern[2][QOBS_NC] = {{k_qobs_gram<false, 1>, k_qobs_gram<false, 2>, k_qobs_gram<false, 3>, k_qobs_gram<false, 4>},
                                       {k_qobs_gram<true, 1>, k_qobs_gram<true, 2>, k_qobs_gram<true, 3>, k_qobs_gram<true, 4>}};
  hipLaunchKernelGGL(kern[dense][nch - 1], dim3(nwg), dim3(TPB), 0, b->stream, Jp, Ji, Jv, b->N, nobs, d_U, d_part);
  hipLaunchKernelGGL(k_qobs_reduce, dim3(nch), dim3(TPB), 0, b->stream, d_part, nwg, ch0, P.pptr, P.prod, P.goff, P.gram);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
