// batch_models.hip -- the built-in fit models of the batch solver as an ordinary batch callback (dogleg.h:
// dogleg_amd_batch_model_callback): x and J of the live problems, ONE launch on the stream it is given, every row through
// dogleg_batch_model_row (include/dogleg_batch_models.h).  This is the route by which every batch entry point takes a built-in
// model, and the comparison leg of the fused solve (dense_batch_kernels.hip: sweep_model), which forms the same rows through the
// same function on their way into the tile and so gives the same bits.  Not the hot path: one thread a row, J stored row by row.
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdio>
#include "../../include/dogleg.h"
#include "../../include/dogleg_batch_models.h"

static_assert(DOGLEG_BATCH_MODEL_EXPDECAY == DOGLEG_AMD_MODEL_EXPDECAY && DOGLEG_BATCH_MODEL_GAUSS1D == DOGLEG_AMD_MODEL_GAUSS1D &&
              DOGLEG_BATCH_MODEL_GAUSS2D == DOGLEG_AMD_MODEL_GAUSS2D &&
              DOGLEG_BATCH_MODEL_GAUSS2D_ELLIPTIC == DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC, "the two headers name the same kinds");

namespace {

std::atomic<unsigned long long> g_invocations{0};

// thread idx takes row idx % M of problem idx / M: x[idx] and the N doubles of J behind idx N, so that the stores of a wavefront
// cover one contiguous piece of J
__global__ void __launch_bounds__(256) k_model_rows(int B, int M, int N, int kind, int width, int t_each,
                                                    const double* __restrict__ y, const double* __restrict__ t,
                                                    const double* __restrict__ scale, const unsigned char* __restrict__ live,
                                                    const double* __restrict__ p, double* __restrict__ x, double* __restrict__ J)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)B*M) return;
  const int b = (int)(idx/M), i = (int)(idx - (size_t)b*M);
  if(!live[b]) return;
  double pv[DOGLEG_BATCH_MODEL_MAX_NSTATE], jr[DOGLEG_BATCH_MODEL_MAX_NSTATE];
#pragma unroll
  for(int j = 0; j < DOGLEG_BATCH_MODEL_MAX_NSTATE; j++) { pv[j] = j < N ? p[(size_t)b*N + j] : 0.0; jr[j] = 0.0; }
  const double ti = t ? t[t_each ? idx : (size_t)i] : (double)i;
  const double si = scale ? scale[idx] : 1.0;
  double xv = 0.0;
  dogleg_batch_model_row(kind, pv, i, width, ti, y[idx], si, &xv, jr);
  x[idx] = xv;
#pragma unroll
  for(int j = 0; j < DOGLEG_BATCH_MODEL_MAX_NSTATE; j++) if(j < N) J[idx*N + j] = jr[j];
}

// the same for the rows of the Poisson likelihood (dogleg_batch_model_row_poisson): x~ and J~, NaN in an infeasible row
__global__ void __launch_bounds__(256) k_model_rows_poisson(int B, int M, int N, int kind, int width, int t_each,
                                                            const double* __restrict__ y, const double* __restrict__ t,
                                                            const unsigned char* __restrict__ live, const double* __restrict__ p,
                                                            double* __restrict__ x, double* __restrict__ J)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)B*M) return;
  const int b = (int)(idx/M), i = (int)(idx - (size_t)b*M);
  if(!live[b]) return;
  double pv[DOGLEG_BATCH_MODEL_MAX_NSTATE], jr[DOGLEG_BATCH_MODEL_MAX_NSTATE];
#pragma unroll
  for(int j = 0; j < DOGLEG_BATCH_MODEL_MAX_NSTATE; j++) { pv[j] = j < N ? p[(size_t)b*N + j] : 0.0; jr[j] = 0.0; }
  const double ti = t ? t[t_each ? idx : (size_t)i] : (double)i;
  double xv = 0.0, dv = 0.0;
  (void)dogleg_batch_model_row_poisson(kind, pv, i, width, ti, y[idx], &xv, jr, &dv);
  x[idx] = xv;
#pragma unroll
  for(int j = 0; j < DOGLEG_BATCH_MODEL_MAX_NSTATE; j++) if(j < N) J[idx*N + j] = jr[j];
}

} // namespace

extern "C" {

int dogleg_amd_batch_model_nstate(int kind) { return dogleg_batch_model_nstate(kind); }

unsigned long long dogleg_amd_batch_model_callback_invocations(void) { return g_invocations.load(); }

// a dogleg_callback_device_batch_t
void dogleg_amd_batch_model_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                     unsigned int B, void* hip_stream, void* cookie)
{
  const dogleg_amd_batch_model_t* m = (const dogleg_amd_batch_model_t*)cookie;
  g_invocations++;
  const int N = m ? dogleg_batch_model_nstate(m->kind) : -1;
  const bool two_d = m && (m->kind == DOGLEG_AMD_MODEL_GAUSS2D || m->kind == DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC);
  if(N < 0 || !m->y || m->Nmeas == 0 || B == 0 || (two_d && (m->width == 0 || m->t)))
  {
    fprintf(stderr, "libdogleg_amd: dogleg_amd_batch_model_callback: the cookie is no usable dogleg_amd_batch_model_t: nothing written\n");
    return;
  }
  const size_t rows = (size_t)B*m->Nmeas;
  hipLaunchKernelGGL(k_model_rows, dim3((unsigned int)((rows + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, (int)B,
                     (int)m->Nmeas, N, m->kind, (int)m->width, m->t_per_problem ? 1 : 0, m->y, m->t, m->scale, live_dev, p_dev,
                     x_dev, J_dev);
}

// a dogleg_callback_device_batch_t for the uncertainty, query and _fit calls of a Poisson fit (dogleg.h): x~ and J~.  Its J~ is not
// the derivative of its x~, so the solve entry points refuse it (api_extensions.cpp: batch_solve_entry)
void dogleg_amd_batch_model_fisher_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                            unsigned int B, void* hip_stream, void* cookie)
{
  const dogleg_amd_batch_model_t* m = (const dogleg_amd_batch_model_t*)cookie;
  const int N = m ? dogleg_batch_model_nstate(m->kind) : -1;
  const bool two_d = m && (m->kind == DOGLEG_AMD_MODEL_GAUSS2D || m->kind == DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC);
  if(N < 0 || !m->y || m->scale || m->Nmeas == 0 || B == 0 || (two_d && (m->width == 0 || m->t)))
  {
    fprintf(stderr, "libdogleg_amd: dogleg_amd_batch_model_fisher_callback: the cookie is no dogleg_amd_batch_model_t usable with the "
                    "Poisson likelihood (scale must be NULL): nothing written\n");
    return;
  }
  const size_t rows = (size_t)B*m->Nmeas;
  hipLaunchKernelGGL(k_model_rows_poisson, dim3((unsigned int)((rows + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, (int)B,
                     (int)m->Nmeas, N, m->kind, (int)m->width, m->t_per_problem ? 1 : 0, m->y, m->t, live_dev, p_dev, x_dev, J_dev);
}

} // extern "C"
