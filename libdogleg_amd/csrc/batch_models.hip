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
#include "dense_batch.h"

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

// the same two for a camera record (dogleg.h: dogleg_amd_batch_camera_t): the datum is formed from the reading and, with
// calibration (offset != nullptr), from the maps at the row's sensor pixel; a window that leaves the sensor reads nothing from the
// maps and its data are NaN.  FISHER: the Poisson rows, with the read-noise variance under calibration
// (dogleg_batch_model_row_poisson_v), else those of the GAUSS definition
struct CameraArgs
{
  int kind, width, height, t_each, dtype, sw, sh;
  const void* raw; const float *offset, *gain_inv, *readvar; const int* origin;
  const double *t, *scale;
};
template <bool FISHER>
__global__ void __launch_bounds__(256) k_camera_rows(int B, int M, int N, CameraArgs C, const unsigned char* __restrict__ live,
                                                     const double* __restrict__ p, double* __restrict__ x, double* __restrict__ J)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)B*M) return;
  const int b = (int)(idx/M), i = (int)(idx - (size_t)b*M);
  if(!live[b]) return;
  double pv[DOGLEG_BATCH_MODEL_MAX_NSTATE], jr[DOGLEG_BATCH_MODEL_MAX_NSTATE];
#pragma unroll
  for(int j = 0; j < DOGLEG_BATCH_MODEL_MAX_NSTATE; j++) { pv[j] = j < N ? p[(size_t)b*N + j] : 0.0; jr[j] = 0.0; }
  const double ti = C.t ? C.t[C.t_each ? idx : (size_t)i] : (double)i;
  const double raw = C.dtype == DOGLEG_AMD_DATA_U16 ? (double)((const unsigned short*)C.raw)[idx] :
                     C.dtype == DOGLEG_AMD_DATA_F32 ? (double)((const float*)C.raw)[idx] : ((const double*)C.raw)[idx];
  double yv = raw, vv = 0.0;
  if(C.offset)
  {
    const int ox = C.origin[2*(size_t)b], oy = C.origin[2*(size_t)b + 1];
    if(ox >= 0 && oy >= 0 && ox <= C.sw - C.width && oy <= C.sh - C.height)
    {
      const int iy = i/C.width, ix = i - iy*C.width;
      const size_t px = (size_t)(oy + iy)*C.sw + (ox + ix);
      dogleg_batch_camera_datum(raw, C.offset[px], C.gain_inv[px], C.readvar ? C.readvar[px] : 0.0f, &yv, &vv);
    }
    else yv = __builtin_nan("");
  }
  double xv = 0.0, dv = 0.0;
  if constexpr(FISHER)
  {
    if(C.offset) (void)dogleg_batch_model_row_poisson_v(C.kind, pv, i, C.width, ti, yv, vv, &xv, jr, &dv);
    else         (void)dogleg_batch_model_row_poisson(C.kind, pv, i, C.width, ti, yv, &xv, jr, &dv);
  }
  else dogleg_batch_model_row(C.kind, pv, i, C.width, ti, yv, C.scale ? C.scale[idx] : 1.0, &xv, jr);
  x[idx] = xv;
#pragma unroll
  for(int j = 0; j < DOGLEG_BATCH_MODEL_MAX_NSTATE; j++) if(j < N) J[idx*N + j] = jr[j];
}

template <bool FISHER>
void camera_rows(const char* who, const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                 void* hip_stream, void* cookie)
{
  const dogleg_amd_batch_camera_t* c = (const dogleg_amd_batch_camera_t*)cookie;
  // (the rules of the fused camera calls, stated once: api_extensions.cpp; FISHER: the Poisson rows, which take no scale)
  if(B == 0 || !dlg_batch_camera_ok(who, c, FISHER ? DOGLEG_AMD_LIKELIHOOD_POISSON : DOGLEG_AMD_LIKELIHOOD_GAUSS))
  {
    fprintf(stderr, "libdogleg_amd: %s: the cookie is no usable dogleg_amd_batch_camera_t: nothing written\n", who);
    return;
  }
  const dogleg_amd_batch_model_t& m = c->model;
  const CameraArgs C{m.kind, (int)m.width, (int)m.height, m.t_per_problem ? 1 : 0, c->dtype, (int)c->sensor_width, (int)c->sensor_height,
                     c->raw, c->offset, c->gain_inv, c->readvar, c->origin, m.t, m.scale};
  const size_t rows = (size_t)B*m.Nmeas;
  hipLaunchKernelGGL(k_camera_rows<FISHER>, dim3((unsigned int)((rows + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, (int)B,
                     (int)m.Nmeas, dogleg_batch_model_nstate(m.kind), C, live_dev, p_dev, x_dev, J_dev);
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

// the two callbacks of a camera record (dogleg.h, item 5 of the built-in models): a dogleg_callback_device_batch_t each, one launch.
// The second writes rows whose J~ is not the derivative of their x~: the solve entry points refuse it as they refuse the one above
void dogleg_amd_batch_camera_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                      unsigned int B, void* hip_stream, void* cookie)
{
  camera_rows<false>(__func__, p_dev, x_dev, J_dev, live_dev, B, hip_stream, cookie);
}
void dogleg_amd_batch_camera_fisher_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                             unsigned int B, void* hip_stream, void* cookie)
{
  camera_rows<true>(__func__, p_dev, x_dev, J_dev, live_dev, B, hip_stream, cookie);
}

} // extern "C"
