// device_batch_rowscale.hip -- a batch callback behind another one: it calls an inner dogleg_callback_device_batch_t (handed
// over as a function pointer, so this library links against nothing) and then multiplies row r of x and of J of every live
// problem by sqrt(w[b][r / fs]) from a device array, with one small kernel on the given stream: a read and a write of all of
// x and J.  This is how a caller had to get the uncertainty of a robust batch fit before the ..._fit entry points took the
// weights themselves; kept as a test input (the fit forms must agree with it) and as the benchmark's opponent.  The host side
// of the same function is problems/batch_rowscale.py's RowScaleHostProblem.
#include <hip/hip_runtime.h>
#include <cstdio>

namespace {
typedef void (inner_cb_t)(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                          void* hip_stream, void* cookie);
struct RowScaleBatch
{
  inner_cb_t* inner; void* inner_cookie;
  int B, M, N, fs;
  double* d_w;                 // [B][M / fs]
};

// element idx of [B][M][N + 1]: column N of a row is its x
__global__ void __launch_bounds__(256) k_scale_rows(size_t n, int M, int N, int fs, const unsigned char* __restrict__ live,
                                                    const double* __restrict__ w, double* __restrict__ x, double* __restrict__ J)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= n) return;
  const size_t row = idx/(size_t)(N + 1);
  const int c = (int)(idx - row*(size_t)(N + 1));
  const size_t b = row/(size_t)M;
  if(!live[b]) return;
  const double sw = sqrt(w[b*(size_t)(M/fs) + (row - b*(size_t)M)/(size_t)fs]);
  if(c == N) x[row] = sw*x[row];
  else       J[row*(size_t)N + c] = sw*J[row*(size_t)N + c];
}
} // namespace

extern "C" {

void synth_rowscale_free(void* h)
{
  RowScaleBatch* P = (RowScaleBatch*)h;
  if(!P) return;
  (void)hipFree(P->d_w);
  delete P;
}
// w: [B][M / fs] on the host
void* synth_rowscale_create(void* inner, void* inner_cookie, int B, int M, int N, int fs, const double* w)
{
  RowScaleBatch* P = new RowScaleBatch();
  P->inner = (inner_cb_t*)inner; P->inner_cookie = inner_cookie; P->B = B; P->M = M; P->N = N; P->fs = fs; P->d_w = nullptr;
  const size_t bytes = sizeof(double)*(size_t)B*(M/fs);
  if(fs < 1 || M % fs || hipMalloc(&P->d_w, bytes) != hipSuccess || hipMemcpy(P->d_w, w, bytes, hipMemcpyHostToDevice) != hipSuccess)
  {
    fprintf(stderr, "synth_rowscale_create: bad feature size or device allocation failed\n"); (void)hipGetLastError();
    synth_rowscale_free(P);
    return nullptr;
  }
  return P;
}

// dogleg_callback_device_batch_t
void synth_cb_device_batch_rowscale(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                    unsigned int B, void* hip_stream, void* cookie)
{
  RowScaleBatch* P = (RowScaleBatch*)cookie;
  P->inner(p_dev, x_dev, J_dev, live_dev, B, hip_stream, P->inner_cookie);
  // (the weights cover P->B problems)
  const size_t n = (size_t)(B < (unsigned int)P->B ? B : (unsigned int)P->B)*P->M*(P->N + 1);
  hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)((n + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, n, P->M, P->N, P->fs,
                     live_dev, P->d_w, x_dev, J_dev);
}

} // extern "C"
