// device_batch_offsets.hip -- a batch callback behind another one: it calls an inner dogleg_callback_device_batch_t (the
// model of device_batch_problems.hip, handed over as a function pointer, so this library links against nothing) and then
// adds a per-problem offset array to x, x[b][r] += off[b][r], with one small kernel on the given stream that leaves the
// problems alone whose live byte is 0.  J is the inner callback's.  Test and benchmark plumbing: the offsets plant gross
// outliers for the robust batch solve; the host side of the same function is problems/batch_offsets.py's OffsetHostProblem.
#include <hip/hip_runtime.h>
#include <cstdio>

namespace {
typedef void (inner_cb_t)(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                          void* hip_stream, void* cookie);
struct OffsetBatch
{
  inner_cb_t* inner; void* inner_cookie;
  int B, M;
  double* d_off;               // [B][M]
};

__global__ void __launch_bounds__(256) k_add_offsets(size_t n, int M, const unsigned char* __restrict__ live,
                                                     const double* __restrict__ off, double* __restrict__ x)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= n) return;
  if(!live[idx / (size_t)M]) return;
  x[idx] = x[idx] + off[idx];
}
} // namespace

extern "C" {

void synth_offsets_free(void* h)
{
  OffsetBatch* P = (OffsetBatch*)h;
  if(!P) return;
  (void)hipFree(P->d_off);
  delete P;
}
// off: [B][M] on the host
void* synth_offsets_create(void* inner, void* inner_cookie, int B, int M, const double* off)
{
  OffsetBatch* P = new OffsetBatch();
  P->inner = (inner_cb_t*)inner; P->inner_cookie = inner_cookie; P->B = B; P->M = M; P->d_off = nullptr;
  const size_t bytes = sizeof(double)*(size_t)B*M;
  if(hipMalloc(&P->d_off, bytes) != hipSuccess || hipMemcpy(P->d_off, off, bytes, hipMemcpyHostToDevice) != hipSuccess)
  {
    fprintf(stderr, "synth_offsets_create: device allocation failed\n"); (void)hipGetLastError();
    synth_offsets_free(P);
    return nullptr;
  }
  return P;
}

// dogleg_callback_device_batch_t
void synth_cb_device_batch_offsets(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                   unsigned int B, void* hip_stream, void* cookie)
{
  OffsetBatch* P = (OffsetBatch*)cookie;
  P->inner(p_dev, x_dev, J_dev, live_dev, B, hip_stream, P->inner_cookie);
  const size_t n = (size_t)B*P->M;
  hipLaunchKernelGGL(k_add_offsets, dim3((unsigned)((n + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, n, P->M, live_dev,
                     P->d_off, x_dev);
}

} // extern "C"
