// expand_u16.hip -- the plain expansion kernel a caller needs in front of the fused solve on doubles: uint16 readings to float64,
// one element a thread, and its time by events on the null stream (tools/bench_batch_camera.py builds and loads this file).
#include <hip/hip_runtime.h>
#include <cstddef>

__global__ void __launch_bounds__(256) k_expand_u16(const unsigned short* __restrict__ in, double* __restrict__ out, size_t n)
{
  const size_t i = (size_t)blockIdx.x*256 + threadIdx.x;
  if(i < n) out[i] = (double)in[i];
}

// ms[0 .. reps-1]: the time of each of `reps` launches behind `warmup` untimed ones; returns 0, or the HIP error
extern "C" int expand_u16_ms(const unsigned short* in_dev, double* out_dev, size_t n, int warmup, int reps, float* ms)
{
  hipEvent_t e0, e1;
  hipError_t rc = hipEventCreate(&e0);
  if(rc != hipSuccess) return (int)rc;
  rc = hipEventCreate(&e1);
  if(rc != hipSuccess) return (int)rc;
  const dim3 grid((unsigned int)((n + 255)/256));
  for(int it = 0; it < warmup + reps && rc == hipSuccess; it++)
  {
    hipEventRecord(e0, nullptr);
    hipLaunchKernelGGL(k_expand_u16, grid, dim3(256), 0, nullptr, in_dev, out_dev, n);
    hipEventRecord(e1, nullptr);
    rc = hipEventSynchronize(e1);
    if(rc == hipSuccess) rc = hipGetLastError();
    float t = 0.0f;
    if(rc == hipSuccess) rc = hipEventElapsedTime(&t, e0, e1);
    if(it >= warmup) ms[it - warmup] = t;
  }
  hipEventDestroy(e0); hipEventDestroy(e1);
  return (int)rc;
}
