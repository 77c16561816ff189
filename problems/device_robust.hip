// device_robust.hip -- two dogleg_callback_device_t for the tests and the benchmark of the robust device solve
// (dogleg_amd_optimize_device2_robust).  Test and benchmark plumbing: nothing here computes what is checked.
//   offsets   calls an inner dogleg_callback_device_t (the model of device_problems.hip, handed over as a function pointer, so
//             this library links against nothing) and then adds a device array off[Nmeas] to x on the same stream: the offsets
//             plant gross outliers.  The host side of the same function is problems/device_robust.py's OffsetHostModel.
//   table     copies caller-given device arrays x_table and J_table into x and J: a constant model, so that any pattern and any
//             values can be put in front of the library.
#include <hip/hip_runtime.h>
#include <cstdio>

namespace {
typedef void (inner_cb_t)(const double* p_dev, double* x_dev, double* J_dev, void* hip_stream, void* cookie);
struct Offsets { inner_cb_t* inner; void* inner_cookie; int M; double* d_off; };
struct Table { size_t M, nJ; double *d_x, *d_J; int ncalls; };

__global__ void __launch_bounds__(256) k_add_offsets(int M, const double* __restrict__ off, double* __restrict__ x)
{
  const int r = blockIdx.x*256 + threadIdx.x;
  if(r < M) x[r] = x[r] + off[r];
}

double* to_device(const double* host, size_t n)
{
  double* d = nullptr;
  const size_t bytes = sizeof(double)*(n ? n : 1);
  if(hipMalloc(&d, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if(n && hipMemcpy(d, host, sizeof(double)*n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(d); return nullptr; }
  return d;
}
} // namespace

extern "C" {

void robust_offsets_free(void* h)
{
  Offsets* P = (Offsets*)h;
  if(!P) return;
  (void)hipFree(P->d_off);
  delete P;
}
// off: [M] on the host
void* robust_offsets_create(void* inner, void* inner_cookie, int M, const double* off)
{
  Offsets* P = new Offsets{(inner_cb_t*)inner, inner_cookie, M, to_device(off, (size_t)M)};
  if(P->d_off) return P;
  fprintf(stderr, "robust_offsets_create: device allocation failed\n");
  delete P;
  return nullptr;
}
// dogleg_callback_device_t
void robust_cb_offsets(const double* p_dev, double* x_dev, double* J_dev, void* hip_stream, void* cookie)
{
  Offsets* P = (Offsets*)cookie;
  P->inner(p_dev, x_dev, J_dev, hip_stream, P->inner_cookie);
  hipLaunchKernelGGL(k_add_offsets, dim3((unsigned)((P->M + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, P->M,
                     (const double*)P->d_off, x_dev);
}

void robust_table_free(void* h)
{
  Table* P = (Table*)h;
  if(!P) return;
  (void)hipFree(P->d_x); (void)hipFree(P->d_J);
  delete P;
}
// x: [M], J: [nJ] (the values of Jt in the order of the pattern, or M * N row-major), on the host
void* robust_table_create(int M, long long nJ, const double* x, const double* J)
{
  Table* P = new Table{(size_t)M, (size_t)nJ, to_device(x, (size_t)M), to_device(J, (size_t)nJ), 0};
  if(P->d_x && P->d_J) return P;
  fprintf(stderr, "robust_table_create: device allocation failed\n");
  robust_table_free(P);
  return nullptr;
}
int robust_table_ncalls(void* h) { return ((Table*)h)->ncalls; }
// measurement (tools/robust_device_bench.py): ms of one device-to-device copy of n doubles, the mean of reps copies behind
// two that are not timed; negative: no device memory
double robust_copy_ms(long long n, int reps)
{
  double *a = nullptr, *b = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = -1.f;
  const size_t bytes = sizeof(double)*(size_t)n;
  if(hipMalloc(&a, bytes) == hipSuccess && hipMalloc(&b, bytes) == hipSuccess && hipMemset(a, 0, bytes) == hipSuccess &&
     hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
  {
    for(int i = 0; i < 2; i++) (void)hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, 0);
    (void)hipEventRecord(e0, 0);
    for(int i = 0; i < reps; i++) (void)hipMemcpyAsync(b, a, bytes, hipMemcpyDeviceToDevice, 0);
    (void)hipEventRecord(e1, 0);
    if(hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = -1.f;
  }
  (void)hipGetLastError();
  if(e0) (void)hipEventDestroy(e0);
  if(e1) (void)hipEventDestroy(e1);
  (void)hipFree(a); (void)hipFree(b);
  return ms < 0.f ? -1.0 : (double)ms/reps;
}
// dogleg_callback_device_t
void robust_cb_table(const double*, double* x_dev, double* J_dev, void* hip_stream, void* cookie)
{
  Table* P = (Table*)cookie;
  P->ncalls++;
  (void)hipMemcpyAsync(x_dev, P->d_x, sizeof(double)*P->M, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream);
  if(P->nJ) (void)hipMemcpyAsync(J_dev, P->d_J, sizeof(double)*P->nJ, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream);
}

} // extern "C"
