// device_batch_linear.hip -- a batch of LINEAR least-squares problems with a prescribed Jacobian, in the
// dogleg_callback_device_batch_t contract (include/dogleg.h): x = A_b p - y_b, J = A_b, with A [B][M][N] and y [B][M] uploaded
// by the caller.  Test plumbing like device_batch_problems.hip, with the same call and evaluation counters: since JtJ and Jt x
// are what the caller chose, a test can place a problem exactly on a branch of the solver's loop.  The row sums run in index
// order, compiled with -ffp-contract=off: the host twin (problems/batch_linear.py) rounds the same way up to its own order.
// The first p the callback sees is kept (synth_lin_first_p): what the solver evaluated first.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
struct LinearBatch
{
  int B, M, N;
  double* d_A;                     // [B][M][N]
  double* d_y;                     // [B][M]
  double* d_first;                 // [B][N]: p of the first invocation
  unsigned long long* d_nevals;    // problem evaluations done
  int ncalls;
};

// one thread per measurement row of one problem
__global__ void __launch_bounds__(256) k_linear_eval(int B, int M, int N, const double* __restrict__ A,
                                                     const double* __restrict__ y, const unsigned char* __restrict__ live,
                                                     const double* __restrict__ p, double* __restrict__ x, double* __restrict__ J,
                                                     unsigned long long* __restrict__ nevals)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)B*M) return;
  const int b = (int)(idx / M), r = (int)(idx - (size_t)b*M);
  if(!live[b]) return;
  if(r == 0) atomicAdd(nevals, 1ull);
  const double* pb = p + (size_t)b*N; const double* Ar = A + idx*N;
  double* Jr = J + idx*N;
  double u = 0.0;
  for(int j = 0; j < N; j++) { u += Ar[j]*pb[j]; Jr[j] = Ar[j]; }
  x[idx] = u - y[idx];
}
} // namespace

extern "C" {

void synth_lin_free(void* h)
{
  LinearBatch* P = (LinearBatch*)h;
  if(!P) return;
  (void)hipFree(P->d_A); (void)hipFree(P->d_y); (void)hipFree(P->d_first); (void)hipFree(P->d_nevals);
  delete P;
}
void* synth_lin_create(int B, int M, int N, const double* A, const double* y)
{
  LinearBatch* P = new LinearBatch();
  P->B = B; P->M = M; P->N = N; P->ncalls = 0;
  P->d_A = nullptr; P->d_y = nullptr; P->d_first = nullptr; P->d_nevals = nullptr;
  const size_t nA = (size_t)B*M*N, ny = (size_t)B*M, np = (size_t)B*N;
  bool ok = hipMalloc(&P->d_A, sizeof(double)*nA) == hipSuccess && hipMalloc(&P->d_y, sizeof(double)*ny) == hipSuccess &&
            hipMalloc(&P->d_first, sizeof(double)*np) == hipSuccess &&
            hipMalloc(&P->d_nevals, sizeof(unsigned long long)) == hipSuccess;
  ok = ok && hipMemcpy(P->d_A, A, sizeof(double)*nA, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_y, y, sizeof(double)*ny, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(P->d_first, 0, sizeof(double)*np) == hipSuccess &&
       hipMemset(P->d_nevals, 0, sizeof(unsigned long long)) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_lin_create: device allocation failed\n"); (void)hipGetLastError(); synth_lin_free(P); return nullptr; }
  return P;
}
int synth_lin_ncalls(void* h) { return ((LinearBatch*)h)->ncalls; }
long long synth_lin_nevals(void* h)
{
  LinearBatch* P = (LinearBatch*)h;
  unsigned long long n = 0;
  if(hipMemcpy(&n, P->d_nevals, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
void synth_lin_reset_counters(void* h)
{
  LinearBatch* P = (LinearBatch*)h;
  P->ncalls = 0;
  (void)hipMemset(P->d_nevals, 0, sizeof(unsigned long long));
}
// p_dev as the first invocation since the counters were reset got it, [B][N]
int synth_lin_first_p(void* h, double* out)
{
  LinearBatch* P = (LinearBatch*)h;
  return hipMemcpy(out, P->d_first, sizeof(double)*(size_t)P->B*P->N, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

// dogleg_callback_device_batch_t
void synth_cb_device_batch_linear(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                                  void* hip_stream, void* cookie)
{
  LinearBatch* P = (LinearBatch*)cookie;
  hipStream_t st = (hipStream_t)hip_stream;
  if(P->ncalls++ == 0) (void)hipMemcpyAsync(P->d_first, p_dev, sizeof(double)*(size_t)B*P->N, hipMemcpyDeviceToDevice, st);
  const size_t rows = (size_t)B*P->M;
  hipLaunchKernelGGL(k_linear_eval, dim3((unsigned)((rows + 255)/256)), dim3(256), 0, st, (int)B, P->M, P->N, P->d_A, P->d_y,
                     live_dev, p_dev, x_dev, J_dev, P->d_nevals);
}

} // extern "C"
