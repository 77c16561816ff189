// device_batch_linear_products.hip -- a RAGGED batch of LINEAR least-squares problems with a prescribed Jacobian in the PRODUCTS
// form: a dogleg_callback_device_batch_products_t (include/dogleg.h) for x = A_b p - y_b, J = A_b, where A_b has its own number of
// rows M[b]: the rows of all problems lie one behind the other, problem b's at off[b] .. off[b + 1] (off [B + 1], uploaded by the
// caller with A [off[B]][N] and y [off[B]]).  The products twin of device_batch_linear.hip, with its counters and its first p:
// since JtJ and Jt x are what the caller chose, a test can place a problem exactly on a branch of the solver's loop.
// One workgroup per live problem; thread e takes entries e, e + 256, ... of the problem's output -- the packed triangle of JtJ,
// then Jt x, then norm2(x) -- and sums its entry over the rows in ascending order (x of a row summed in index order, compiled with
// -ffp-contract=off), so a problem's bits depend neither on B nor on its neighbours.
// The layout switch is that of device_batch_products.hip: packed upper; unpacked with both triangles; unpacked with the strict
// lower triangle, which the library must never read, filled with NaN.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>

namespace {
enum { LAYOUT_PACKED_UPPER = 0, LAYOUT_UNPACKED = 1, LAYOUT_UNPACKED_NAN_LOWER = 2 };

struct LinearProductsBatch
{
  int B, N, layout;
  long long rows;                  // off[B]
  double* d_A;                     // [rows][N]
  double* d_y;                     // [rows]
  long long* d_off;                // [B + 1]
  double* d_first;                 // [B][N]: p of the first invocation
  unsigned long long* d_nevals;    // problem evaluations done
  int ncalls;
};

// first entry of column c of the packed lower triangle, column-major: the same bytes as the row-major packed upper
__device__ inline int col_off(int c, int N) { return c*N - c*(c - 1)/2; }

__global__ void __launch_bounds__(256) k_linear_products(int B, int N, int layout, const double* __restrict__ A,
                                                         const double* __restrict__ y, const long long* __restrict__ off,
                                                         const unsigned char* __restrict__ live, const double* __restrict__ p,
                                                         double* __restrict__ norm2x, double* __restrict__ xtJ,
                                                         double* __restrict__ JtJ, unsigned long long* __restrict__ nevals)
{
  const int b = blockIdx.x;
  if(b >= B || !live[b]) return;
  if(threadIdx.x == 0) atomicAdd(nevals, 1ull);
  const int NP = N*(N + 1)/2;
  const long long r0 = off[b], r1 = off[b + 1];
  const double* pb = p + (size_t)b*N;
  for(int e = threadIdx.x; e < NP + N + 1; e += 256)
  {
    if(e < NP)
    {
      int c = 0;
      while(e >= col_off(c + 1, N)) c++;
      const int i = c + e - col_off(c, N);                  // i >= c: JtJ[c][i] lies in the upper triangle
      double s = 0.0;
      for(long long r = r0; r < r1; r++) s += A[(size_t)r*N + c]*A[(size_t)r*N + i];
      if(layout == LAYOUT_PACKED_UPPER) JtJ[(size_t)b*NP + e] = s;
      else
      {
        double* G = JtJ + (size_t)b*N*N;
        G[c*N + i] = s;
        if(i != c) G[i*N + c] = layout == LAYOUT_UNPACKED_NAN_LOWER ? nan("") : s;
      }
      continue;
    }
    // x of a row: u summed in index order, as the host's loop
    const int j = e - NP;                                   // j < N: entry j of Jt x; j == N: norm2(x)
    double s = 0.0;
    for(long long r = r0; r < r1; r++)
    {
      const double* Ar = A + (size_t)r*N;
      double u = 0.0;
      for(int k = 0; k < N; k++) u += Ar[k]*pb[k];
      const double xr = u - y[r];
      s += j < N ? Ar[j]*xr : xr*xr;
    }
    if(j < N) xtJ[(size_t)b*N + j] = s; else norm2x[b] = s;
  }
}
} // namespace

extern "C" {

void synth_linp_free(void* h)
{
  LinearProductsBatch* P = (LinearProductsBatch*)h;
  if(!P) return;
  (void)hipFree(P->d_A); (void)hipFree(P->d_y); (void)hipFree(P->d_off); (void)hipFree(P->d_first); (void)hipFree(P->d_nevals);
  delete P;
}
// off[B + 1]: ascending from 0, problem b's rows are off[b] .. off[b + 1] (at least one) of A [off[B]][N] and y [off[B]]
void* synth_linp_create(int B, int N, const long long* off, const double* A, const double* y)
{
  if(B <= 0 || N <= 0 || off[0] != 0) { fprintf(stderr, "synth_linp_create: B = %d, N = %d, off[0] = %lld\n", B, N, off[0]); return nullptr; }
  for(int b = 0; b < B; b++)
    if(off[b + 1] <= off[b]) { fprintf(stderr, "synth_linp_create: problem %d has no rows\n", b); return nullptr; }
  LinearProductsBatch* P = new LinearProductsBatch();
  P->B = B; P->N = N; P->layout = LAYOUT_PACKED_UPPER; P->rows = off[B]; P->ncalls = 0;
  P->d_A = nullptr; P->d_y = nullptr; P->d_off = nullptr; P->d_first = nullptr; P->d_nevals = nullptr;
  const size_t nA = (size_t)P->rows*N, ny = (size_t)P->rows, np = (size_t)B*N, no = (size_t)B + 1;
  bool ok = hipMalloc(&P->d_A, sizeof(double)*nA) == hipSuccess && hipMalloc(&P->d_y, sizeof(double)*ny) == hipSuccess &&
            hipMalloc(&P->d_off, sizeof(long long)*no) == hipSuccess && hipMalloc(&P->d_first, sizeof(double)*np) == hipSuccess &&
            hipMalloc(&P->d_nevals, sizeof(unsigned long long)) == hipSuccess;
  ok = ok && hipMemcpy(P->d_A, A, sizeof(double)*nA, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_y, y, sizeof(double)*ny, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_off, off, sizeof(long long)*no, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(P->d_first, 0, sizeof(double)*np) == hipSuccess &&
       hipMemset(P->d_nevals, 0, sizeof(unsigned long long)) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_linp_create: device allocation failed\n"); (void)hipGetLastError(); synth_linp_free(P); return nullptr; }
  return P;
}
// 0 packed upper, 1 unpacked (both triangles written), 2 unpacked with the strict lower triangle NaN; the caller passes the
// matching JtJ_packed / JtJ_upper to the library
int synth_linp_set_layout(void* h, int layout)
{
  if(layout < LAYOUT_PACKED_UPPER || layout > LAYOUT_UNPACKED_NAN_LOWER) return -1;
  ((LinearProductsBatch*)h)->layout = layout;
  return 0;
}
int synth_linp_ncalls(void* h) { return ((LinearProductsBatch*)h)->ncalls; }
long long synth_linp_nevals(void* h)
{
  LinearProductsBatch* P = (LinearProductsBatch*)h;
  unsigned long long n = 0;
  if(hipMemcpy(&n, P->d_nevals, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
void synth_linp_reset_counters(void* h)
{
  LinearProductsBatch* P = (LinearProductsBatch*)h;
  P->ncalls = 0;
  (void)hipMemset(P->d_nevals, 0, sizeof(unsigned long long));
}
// p_dev as the first invocation since the counters were reset got it, [B][N]
int synth_linp_first_p(void* h, double* out)
{
  LinearProductsBatch* P = (LinearProductsBatch*)h;
  return hipMemcpy(out, P->d_first, sizeof(double)*(size_t)P->B*P->N, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

// dogleg_callback_device_batch_products_t; B is the B of synth_linp_create (d_first and off are of that size)
void synth_cb_device_batch_linear_products(const double* p_dev, double* norm2x_dev, double* xtJ_dev, double* JtJ_dev,
                                           const unsigned char* live_dev, unsigned int B, void* hip_stream, void* cookie)
{
  LinearProductsBatch* P = (LinearProductsBatch*)cookie;
  hipStream_t st = (hipStream_t)hip_stream;
  if((int)B != P->B) { fprintf(stderr, "synth_cb_device_batch_linear_products: B = %u, created with %d\n", B, P->B); return; }
  if(P->ncalls++ == 0) (void)hipMemcpyAsync(P->d_first, p_dev, sizeof(double)*(size_t)B*P->N, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(k_linear_products, dim3(B), dim3(256), 0, st, (int)B, P->N, P->layout, P->d_A, P->d_y, P->d_off, live_dev, p_dev,
                     norm2x_dev, xtJ_dev, JtJ_dev, P->d_nevals);
}

} // extern "C"
