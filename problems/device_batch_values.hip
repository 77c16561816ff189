// device_batch_values.hip -- the dense synthetic problems of device_batch_problems.hip as a VALUES-ONLY model, in the
// dogleg_callback_device_batch_values_t contract (include/dogleg.h, dogleg_amd_batch_numeric_create): problem b is
// DenseProblem(M, N, seed[b], eps, noise, p0_spread) of problems.c, x per measurement row in the operation order of
// k_batch_eval / synth_cb_dense, compiled with -ffp-contract=off.  Test and benchmark plumbing, a library of its own.
//
// Switches (synth_vbatch_set_mode): problem b returns x[0] = NaN (mode 1), does not depend on variable zero_col (mode 2), or
// returns NaN in every x when any of its variables lies outside the box given with synth_vbatch_set_box (mode 3: a model
// that is not defined out there, like sqrt(amplitude)).
//
// The naive reference (synth_vnaive_create, synth_cb_device_batch_naive): a dogleg_callback_device_batch_t that forms the
// numeric Jacobian the plain way -- the copies written by one thread per variable, ONE LAUNCH OF THE VALUES KERNEL PER
// COPY, then one thread per entry of J -- with the step function of include/dogleg_numeric_step.h.  What the library's
// adapter must reproduce bit for bit.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "../include/dogleg_numeric_step.h"

namespace {
__host__ __device__ inline uint64_t mix64(uint64_t z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline double urand(uint64_t seed, uint64_t stream, uint64_t idx)
{
  const uint64_t h = mix64(mix64(seed ^ (stream*0xD6E8FEB86659FD93ull)) + idx);
  return (double)(h >> 11) * (2.0/9007199254740992.0) - 1.0;
}

struct ValuesProblem
{
  int B, M, N, zero_col;
  double eps, noise, p0_spread;
  std::vector<uint64_t> seed;      // host copy
  uint64_t* d_seed;
  double* d_pstar;                 // [B][N]
  unsigned char* d_mode;           // [B]
  double* d_box;                   // lower | upper, each [B][N]
  unsigned long long* d_nevals;    // problem-copies evaluated
  int ncalls;
  long long ncopies;               // problem-copies requested: copies * B, summed
};

// one thread per measurement row of one problem of one copy: u summed in index order, as the host's loop.  p [copies][B][N],
// x [copies][B][M]; seed, pstar, mode, box [Bp]... of the problem, B <= Bp problems of them evaluated
__global__ void __launch_bounds__(256) k_values_eval(int B, int copies, int M, int N, const uint64_t* __restrict__ seed,
                                                     const double* __restrict__ pstar, const unsigned char* __restrict__ mode,
                                                     int zero_col, const double* __restrict__ box_lo,
                                                     const double* __restrict__ box_hi, const unsigned char* __restrict__ live,
                                                     const double* __restrict__ p, double eps, double noise,
                                                     double* __restrict__ x, unsigned long long* __restrict__ nevals)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  const size_t BM = (size_t)B*M;
  if(idx >= BM*(size_t)copies) return;
  const size_t k = idx/BM, e = idx - k*BM;
  const int b = (int)(e / M), r = (int)(e - (size_t)b*M);
  if(!live[b]) return;
  if(r == 0) atomicAdd(nevals, 1ull);
  const uint64_t sd = seed[b];
  const int md = mode[b];
  const double* pb = p + (k*(size_t)B + b)*N; const double* ps = pstar + (size_t)b*N;
  const double sq = sqrt((double)N);
  double u = 0.0;
  bool outside = false;
  for(int j = 0; j < N; j++)
  {
    const double c = urand(sd, 3, (uint64_t)r*(uint64_t)N + (uint64_t)j) / sq;
    const double dp = (md == 2 && j == zero_col) ? 0.0 : pb[j] - ps[j];
    if(md == 3 && (pb[j] < box_lo[(size_t)b*N + j] || pb[j] > box_hi[(size_t)b*N + j])) outside = true;
    u += c*dp;
  }
  double xr = u + eps*sin(u) - noise*urand(sd, 5, (uint64_t)r);
  if(md == 1 && r == 0) xr = nan("");
  if(outside) xr = nan("");
  x[idx] = xr;
}

void launch_values(ValuesProblem* P, const double* p, double* x, const unsigned char* live, unsigned int B, unsigned int copies,
                   hipStream_t st)
{
  const size_t rows = (size_t)B*P->M*copies;
  hipLaunchKernelGGL(k_values_eval, dim3((unsigned)((rows + 255)/256)), dim3(256), 0, st, (int)B, (int)copies, P->M, P->N, P->d_seed,
                     P->d_pstar, P->d_mode, P->zero_col, P->d_box, P->d_box + (size_t)P->B*P->N, live, p, P->eps, P->noise, x,
                     P->d_nevals);
}

// ---- the naive reference ----
struct NaiveRef
{
  ValuesProblem* P;
  int scheme, K;
  double delta_rel, delta_abs;
  double* d_lower; double* d_upper;    // [B][N] or nullptr
  double* d_pc; double* d_xc; double* d_div;
};

// one thread per variable of a live problem: its step, and its entry of every copy
__global__ void __launch_bounds__(256) k_naive_copies(int B, int N, int K, int scheme, double delta_rel, double delta_abs,
                                                      const double* __restrict__ p, const double* __restrict__ lower,
                                                      const double* __restrict__ upper, const unsigned char* __restrict__ live,
                                                      double* __restrict__ pc, double* __restrict__ div)
{
  const size_t e = (size_t)blockIdx.x*256 + threadIdx.x;
  if(e >= (size_t)B*N) return;
  const int b = (int)(e/N), j = (int)(e - (size_t)b*N);
  if(!live[b]) return;
  double tp, tm, d;
  dogleg_numeric_step(scheme, p[e], lower ? lower[e] : -INFINITY, upper ? upper[e] : INFINITY, delta_rel, delta_abs, &tp, &tm, &d);
  div[e] = d;
  for(int k = 0; k < K; k++)
    pc[(size_t)k*B*N + e] = k == 1 + j ? tp : (k == 1 + N + j ? tm : p[e]);
}
// one thread per entry of J (and the thread of variable 0 copies x)
__global__ void __launch_bounds__(256) k_naive_jacobian(int B, int N, int M, int central, const double* __restrict__ xc,
                                                        const double* __restrict__ div, const unsigned char* __restrict__ live,
                                                        double* __restrict__ x, double* __restrict__ J)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  const size_t BM = (size_t)B*M;
  if(idx >= BM*N) return;
  const size_t row = idx/N;
  const int j = (int)(idx - row*N), b = (int)(row/M);
  if(!live[b]) return;
  if(j == 0) x[row] = xc[row];
  const double xp = xc[(size_t)(1 + j)*BM + row];
  const double xm = central ? xc[(size_t)(1 + N + j)*BM + row] : xc[row];
  const double d = div[(size_t)b*N + j];
  J[idx] = d == 0.0 ? 0.0 : (xp - xm)/d;
}
} // namespace

extern "C" {

void synth_vbatch_free(void* h)
{
  ValuesProblem* P = (ValuesProblem*)h;
  if(!P) return;
  (void)hipFree(P->d_seed); (void)hipFree(P->d_pstar); (void)hipFree(P->d_mode); (void)hipFree(P->d_box); (void)hipFree(P->d_nevals);
  delete P;
}
void* synth_vbatch_create(int B, int M, int N, const uint64_t* seeds, double eps, double noise, double p0_spread)
{
  ValuesProblem* P = new ValuesProblem();
  P->B = B; P->M = M; P->N = N; P->zero_col = 0; P->eps = eps; P->noise = noise; P->p0_spread = p0_spread; P->ncalls = 0; P->ncopies = 0;
  P->seed.assign(seeds, seeds + B);
  P->d_seed = nullptr; P->d_pstar = nullptr; P->d_mode = nullptr; P->d_box = nullptr; P->d_nevals = nullptr;
  std::vector<double> ps((size_t)B*N);
  for(int b = 0; b < B; b++)
    for(int j = 0; j < N; j++) ps[(size_t)b*N + j] = urand(seeds[b], 1, (uint64_t)j);
  bool ok = hipMalloc(&P->d_seed, sizeof(uint64_t)*(size_t)B) == hipSuccess &&
            hipMalloc(&P->d_pstar, sizeof(double)*ps.size()) == hipSuccess &&
            hipMalloc(&P->d_box, 2*sizeof(double)*ps.size()) == hipSuccess &&
            hipMalloc(&P->d_mode, (size_t)B) == hipSuccess && hipMalloc(&P->d_nevals, sizeof(unsigned long long)) == hipSuccess;
  ok = ok && hipMemcpy(P->d_seed, seeds, sizeof(uint64_t)*(size_t)B, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_pstar, ps.data(), sizeof(double)*ps.size(), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(P->d_box, 0, 2*sizeof(double)*ps.size()) == hipSuccess &&
       hipMemset(P->d_mode, 0, (size_t)B) == hipSuccess && hipMemset(P->d_nevals, 0, sizeof(unsigned long long)) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_vbatch_create: device allocation failed\n"); (void)hipGetLastError(); synth_vbatch_free(P); return nullptr; }
  return P;
}
// the start points synth_p0 gives the B problems, [B][N]
void synth_vbatch_p0(void* h, double* out)
{
  ValuesProblem* P = (ValuesProblem*)h;
  for(int b = 0; b < P->B; b++)
    for(int j = 0; j < P->N; j++)
    {
      const double ps = urand(P->seed[b], 1, (uint64_t)j);
      out[(size_t)b*P->N + j] = ps + P->p0_spread * urand(P->seed[b], 4, (uint64_t)j);
    }
}
// the optima of the noise-free problems, [B][N]
void synth_vbatch_pstar(void* h, double* out)
{
  ValuesProblem* P = (ValuesProblem*)h;
  for(int b = 0; b < P->B; b++)
    for(int j = 0; j < P->N; j++) out[(size_t)b*P->N + j] = urand(P->seed[b], 1, (uint64_t)j);
}
// mode[B]: 0 the model, 1 x[0] = NaN, 2 no dependence on variable zero_col, 3 NaN outside the box
int synth_vbatch_set_mode(void* h, const unsigned char* mode, int zero_col)
{
  ValuesProblem* P = (ValuesProblem*)h;
  P->zero_col = zero_col;
  return hipMemcpy(P->d_mode, mode, (size_t)P->B, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// the box of mode 3: lower, upper [B][N] on the host
int synth_vbatch_set_box(void* h, const double* lower, const double* upper)
{
  ValuesProblem* P = (ValuesProblem*)h;
  const size_t n = (size_t)P->B*P->N;
  return hipMemcpy(P->d_box, lower, sizeof(double)*n, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(P->d_box + n, upper, sizeof(double)*n, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
int synth_vbatch_ncalls(void* h) { return ((ValuesProblem*)h)->ncalls; }
long long synth_vbatch_ncopies(void* h) { return ((ValuesProblem*)h)->ncopies; }
long long synth_vbatch_nevals(void* h)
{
  ValuesProblem* P = (ValuesProblem*)h;
  unsigned long long n = 0;
  if(hipMemcpy(&n, P->d_nevals, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
void synth_vbatch_reset_counters(void* h)
{
  ValuesProblem* P = (ValuesProblem*)h;
  P->ncalls = 0; P->ncopies = 0;
  (void)hipMemset(P->d_nevals, 0, sizeof(unsigned long long));
}

// dogleg_callback_device_batch_values_t
void synth_cb_device_batch_values(const double* p_dev, double* x_dev, const unsigned char* live_dev, unsigned int B,
                                  unsigned int copies, void* hip_stream, void* cookie)
{
  ValuesProblem* P = (ValuesProblem*)cookie;
  P->ncalls++; P->ncopies += (long long)copies*B;
  launch_values(P, p_dev, x_dev, live_dev, B, copies, (hipStream_t)hip_stream);
}

void synth_vnaive_free(void* h)
{
  NaiveRef* R = (NaiveRef*)h;
  if(!R) return;
  (void)hipFree(R->d_lower); (void)hipFree(R->d_upper); (void)hipFree(R->d_pc); (void)hipFree(R->d_xc); (void)hipFree(R->d_div);
  delete R;
}
// the naive reference over the values problem h: the deltas as they are (no defaults), lower / upper [B][N] on the host or NULL
void* synth_vnaive_create(void* h, int scheme, double delta_rel, double delta_abs, const double* lower, const double* upper)
{
  ValuesProblem* P = (ValuesProblem*)h;
  NaiveRef* R = new NaiveRef();
  R->P = P; R->scheme = scheme; R->K = scheme == DOGLEG_NUMERIC_STEP_CENTRAL ? 2*P->N + 1 : P->N + 1;
  R->delta_rel = delta_rel; R->delta_abs = delta_abs;
  R->d_lower = R->d_upper = R->d_pc = R->d_xc = R->d_div = nullptr;
  const size_t vec = sizeof(double)*(size_t)P->B*P->N;
  bool ok = hipMalloc(&R->d_pc, vec*R->K) == hipSuccess && hipMalloc(&R->d_xc, sizeof(double)*(size_t)P->B*P->M*R->K) == hipSuccess &&
            hipMalloc(&R->d_div, vec) == hipSuccess;
  if(lower) ok = ok && hipMalloc(&R->d_lower, vec) == hipSuccess && hipMemcpy(R->d_lower, lower, vec, hipMemcpyHostToDevice) == hipSuccess;
  if(upper) ok = ok && hipMalloc(&R->d_upper, vec) == hipSuccess && hipMemcpy(R->d_upper, upper, vec, hipMemcpyHostToDevice) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_vnaive_create: device allocation failed\n"); (void)hipGetLastError(); synth_vnaive_free(R); return nullptr; }
  return R;
}
// dogleg_callback_device_batch_t; B must not exceed the problem's
void synth_cb_device_batch_naive(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                                 void* hip_stream, void* cookie)
{
  NaiveRef* R = (NaiveRef*)cookie;
  ValuesProblem* P = R->P;
  hipStream_t st = (hipStream_t)hip_stream;
  const int N = P->N, M = P->M;
  if((int)B > P->B) { fprintf(stderr, "synth_cb_device_batch_naive: B = %u above the problem's %d\n", B, P->B); return; }
  const size_t BN = (size_t)B*N, BM = (size_t)B*M;
  hipLaunchKernelGGL(k_naive_copies, dim3((unsigned)((BN + 255)/256)), dim3(256), 0, st, (int)B, N, R->K, R->scheme, R->delta_rel,
                     R->delta_abs, p_dev, R->d_lower, R->d_upper, live_dev, R->d_pc, R->d_div);
  for(int k = 0; k < R->K; k++)
    launch_values(P, R->d_pc + (size_t)k*BN, R->d_xc + (size_t)k*BM, live_dev, B, 1, st);
  hipLaunchKernelGGL(k_naive_jacobian, dim3((unsigned)((BM*N + 255)/256)), dim3(256), 0, st, (int)B, N, M,
                     R->scheme == DOGLEG_NUMERIC_STEP_CENTRAL ? 1 : 0, R->d_xc, R->d_div, live_dev, x_dev, J_dev);
}

// ---- tools/batch_numeric_bench.py: a device-to-device copy that moves `bytes_moved` bytes (half read, half written), timed by
// events on the null stream, as the yardstick of the adapter's kernels
struct CopyLeg { void* a; void* b; size_t half; hipEvent_t e0, e1; };
void synth_copy_free(void* h)
{
  CopyLeg* L = (CopyLeg*)h;
  if(!L) return;
  (void)hipFree(L->a); (void)hipFree(L->b);
  if(L->e0) (void)hipEventDestroy(L->e0);
  if(L->e1) (void)hipEventDestroy(L->e1);
  delete L;
}
void* synth_copy_create(size_t bytes_moved)
{
  CopyLeg* L = new CopyLeg();
  L->a = L->b = nullptr; L->e0 = L->e1 = nullptr; L->half = bytes_moved/2;
  const bool ok = hipMalloc(&L->a, L->half) == hipSuccess && hipMalloc(&L->b, L->half) == hipSuccess &&
                  hipMemset(L->a, 1, L->half) == hipSuccess && hipEventCreate(&L->e0) == hipSuccess && hipEventCreate(&L->e1) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_copy_create: %zu bytes: allocation failed\n", bytes_moved); (void)hipGetLastError(); synth_copy_free(L); return nullptr; }
  return L;
}
// one copy; its time in ms, negative on an error
double synth_copy_run(void* h)
{
  CopyLeg* L = (CopyLeg*)h;
  float ms = -1.f;
  if(hipEventRecord(L->e0, nullptr) != hipSuccess || hipMemcpyAsync(L->b, L->a, L->half, hipMemcpyDeviceToDevice, nullptr) != hipSuccess ||
     hipEventRecord(L->e1, nullptr) != hipSuccess || hipEventSynchronize(L->e1) != hipSuccess ||
     hipEventElapsedTime(&ms, L->e0, L->e1) != hipSuccess) { (void)hipGetLastError(); return -1.0; }
  return (double)ms;
}

} // extern "C"
