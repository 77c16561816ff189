// device_batch_problems.hip -- a batch of the dense synthetic problems of problems.c evaluated ON THE GPU, in the
// dogleg_callback_device_batch_t contract (include/dogleg.h, dogleg_amd_optimize_dense_batch).  Test and benchmark
// plumbing like device_problems.hip: problem b is DenseProblem(M, N, seed[b], eps, noise, p0_spread) of problems.c
// (synth_dense_create, dense_coef, synth_p0), with the operation order of synth_cb_dense / k_dense_eval per
// measurement row and compiled with -ffp-contract=off, so the host callback handed to the CPU oracle and this batch
// callback describe the same function up to the last bits of sin / cos.
//
// Switches for the failure and lambda tests (synth_batch_set_mode): problem b returns x[0] = NaN (mode 1), or has
// column zero_col of J exactly zero (mode 2: the model does not depend on that variable).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

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

struct BatchProblem
{
  int B, M, N, zero_col;
  double eps, noise, p0_spread;
  std::vector<uint64_t> seed;      // host copy
  uint64_t* d_seed;
  double* d_pstar;                 // [B][N]
  unsigned char* d_mode;           // [B]
  unsigned long long* d_nevals;    // problem evaluations done
  int ncalls;
};

// one thread per measurement row of one problem: u summed in index order, as the host's loop
__global__ void __launch_bounds__(256) k_batch_eval(int B, int M, int N, const uint64_t* __restrict__ seed,
                                                    const double* __restrict__ pstar, const unsigned char* __restrict__ mode,
                                                    int zero_col, const unsigned char* __restrict__ live,
                                                    const double* __restrict__ p, double eps, double noise,
                                                    double* __restrict__ x, double* __restrict__ J,
                                                    unsigned long long* __restrict__ nevals)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)B*M) return;
  const int b = (int)(idx / M), r = (int)(idx - (size_t)b*M);
  if(!live[b]) return;
  if(r == 0) atomicAdd(nevals, 1ull);
  const uint64_t sd = seed[b];
  const int md = mode[b];
  const double* pb = p + (size_t)b*N; const double* ps = pstar + (size_t)b*N;
  double* Jr = J + idx*N;
  const double sq = sqrt((double)N);
  double u = 0.0;
  for(int j = 0; j < N; j++)
  {
    const double c = urand(sd, 3, (uint64_t)r*(uint64_t)N + (uint64_t)j) / sq;
    const double dp = (md == 2 && j == zero_col) ? 0.0 : pb[j] - ps[j];
    u += c*dp;
  }
  double xr = u + eps*sin(u) - noise*urand(sd, 5, (uint64_t)r);
  if(md == 1 && r == 0) xr = nan("");
  x[idx] = xr;
  const double d = 1.0 + eps*cos(u);
  for(int j = 0; j < N; j++)
  {
    const double c = urand(sd, 3, (uint64_t)r*(uint64_t)N + (uint64_t)j) / sq;
    Jr[j] = (md == 2 && j == zero_col) ? 0.0 : c*d;
  }
}
} // namespace

extern "C" {

void synth_batch_free(void* h)
{
  BatchProblem* P = (BatchProblem*)h;
  if(!P) return;
  (void)hipFree(P->d_seed); (void)hipFree(P->d_pstar); (void)hipFree(P->d_mode); (void)hipFree(P->d_nevals);
  delete P;
}
void* synth_batch_create(int B, int M, int N, const uint64_t* seeds, double eps, double noise, double p0_spread)
{
  BatchProblem* P = new BatchProblem();
  P->B = B; P->M = M; P->N = N; P->zero_col = 0; P->eps = eps; P->noise = noise; P->p0_spread = p0_spread; P->ncalls = 0;
  P->seed.assign(seeds, seeds + B);
  P->d_seed = nullptr; P->d_pstar = nullptr; P->d_mode = nullptr; P->d_nevals = nullptr;
  std::vector<double> ps((size_t)B*N);
  for(int b = 0; b < B; b++)
    for(int j = 0; j < N; j++) ps[(size_t)b*N + j] = urand(seeds[b], 1, (uint64_t)j);
  bool ok = hipMalloc(&P->d_seed, sizeof(uint64_t)*(size_t)B) == hipSuccess &&
            hipMalloc(&P->d_pstar, sizeof(double)*ps.size()) == hipSuccess &&
            hipMalloc(&P->d_mode, (size_t)B) == hipSuccess && hipMalloc(&P->d_nevals, sizeof(unsigned long long)) == hipSuccess;
  ok = ok && hipMemcpy(P->d_seed, seeds, sizeof(uint64_t)*(size_t)B, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_pstar, ps.data(), sizeof(double)*ps.size(), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(P->d_mode, 0, (size_t)B) == hipSuccess && hipMemset(P->d_nevals, 0, sizeof(unsigned long long)) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_batch_create: device allocation failed\n"); (void)hipGetLastError(); synth_batch_free(P); return nullptr; }
  return P;
}
// the start points synth_p0 gives the B problems, [B][N]
void synth_batch_p0(void* h, double* out)
{
  BatchProblem* P = (BatchProblem*)h;
  for(int b = 0; b < P->B; b++)
    for(int j = 0; j < P->N; j++)
    {
      const double ps = urand(P->seed[b], 1, (uint64_t)j);
      out[(size_t)b*P->N + j] = ps + P->p0_spread * urand(P->seed[b], 4, (uint64_t)j);
    }
}
// mode[B]: 0 the model, 1 x[0] = NaN, 2 column zero_col of J exactly zero
int synth_batch_set_mode(void* h, const unsigned char* mode, int zero_col)
{
  BatchProblem* P = (BatchProblem*)h;
  P->zero_col = zero_col;
  return hipMemcpy(P->d_mode, mode, (size_t)P->B, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
int synth_batch_ncalls(void* h) { return ((BatchProblem*)h)->ncalls; }
long long synth_batch_nevals(void* h)
{
  BatchProblem* P = (BatchProblem*)h;
  unsigned long long n = 0;
  if(hipMemcpy(&n, P->d_nevals, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
void synth_batch_reset_counters(void* h)
{
  BatchProblem* P = (BatchProblem*)h;
  P->ncalls = 0;
  (void)hipMemset(P->d_nevals, 0, sizeof(unsigned long long));
}

// dogleg_callback_device_batch_t
void synth_cb_device_batch(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                           void* hip_stream, void* cookie)
{
  BatchProblem* P = (BatchProblem*)cookie;
  P->ncalls++;
  const size_t rows = (size_t)B*P->M;
  hipLaunchKernelGGL(k_batch_eval, dim3((unsigned)((rows + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, (int)B, P->M, P->N,
                     P->d_seed, P->d_pstar, P->d_mode, P->zero_col, live_dev, p_dev, P->eps, P->noise, x_dev, J_dev, P->d_nevals);
}

} // extern "C"
