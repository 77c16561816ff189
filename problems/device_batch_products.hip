// device_batch_products.hip -- a batch of the dense synthetic problems of problems.c evaluated ON THE GPU in the PRODUCTS
// form: a dogleg_callback_device_batch_products_t (include/dogleg.h, dogleg_amd_optimize_dense_products_batch) that hands
// back norm2(x), Jt x and JtJ of every live problem and never writes x or J to memory.  Problem b is
// DenseProblem(M[b], N, seed[b], eps, noise, p0_spread) of problems.c WITH ITS OWN NUMBER OF MEASUREMENTS M[b]; each row
// is evaluated with the arithmetic of k_batch_eval (device_batch_problems.hip) and the file is compiled with the same
// -ffp-contract=off, so the J-form twin, the host callback handed to the CPU oracle and this callback describe the same
// function up to the last bits of sin / cos.
//
// This is also the worked example of a fused model kernel: one wavefront per live problem walks the
// problem's rows in tiles of 64.  Lane t evaluates row r0 + t and puts that row of J into an LDS tile (row stride N | 1:
// the lanes write different rows, an odd stride keeps them on different banks); then lane l adds the tile's rows, in
// ascending row order, into its entries l, l + 64, ... of the packed triangle of JtJ, and the lanes below N add them
// into Jt x.  norm2(x) is one wave sum at the end.  No atomics in the sums and no sum across problems: the same bits come
// out whatever B is and wherever the problem lies in the batch.
//
// Switches for the tests (synth_pbatch_set_mode, synth_pbatch_set_layout): the layout of JtJ (packed upper; unpacked
// with both triangles; unpacked with the strict lower triangle, which the library must never read, filled with NaN), and
// per problem: x[0] = NaN (mode 1), column zero_col of J exactly zero (mode 2), or a NaN in the one entry (0, 1) of JtJ
// and nowhere else (mode 3).
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

constexpr int NSTATE_MAX = 64;           // DOGLEG_AMD_BATCH_MAX_NSTATE
// problems (wavefronts) per workgroup: a wavefront's tile is 64 (N | 1) + 64 doubles, 33 792 bytes at N = 64
constexpr int wpb_of(int NMAX) { return NMAX <= 32 ? 2 : 1; }
enum { LAYOUT_PACKED_UPPER = 0, LAYOUT_UNPACKED = 1, LAYOUT_UNPACKED_NAN_LOWER = 2 };
enum { MODE_MODEL = 0, MODE_NAN = 1, MODE_ZERO_COLUMN = 2, MODE_NAN_OFFDIAGONAL = 3 };

struct ProductsBatch
{
  int B, N, zero_col, layout;
  double eps, noise, p0_spread;
  std::vector<uint64_t> seed;      // host copy
  uint64_t* d_seed;
  int* d_M;                        // [B]
  double* d_pstar;                 // [B][N]
  unsigned char* d_mode;           // [B]
  unsigned long long* d_nevals;    // problem evaluations done
  int ncalls;
};

struct EvalArgs
{
  int B, N, zero_col, layout;
  const uint64_t* seed; const int* M; const double* pstar; const unsigned char* mode; const unsigned char* live;
  const double* p;
  double eps, noise;
  double *norm2x, *xtJ, *JtJ;
  unsigned long long* nevals;
};

// LDS of one wavefront written by some lanes and read by others
__device__ inline void wsync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// first entry of column c of the packed lower triangle, column-major: the same bytes as the row-major packed upper
__device__ inline int col_off(int c, int N) { return c*N - c*(c - 1)/2; }

// NMAX: 8, 16, 24, 32, 48 or 64, the size class of N (how many entries of the triangle a lane holds)
template <int NMAX>
__global__ void __launch_bounds__(64*wpb_of(NMAX)) k_products_eval(EvalArgs A)
{
  constexpr int NE = (NMAX*(NMAX + 1)/2 + 63)/64, WPB = wpb_of(NMAX);
  extern __shared__ double lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x*WPB + w;
  if(b >= A.B || !A.live[b]) return;
  const int N = A.N, NS = N | 1, NP = N*(N + 1)/2, M = A.M[b];
  double* tile = lds + (size_t)w*(64*NS + 64);          // 64 rows of J
  double* xt = tile + 64*NS;                            // and their x
  if(lane == 0) atomicAdd(A.nevals, 1ull);
  const uint64_t sd = A.seed[b];
  const int md = A.mode[b];
  const double* pb = A.p + (size_t)b*N; const double* ps = A.pstar + (size_t)b*N;
  const double sq = sqrt((double)N);

  // entry lane + 64 k of the packed triangle is (ei[k], ej[k]), ei >= ej
  int ei[NE], ej[NE];
#pragma unroll
  for(int k = 0; k < NE; k++)
  {
    const int e = lane + 64*k;
    int c = 0;
    if(e < NP) { while(e >= col_off(c + 1, N)) c++; }
    ej[k] = c; ei[k] = e < NP ? c + e - col_off(c, N) : 0;
  }
  double acc[NE], gacc = 0.0, n2 = 0.0;
#pragma unroll
  for(int k = 0; k < NE; k++) acc[k] = 0.0;

  for(int r0 = 0; r0 < M; r0 += 64)
  {
    const int tc = min(64, M - r0), r = r0 + lane;
    wsync();
    if(lane < tc)
    {
      // the row's arithmetic of k_batch_eval: u summed in index order, as the host's loop
      double u = 0.0;
      for(int j = 0; j < N; j++)
      {
        const double c = urand(sd, 3, (uint64_t)r*(uint64_t)N + (uint64_t)j) / sq;
        const double dp = (md == MODE_ZERO_COLUMN && j == A.zero_col) ? 0.0 : pb[j] - ps[j];
        u += c*dp;
      }
      double xr = u + A.eps*sin(u) - A.noise*urand(sd, 5, (uint64_t)r);
      if(md == MODE_NAN && r == 0) xr = nan("");
      const double d = 1.0 + A.eps*cos(u);
      double* Jr = tile + lane*NS;
      for(int j = 0; j < N; j++)
      {
        const double c = urand(sd, 3, (uint64_t)r*(uint64_t)N + (uint64_t)j) / sq;
        Jr[j] = (md == MODE_ZERO_COLUMN && j == A.zero_col) ? 0.0 : c*d;
      }
      xt[lane] = xr;
      n2 += xr*xr;
    }
    wsync();
    for(int t = 0; t < tc; t++)
    {
      const double* row = tile + t*NS;
#pragma unroll
      for(int k = 0; k < NE; k++) acc[k] += row[ei[k]]*row[ej[k]];
      if(lane < N) gacc += row[lane]*xt[t];
    }
  }
  for(int o = 32; o > 0; o >>= 1) n2 += __shfl_xor(n2, o, 64);
  if(lane == 0) A.norm2x[b] = n2;
  if(lane < N) A.xtJ[(size_t)b*N + lane] = gacc;
#pragma unroll
  for(int k = 0; k < NE; k++)
  {
    const int e = lane + 64*k;
    if(e >= NP) continue;
    const int i = ei[k], j = ej[k];          // i >= j: JtJ[j][i] lies in the upper triangle
    double v = acc[k];
    if(md == MODE_NAN_OFFDIAGONAL && i == 1 && j == 0) v = nan("");
    if(A.layout == LAYOUT_PACKED_UPPER) A.JtJ[(size_t)b*NP + e] = v;
    else
    {
      double* G = A.JtJ + (size_t)b*N*N;
      G[j*N + i] = v;
      if(i != j) G[i*N + j] = A.layout == LAYOUT_UNPACKED_NAN_LOWER ? nan("") : v;
    }
  }
}
// the grid, the block and the LDS follow the size class: at most 34 816 bytes (two problems of 32 variables)
template <int NMAX> void launch_eval(const EvalArgs& A, hipStream_t st)
{
  constexpr int WPB = wpb_of(NMAX);
  const size_t lds = sizeof(double)*(size_t)WPB*(64*(A.N | 1) + 64);
  hipLaunchKernelGGL(k_products_eval<NMAX>, dim3((A.B + WPB - 1)/WPB), dim3(64*WPB), lds, st, A);
}
} // namespace

extern "C" {

void synth_pbatch_free(void* h)
{
  ProductsBatch* P = (ProductsBatch*)h;
  if(!P) return;
  (void)hipFree(P->d_seed); (void)hipFree(P->d_M); (void)hipFree(P->d_pstar); (void)hipFree(P->d_mode); (void)hipFree(P->d_nevals);
  delete P;
}
// M[B]: every problem's own number of measurements
void* synth_pbatch_create(int B, int N, const int* M, const uint64_t* seeds, double eps, double noise, double p0_spread)
{
  if(B <= 0 || N <= 0 || N > NSTATE_MAX) { fprintf(stderr, "synth_pbatch_create: B = %d, N = %d\n", B, N); return nullptr; }
  for(int b = 0; b < B; b++) if(M[b] <= 0) { fprintf(stderr, "synth_pbatch_create: M[%d] = %d\n", b, M[b]); return nullptr; }
  ProductsBatch* P = new ProductsBatch();
  P->B = B; P->N = N; P->zero_col = 0; P->layout = LAYOUT_PACKED_UPPER; P->eps = eps; P->noise = noise; P->p0_spread = p0_spread;
  P->ncalls = 0;
  P->seed.assign(seeds, seeds + B);
  P->d_seed = nullptr; P->d_M = nullptr; P->d_pstar = nullptr; P->d_mode = nullptr; P->d_nevals = nullptr;
  std::vector<double> ps((size_t)B*N);
  for(int b = 0; b < B; b++)
    for(int j = 0; j < N; j++) ps[(size_t)b*N + j] = urand(seeds[b], 1, (uint64_t)j);
  bool ok = hipMalloc(&P->d_seed, sizeof(uint64_t)*(size_t)B) == hipSuccess && hipMalloc(&P->d_M, sizeof(int)*(size_t)B) == hipSuccess &&
            hipMalloc(&P->d_pstar, sizeof(double)*ps.size()) == hipSuccess &&
            hipMalloc(&P->d_mode, (size_t)B) == hipSuccess && hipMalloc(&P->d_nevals, sizeof(unsigned long long)) == hipSuccess;
  ok = ok && hipMemcpy(P->d_seed, seeds, sizeof(uint64_t)*(size_t)B, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_M, M, sizeof(int)*(size_t)B, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(P->d_pstar, ps.data(), sizeof(double)*ps.size(), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset(P->d_mode, 0, (size_t)B) == hipSuccess && hipMemset(P->d_nevals, 0, sizeof(unsigned long long)) == hipSuccess;
  if(!ok) { fprintf(stderr, "synth_pbatch_create: device allocation failed\n"); (void)hipGetLastError(); synth_pbatch_free(P); return nullptr; }
  return P;
}
// the start points synth_p0 gives the B problems, [B][N] (they do not depend on M)
void synth_pbatch_p0(void* h, double* out)
{
  ProductsBatch* P = (ProductsBatch*)h;
  for(int b = 0; b < P->B; b++)
    for(int j = 0; j < P->N; j++)
    {
      const double ps = urand(P->seed[b], 1, (uint64_t)j);
      out[(size_t)b*P->N + j] = ps + P->p0_spread * urand(P->seed[b], 4, (uint64_t)j);
    }
}
// mode[B]: 0 the model, 1 x[0] = NaN, 2 column zero_col of J exactly zero, 3 JtJ[0][1] = NaN (needs N >= 2)
int synth_pbatch_set_mode(void* h, const unsigned char* mode, int zero_col)
{
  ProductsBatch* P = (ProductsBatch*)h;
  if(zero_col < 0 || zero_col >= P->N) return -1;
  P->zero_col = zero_col;
  return hipMemcpy(P->d_mode, mode, (size_t)P->B, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
}
// 0 packed upper, 1 unpacked (both triangles written), 2 unpacked with the strict lower triangle NaN; the caller passes
// the matching JtJ_packed / JtJ_upper to the library
int synth_pbatch_set_layout(void* h, int layout)
{
  if(layout < LAYOUT_PACKED_UPPER || layout > LAYOUT_UNPACKED_NAN_LOWER) return -1;
  ((ProductsBatch*)h)->layout = layout;
  return 0;
}
int synth_pbatch_ncalls(void* h) { return ((ProductsBatch*)h)->ncalls; }
long long synth_pbatch_nevals(void* h)
{
  ProductsBatch* P = (ProductsBatch*)h;
  unsigned long long n = 0;
  if(hipMemcpy(&n, P->d_nevals, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
void synth_pbatch_reset_counters(void* h)
{
  ProductsBatch* P = (ProductsBatch*)h;
  P->ncalls = 0;
  (void)hipMemset(P->d_nevals, 0, sizeof(unsigned long long));
}

// dogleg_callback_device_batch_products_t
void synth_cb_device_batch_products(const double* p_dev, double* norm2x_dev, double* xtJ_dev, double* JtJ_dev,
                                    const unsigned char* live_dev, unsigned int B, void* hip_stream, void* cookie)
{
  ProductsBatch* P = (ProductsBatch*)cookie;
  P->ncalls++;
  EvalArgs A;
  A.B = (int)B; A.N = P->N; A.zero_col = P->zero_col; A.layout = P->layout;
  A.seed = P->d_seed; A.M = P->d_M; A.pstar = P->d_pstar; A.mode = P->d_mode; A.live = live_dev; A.p = p_dev;
  A.eps = P->eps; A.noise = P->noise; A.norm2x = norm2x_dev; A.xtJ = xtJ_dev; A.JtJ = JtJ_dev; A.nevals = P->d_nevals;
  const int N = P->N;
  hipStream_t st = (hipStream_t)hip_stream;
  if(N <= 8)       launch_eval<8>(A, st);
  else if(N <= 16) launch_eval<16>(A, st);
  else if(N <= 24) launch_eval<24>(A, st);
  else if(N <= 32) launch_eval<32>(A, st);
  else if(N <= 48) launch_eval<48>(A, st);
  else             launch_eval<64>(A, st);
}

} // extern "C"
