// dense_batch.hip -- dogleg_amd_optimize_dense_batch: B small dense problems of one shape, the whole dog-leg loop
// (dogleg.c:1016-1022, 529-998, 1172-1476) per problem on the device.
//
// A round: the caller's batch callback evaluates x, J at the live problems' trial points (its kernels, on our stream),
// then ONE launch of k_batch_round does for every live problem what eval_point + evaluate_step + take_step do, then
// the host reads one counter of live problems (a 4-byte copy into page-locked memory).  Launches and synchronisations
// per round: constant, whatever B is.
//
// One wavefront per problem, BATCH_WPB problems per workgroup.  The wave sweeps the problem's J ONCE (coalesced loads
// of row tiles into LDS, the next tile's loads in flight while the current one is used): norm2(x), Jt x and the packed
// lower triangle of JtJ come out of that sweep, JtJ in registers (lane l holds entries l, l + 64, ...), then in LDS.
// Everything after it -- |J g|^2 = g' JtJ g, the packed Cholesky with the lambda loop, the two triangular solves, the
// choice of step, |J s|^2 = s' JtJ s -- is wave-level code on that on-chip copy.  What a rejected trial needs again of
// the point it started from (p, Jt x, the Cauchy and Gauss-Newton steps, JtJ: N (N + 11) / 2 doubles) lies in device
// memory per problem; the J of a point is never read a second time and only one x / J buffer per problem exists.
// Plain FMAs, no MFMA: DESIGN.md section 3, "Batches of small dense problems".
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <mutex>
#include <vector>
#include "dense_batch.h"

void dlg_set_error(const char* fmt, ...);

#define BMSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)

namespace {

constexpr int BATCH_WPB = 4;            // problems (wavefronts) per workgroup
constexpr int BATCH_TILE = 256;         // doubles of J staged per tile (and 64 of x behind them)
constexpr double LAMBDA_INITIAL = 1e-10;       // dogleg.c:138

enum { F_CAUCHY = 1, F_GN = 2, F_EDGE = 4, F_STARTED = 8 };
enum { SC_N2X, SC_TR, SC_LAMBDA, SC_N2C, SC_N2GN, SC_EI, SC_COUNT = 8 };
enum { ST_FLAGS, ST_ITER, ST_EVAL, ST_STATUS, ST_COUNT = 4 };

struct BatchDev
{
  int B, N, M, NP;
  const double* x; const double* J;
  double *p_before, *p_trial, *g, *cauchy, *gn, *JtJ, *sc;
  int* st; unsigned char* live; int* counter;
  int max_iterations;
  double trustregion0, dec_factor, dec_thr, inc_factor, inc_thr, jtx_thr, upd_thr, tr_thr;
};

template <int NMAX> struct BatchCfg
{
  static constexpr int NP = NMAX*(NMAX + 1)/2;
  static constexpr int NE = (NP + 63)/64;                       // entries of JtJ a lane accumulates
  static constexpr int SCR = NP > BATCH_TILE + 64 ? NP : BATCH_TILE + 64;     // the factor; during the sweep: the tile and its x
  static constexpr int LDSW = NP + SCR + NMAX;                  // doubles of LDS per wavefront
};

// LDS of ONE wavefront written by some lanes and read by others: the hardware keeps a wave's LDS operations in
// order, the compiler must not move them across this point
__device__ inline void wsync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// butterfly sums: every lane ends with the same bits (a + b == b + a at every level)
__device__ inline double wave_sum(double v)
{
  for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_max(double v)
{
  for(int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// first entry of column c of the packed lower triangle (column-major; the same bytes as the reference's row-major
// packed upper, dogleg.c:788-790)
__device__ inline int col_off(int c, int N) { return c*N - c*(c - 1)/2; }
__device__ inline double sym_at(const double* A, int i, int j, int N)
{
  return i >= j ? A[col_off(j, N) + i - j] : A[col_off(i, N) + j - i];
}
// v' A v, lane i holds v[i] (0 beyond N); V: N doubles of LDS
__device__ inline double quad_form(const double* A, double* V, double v, int N, int lane)
{
  wsync();
  if(lane < N) V[lane] = v;
  wsync();
  double r = 0.0;
  if(lane < N)
    for(int j = 0; j < N; j++) r += sym_at(A, lane, j, N)*V[j];
  return wave_sum(r*v);
}
// DPPTRF 'L' on the packed triangle in LDS (right-looking, as the reference's LAPACK call dogleg.c:782): false where
// a pivot is <= 0
__device__ inline bool chol_packed(double* L, int N, int lane)
{
  for(int j = 0; j < N; j++)
  {
    const int jj = col_off(j, N), m = N - j - 1;
    const double ajj = L[jj];
    if(ajj <= 0.0) return false;
    const double d = sqrt(ajj), inv = 1.0/d;
    double ci = 0.0;
    if(lane < m) ci = L[jj + 1 + lane]*inv;
    wsync();
    if(lane == 0) L[jj] = d;
    if(lane < m) L[jj + 1 + lane] = ci;
    wsync();
    if(lane < m)
      for(int c = 0; c <= lane; c++)
        L[col_off(j + 1 + c, N) + lane - c] -= ci*L[jj + 1 + c];
    wsync();
  }
  return true;
}
// (L L') u = rhs, lane i holds rhs[i] and gets u[i]
__device__ inline double solve_packed(const double* L, double b, int N, int lane)
{
  for(int j = 0; j < N; j++)
  {
    const double bj = __shfl(b, j, 64)/L[col_off(j, N)];
    if(lane == j) b = bj;
    else if(lane > j && lane < N) b -= bj*L[col_off(j, N) + lane - j];
  }
  for(int j = N - 1; j >= 0; j--)
  {
    const double xj = __shfl(b, j, 64)/L[col_off(j, N)];
    if(lane == j) b = xj;
    else if(lane < j) b -= xj*L[col_off(lane, N) + j - lane];
  }
  return b;
}

// one round of problem b; returns whether the problem is still live
template <int NMAX>
__device__ bool batch_problem(const BatchDev& A, int b, int lane, double* S)
{
  using C = BatchCfg<NMAX>;
  const int N = A.N, M = A.M, NP = A.NP;
  double* SA = S;                      // JtJ of the point the step is taken from
  double* SL = S + C::NP;              // its factor; during the sweep the row tile
  double* SV = SL + C::SCR;            // an N-vector
  double* tile = SL; double* xt = SL + BATCH_TILE;
  const size_t bN = (size_t)b*N;

  // ---- the sweep over the trial point's x and J: norm2(x), Jt x, JtJ (eval_point, dogleg.c:1004-1083, and the rows'
  // outer products dogleg.c:712-714) ----
  int ei[C::NE], ej[C::NE];
#pragma unroll
  for(int k = 0; k < C::NE; k++)
  {
    const int e = lane + 64*k;
    int c = 0;
    if(e < NP) { while(e >= col_off(c + 1, N)) c++; }
    ej[k] = c; ei[k] = e < NP ? c + e - col_off(c, N) : 0;
  }
  const double* Jb = A.J + (size_t)b*M*N;
  const double* xb = A.x + (size_t)b*M;
  const int T = min(64, BATCH_TILE/N);
  double acc[C::NE], gacc = 0.0, n2 = 0.0;
#pragma unroll
  for(int k = 0; k < C::NE; k++) acc[k] = 0.0;
  constexpr int NL = BATCH_TILE/64;
  double v[NL], xv;
  {
    const int tc = min(T, M), cnt = tc*N;
#pragma unroll
    for(int u = 0; u < NL; u++) v[u] = lane + 64*u < cnt ? Jb[lane + 64*u] : 0.0;
    xv = lane < tc ? xb[lane] : 0.0;
  }
  for(int r0 = 0; r0 < M; r0 += T)
  {
    const int tc = min(T, M - r0);
    wsync();
#pragma unroll
    for(int u = 0; u < NL; u++) tile[lane + 64*u] = v[u];
    xt[lane] = xv;
    wsync();
    n2 += xv*xv;
    if(r0 + T < M)
    {
      const int r1 = r0 + T, tn = min(T, M - r1), cnt = tn*N;
      const double* Jn = Jb + (size_t)r1*N;
#pragma unroll
      for(int u = 0; u < NL; u++) v[u] = lane + 64*u < cnt ? Jn[lane + 64*u] : 0.0;
      xv = lane < tn ? xb[r1 + lane] : 0.0;
    }
    for(int t = 0; t < tc; t++)
    {
      const double* row = tile + t*N;
#pragma unroll
      for(int k = 0; k < C::NE; k++) acc[k] += row[ei[k]]*row[ej[k]];
      if(lane < N) gacc += row[lane]*xt[t];
    }
  }
  const double n2x = wave_sum(n2);
  wsync();
#pragma unroll
  for(int k = 0; k < C::NE; k++) if(lane + 64*k < NP) SA[lane + 64*k] = acc[k];
  wsync();
  // a non-finite x or J shows in norm2(x) or on the diagonal of JtJ
  const double dg = lane < N ? SA[col_off(lane, N)] : 0.0;
  const bool finite = __all(isfinite(n2x) && isfinite(gacc) && isfinite(dg));

  // ---- evaluate_step (dogleg.c:1303-1356) and the swap of the two points (1427-1470) ----
  int* st = A.st + (size_t)ST_COUNT*b; double* sc = A.sc + (size_t)SC_COUNT*b;
  int flags = st[ST_FLAGS], iters = st[ST_ITER], status = 0;
  const int evals = st[ST_EVAL] + 1;
  double n2x_b = sc[SC_N2X], tr = sc[SC_TR], lam = sc[SC_LAMBDA], n2c = sc[SC_N2C], n2gn = sc[SC_N2GN];
  double EI = sc[SC_EI];
  double p_r = 0.0, g_r = 0.0, ca_r = 0.0, gn_r = 0.0;
  bool take = false;           // the trial point becomes the point to step from
  if(!finite) status = DOGLEG_AMD_BATCH_FAILED;
  else if(!(flags & F_STARTED)) take = true;
  else
  {
    const double rho = (n2x_b - n2x)/EI;
    if(rho != rho) status = DOGLEG_AMD_BATCH_FAILED;         // (the reference never leaves its retry loop there)
    else
    {
      if(rho < A.dec_thr)
      {
        if(!(flags & F_EDGE)) tr = sqrt(n2gn);
        tr *= A.dec_factor;
      }
      else if(rho > A.inc_thr && (flags & F_EDGE)) tr *= A.inc_factor;
      if(rho > 0.0) { take = true; iters++; }
      else if(tr < A.tr_thr) status = DOGLEG_AMD_BATCH_TRUSTREGION;
      else
      {
        // rejected: again from the cached steps of the point before (no evaluation, no factorisation)
        if(lane < N)
        {
          p_r = A.p_before[bN + lane]; g_r = A.g[bN + lane];
          if(flags & F_CAUCHY) ca_r = A.cauchy[bN + lane];
          if(flags & F_GN) gn_r = A.gn[bN + lane];
        }
        const double* Gb = A.JtJ + (size_t)b*NP;
        wsync();
        for(int e = lane; e < NP; e += 64) SA[e] = Gb[e];
        wsync();
      }
    }
  }
  if(take)
  {
    flags = F_STARTED; n2x_b = n2x; g_r = gacc;
    if(lane < N)
    {
      p_r = A.p_trial[bN + lane];
      A.p_before[bN + lane] = p_r; A.g[bN + lane] = g_r;
    }
    double* Gb = A.JtJ + (size_t)b*NP;
    for(int e = lane; e < NP; e += 64) Gb[e] = SA[e];
    if(wave_max(fabs(g_r)) <= A.jtx_thr) status = DOGLEG_AMD_BATCH_JTX;
    else if(iters >= A.max_iterations) status = DOGLEG_AMD_BATCH_MAX_ITERATIONS;
  }

  // ---- take_step (dogleg.c:1172-1297) ----
  if(status == 0)
  {
    const double tr2 = tr*tr;
    if(!(flags & F_CAUCHY))
    {
      const double g2 = wave_sum(g_r*g_r);
      const double Jg2 = quad_form(SA, SV, g_r, N, lane);
      const double k = -g2/Jg2;
      n2c = k*k*g2; ca_r = k*g_r;
      if(lane < N) A.cauchy[bN + lane] = ca_r;
      flags |= F_CAUCHY;
    }
    double s_r = 0.0;
    if(n2c >= tr2)
    {
      s_r = tr/sqrt(n2c)*ca_r;
      flags |= F_EDGE;
    }
    else
    {
      if(!(flags & F_GN))
      {
        // the factorisation is attempted only here, so lambda moves only here (dogleg.c:634-820)
        while(true)
        {
          wsync();
          for(int e = lane; e < NP; e += 64) SL[e] = SA[e];
          wsync();
          if(lam > 0.0 && lane < N) SL[col_off(lane, N)] += lam;
          wsync();
          if(chol_packed(SL, N, lane)) break;
          lam = lam == 0.0 ? LAMBDA_INITIAL : lam*10.0;
          if(!isfinite(lam)) { status = DOGLEG_AMD_BATCH_FAILED; break; }
        }
        if(status == 0)
        {
          gn_r = -solve_packed(SL, g_r, N, lane);
          if(lane >= N) gn_r = 0.0;
          n2gn = wave_sum(gn_r*gn_r);
          if(lane < N) A.gn[bN + lane] = gn_r;
          flags |= F_GN;
        }
      }
      if(status == 0)
      {
        if(n2gn <= tr2) { s_r = gn_r; flags &= ~F_EDGE; }
        else
        {
          // dogleg.c:927-998
          const double d = ca_r - gn_r;
          const double l2 = wave_sum(d*d), neg_c = wave_sum(d*ca_r);
          double disc = neg_c*neg_c - l2*(n2c - tr2);
          if(disc < 0.0) disc = 0.0;
          const double k = (neg_c + sqrt(disc))/l2;
          s_r = ca_r + k*(gn_r - ca_r);
          flags |= F_EDGE;
        }
      }
    }
    if(status == 0)
    {
      const double Js2 = quad_form(SA, SV, s_r, N, lane);
      EI = -2.0*wave_sum(g_r*s_r) - Js2;
      // the terminal small step is neither applied nor evaluated (dogleg.c:1289-1296, 1403-1408)
      if(wave_max(fabs(s_r)) <= A.upd_thr) status = DOGLEG_AMD_BATCH_SMALL_STEP;
      else if(lane < N) A.p_trial[bN + lane] = p_r + s_r;
    }
  }
  if(lane == 0)
  {
    sc[SC_N2X] = n2x_b; sc[SC_TR] = tr; sc[SC_LAMBDA] = lam; sc[SC_N2C] = n2c; sc[SC_N2GN] = n2gn; sc[SC_EI] = EI;
    st[ST_FLAGS] = flags; st[ST_ITER] = iters; st[ST_EVAL] = evals; st[ST_STATUS] = status;
    if(status != 0) A.live[b] = 0;
  }
  return status == 0;
}

template <int NMAX>
__global__ void __launch_bounds__(64*BATCH_WPB) k_batch_round(BatchDev A)
{
  __shared__ double lds[BATCH_WPB*BatchCfg<NMAX>::LDSW];
  __shared__ int s_live[BATCH_WPB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x*BATCH_WPB + w;
  bool still = false;
  if(b < A.B && A.live[b]) still = batch_problem<NMAX>(A, b, lane, lds + w*BatchCfg<NMAX>::LDSW);
  if(lane == 0) s_live[w] = still ? 1 : 0;
  __syncthreads();
  if(threadIdx.x == 0)
  {
    int n = 0;
    for(int k = 0; k < BATCH_WPB; k++) n += s_live[k];
    if(n) atomicAdd(A.counter, n);
  }
}

__global__ void __launch_bounds__(256) k_batch_init(BatchDev A)
{
  const int b = blockIdx.x*256 + threadIdx.x;
  if(b >= A.B) return;
  double* sc = A.sc + (size_t)SC_COUNT*b; int* st = A.st + (size_t)ST_COUNT*b;
  for(int k = 0; k < SC_COUNT; k++) sc[k] = 0.0;
  sc[SC_TR] = A.trustregion0;
  for(int k = 0; k < ST_COUNT; k++) st[k] = 0;
  A.live[b] = 1;
}

// ---- what is kept between calls ----
struct BatchCache
{
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int* h_counter = nullptr;
  void* d_eval = nullptr; size_t eval_bytes = 0;      // x, J of the trial points
  void* d_state = nullptr; size_t state_bytes = 0;    // everything else
};
std::mutex g_mu;
BatchCache g_cache;
thread_local double t_stats[3] = {0.0, 0.0, 0.0};

void release_locked()
{
  BatchCache& K = g_cache;
  if(K.device >= 0)
  {
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != K.device && hipSetDevice(K.device) == hipSuccess;
    if(K.d_eval) (void)hipFree(K.d_eval);
    if(K.d_state) (void)hipFree(K.d_state);
    if(K.h_counter) (void)hipHostFree(K.h_counter);
    for(hipEvent_t& e : K.ev) if(e) (void)hipEventDestroy(e);
    if(K.stream) (void)hipStreamDestroy(K.stream);
    if(sw) (void)hipSetDevice(cur);
  }
  K = BatchCache();
}

#define BHIP(call) \
  do { hipError_t e__ = (call); \
       if(e__ != hipSuccess) { dlg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
                               BMSG("dogleg_amd_optimize_dense_batch: %s -> %s", #call, hipGetErrorString(e__)); (void)hipGetLastError(); return -1; } } while(0)

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int run_locked(double* p, unsigned int B, unsigned int N, unsigned int M, dogleg_callback_device_batch_t* f, void* cookie,
               const dogleg_parameters2_t* prm, dogleg_amd_batch_result_t* results)
{
  const char* who = "dogleg_amd_optimize_dense_batch";
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    (void)hipGetLastError();
    dlg_set_error("%s: no HIP device", who); BMSG("%s: no HIP device (there is no CPU fallback)", who);
    return -1;
  }
  int dev = 0;
  BHIP(hipGetDevice(&dev));
  BatchCache& K = g_cache;
  if(K.device != dev) release_locked();
  if(K.device < 0)
  {
    BHIP(hipStreamCreateWithFlags(&K.stream, hipStreamNonBlocking));
    K.device = dev;
    BHIP(hipHostMalloc((void**)&K.h_counter, sizeof(int)));
  }
  const int NP = (int)(N*(N + 1)/2);
  // sizes in doubles first: B * M * (N + 1) can pass 2^64 bytes
  const double eval_d = (double)B*(double)M*((double)N + 1.0);
  const double state_d = (double)B*(5.0*N + NP + SC_COUNT + 1.0);
  if((eval_d + state_d)*8.0 > 1.0e15)
  {
    dlg_set_error("%s: %.3g bytes of device memory", who, (eval_d + state_d)*8.0);
    BMSG("%s: B = %u problems of %u x %u need %.3g bytes of device memory", who, B, M, N, (eval_d + state_d)*8.0);
    return -1;
  }
  const size_t x_bytes = align256(sizeof(double)*(size_t)B*M), J_bytes = align256(sizeof(double)*(size_t)B*M*N);
  const size_t vec_bytes = align256(sizeof(double)*(size_t)B*N), G_bytes = align256(sizeof(double)*(size_t)B*NP);
  const size_t sc_bytes = align256(sizeof(double)*(size_t)B*SC_COUNT), st_bytes = align256(sizeof(int)*(size_t)B*ST_COUNT);
  const size_t live_bytes = align256(B);
  const size_t eval_bytes = x_bytes + J_bytes, state_bytes = 5*vec_bytes + G_bytes + sc_bytes + st_bytes + live_bytes + 256;
  auto ensure = [&](void** ptr, size_t* have, size_t want) -> bool {
    if(*have >= want) return true;
    if(*ptr) { (void)hipFree(*ptr); *ptr = nullptr; *have = 0; }
    if(hipMalloc(ptr, want) != hipSuccess)
    {
      (void)hipGetLastError(); *ptr = nullptr;
      dlg_set_error("%s: cannot allocate %zu bytes of device memory", who, want);
      BMSG("%s: B = %u problems of %u x %u need %zu + %zu bytes of device memory: the allocation of %zu failed", who, B, M, N,
           eval_bytes, state_bytes, want);
      return false;
    }
    *have = want;
    return true;
  };
  if(!ensure(&K.d_eval, &K.eval_bytes, eval_bytes) || !ensure(&K.d_state, &K.state_bytes, state_bytes)) return -1;

  BatchDev A;
  A.B = (int)B; A.N = (int)N; A.M = (int)M; A.NP = NP;
  char* q = (char*)K.d_eval;
  A.x = (double*)q; q += x_bytes; A.J = (double*)q;
  q = (char*)K.d_state;
  A.p_before = (double*)q; q += vec_bytes; A.p_trial = (double*)q; q += vec_bytes; A.g = (double*)q; q += vec_bytes;
  A.cauchy = (double*)q; q += vec_bytes; A.gn = (double*)q; q += vec_bytes; A.JtJ = (double*)q; q += G_bytes;
  A.sc = (double*)q; q += sc_bytes; A.st = (int*)q; q += st_bytes; A.live = (unsigned char*)q; q += live_bytes;
  A.counter = (int*)q;
  A.max_iterations = prm->max_iterations; A.trustregion0 = prm->trustregion0;
  A.dec_factor = prm->trustregion_decrease_factor; A.dec_thr = prm->trustregion_decrease_threshold;
  A.inc_factor = prm->trustregion_increase_factor; A.inc_thr = prm->trustregion_increase_threshold;
  A.jtx_thr = prm->Jt_x_threshold; A.upd_thr = prm->update_threshold; A.tr_thr = prm->trustregion_threshold;

  const bool timing = getenv("DOGLEG_AMD_BATCH_TIMING") != nullptr;
  if(timing) for(hipEvent_t& e : K.ev) if(!e) BHIP(hipEventCreate(&e));
  hipStream_t st = K.stream;
  BHIP(hipMemcpyAsync(A.p_trial, p, sizeof(double)*(size_t)B*N, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_batch_init, dim3((B + 255)/256), dim3(256), 0, st, A);
  BHIP(hipGetLastError());
  const dim3 grid((B + BATCH_WPB - 1)/BATCH_WPB), block(64*BATCH_WPB);
  // a problem leaves a round finished or with a new trial point; rejected trials shrink the trust region until the
  // threshold stops them, so the rounds are bounded wherever the reference's own loop is.  The cap only keeps a
  // parameter set under which the reference would never return (a decrease factor >= 1) from holding the device.
  const long max_rounds = 1000000;
  long rounds = 0;
  double ms_cb = 0.0, ms_lib = 0.0;
  while(true)
  {
    if(rounds >= max_rounds)
    {
      dlg_set_error("%s: %ld rounds", who, rounds); BMSG("%s: still live problems after %ld rounds: giving up", who, rounds);
      return -1;
    }
    BHIP(hipMemsetAsync(A.counter, 0, sizeof(int), st));
    if(timing) BHIP(hipEventRecord(K.ev[0], st));
    f(A.p_trial, const_cast<double*>(A.x), const_cast<double*>(A.J), A.live, B, (void*)st, cookie);
    if(timing) BHIP(hipEventRecord(K.ev[1], st));
    if(N <= 8)       hipLaunchKernelGGL(k_batch_round<8>, grid, block, 0, st, A);
    else if(N <= 16) hipLaunchKernelGGL(k_batch_round<16>, grid, block, 0, st, A);
    else if(N <= 24) hipLaunchKernelGGL(k_batch_round<24>, grid, block, 0, st, A);
    else             hipLaunchKernelGGL(k_batch_round<32>, grid, block, 0, st, A);
    BHIP(hipGetLastError());
    if(timing) BHIP(hipEventRecord(K.ev[2], st));
    BHIP(hipMemcpyAsync(K.h_counter, A.counter, sizeof(int), hipMemcpyDeviceToHost, st));
    BHIP(hipStreamSynchronize(st));
    rounds++;
    if(timing)
    {
      float a = 0.f, c = 0.f;
      BHIP(hipEventElapsedTime(&a, K.ev[0], K.ev[1])); BHIP(hipEventElapsedTime(&c, K.ev[1], K.ev[2]));
      ms_cb += a; ms_lib += c;
    }
    if(*K.h_counter == 0) break;
  }
  std::vector<double> sc((size_t)B*SC_COUNT), pb((size_t)B*N);
  std::vector<int> sti((size_t)B*ST_COUNT);
  BHIP(hipMemcpyAsync(sc.data(), A.sc, sizeof(double)*sc.size(), hipMemcpyDeviceToHost, st));
  BHIP(hipMemcpyAsync(sti.data(), A.st, sizeof(int)*sti.size(), hipMemcpyDeviceToHost, st));
  BHIP(hipMemcpyAsync(pb.data(), A.p_before, sizeof(double)*pb.size(), hipMemcpyDeviceToHost, st));
  BHIP(hipStreamSynchronize(st));
  for(size_t b = 0; b < B; b++)
  {
    dogleg_amd_batch_result_t& R = results[b];
    const int status = sti[b*ST_COUNT + ST_STATUS];
    const bool failed = status == DOGLEG_AMD_BATCH_FAILED;
    R.norm2_x = failed ? -1.0 : sc[b*SC_COUNT + SC_N2X];
    R.trustregion = sc[b*SC_COUNT + SC_TR]; R.lambda = sc[b*SC_COUNT + SC_LAMBDA];
    R.iterations = sti[b*ST_COUNT + ST_ITER]; R.evaluations = sti[b*ST_COUNT + ST_EVAL]; R.status = status;
    if(!failed) memcpy(p + b*N, pb.data() + b*N, sizeof(double)*N);
  }
  t_stats[0] = (double)rounds; t_stats[1] = ms_cb; t_stats[2] = ms_lib;
  return 0;
}

} // namespace

int dlg_dense_batch_run(double* p, unsigned int B, unsigned int N, unsigned int M, dogleg_callback_device_batch_t* f,
                        void* cookie, const dogleg_parameters2_t* prm, dogleg_amd_batch_result_t* results)
{
  std::lock_guard<std::mutex> lk(g_mu);
  const int rc = run_locked(p, B, N, M, f, cookie, prm, results);
  if(getenv("DOGLEG_AMD_NO_BACKEND_CACHE")) release_locked();
  return rc;
}
void dlg_dense_batch_release()
{
  std::lock_guard<std::mutex> lk(g_mu);
  release_locked();
}
int dlg_dense_batch_last_stats(double* out, int n)
{
  int k = 0;
  for(; k < n && k < 3; k++) out[k] = t_stats[k];
  return k;
}
