// batch_numeric.hip -- numeric Jacobians for a batch whose model comes as values only (dogleg.h: dogleg_amd_batch_numeric_*).
// An adapter in front of the batch entry points, none of which changes: dogleg_amd_batch_numeric_callback is a
// dogleg_callback_device_batch_t that writes K copies of p (k_numeric_perturb), calls the caller's values model once for all
// of them, and forms J in the buffer it was handed from the copies' x (k_numeric_jacobian).  Two launches and one call of the
// model per invocation whatever B is, everything on the stream it is given, no synchronisation.  The step rule is
// include/dogleg_numeric_step.h; this file is compiled with -ffp-contract=off (build.py) on top of that header's pragma.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>
#include "../../include/dogleg.h"
#include "../../include/dogleg_numeric_step.h"

void dlg_set_error(const char* fmt, ...);

#define NMSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)

namespace {

// rows of J per tile of k_numeric_jacobian.  Not measured; the reasoning:
//  * the reads of a tile are one segment of TR doubles per variable and copy.  32 doubles are 256 bytes, two whole 128-byte
//    lines, and half a wavefront, so a wavefront reads two variables' segments at once; a shorter tile would split lines
//    between blocks.
//  * the shapes this is for have few measurements (40, 96): a tile of 32 leaves 3 full tiles of 96 and 32 + 8 of 40, a tile of
//    64 would leave 64 + 32 and 40 of 64 -- no better -- with twice the LDS, 33 KiB at Nstate = 64, and half as many blocks to
//    spread over the CUs when B is small.
constexpr int NUM_TR = 32;
constexpr int NUM_THREADS = 256;
constexpr int NUM_JG = NUM_THREADS/NUM_TR;      // variables filled at once: 8
constexpr unsigned NUM_MAX_GRID = 256*8;        // memory-bound kernels: at most 8 blocks per CU, the rest by grid stride

// The LDS tile holds TR rows of S doubles, S = Nstate | 1: odd.
//  * the fill is column-wise: a lane writes tile[r][j], the 16 lanes that one ds_write_b64 group serves have 16 consecutive r
//    and one j, so their addresses are S doubles apart.  A double covers two of the 32 four-byte banks a 64-bit store is
//    banked over (16 double-wide slots): the 16 lanes hit 16 different slots exactly when S is odd.  With S = Nstate and
//    Nstate = 16, 32, 48 or 64 all 16 would land on ONE slot, a 16-way conflict.
//  * the read-out is row-wise: lane e reads tile[e / Nstate][e % Nstate], that is address e + (e / Nstate)(S - Nstate).  A
//    64-bit read is served in groups of 32 lanes over 64 banks (32 double-wide slots).  With Nstate odd there is no padding
//    and the 32 addresses are consecutive: no conflict.  With Nstate even the padding is one double: every row boundary inside
//    the group shifts the rest by one, the 32 addresses span at most 32 + 31 slots, so no slot is hit more than twice (and
//    with Nstate >= 32 by at most one lane pair).  Padding by more than one double buys nothing on the fill and costs
//    this.
__host__ __device__ inline int tile_stride(int N) { return N | 1; }

// the K copies of p and the divisors; one thread per double of the copies.  Copy 0 is p, copy 1 + j has variable j at its plus
// point, copy 1 + N + j (central) at its minus point.  The threads of copy 0 write the divisors.  Dead problems are skipped.
__global__ void __launch_bounds__(NUM_THREADS)
k_numeric_perturb(unsigned int B, int N, int K, int scheme, double delta_rel, double delta_abs,
                  const double* __restrict__ p, const double* __restrict__ lower, const double* __restrict__ upper,
                  const unsigned char* __restrict__ live, double* __restrict__ pc, double* __restrict__ div)
{
  const size_t BN = (size_t)B*N, total = BN*(size_t)K;
  for(size_t idx = (size_t)blockIdx.x*NUM_THREADS + threadIdx.x; idx < total; idx += (size_t)gridDim.x*NUM_THREADS)
  {
    const int k = (int)(idx/BN);
    const size_t e = idx - (size_t)k*BN;
    const unsigned int b = (unsigned int)(e/N);
    if(!live[b]) continue;
    const int j = (int)(e - (size_t)b*N);
    const double pj = p[e];
    double v = pj;
    const int which = k == 0 ? 0 : (k - 1 == j ? 1 : (k - 1 - N == j ? 2 : -1));    // divisor / plus / minus point / p itself
    if(which >= 0)
    {
      double tp, tm, d;
      dogleg_numeric_step(scheme, pj, lower ? lower[e] : -INFINITY, upper ? upper[e] : INFINITY, delta_rel, delta_abs, &tp, &tm, &d);
      if(which == 0) div[e] = d;
      if(which == 1) v = tp;
      if(which == 2) v = tm;
    }
    pc[idx] = v;
  }
}

// J and x of the live problems from the copies' x.  A block takes tiles of TR measurement rows of one problem.  Fill: lane
// (r, jg) reads the segments x+[j][r0 + r] and x-[j][r0 + r] for j = jg, jg + 8, ..., contiguous along r, and puts the quotient
// at tile[r][j].  Read-out: the tile's rows are ONE span of rows * N doubles of J[b], stored by consecutive lanes.
__global__ void __launch_bounds__(NUM_THREADS)
k_numeric_jacobian(unsigned int B, int N, int M, int central, const double* __restrict__ xc, const double* __restrict__ div,
                   const unsigned char* __restrict__ live, double* __restrict__ x, double* __restrict__ J)
{
  extern __shared__ double tile[];
  const int S = tile_stride(N);
  const int ntiles = (M + NUM_TR - 1)/NUM_TR;
  const size_t BM = (size_t)B*M, work = (size_t)B*ntiles;
  const int r = threadIdx.x % NUM_TR, jg = threadIdx.x / NUM_TR;
  for(size_t w = blockIdx.x; w < work; w += gridDim.x)
  {
    const unsigned int b = (unsigned int)(w/ntiles);
    if(!live[b]) continue;                                 // (the whole block: no barrier is skipped by a part of it)
    const int r0 = (int)(w - (size_t)b*ntiles)*NUM_TR;
    const int rows = min(NUM_TR, M - r0);
    const size_t row = (size_t)b*M + r0 + r;
    if(r < rows)
    {
      const double x0 = xc[row];
      if(jg == 0) x[row] = x0;
      for(int j = jg; j < N; j += NUM_JG)
      {
        const double xp = xc[(size_t)(1 + j)*BM + row];
        const double xm = central ? xc[(size_t)(1 + N + j)*BM + row] : x0;
        const double d = div[(size_t)b*N + j];
        tile[r*S + j] = d == 0.0 ? 0.0 : (xp - xm)/d;
      }
    }
    __syncthreads();
    double* Jt = J + ((size_t)b*M + r0)*N;
    for(int e = threadIdx.x; e < rows*N; e += NUM_THREADS)
    {
      const int rr = e/N;
      Jt[e] = tile[rr*S + (e - rr*N)];
    }
    __syncthreads();
  }
}

// the adapter invoked with more problems than its handle has: NaN into x of the live ones, which then fail alone
__global__ void __launch_bounds__(NUM_THREADS)
k_numeric_refuse(unsigned int B, int M, const unsigned char* __restrict__ live, double* __restrict__ x)
{
  const size_t total = (size_t)B*M;
  for(size_t idx = (size_t)blockIdx.x*NUM_THREADS + threadIdx.x; idx < total; idx += (size_t)gridDim.x*NUM_THREADS)
    if(live[idx/M]) x[idx] = nan("");
}

unsigned grid_for(size_t items_per_thread_total)
{
  const size_t blocks = (items_per_thread_total + NUM_THREADS - 1)/NUM_THREADS;
  return (unsigned)(blocks < 1 ? 1 : (blocks > NUM_MAX_GRID ? NUM_MAX_GRID : blocks));
}

struct TimedCall { hipEvent_t ev[4]; };        // before the copies | before f | behind f | behind J
constexpr size_t NUM_MAX_PENDING = 4096;       // timed invocations kept until dogleg_amd_batch_numeric_stats reads them

} // namespace

struct dogleg_amd_batch_numeric
{
  unsigned int B, N, M;
  int K, scheme;
  double delta_rel, delta_abs;
  dogleg_callback_device_batch_values_t* f;
  void* cookie;
  int device;
  double* d_pc;          // [K][B][N]
  double* d_xc;          // [K][B][M]
  double* d_div;         // [B][N]
  double* d_bounds;      // host bounds copied: lower | upper, each [B][N] where given
  const double* lower;   // device, or nullptr
  const double* upper;
  bool said_mismatch;
  double invocations, f_calls, copies, launches, ms_f, ms_lib;
  std::vector<TimedCall> pending;
};

namespace {

bool refuse(const char* why)
{
  dlg_set_error("dogleg_amd_batch_numeric_create: %s", why); NMSG("dogleg_amd_batch_numeric_create: %s", why);
  return false;
}

bool check_arguments(unsigned B, unsigned N, unsigned M, dogleg_callback_device_batch_values_t* f,
                     const dogleg_amd_numeric_options_t* opt)
{
  if(B == 0 || N == 0 || M == 0) return refuse("B, Nstate and Nmeas must not be 0");
  if(N > DOGLEG_AMD_BATCH_MAX_NSTATE) return refuse("Nstate above DOGLEG_AMD_BATCH_MAX_NSTATE = 64");
  if(!f) return refuse("f is NULL");
  if(!opt) return true;
  if(opt->scheme != DOGLEG_AMD_NUMERIC_FORWARD && opt->scheme != DOGLEG_AMD_NUMERIC_CENTRAL)
    return refuse("unknown scheme (DOGLEG_AMD_NUMERIC_FORWARD or DOGLEG_AMD_NUMERIC_CENTRAL)");
  if(!(opt->delta_rel >= 0.0) || !(opt->delta_abs >= 0.0)) return refuse("delta_rel and delta_abs must not be negative or NaN");
  if(!opt->bounds_on_device)
    for(size_t i = 0; i < (size_t)B*N; i++)
    {
      const double lo = opt->lower ? opt->lower[i] : -INFINITY, hi = opt->upper ? opt->upper[i] : INFINITY;
      if(!(lo <= hi))
      {
        dlg_set_error("dogleg_amd_batch_numeric_create: lower > upper");
        NMSG("dogleg_amd_batch_numeric_create: problem %zu, variable %zu: lower %g > upper %g (or a NaN)", i/N, i%N, lo, hi);
        return false;
      }
    }
  return true;
}

void harvest(dogleg_amd_batch_numeric* h)
{
  if(h->pending.empty()) return;
  (void)hipEventSynchronize(h->pending.back().ev[3]);
  for(TimedCall& c : h->pending)
  {
    float a = 0.f, b = 0.f, d = 0.f;
    if(hipEventElapsedTime(&a, c.ev[0], c.ev[1]) == hipSuccess && hipEventElapsedTime(&b, c.ev[1], c.ev[2]) == hipSuccess &&
       hipEventElapsedTime(&d, c.ev[2], c.ev[3]) == hipSuccess) { h->ms_lib += (double)a + (double)d; h->ms_f += b; }
    for(hipEvent_t e : c.ev) (void)hipEventDestroy(e);
  }
  (void)hipGetLastError();
  h->pending.clear();
}

} // namespace

extern "C" {

void dogleg_amd_numeric_step(int scheme, double p, double lo, double hi, double delta_rel, double delta_abs,
                             double* tp, double* tm, double* d)
{
  dogleg_numeric_step(scheme, p, lo, hi, delta_rel, delta_abs, tp, tm, d);
}

void dogleg_amd_batch_numeric_destroy(struct dogleg_amd_batch_numeric* h)
{
  if(!h) return;
  int cur = -1;
  const bool sw = h->device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != h->device && hipSetDevice(h->device) == hipSuccess;
  harvest(h);
  if(h->d_pc) (void)hipFree(h->d_pc);
  if(h->d_xc) (void)hipFree(h->d_xc);
  if(h->d_div) (void)hipFree(h->d_div);
  if(h->d_bounds) (void)hipFree(h->d_bounds);
  if(sw) (void)hipSetDevice(cur);
  (void)hipGetLastError();
  delete h;
}

struct dogleg_amd_batch_numeric* dogleg_amd_batch_numeric_create(unsigned B, unsigned Nstate, unsigned Nmeas,
                                                                 dogleg_callback_device_batch_values_t* f, void* cookie,
                                                                 const dogleg_amd_numeric_options_t* opt)
{
  const char* who = "dogleg_amd_batch_numeric_create";
  if(!check_arguments(B, Nstate, Nmeas, f, opt)) return nullptr;
  const int scheme = opt ? opt->scheme : DOGLEG_AMD_NUMERIC_FORWARD;
  const int K = scheme == DOGLEG_AMD_NUMERIC_CENTRAL ? 2*(int)Nstate + 1 : (int)Nstate + 1;
  const bool host_lo = opt && !opt->bounds_on_device && opt->lower, host_hi = opt && !opt->bounds_on_device && opt->upper;
  const double doubles = (double)K*(double)B*((double)Nstate + (double)Nmeas) + (double)B*Nstate*(1.0 + (host_lo ? 1 : 0) + (host_hi ? 1 : 0));
  if(doubles*8.0 > 1.0e15)
  {
    dlg_set_error("%s: %.3g bytes of device memory", who, doubles*8.0);
    NMSG("%s: B = %u problems of %u x %u with %d copies need %.3g bytes of device memory", who, B, Nmeas, Nstate, K, doubles*8.0);
    return nullptr;
  }
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    (void)hipGetLastError();
    dlg_set_error("%s: no HIP device", who); NMSG("%s: no HIP device (there is no CPU fallback)", who);
    return nullptr;
  }
  dogleg_amd_batch_numeric* h = new (std::nothrow) dogleg_amd_batch_numeric();
  if(!h) return nullptr;
  h->B = B; h->N = Nstate; h->M = Nmeas; h->K = K; h->scheme = scheme;
  const double dflt = scheme == DOGLEG_AMD_NUMERIC_CENTRAL ? DOGLEG_NUMERIC_DELTA_CENTRAL : DOGLEG_NUMERIC_DELTA_FORWARD;
  const bool defaults = !opt || (opt->delta_rel <= 0.0 && opt->delta_abs <= 0.0);
  h->delta_rel = defaults ? dflt : opt->delta_rel; h->delta_abs = defaults ? dflt : opt->delta_abs;
  h->f = f; h->cookie = cookie; h->device = -1;
  h->d_pc = h->d_xc = h->d_div = h->d_bounds = nullptr; h->lower = h->upper = nullptr;
  h->said_mismatch = false;
  h->invocations = h->f_calls = h->copies = h->launches = h->ms_f = h->ms_lib = 0.0;
  const size_t vec = sizeof(double)*(size_t)B*Nstate;
  const size_t pc_bytes = (size_t)K*vec, xc_bytes = sizeof(double)*(size_t)K*B*Nmeas;
  const size_t bounds_bytes = vec*((host_lo ? 1 : 0) + (host_hi ? 1 : 0));
  bool ok = hipGetDevice(&h->device) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_pc, pc_bytes) == hipSuccess && hipMalloc((void**)&h->d_xc, xc_bytes) == hipSuccess &&
       hipMalloc((void**)&h->d_div, vec) == hipSuccess && (bounds_bytes == 0 || hipMalloc((void**)&h->d_bounds, bounds_bytes) == hipSuccess);
  if(!ok)
  {
    (void)hipGetLastError();
    dlg_set_error("%s: cannot allocate %.3g bytes of device memory", who, doubles*8.0);
    NMSG("%s: B = %u problems of %u x %u with %d copies need %zu + %zu + %zu + %zu bytes of device memory: the allocation failed",
         who, B, Nmeas, Nstate, K, pc_bytes, xc_bytes, vec, bounds_bytes);
    dogleg_amd_batch_numeric_destroy(h);
    return nullptr;
  }
  if(opt && opt->bounds_on_device) { h->lower = opt->lower; h->upper = opt->upper; }
  else
  {
    double* q = h->d_bounds;
    if(host_lo) { ok = ok && hipMemcpy(q, opt->lower, vec, hipMemcpyHostToDevice) == hipSuccess; h->lower = q; q += (size_t)B*Nstate; }
    if(host_hi) { ok = ok && hipMemcpy(q, opt->upper, vec, hipMemcpyHostToDevice) == hipSuccess; h->upper = q; }
    if(!ok)
    {
      dlg_set_error("%s: the upload of the bounds failed", who); NMSG("%s: the upload of the bounds failed", who);
      (void)hipGetLastError();
      dogleg_amd_batch_numeric_destroy(h);
      return nullptr;
    }
  }
  return h;
}

void dogleg_amd_batch_numeric_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                       unsigned int B, void* hip_stream, void* cookie)
{
  dogleg_amd_batch_numeric* h = (dogleg_amd_batch_numeric*)cookie;
  hipStream_t st = (hipStream_t)hip_stream;
  h->invocations += 1.0;
  if(B > h->B)
  {
    if(!h->said_mismatch)
      NMSG("dogleg_amd_batch_numeric_callback: invoked for B = %u problems, the handle was made for %u: every problem fails", B, h->B);
    h->said_mismatch = true;
    hipLaunchKernelGGL(k_numeric_refuse, dim3(grid_for((size_t)B*h->M)), dim3(NUM_THREADS), 0, st, B, (int)h->M, live_dev, x_dev);
    h->launches += 1.0;
    return;
  }
  const int N = (int)h->N, M = (int)h->M, K = h->K;
  TimedCall T;
  bool timed = getenv("DOGLEG_AMD_BATCH_TIMING") != nullptr && h->pending.size() < NUM_MAX_PENDING;
  if(timed)
    for(int i = 0; i < 4; i++)
      if(hipEventCreate(&T.ev[i]) != hipSuccess) { for(int k = 0; k < i; k++) (void)hipEventDestroy(T.ev[k]); (void)hipGetLastError(); timed = false; break; }
  if(timed) (void)hipEventRecord(T.ev[0], st);
  hipLaunchKernelGGL(k_numeric_perturb, dim3(grid_for((size_t)K*B*N)), dim3(NUM_THREADS), 0, st, B, N, K, h->scheme, h->delta_rel,
                     h->delta_abs, p_dev, h->lower, h->upper, live_dev, h->d_pc, h->d_div);
  if(timed) (void)hipEventRecord(T.ev[1], st);
  h->f(h->d_pc, h->d_xc, live_dev, B, (unsigned int)K, hip_stream, h->cookie);
  if(timed) (void)hipEventRecord(T.ev[2], st);
  const int ntiles = (M + NUM_TR - 1)/NUM_TR;
  const size_t work = (size_t)B*ntiles;
  hipLaunchKernelGGL(k_numeric_jacobian, dim3((unsigned)(work > NUM_MAX_GRID ? NUM_MAX_GRID : work)), dim3(NUM_THREADS),
                     sizeof(double)*(size_t)NUM_TR*tile_stride(N), st, B, N, M, h->scheme == DOGLEG_AMD_NUMERIC_CENTRAL ? 1 : 0,
                     h->d_xc, h->d_div, live_dev, x_dev, J_dev);
  if(timed) { (void)hipEventRecord(T.ev[3], st); h->pending.push_back(T); }
  h->f_calls += 1.0; h->copies += (double)K*(double)B; h->launches += 2.0;
}

int dogleg_amd_batch_numeric_stats(struct dogleg_amd_batch_numeric* h, double* out, int n)
{
  if(!h || !out || n <= 0) return 0;
  harvest(h);
  const double v[6] = {h->invocations, h->f_calls, h->copies, h->launches, h->ms_f, h->ms_lib};
  const int m = n < 6 ? n : 6;
  for(int i = 0; i < m; i++) out[i] = v[i];
  return m;
}

int dogleg_amd_batch_numeric_buffers(struct dogleg_amd_batch_numeric* h, const double** p_copies_dev,
                                     const double** x_copies_dev, const double** divisor_dev)
{
  if(!h) return -1;
  if(p_copies_dev) *p_copies_dev = h->d_pc;
  if(x_copies_dev) *x_copies_dev = h->d_xc;
  if(divisor_dev) *divisor_dev = h->d_div;
  return h->K;
}

} // extern "C"
