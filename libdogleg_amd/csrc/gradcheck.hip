// gradcheck.hip -- dogleg_amd_check_jacobian_device{,_batch} and dogleg_amd_testGradient_device: the Jacobian a DEVICE
// callback reports against central differences of its x, with the arithmetic of the reference's dogleg_testGradient
// (dogleg.c:352-522, gradtest.cpp here) and everything on the device.
//
// Sparse problems are checked one COLOUR at a time (gradcheck_plan.h): the variables of a colour share no measurement
// row, so one pair of evaluations at p0 -+ delta/2 sum_{v in colour} e_v gives the central difference of every declared
// entry of those variables.  Per colour the stream gets
//   k_gc_perturb           the two perturbed p
//   the callback, twice    x0, J0 and x1, J1 (its kernels, on our stream)
//   k_gc_compare_sparse    one lane per entry of the colour's list (Jt index t, row r, variable v; sorted by variable, so
//                          a wave's lanes mostly share v): gathers J0[t], J1[t], x0[r], x1[r]
//   k_gc_outside           the colour's rows WITHOUT an entry: they must not have moved
// and the four buffers are reused by the next colour under stream order.  Dense problems and batches take one column at
// a time with k_gc_compare_dense, one thread per (problem, row).  One synchronisation and one download end the call.
//
// Reductions: per lane, then per wave (shuffles), then per workgroup (LDS), then ONE atomicMax / atomicAdd per workgroup
// and quantity into the problem's accumulator.  Non-negative doubles order as their unsigned 64-bit patterns, so the
// maxima are integer atomicMax on the bits and do not depend on the order of arrival.  The entry that attains the
// maximum cannot ride on that atomic: workgroup i of every launch keeps the best entry it has seen in slot i (the
// launches are stream-ordered, so the slot has one writer at a time) and the host takes the best of the slots; ties go
// to the smaller (row, variable), so the answer does not depend on how the entries were grouped.
// Plain C++ and vector atomics only.  Its own stream and buffers, allocated in the call and freed before it returns.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gradcheck.h"
#include "gradcheck_plan.h"

void dlg_set_error(const char* fmt, ...);

#define GMSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)

namespace {

constexpr int GC_BLOCK = 256;            // threads of a compare workgroup (4 wavefronts)
constexpr int GC_MAX_SLOTS = 1024;       // workgroups of a sparse compare launch (grid-stride beyond)

struct GcAcc                             // one per problem
{
  unsigned long long max_err, max_rel;   // bit patterns of non-negative doubles
  long long nchecked, nbad, nnonfinite, noutside;
};
struct GcCand { double err, rep, obs; int var, meas; };     // meas < 0: nothing yet
struct GcPrm
{
  double delta, rtol, atol;
  unsigned long long max_bad;
  GcAcc* acc; GcCand* cand; unsigned long long* bad_count; dogleg_amd_jacobian_entry_t* bad; double* var_error;
};

__device__ inline bool cand_better(double e, int m, int v, double e2, int m2, int v2)
{
  if(m < 0) return false;
  if(m2 < 0) return true;
  if(e != e2) return e > e2;
  return m != m2 ? m < m2 : v < v2;
}

// what a lane has seen
struct GcLane
{
  double merr, mrel;
  long long nchk, nbad, nnf;
  GcCand best;
};
__device__ inline GcLane lane_start() { return {0.0, 0.0, 0, 0, 0, {-1.0, 0.0, 0.0, -1, -1}}; }

// one entry: reported, observed and what follows from them.  Returns the finite err (0 for a non-finite entry)
__device__ inline double gc_entry(GcLane& L, const GcPrm& P, int problem, int v, int r, double j0, double j1, double a, double b)
{
  const double obs = (b - a)/P.delta;
  const double rep = (j0 + j1)/2.0;
  L.nchk++;
  bool isbad;
  double err = 0.0;
  if(!(isfinite(rep) && isfinite(obs))) { L.nnf++; isbad = true; }
  else
  {
    const double sum = fabs(rep) + fabs(obs);
    err = fabs(rep - obs);
    const double rel = sum == 0.0 ? 0.0 : err/(sum/2.0);
    L.merr = fmax(L.merr, err); L.mrel = fmax(L.mrel, rel);
    isbad = err > P.atol + P.rtol*(sum/2.0);
    if(cand_better(err, r, v, L.best.err, L.best.meas, L.best.var)) L.best = {err, rep, obs, v, r};
  }
  if(isbad)
  {
    L.nbad++;
    const unsigned long long pos = atomicAdd(P.bad_count, 1ull);
    if(pos < P.max_bad) P.bad[pos] = {problem, v, r, rep, obs};
  }
  return err;
}

// lanes -> wave -> workgroup -> one atomic per quantity into acc, and the workgroup's slot.  Every thread of the
// workgroup calls it.
__device__ inline void gc_commit(GcLane L, GcAcc* acc, GcCand* slot)
{
  __shared__ GcLane s[GC_BLOCK/64];
  for(int d = 32; d > 0; d >>= 1)
  {
    L.merr = fmax(L.merr, __shfl_down(L.merr, d, 64)); L.mrel = fmax(L.mrel, __shfl_down(L.mrel, d, 64));
    L.nchk += __shfl_down(L.nchk, d, 64); L.nbad += __shfl_down(L.nbad, d, 64); L.nnf += __shfl_down(L.nnf, d, 64);
    GcCand o;
    o.err = __shfl_down(L.best.err, d, 64); o.rep = __shfl_down(L.best.rep, d, 64); o.obs = __shfl_down(L.best.obs, d, 64);
    o.var = __shfl_down(L.best.var, d, 64); o.meas = __shfl_down(L.best.meas, d, 64);
    if(cand_better(o.err, o.meas, o.var, L.best.err, L.best.meas, L.best.var)) L.best = o;
  }
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if((threadIdx.x & 63) == 0) s[w] = L;
  __syncthreads();
  if(threadIdx.x != 0) return;
  for(int k = 1; k < nw; k++)
  {
    const GcLane& o = s[k];
    L.merr = fmax(L.merr, o.merr); L.mrel = fmax(L.mrel, o.mrel);
    L.nchk += o.nchk; L.nbad += o.nbad; L.nnf += o.nnf;
    if(cand_better(o.best.err, o.best.meas, o.best.var, L.best.err, L.best.meas, L.best.var)) L.best = o.best;
  }
  if(L.merr > 0.0) atomicMax(&acc->max_err, (unsigned long long)__double_as_longlong(L.merr));
  if(L.mrel > 0.0) atomicMax(&acc->max_rel, (unsigned long long)__double_as_longlong(L.mrel));
  if(L.nchk) atomicAdd((unsigned long long*)&acc->nchecked, (unsigned long long)L.nchk);
  if(L.nbad) atomicAdd((unsigned long long*)&acc->nbad, (unsigned long long)L.nbad);
  if(L.nnf) atomicAdd((unsigned long long*)&acc->nnonfinite, (unsigned long long)L.nnf);
  const GcCand cur = *slot;
  if(cand_better(L.best.err, L.best.meas, L.best.var, cur.err, cur.meas, cur.var)) *slot = L.best;
}

__global__ void __launch_bounds__(256) k_gc_init(unsigned long long* words, size_t nwords, GcCand* cand, size_t ncand)
{
  const size_t i0 = (size_t)blockIdx.x*256 + threadIdx.x, step = (size_t)gridDim.x*256;
  for(size_t i = i0; i < nwords; i += step) words[i] = 0ull;
  for(size_t i = i0; i < ncand; i += step) cand[i] = {-1.0, 0.0, 0.0, -1, -1};
}

// pm / pp = p0 -+ h on the variables of the group `cur` (colour == nullptr: the group of variable v is v), n = B * N
__global__ void __launch_bounds__(256) k_gc_perturb(size_t n, int N, const int* __restrict__ colour, int cur,
                                                    const double* __restrict__ p0, double h, double* __restrict__ pm,
                                                    double* __restrict__ pp)
{
  const size_t step = (size_t)gridDim.x*256;
  for(size_t i = (size_t)blockIdx.x*256 + threadIdx.x; i < n; i += step)
  {
    const int v = (int)(i % (size_t)N);
    const bool hit = (colour ? colour[v] : v) == cur;
    const double p = p0[i];
    pm[i] = hit ? p - h : p;
    pp[i] = hit ? p + h : p;
  }
}

// the n entries of one colour, sorted by (variable, row).  The workgroup's trip count is uniform: the shuffles of the
// per-variable reduction see whole waves.
__global__ void __launch_bounds__(GC_BLOCK) k_gc_compare_sparse(int n, const int* __restrict__ ent_t, const int* __restrict__ ent_r,
                                                                const int* __restrict__ ent_v, const double* __restrict__ x0,
                                                                const double* __restrict__ x1, const double* __restrict__ J0,
                                                                const double* __restrict__ J1, GcPrm P)
{
  GcLane L = lane_start();
  const int lane = threadIdx.x & 63;
  for(int base = blockIdx.x*GC_BLOCK; base < n; base += gridDim.x*GC_BLOCK)
  {
    const int e = base + threadIdx.x;
    int v = -1;
    double err = 0.0;
    if(e < n)
    {
      const int t = ent_t[e], r = ent_r[e];
      v = ent_v[e];
      err = gc_entry(L, P, 0, v, r, J0[t], J1[t], x0[r], x1[r]);
    }
    if(P.var_error)
    {
      // the lanes of one variable are neighbours: the first of each run collects the run's maximum
      for(int d = 1; d < 64; d <<= 1)
      {
        const double oe = __shfl_down(err, d, 64);
        const int ov = __shfl_down(v, d, 64);
        if(lane + d < 64 && ov == v) err = fmax(err, oe);
      }
      const int pv = __shfl_up(v, 1, 64);
      if(v >= 0 && (lane == 0 || pv != v) && err > 0.0)
        atomicMax((unsigned long long*)&P.var_error[v], (unsigned long long)__double_as_longlong(err));
    }
  }
  gc_commit(L, P.acc, P.cand + blockIdx.x);
}

// the rows of a group that hold none of its variables: x must be the same on both sides
__global__ void __launch_bounds__(256) k_gc_outside(int n, const int* __restrict__ out_r, int group, const double* __restrict__ x0,
                                                    const double* __restrict__ x1, GcPrm P)
{
  for(int i = blockIdx.x*256 + threadIdx.x; i < n; i += gridDim.x*256)
  {
    const int r = out_r[i];
    const double a = x0[r], b = x1[r];
    if(b != a)
    {
      atomicAdd((unsigned long long*)&P.acc->noutside, 1ull);
      const unsigned long long pos = atomicAdd(P.bad_count, 1ull);
      if(pos < P.max_bad) P.bad[pos] = {0, -1 - group, r, 0.0, (b - a)/P.delta};
    }
  }
}

// column v of B dense problems: workgroup = (problem, chunk of rows), one thread per row
__global__ void __launch_bounds__(GC_BLOCK) k_gc_compare_dense(int M, int N, int v, int chunks, const double* __restrict__ x0,
                                                               const double* __restrict__ x1, const double* __restrict__ J0,
                                                               const double* __restrict__ J1, GcPrm P)
{
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b*chunks;
  GcLane L = lane_start();
  for(int r = chunk*blockDim.x + threadIdx.x; r < M; r += chunks*blockDim.x)
  {
    const size_t row = (size_t)b*M + r, k = row*N + v;
    gc_entry(L, P, b, v, r, J0[k], J1[k], x0[row], x1[row]);
  }
  GcAcc* acc = P.acc + b;
  const double colmax = L.merr;
  gc_commit(L, acc, P.cand + blockIdx.x);
  if(P.var_error)
  {
    // (single problem only) the column is one variable: the wave's maximum, one atomic per wave
    double m = colmax;
    for(int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d, 64));
    if((threadIdx.x & 63) == 0 && m > 0.0)
      atomicMax((unsigned long long*)&P.var_error[v], (unsigned long long)__double_as_longlong(m));
  }
}

// dogleg_amd_testGradient_device: reported and observed of variable var in every row
__global__ void __launch_bounds__(256) k_gc_table(int M, int N, int var, const int* __restrict__ colptr,
                                                  const int* __restrict__ rowidx, const double* __restrict__ x0,
                                                  const double* __restrict__ x1, const double* __restrict__ J0,
                                                  const double* __restrict__ J1, double delta, double* __restrict__ out)
{
  const int r = blockIdx.x*256 + threadIdx.x;
  if(r >= M) return;
  double j0 = 0.0, j1 = 0.0;                   // an entry that is not declared is 0 (dogleg.c:353-367)
  if(colptr)
  {
    for(int t = colptr[r]; t < colptr[r + 1]; t++)
      if(rowidx[t] == var) { j0 = J0[t]; j1 = J1[t]; break; }
  }
  else { j0 = J0[(size_t)r*N + var]; j1 = J1[(size_t)r*N + var]; }
  out[2*(size_t)r] = (j0 + j1)/2.0;
  out[2*(size_t)r + 1] = (x1[r] - x0[r])/delta;
}

// callback calls, launches, synchronisations, copies; with DOGLEG_AMD_CHECK_TIMING=1 (single problem): ms in the callback's
// kernels, ms in the library's
thread_local double t_stats[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// the device side of one call: the stream and the one allocation, given back when it goes out of scope
struct GcDevice
{
  hipStream_t stream = nullptr;
  char* mem = nullptr;
  std::vector<hipEvent_t> events;                // timing only: three per group
  ~GcDevice()
  {
    for(hipEvent_t e : events) (void)hipEventDestroy(e);
    if(mem) (void)hipFree(mem);
    if(stream) (void)hipStreamDestroy(stream);
  }
};

#define GHIP(call) \
  do { hipError_t e__ = (call); \
       if(e__ != hipSuccess) { dlg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
                               GMSG("%s: %s -> %s", who, #call, hipGetErrorString(e__)); (void)hipGetLastError(); return -1; } } while(0)

// the carve-up of the allocation
struct GcLayout
{
  size_t Xn = 0, Jn = 0, Pn = 0;                 // doubles of one x, one J, one p
  size_t nint = 0;                               // ints of the plan
  size_t nlive = 0, nacc = 0, ncand = 0, nvar = 0, nbad = 0;
  size_t o_x0, o_x1, o_J0, o_J1, o_p0, o_pm, o_pp, o_int, o_live, o_res, o_count, o_var, o_cand, o_bad, total;
  void finish()
  {
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    o_x0 = take(8*Xn); o_x1 = take(8*Xn); o_J0 = take(8*Jn); o_J1 = take(8*Jn);
    o_p0 = take(8*Pn); o_pm = take(8*Pn); o_pp = take(8*Pn);
    o_int = take(4*nint); o_live = take(nlive);
    o_res = take(sizeof(GcAcc)*nacc); o_count = take(8); o_var = take(8*nvar);
    o_cand = take(sizeof(GcCand)*ncand); o_bad = take(sizeof(dogleg_amd_jacobian_entry_t)*nbad);
    total = o;
  }
  size_t res_bytes() const { return total - o_res; }
  size_t zero_words() const { return (o_cand - o_res)/8; }       // accumulators, the counter, var_error
};

int open_device(const char* who, const char* what, GcDevice& D, const GcLayout& Y)
{
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    (void)hipGetLastError();
    dlg_set_error("%s: no HIP device", who); GMSG("%s: no HIP device (there is no CPU fallback)", who);
    return -1;
  }
  GHIP(hipStreamCreateWithFlags(&D.stream, hipStreamNonBlocking));
  if(hipMalloc((void**)&D.mem, Y.total) != hipSuccess)
  {
    (void)hipGetLastError(); D.mem = nullptr;
    dlg_set_error("%s: cannot allocate %zu bytes of device memory", who, Y.total);
    GMSG("%s: %s needs %zu bytes of device memory: the allocation failed", who, what, Y.total);
    return -1;
  }
  return 0;
}

// refused from the sizes alone, before any device work
bool too_large(const char* who, const char* what, double bytes)
{
  if(bytes <= 1.0e15) return false;
  dlg_set_error("%s: %.3g bytes of device memory", who, bytes);
  GMSG("%s: %s needs %.3g bytes of device memory", who, what, bytes);
  return true;
}

GcPrm make_prm(const GcDevice& D, const GcLayout& Y, double delta, double rtol, double atol)
{
  GcPrm P;
  P.delta = delta; P.rtol = rtol; P.atol = atol; P.max_bad = Y.nbad;
  P.acc = (GcAcc*)(D.mem + Y.o_res); P.cand = (GcCand*)(D.mem + Y.o_cand);
  P.bad_count = (unsigned long long*)(D.mem + Y.o_count);
  P.bad = (dogleg_amd_jacobian_entry_t*)(D.mem + Y.o_bad);
  P.var_error = Y.nvar ? (double*)(D.mem + Y.o_var) : nullptr;
  return P;
}

unsigned int blocks_for(size_t n, unsigned int per, unsigned int cap)
{
  const size_t b = (n + per - 1)/per;
  return (unsigned int)std::min<size_t>(std::max<size_t>(b, 1), cap);
}

double bits_to_double(unsigned long long u) { double d; memcpy(&d, &u, sizeof(d)); return d; }

// accumulator + slots of one problem -> its report
void fill_report(dogleg_amd_jacobian_report_t& R, const GcAcc& A, const GcCand* cand, size_t ncand, int ncolours)
{
  R.nchecked = A.nchecked; R.nbad = A.nbad; R.nnonfinite = A.nnonfinite; R.noutside = A.noutside;
  R.max_error = bits_to_double(A.max_err); R.max_error_relative = bits_to_double(A.max_rel);
  GcCand best = {-1.0, 0.0, 0.0, -1, -1};
  for(size_t k = 0; k < ncand; k++)
  {
    const GcCand& c = cand[k];
    if(c.meas < 0) continue;
    if(best.meas < 0 || c.err > best.err || (c.err == best.err && (c.meas != best.meas ? c.meas < best.meas : c.var < best.var)))
      best = c;
  }
  R.worst_var = best.var; R.worst_meas = best.meas; R.worst_reported = best.rep; R.worst_observed = best.obs;
  R.ncolours = ncolours; R.evaluations = 2*ncolours;
}

// the records the device appended, sorted by (problem, meas, var), into the caller's array
long long take_bad(const char* res, const GcLayout& Y, dogleg_amd_jacobian_entry_t* bad)
{
  unsigned long long count = 0;
  memcpy(&count, res + (Y.o_count - Y.o_res), sizeof(count));
  const size_t n = (size_t)std::min<unsigned long long>(count, Y.nbad);
  if(n == 0) return 0;
  memcpy(bad, res + (Y.o_bad - Y.o_res), sizeof(dogleg_amd_jacobian_entry_t)*n);
  std::sort(bad, bad + n, [](const dogleg_amd_jacobian_entry_t& a, const dogleg_amd_jacobian_entry_t& b) {
    if(a.problem != b.problem) return a.problem < b.problem;
    if(a.meas != b.meas) return a.meas < b.meas;
    return a.var < b.var; });
  return (long long)n;
}

} // namespace

int dlg_gradcheck_run(const double* p0, unsigned int N, unsigned int M, unsigned int nnz, const int* colptr,
                      const int* rowidx, dogleg_callback_device_t* f, void* cookie, double delta, double rtol, double atol,
                      int flags, dogleg_amd_jacobian_report_t* report, double* var_error,
                      dogleg_amd_jacobian_entry_t* bad, int max_bad)
{
  const char* who = "dogleg_amd_check_jacobian_device";
  double* const ts = t_stats;
  for(int k = 0; k < 6; k++) ts[k] = 0.0;
  const bool sparse = nnz > 0;
  char what[128], err[512];
  snprintf(what, sizeof(what), "a %u x %u problem with %u Jacobian entries", M, N, nnz);
  GradcheckPlan plan;
  if(sparse && gradcheck_plan(plan, (int)N, (int)M, colptr, rowidx, (flags & DOGLEG_AMD_JACOBIAN_ONE_AT_A_TIME) != 0, err, sizeof(err)))
  { dlg_set_error("%s: %s", who, err); GMSG("%s: %s", who, err); return -1; }
  const int ncolours = sparse ? plan.ncolours : (int)N;

  GcLayout Y;
  Y.Xn = M; Y.Jn = sparse ? (size_t)nnz : (size_t)M*N; Y.Pn = N;
  Y.nint = sparse ? (size_t)N + 3*(size_t)nnz + plan.out_r.size() : 0;
  Y.nacc = 1; Y.nvar = var_error ? N : 0; Y.nbad = (bad && max_bad > 0) ? (size_t)max_bad : 0;
  // dense: (problem, chunk) workgroups of GC_BLOCK rows; sparse: up to GC_MAX_SLOTS workgroups a launch
  const int chunks = (int)blocks_for(M, GC_BLOCK, GC_MAX_SLOTS);
  Y.ncand = sparse ? blocks_for((size_t)plan.max_entries, GC_BLOCK, GC_MAX_SLOTS) : (size_t)chunks;
  if(too_large(who, what, 16.0*M + 16.0*(sparse ? (double)nnz : (double)M*N) + 24.0*N + 4.0*Y.nint + 32.0*Y.nbad)) return -1;
  Y.finish();

  GcDevice D;
  if(open_device(who, what, D, Y)) return -1;
  hipStream_t st = D.stream;
  char* d = D.mem;
  double *x0 = (double*)(d + Y.o_x0), *x1 = (double*)(d + Y.o_x1), *J0 = (double*)(d + Y.o_J0), *J1 = (double*)(d + Y.o_J1);
  double *dp0 = (double*)(d + Y.o_p0), *pm = (double*)(d + Y.o_pm), *pp = (double*)(d + Y.o_pp);
  int* d_colour = (int*)(d + Y.o_int);
  int *d_t = d_colour + N, *d_r = d_t + nnz, *d_v = d_r + nnz, *d_out = d_v + nnz;
  const GcPrm P = make_prm(D, Y, delta, rtol, atol);
  // measurement: events before a group's callbacks, behind them and behind its compare kernels, read after the one
  // synchronisation
  const bool timing = getenv("DOGLEG_AMD_CHECK_TIMING") != nullptr;
  if(timing)
    for(int k = 0; k < 3*ncolours; k++)
    {
      hipEvent_t e = nullptr;
      GHIP(hipEventCreate(&e));
      D.events.push_back(e);
    }

  GHIP(hipMemcpyAsync(dp0, p0, sizeof(double)*N, hipMemcpyHostToDevice, st)); ts[3] += 1.0;
  std::vector<int> ints;
  if(sparse)
  {
    ints.reserve(Y.nint);
    ints.insert(ints.end(), plan.colour.begin(), plan.colour.end());
    ints.insert(ints.end(), plan.ent_t.begin(), plan.ent_t.end());
    ints.insert(ints.end(), plan.ent_r.begin(), plan.ent_r.end());
    ints.insert(ints.end(), plan.ent_v.begin(), plan.ent_v.end());
    ints.insert(ints.end(), plan.out_r.begin(), plan.out_r.end());
    GHIP(hipMemcpyAsync(d_colour, ints.data(), sizeof(int)*ints.size(), hipMemcpyHostToDevice, st)); ts[3] += 1.0;
  }
  hipLaunchKernelGGL(k_gc_init, dim3(blocks_for(Y.zero_words() + Y.ncand, 256, 1024)), dim3(256), 0, st,
                     (unsigned long long*)(d + Y.o_res), Y.zero_words(), P.cand, Y.ncand);
  GHIP(hipGetLastError()); ts[1] += 1.0;
  for(int c = 0; c < ncolours; c++)
  {
    hipLaunchKernelGGL(k_gc_perturb, dim3(blocks_for(N, 256, 1024)), dim3(256), 0, st, (size_t)N, (int)N,
                       sparse ? d_colour : (const int*)nullptr, c, dp0, delta/2.0, pm, pp);
    GHIP(hipGetLastError()); ts[1] += 1.0;
    if(timing) GHIP(hipEventRecord(D.events[3*(size_t)c], st));
    f(pm, x0, J0, (void*)st, cookie); ts[0] += 1.0;
    f(pp, x1, J1, (void*)st, cookie); ts[0] += 1.0;
    if(timing) GHIP(hipEventRecord(D.events[3*(size_t)c + 1], st));
    if(sparse)
    {
      const int e0 = plan.ent_ptr[c], ne = plan.ent_ptr[(size_t)c + 1] - e0;
      if(ne > 0)
      {
        hipLaunchKernelGGL(k_gc_compare_sparse, dim3(blocks_for(ne, GC_BLOCK, (unsigned int)Y.ncand)), dim3(GC_BLOCK), 0, st,
                           ne, d_t + e0, d_r + e0, d_v + e0, x0, x1, J0, J1, P);
        GHIP(hipGetLastError()); ts[1] += 1.0;
      }
      const int o0 = plan.out_ptr[c], no = plan.out_ptr[(size_t)c + 1] - o0;
      if(no > 0)
      {
        hipLaunchKernelGGL(k_gc_outside, dim3(blocks_for(no, 256, 1024)), dim3(256), 0, st, no, d_out + o0, c, x0, x1, P);
        GHIP(hipGetLastError()); ts[1] += 1.0;
      }
    }
    else
    {
      hipLaunchKernelGGL(k_gc_compare_dense, dim3(chunks), dim3(GC_BLOCK), 0, st, (int)M, (int)N, c, chunks, x0, x1, J0, J1, P);
      GHIP(hipGetLastError()); ts[1] += 1.0;
    }
    if(timing) GHIP(hipEventRecord(D.events[3*(size_t)c + 2], st));
  }
  std::vector<char> res(Y.res_bytes());
  GHIP(hipMemcpyAsync(res.data(), d + Y.o_res, res.size(), hipMemcpyDeviceToHost, st)); ts[3] += 1.0;
  GHIP(hipStreamSynchronize(st)); ts[2] += 1.0;
  if(timing)
    for(int c = 0; c < ncolours; c++)
    {
      float a = 0.f, b = 0.f;
      GHIP(hipEventElapsedTime(&a, D.events[3*(size_t)c], D.events[3*(size_t)c + 1]));
      GHIP(hipEventElapsedTime(&b, D.events[3*(size_t)c + 1], D.events[3*(size_t)c + 2]));
      ts[4] += a; ts[5] += b;
    }

  GcAcc A;
  memcpy(&A, res.data(), sizeof(A));
  fill_report(*report, A, (const GcCand*)(res.data() + (Y.o_cand - Y.o_res)), Y.ncand, ncolours);
  if(var_error) memcpy(var_error, res.data() + (Y.o_var - Y.o_res), sizeof(double)*N);
  return (int)take_bad(res.data(), Y, bad);
}

int dlg_gradcheck_batch_run(const double* p0, unsigned int B, unsigned int N, unsigned int M,
                            dogleg_callback_device_batch_t* f, void* cookie, double delta, double rtol, double atol,
                            dogleg_amd_jacobian_report_t* reports, dogleg_amd_jacobian_entry_t* bad, int max_bad,
                            long long* nbad_total)
{
  const char* who = "dogleg_amd_check_jacobian_device_batch";
  double* const ts = t_stats;
  for(int k = 0; k < 6; k++) ts[k] = 0.0;
  char what[128];
  snprintf(what, sizeof(what), "B = %u problems of %u x %u", B, M, N);
  GcLayout Y;
  Y.Xn = (size_t)B*M; Y.Jn = (size_t)B*M*N; Y.Pn = (size_t)B*N; Y.nlive = B;
  const int chunks = (int)blocks_for(M, GC_BLOCK, 64);
  Y.nacc = B; Y.ncand = (size_t)B*chunks; Y.nbad = (bad && max_bad > 0) ? (size_t)max_bad : 0;
  if(too_large(who, what, 16.0*B*(double)M*((double)N + 1.0) + 24.0*B*(double)N + (double)B*(1.0 + 48.0 + 32.0*chunks) + 32.0*Y.nbad))
    return -1;
  if((double)B*chunks > 2147483647.0)
  { GMSG("%s: %s: beyond the index range of the compare kernel", who, what); return -1; }
  Y.finish();

  GcDevice D;
  if(open_device(who, what, D, Y)) return -1;
  hipStream_t st = D.stream;
  char* d = D.mem;
  double *x0 = (double*)(d + Y.o_x0), *x1 = (double*)(d + Y.o_x1), *J0 = (double*)(d + Y.o_J0), *J1 = (double*)(d + Y.o_J1);
  double *dp0 = (double*)(d + Y.o_p0), *pm = (double*)(d + Y.o_pm), *pp = (double*)(d + Y.o_pp);
  unsigned char* live = (unsigned char*)(d + Y.o_live);
  const GcPrm P = make_prm(D, Y, delta, rtol, atol);
  // rows of a workgroup: whole waves, no more than the problem has
  const int block = std::min(GC_BLOCK, (int)((M + 63)/64)*64);

  GHIP(hipMemcpyAsync(dp0, p0, sizeof(double)*Y.Pn, hipMemcpyHostToDevice, st)); ts[3] += 1.0;
  GHIP(hipMemsetAsync(live, 1, B, st)); ts[3] += 1.0;
  hipLaunchKernelGGL(k_gc_init, dim3(blocks_for(Y.zero_words() + Y.ncand, 256, 1024)), dim3(256), 0, st,
                     (unsigned long long*)(d + Y.o_res), Y.zero_words(), P.cand, Y.ncand);
  GHIP(hipGetLastError()); ts[1] += 1.0;
  for(unsigned int v = 0; v < N; v++)
  {
    hipLaunchKernelGGL(k_gc_perturb, dim3(blocks_for(Y.Pn, 256, 4096)), dim3(256), 0, st, Y.Pn, (int)N, (const int*)nullptr,
                       (int)v, dp0, delta/2.0, pm, pp);
    GHIP(hipGetLastError()); ts[1] += 1.0;
    f(pm, x0, J0, live, B, (void*)st, cookie); ts[0] += 1.0;
    f(pp, x1, J1, live, B, (void*)st, cookie); ts[0] += 1.0;
    hipLaunchKernelGGL(k_gc_compare_dense, dim3((unsigned int)((size_t)B*chunks)), dim3(block), 0, st, (int)M, (int)N, (int)v,
                       chunks, x0, x1, J0, J1, P);
    GHIP(hipGetLastError()); ts[1] += 1.0;
  }
  std::vector<char> res(Y.res_bytes());
  GHIP(hipMemcpyAsync(res.data(), d + Y.o_res, res.size(), hipMemcpyDeviceToHost, st)); ts[3] += 1.0;
  GHIP(hipStreamSynchronize(st)); ts[2] += 1.0;

  const GcCand* cand = (const GcCand*)(res.data() + (Y.o_cand - Y.o_res));
  for(size_t b = 0; b < B; b++)
  {
    GcAcc A;
    memcpy(&A, res.data() + sizeof(GcAcc)*b, sizeof(A));
    fill_report(reports[b], A, cand + b*chunks, (size_t)chunks, (int)N);
  }
  const long long n = take_bad(res.data(), Y, bad);
  if(nbad_total) *nbad_total = n;
  return 0;
}

int dlg_gradcheck_table(unsigned int var, const double* p0, unsigned int N, unsigned int M, unsigned int nnz,
                        const int* colptr, const int* rowidx, dogleg_callback_device_t* f, void* cookie, double delta,
                        double* table)
{
  const char* who = "dogleg_amd_testGradient_device";
  double* const ts = t_stats;
  for(int k = 0; k < 6; k++) ts[k] = 0.0;
  const bool sparse = nnz > 0;
  char what[128];
  snprintf(what, sizeof(what), "a %u x %u problem with %u Jacobian entries", M, N, nnz);
  GcLayout Y;
  Y.Xn = M; Y.Jn = sparse ? (size_t)nnz : (size_t)M*N; Y.Pn = N;
  Y.nint = sparse ? (size_t)M + 1 + nnz : 0;
  Y.nvar = 2*(size_t)M;                           // the table sits where var_error would
  if(too_large(who, what, 32.0*M + 16.0*(sparse ? (double)nnz : (double)M*N) + 24.0*N + 4.0*Y.nint)) return -1;
  Y.finish();
  GcDevice D;
  if(open_device(who, what, D, Y)) return -1;
  hipStream_t st = D.stream;
  char* d = D.mem;
  double *x0 = (double*)(d + Y.o_x0), *x1 = (double*)(d + Y.o_x1), *J0 = (double*)(d + Y.o_J0), *J1 = (double*)(d + Y.o_J1);
  double *dp0 = (double*)(d + Y.o_p0), *pm = (double*)(d + Y.o_pm), *pp = (double*)(d + Y.o_pp);
  int* d_cp = (int*)(d + Y.o_int);
  int* d_ri = d_cp + M + 1;
  double* d_table = (double*)(d + Y.o_var);
  GHIP(hipMemcpyAsync(dp0, p0, sizeof(double)*N, hipMemcpyHostToDevice, st)); ts[3] += 1.0;
  if(sparse)
  {
    GHIP(hipMemcpyAsync(d_cp, colptr, sizeof(int)*((size_t)M + 1), hipMemcpyHostToDevice, st)); ts[3] += 1.0;
    GHIP(hipMemcpyAsync(d_ri, rowidx, sizeof(int)*(size_t)nnz, hipMemcpyHostToDevice, st)); ts[3] += 1.0;
  }
  hipLaunchKernelGGL(k_gc_perturb, dim3(blocks_for(N, 256, 1024)), dim3(256), 0, st, (size_t)N, (int)N, (const int*)nullptr,
                     (int)var, dp0, delta/2.0, pm, pp);
  GHIP(hipGetLastError()); ts[1] += 1.0;
  f(pm, x0, J0, (void*)st, cookie); ts[0] += 1.0;
  f(pp, x1, J1, (void*)st, cookie); ts[0] += 1.0;
  hipLaunchKernelGGL(k_gc_table, dim3((M + 255)/256), dim3(256), 0, st, (int)M, (int)N, (int)var,
                     sparse ? d_cp : (const int*)nullptr, sparse ? d_ri : (const int*)nullptr, x0, x1, J0, J1, delta, d_table);
  GHIP(hipGetLastError()); ts[1] += 1.0;
  GHIP(hipMemcpyAsync(table, d_table, sizeof(double)*2*(size_t)M, hipMemcpyDeviceToHost, st)); ts[3] += 1.0;
  GHIP(hipStreamSynchronize(st)); ts[2] += 1.0;
  return 0;
}

int dlg_gradcheck_last_stats(double* out, int n)
{
  int k = 0;
  for(; k < n && k < 6; k++) out[k] = t_stats[k];
  return k;
}
