// robust_prelude.hip -- a loss function on a device solve (dogleg.h: dogleg_amd_optimize_device2_robust).  Directly behind the
// user's callback, on the backend's stream, the prelude turns the callback's (x, J) into the weighted rows the plain solve then
// works on, and leaves F = sum_f rho(s_f) where the driver reads it:
//   k_robust_weights   a thread a feature: s_f from up to 4 rows of x in row order, rho and w = rho', w_f to the slot's weight
//                      array, the feature's rows of x times sqrt(w_f), the workgroup's sum of rho in a fixed order
//   k_robust_scale_*   J in place, flat over its entries, 16 bytes a lane where the address allows: row r times sqrt(w_{r / fs});
//                      its workgroup 0 first adds the partial sums of the launch before in a fixed order -> F of the slot (no
//                      atomics: the same bits every run; a launch of its own for that cost 5 us, as much as the weights of
//                      config #3)
//                      sparse: a workgroup takes ROWS consecutive rows, stages their colptr and sqrt(w) in LDS and walks the
//                              contiguous entry span of the chunk; a lane finds its entry's row by bisection in the staged colptr
//                      dense:  the row of entry e is e / Nstate, one division a lane, then carried along
// followed by an 8-byte copy of F to page-locked memory and an event.  The sparse pass reads the colptr of THIS solve, which
// robust_set_up uploads: a backend taken over from the previous solve may still hold another pattern of the same shape while the
// first evaluation runs (driver.hip: start_pattern_check), and J must never be scaled with that one's row boundaries.
// F on the host: robust_F waits for the event recorded behind the copy of that slot's last prelude.  The wait is explicit rather
// than argued from dlg_point_eval's stream order, which moves work to a second stream on some schedules: by the time the driver
// asks, dlg_point_eval has waited for work enqueued behind the copy, so the event is long complete and the wait costs nothing.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>
#include "driver_internal.h"

namespace {

constexpr int TPB = 256;           // threads a workgroup, every kernel
constexpr int ROWS = 256;          // sparse: rows a workgroup stages
constexpr int DENSE_ITERS = 8;     // dense: pairs a lane (a workgroup covers 2 TPB DENSE_ITERS = 4096 entries)

struct LossDev { int kind, fs; double a, c; };

// rho(s) and w = rho'(s): the second copy of loss_eval in dense_batch_kernels.hip (kept apart so that the batch kernels' code
// does not change); tests/batch_robust_oracle.py Loss.rho_w, soft-L1 in its cancellation-free form
__device__ __forceinline__ void loss_eval(const LossDev& L, double s, double& rho, double& w)
{
  const double q = s/L.c;
  switch(L.kind)
  {
  case DOGLEG_AMD_LOSS_HUBER:
    if(s <= L.c) { rho = s; w = 1.0; }
    else { const double r = sqrt(s); rho = 2.0*L.a*r - L.c; w = L.a/r; }
    break;
  case DOGLEG_AMD_LOSS_SOFT_L1:
  {
    const double r = sqrt(1.0 + q);
    rho = 2.0*s/(r + 1.0); w = 1.0/r;
    break;
  }
  case DOGLEG_AMD_LOSS_CAUCHY:
    rho = L.c*log1p(q); w = 1.0/(1.0 + q);
    break;
  default:
    rho = s; w = 1.0;
  }
}

// the workgroup's sum of v in a fixed order (a tree over the thread index); valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red)
{
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for(int h = TPB/2; h > 0; h >>= 1)
  {
    if(t < h) red[t] = red[t] + red[t + h];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(TPB) k_robust_weights(double* __restrict__ x, int nfeat, LossDev L, double* __restrict__ w,
                                                        double* __restrict__ partial)
{
#pragma clang fp contract(off)
  __shared__ double red[TPB];
  const int f = blockIdx.x*TPB + threadIdx.x;
  double rho = 0.0;
  if(f < nfeat)
  {
    double* xf = x + (size_t)f*L.fs;
    double xv[DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE];
    double s = 0.0;
#pragma unroll
    for(int k = 0; k < DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE; k++)
      if(k < L.fs) { xv[k] = xf[k]; const double q = xv[k]*xv[k]; s = k == 0 ? q : s + q; }
    double wf;
    loss_eval(L, s, rho, wf);
    w[f] = wf;
    const double sq = sqrt(wf);
#pragma unroll
    for(int k = 0; k < DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE; k++)
      if(k < L.fs) xf[k] = xv[k]*sq;
  }
  const double sum = block_sum(rho, red);
  if(threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// F = the partial sums of k_robust_weights in a fixed order: every thread its stride, then the tree.  One workgroup (the first
// of the pass over J, which runs behind k_robust_weights on the stream: the partial sums are complete).
__device__ __forceinline__ void sum_partials(const double* __restrict__ partial, int n, double* __restrict__ F)
{
  __shared__ double red[TPB];
  double v = 0.0;
  for(int i = threadIdx.x; i < n; i += TPB) v += partial[i];
  const double sum = block_sum(v, red);
  if(threadIdx.x == 0) F[0] = sum;
}

// q[0], q[1] *= s0, s1 with q on a 16-byte boundary
__device__ __forceinline__ void scale_pair(double* q, double s0, double s1)
{
  double2 v = *reinterpret_cast<double2*>(q);
  v.x *= s0; v.y *= s1;
  *reinterpret_cast<double2*>(q) = v;
}

// colptr: [M + 1], non-decreasing from 0 to nnz (checked on the host; every value is clamped into [0, nnz] here all the same)
__global__ void __launch_bounds__(TPB) k_robust_scale_sparse(double* __restrict__ J, const int* __restrict__ colptr, const double* __restrict__ w,
                                                             int M, int nfeat, int fs, int nnz,
                                                             const double* __restrict__ partial, int npartial, double* __restrict__ F)
{
  if(blockIdx.x == 0) sum_partials(partial, npartial, F);
  __shared__ int cp_s[ROWS + 1];
  __shared__ double sq_s[ROWS];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x*ROWS;
  const int nr = min(ROWS, M - r0);
  if(nr <= 0) return;
  for(int i = t; i <= nr; i += TPB) cp_s[i] = min(max(colptr[r0 + i], 0), nnz);
  if(t < nr) sq_s[t] = sqrt(w[min((r0 + t)/fs, nfeat - 1)]);
  __syncthreads();
  const long long e0 = cp_s[0], e1 = cp_s[nr];
  if(e1 <= e0) return;
  // the row of entry e, e0 <= e < e1: the first r with cp_s[r + 1] > e (rows that end at or before e, empty ones among them, are passed)
  // The bisection starts from a guess, the row the entry would lie in if all rows of the chunk had the same length (bundle
  // adjustment: they have, and the guess is the row: two LDS reads in place of a chain of nine dependent ones); the guess only
  // narrows the interval, so any pattern gets its row.
  const double rows_per_entry = (double)nr/(double)(e1 - e0);
  auto row_of = [&](long long e)
  {
    int lo = 0, hi = nr - 1;
    const int g = min(nr - 1, (int)(((double)(e - e0) + 0.5)*rows_per_entry));
    if(cp_s[g + 1] <= e) lo = g + 1; else if(cp_s[g] > e) hi = g - 1; else return g;
    while(lo < hi) { const int mid = (lo + hi) >> 1; if(cp_s[mid + 1] <= e) lo = mid + 1; else hi = mid; }
    return lo;
  };
  // the first entry of the span on a 16-byte boundary; the one in front of it, if any, on its own
  const long long a = e0 + (long long)((reinterpret_cast<uintptr_t>(J + e0) >> 3) & 1);
  if(t == 0 && a > e0) J[e0] *= sq_s[row_of(e0)];
  for(long long e = a + 2*t; e < e1; e += 2*TPB)
  {
    const int r = row_of(e);
    if(e + 1 < e1) scale_pair(J + e, sq_s[r], sq_s[cp_s[r + 1] > e + 1 ? r : row_of(e + 1)]);
    else J[e] *= sq_s[r];
  }
}

// J: [M][N] row-major, total = M N entries; head: 1 if J itself is not on a 16-byte boundary (entry 0 then goes alone)
__global__ void __launch_bounds__(TPB) k_robust_scale_dense(double* __restrict__ J, const double* __restrict__ w, long long total, int N,
                                                            int nfeat, int fs, int head,
                                                            const double* __restrict__ partial, int npartial, double* __restrict__ F)
{
  if(blockIdx.x == 0) sum_partials(partial, npartial, F);
  const int t = threadIdx.x;
  if(blockIdx.x == 0 && t == 0 && head && total > 0) J[0] *= sqrt(w[0]);
  long long e = head + (long long)blockIdx.x*(2*TPB*DENSE_ITERS) + 2*t;
  if(e >= total) return;
  int row = (int)(e/N), col = (int)(e - (long long)row*N);          // (row < M: an int)
  const int qstep = (2*TPB)/N, rstep = (2*TPB)%N;
  for(int it = 0; it < DENSE_ITERS && e < total; it++)
  {
    const double s0 = sqrt(w[min(row/fs, nfeat - 1)]);
    if(e + 1 < total)
    {
      const int row1 = col + 1 == N ? row + 1 : row;
      scale_pair(J + e, s0, row1 == row ? s0 : sqrt(w[min(row1/fs, nfeat - 1)]));
    }
    else J[e] *= s0;
    e += 2*TPB; row += qstep; col += rstep;
    if(col >= N) { col -= N; row++; }
  }
}

thread_local double t_stats[3];

bool hip_ok(hipError_t e, const char* what)
{
  if(e == hipSuccess) return true;
  MSG("robust device solve: %s failed: %s", what, hipGetErrorString(e));
  (void)hipGetLastError();
  return false;
}

// Between solves the library keeps the device block of the last robust solve, as it keeps the idle backend (driver_cache.hip):
// the next robust solve of the same size on the same GPU takes it over -- hipMalloc and hipFree of it cost more than the
// preludes of a whole solve of config #3.  dogleg_amd_release_cache gives it back, DOGLEG_AMD_NO_BACKEND_CACHE never keeps it.
struct KeptBlock { void* p = nullptr; size_t bytes = 0; int device = -1; };
std::mutex g_kept_mu;
KeptBlock g_kept;

void* block_take(size_t bytes, int device)
{
  {
    std::lock_guard<std::mutex> lk(g_kept_mu);
    if(g_kept.p && g_kept.bytes == bytes && g_kept.device == device) { void* p = g_kept.p; g_kept = KeptBlock(); return p; }
  }
  return dlg_mem_alloc(bytes);
}
void block_give(void* p, size_t bytes, int device, bool keep)
{
  void* old = p;
  if(keep && cache_on())
  {
    std::lock_guard<std::mutex> lk(g_kept_mu);
    old = g_kept.p;
    g_kept.p = p; g_kept.bytes = bytes; g_kept.device = device;
  }
  if(old) dlg_mem_free(old);
}

} // namespace

void robust_release_cache()
{
  void* p = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_kept_mu);
    p = g_kept.p; g_kept = KeptBlock();
  }
  if(p) dlg_mem_free(p);
}

struct Robust
{
  LossDev L;
  int nfeat, nblk;                   // features; workgroups of k_robust_weights = partial sums
  void* block; size_t block_bytes; int device;      // ONE device allocation: the arrays below, the doubles first
  int* cp_dev;                       // sparse: this solve's Jt_colptr
  double* w_dev[2];                  // per slot: rho'(s_f)
  double* F_dev[2];                  // per slot: [0] F, [1 ..] the partial sums
  double* F_host;                    // page-locked [2]
  hipEvent_t landed[2];              // per slot: behind the copy of F of its last prelude
  int nprelude;
  std::vector<hipEvent_t> tm;        // DOGLEG_AMD_TIMING: a pair of events an evaluation
};

bool robust_loss_ok(const dogleg_amd_batch_loss_t* loss, unsigned int Nmeas, unsigned int NJnnz, const int* Jt_colptr)
{
  const char* who = "dogleg_amd_optimize_device2_robust";
  if(!loss) { MSG("%s: a NULL loss", who); return false; }
  if(loss->kind < DOGLEG_AMD_LOSS_TRIVIAL || loss->kind > DOGLEG_AMD_LOSS_CAUCHY) { MSG("%s: unknown loss kind %d", who, loss->kind); return false; }
  if(loss->kind != DOGLEG_AMD_LOSS_TRIVIAL && !(std::isfinite(loss->scale) && loss->scale > 0.0))
  { MSG("%s: the scale of the loss must be finite and > 0, got %g", who, loss->scale); return false; }
  if(loss->featureSize > DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE)
  { MSG("%s: featureSize %d above %d", who, loss->featureSize, DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE); return false; }
  const unsigned int fs = loss->featureSize <= 1 ? 1u : (unsigned int)loss->featureSize;
  if(Nmeas == 0 || Nmeas % fs != 0) { MSG("%s: Nmeas %u is not a positive multiple of featureSize %u", who, Nmeas, fs); return false; }
  if(NJnnz > 0)
  {
    // (the prelude walks the entries of J by these row boundaries)
    if(!Jt_colptr) { MSG("%s: a sparse device solve needs the pattern of Jt", who); return false; }
    // (no exit from inside the loop: a million rows then go through vector compares)
    int down = 0;
    for(unsigned int r = 0; r < Nmeas; r++) down |= Jt_colptr[r + 1] < Jt_colptr[r];
    if(down) { MSG("%s: Jt_colptr decreases somewhere; it must run from 0 to NJnnz without a step down", who); return false; }
  }
  return true;
}

Robust* robust_create(const dogleg_amd_batch_loss_t* loss)
{
  Robust* R = new (std::nothrow) Robust();
  if(!R) return nullptr;
  const bool trivial = loss->kind == DOGLEG_AMD_LOSS_TRIVIAL;
  R->L.kind = loss->kind; R->L.fs = loss->featureSize <= 1 ? 1 : loss->featureSize;
  R->L.a = trivial ? 1.0 : loss->scale; R->L.c = R->L.a*R->L.a;
  R->block = nullptr; R->block_bytes = 0; R->device = -1;
  R->cp_dev = nullptr; R->F_host = nullptr; R->nprelude = 0;
  for(int s = 0; s < 2; s++) { R->w_dev[s] = R->F_dev[s] = nullptr; R->landed[s] = nullptr; }
  return R;
}

bool robust_set_up(Driver* d)
{
  Robust* R = d->robust;
  const size_t M = (size_t)d->pub.Nmeasurements;
  R->nfeat = (int)(M/(size_t)R->L.fs);
  R->nblk = (R->nfeat + TPB - 1)/TPB;
  const bool sparse = d->pub.solve_type == DOGLEG_SPARSE;
  const size_t nw = (size_t)R->nfeat, nF = (size_t)(1 + R->nblk);
  R->block_bytes = sizeof(double)*2*(nw + nF) + (sparse ? sizeof(int)*(M + 1) : 0);
  R->device = dlg_backend_device(d->be);
  R->block = block_take(R->block_bytes, R->device);
  if(!R->block) { MSG("out of device memory"); return false; }
  double* q = (double*)R->block;
  for(int s = 0; s < 2; s++)
  {
    R->w_dev[s] = q; q += nw;
    R->F_dev[s] = q; q += nF;
    if(!hip_ok(hipEventCreateWithFlags(&R->landed[s], hipEventDisableTiming), "event creation")) return false;
  }
  // (16 page-locked bytes: from the pool of the operating points' buffers, to which robust_destroy gives them back)
  R->F_host = (double*)pinned_take(sizeof(double)*2);
  if(!R->F_host) R->F_host = (double*)dlg_host_alloc(sizeof(double)*2);
  if(!R->F_host) { MSG("out of (pinned) host memory"); return false; }
  if(sparse)
  {
    R->cp_dev = (int*)q;
    if(!be_ok(dlg_mem_upload(R->cp_dev, d->dev_cp, sizeof(int)*(M + 1)), "upload of Jt_colptr")) return false;
  }
  return true;
}

void robust_enqueue(Driver* d, int s, double* x, double* J)
{
  Robust* R = d->robust;
  hipStream_t st = (hipStream_t)dlg_backend_get_stream(d->be);
  const int M = d->pub.Nmeasurements, N = d->pub.Nstate;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if(d->timing && hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess) (void)hipEventRecord(t0, st);
  hipLaunchKernelGGL(k_robust_weights, dim3((unsigned)R->nblk), dim3(TPB), 0, st, x, R->nfeat, R->L, R->w_dev[s], R->F_dev[s] + 1);
  const double* partial = R->F_dev[s] + 1;
  if(d->pub.solve_type == DOGLEG_SPARSE)
    hipLaunchKernelGGL(k_robust_scale_sparse, dim3((unsigned)((M + ROWS - 1)/ROWS)), dim3(TPB), 0, st, J, (const int*)R->cp_dev,
                       (const double*)R->w_dev[s], M, R->nfeat, R->L.fs, (int)d->nnz, partial, R->nblk, R->F_dev[s]);
  else
  {
    const long long total = (long long)M*N;
    const int head = (int)((reinterpret_cast<uintptr_t>(J) >> 3) & 1);
    const long long per = 2LL*TPB*DENSE_ITERS;
    hipLaunchKernelGGL(k_robust_scale_dense, dim3((unsigned)((total + per - 1)/per)), dim3(TPB), 0, st, J, (const double*)R->w_dev[s],
                       total, N, R->nfeat, R->L.fs, head, partial, R->nblk, R->F_dev[s]);
  }
  if(t1) { (void)hipEventRecord(t1, st); R->tm.push_back(t0); R->tm.push_back(t1); }
  else if(t0) (void)hipEventDestroy(t0);
  (void)hipMemcpyAsync(R->F_host + s, R->F_dev[s], sizeof(double), hipMemcpyDeviceToHost, st);
  (void)hipEventRecord(R->landed[s], st);
  R->nprelude++;
}

bool robust_F(Driver* d, int s, double* F)
{
  Robust* R = d->robust;
  if(!hip_ok(hipEventSynchronize(R->landed[s]), "the copy of F")) return false;
  *F = R->F_host[s];
  return true;
}

// the end of a solve: the weights of slot s to the caller (NULL: not asked for), and the record dogleg_amd_robust_last_stats reads
bool robust_weights(Driver* d, int s, double* weights_host)
{
  Robust* R = d->robust;
  if(weights_host && !be_ok(dlg_mem_download(weights_host, R->w_dev[s], sizeof(double)*(size_t)R->nfeat), "download of the weights")) return false;
  double ms = 0.0;
  for(size_t i = 0; i + 1 < R->tm.size(); i += 2)
  {
    float one = 0.f;
    if(hipEventSynchronize(R->tm[i + 1]) == hipSuccess && hipEventElapsedTime(&one, R->tm[i], R->tm[i + 1]) == hipSuccess) ms += one;
  }
  t_stats[0] = R->nprelude; t_stats[1] = 2; t_stats[2] = ms;
  return true;
}

void robust_destroy(Driver* d)
{
  Robust* R = d->robust;
  if(!R) return;
  for(hipEvent_t e : R->tm) (void)hipEventDestroy(e);
  for(int s = 0; s < 2; s++)
  {
    // (the last thing a prelude enqueues: behind it nothing of this solve touches the block)
    if(R->landed[s]) { (void)hipEventSynchronize(R->landed[s]); (void)hipEventDestroy(R->landed[s]); }
  }
  if(R->block) block_give(R->block, R->block_bytes, R->device, !d->failed);
  if(R->F_host) pinned_give(R->F_host, sizeof(double)*2);
  delete R;
  d->robust = nullptr;
}

extern "C" int dogleg_amd_robust_last_stats(double* out, int n)
{
  int k = 0;
  for(; k < n && k < 3 && out; k++) out[k] = t_stats[k];
  return k;
}
