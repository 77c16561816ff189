// bounds_device.hip -- box bounds on a device solve (dogleg.h: dogleg_amd_optimize_device2_bounded).  The eight steps of the batch
// contract (dogleg.h, above dogleg_amd_optimize_dense_batch_bounded) placed in the host driver's loop; everything between them --
// Cauchy step, assembly, factorisation, Gauss-Newton solve, the step, the expected improvement of an unclipped step -- is the plain
// solve's code on the masked point (J_F, g_F).  Behind dlg_point_eval of slot s, on the backend's stream:
//   k_bounds_hold      a thread a variable: the held byte (0 free, 1 at lower, 2 at upper) from p, g and the bounds, g_F in place
//                      into the slot's Jt_x, the workgroup's max |g_F|, count of held variables and sum g_F^2
//   k_bounds_reduce    one workgroup: the partials of the launch before in a fixed order (no floating-point atomics: the same
//                      bits every run) -> {max, count, sum of squares}
//   k_bounds_mask_*    flat over the entries of J: 0.0 into the held columns.  It does not read J: 4 bytes of index (sparse: THIS
//                      solve's Jt_rowidx, of which the solve keeps a device copy -- a backend taken over from the previous solve
//                      may hold another pattern of the same shape; dense: the column is e % Nstate) and one held byte an entry.
//                      Returns at once, the same way in every wave, when the count is 0.
// followed by a 24-byte copy to page-locked memory, the one read-back of an evaluation.  Behind the step:
//   k_bounds_clip      a thread a variable: p and the step of slot `to` clamped in place -> {max |s'|, clamped components, |s'|^2}
//   k_bounds_ratio     the fallback (step 6): the workgroup's min over (far_i - p_i) / d_i, d = t0 Cauchy
//   k_bounds_fallback  alpha = min(1, min of those), the step alpha d clamped, p of slot `to` -> the same three scalars; a component
//                      whose own ratio IS alpha -- the first bound the step meets -- is put on that bound's bits
// The held bytes belong to the callback invocation, per slot: a rejected trial steps again from the other slot's bytes, and
// nothing forms a held set from a g that has been masked already.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <vector>
#include "driver_internal.h"

namespace {

constexpr int TPB = 256;           // threads a workgroup, every kernel
constexpr int MASK_ITERS = 8;      // entries of J a lane of the mask pass visits
constexpr int NOUT = 4;            // {max, count, sum of squares, spare}

// the workgroup's max, sum a (counts: exact in a double) and sum b in a fixed order (a tree over the thread index); thread 0 stores
__device__ __forceinline__ void block_reduce3(double vmax, double va, double vb, double* __restrict__ part3)
{
  __shared__ double rm[TPB], ra[TPB], rb[TPB];
  const int t = threadIdx.x;
  rm[t] = vmax; ra[t] = va; rb[t] = vb;
  __syncthreads();
#pragma unroll
  for(int h = TPB/2; h > 0; h >>= 1)
  {
    if(t < h) { rm[t] = fmax(rm[t], rm[t + h]); ra[t] = ra[t] + ra[t + h]; rb[t] = rb[t] + rb[t + h]; }
    __syncthreads();
  }
  if(t == 0) { part3[0] = rm[0]; part3[1] = ra[0]; part3[2] = rb[0]; }
}

// step 2 and 3.  held, g: [n]; part: [gridDim.x][3]
__global__ void __launch_bounds__(TPB) k_bounds_hold(const double* __restrict__ p, double* __restrict__ g, const double* __restrict__ lo,
                                                     const double* __restrict__ hi, unsigned char* __restrict__ held, int n,
                                                     double* __restrict__ part)
{
#pragma clang fp contract(off)
  const int i = blockIdx.x*TPB + threadIdx.x;
  double a = 0.0, c = 0.0, q = 0.0;
  if(i < n)
  {
    const double pi = p[i], gi = g[i];
    const unsigned char h = (pi == lo[i] && gi > 0.0) ? 1 : ((pi == hi[i] && gi < 0.0) ? 2 : 0);
    held[i] = h;
    if(h) { g[i] = 0.0; c = 1.0; }
    else  { a = fabs(gi); q = gi*gi; }
  }
  block_reduce3(a, c, q, part + 3*(size_t)blockIdx.x);
}

// out[0 .. 2] = {max, sum, sum} of np partial triples: every thread its stride, then the tree.  One workgroup.
__global__ void __launch_bounds__(TPB) k_bounds_reduce(const double* __restrict__ part, int np, double* __restrict__ out)
{
#pragma clang fp contract(off)
  double a = 0.0, c = 0.0, q = 0.0;
  for(int i = threadIdx.x; i < np; i += TPB) { a = fmax(a, part[3*(size_t)i]); c += part[3*(size_t)i + 1]; q += part[3*(size_t)i + 2]; }
  block_reduce3(a, c, q, out);
}

// rowidx: [nnz], the variable of entry e (guarded against [0, n)); count: out[1] of the hold pass
__global__ void __launch_bounds__(TPB) k_bounds_mask_sparse(double* __restrict__ J, const int* __restrict__ rowidx,
                                                            const unsigned char* __restrict__ held, long long nnz, int n,
                                                            const double* __restrict__ count)
{
  if(count[0] == 0.0) return;                  // (one address for every lane: the same way in every wave)
  long long e = (long long)blockIdx.x*(TPB*MASK_ITERS) + threadIdx.x;
#pragma unroll
  for(int it = 0; it < MASK_ITERS; it++, e += TPB)
  {
    if(e >= nnz) return;
    const int v = rowidx[e];
    if((unsigned)v < (unsigned)n && held[v] != 0) J[e] = 0.0;
  }
}

// J: [M][n] row-major, total = M n entries: the column of entry e is e % n, one division a lane, then carried along
__global__ void __launch_bounds__(TPB) k_bounds_mask_dense(double* __restrict__ J, const unsigned char* __restrict__ held,
                                                           long long total, int n, const double* __restrict__ count)
{
  if(count[0] == 0.0) return;
  long long e = (long long)blockIdx.x*(TPB*MASK_ITERS) + threadIdx.x;
  if(e >= total) return;
  int col = (int)(e % n);
  const int cstep = TPB % n;
#pragma unroll
  for(int it = 0; it < MASK_ITERS; it++)
  {
    if(e >= total) return;
    if(held[col] != 0) J[e] = 0.0;
    e += TPB; col += cstep;
    if(col >= n) col -= n;
  }
}

// step 5.  p_to holds p_from + step (the step kernel's sum, the oracle's `p + s`); clamped components get the bound's bits and
// s' = bound - p.  part: {max |s'|, clamped components, sum s'^2}
__global__ void __launch_bounds__(TPB) k_bounds_clip(const double* __restrict__ p_from, double* __restrict__ p_to, double* __restrict__ step,
                                                     const double* __restrict__ lo, const double* __restrict__ hi, int n,
                                                     double* __restrict__ part)
{
#pragma clang fp contract(off)
  const int i = blockIdx.x*TPB + threadIdx.x;
  double a = 0.0, c = 0.0, q = 0.0;
  if(i < n)
  {
    const double t = p_to[i];
    double s = step[i];
    const double l = lo[i], u = hi[i];
    if(t < l)      { s = l - p_from[i]; p_to[i] = l; step[i] = s; c = 1.0; }
    else if(t > u) { s = u - p_from[i]; p_to[i] = u; step[i] = s; c = 1.0; }
    a = fabs(s); q = s*s;
  }
  block_reduce3(a, c, q, part + 3*(size_t)blockIdx.x);
}

// step 6, first launch: the workgroup's min of (far_i - p_i) / d_i over d_i != 0, d = t0 cauchy, far = upper where d_i > 0
__global__ void __launch_bounds__(TPB) k_bounds_ratio(const double* __restrict__ cauchy, const double* __restrict__ p, const double* __restrict__ lo,
                                                      const double* __restrict__ hi, double t0, int n, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double red[TPB];
  const int t = threadIdx.x, i = blockIdx.x*TPB + t;
  double r = INFINITY;
  if(i < n)
  {
    const double d = t0*cauchy[i];
    if(d != 0.0) r = ((d > 0.0 ? hi[i] : lo[i]) - p[i])/d;
  }
  red[t] = r;
  __syncthreads();
#pragma unroll
  for(int h = TPB/2; h > 0; h >>= 1)
  {
    if(t < h) red[t] = fmin(red[t], red[t + h]);
    __syncthreads();
  }
  if(t == 0) part[blockIdx.x] = red[0];
}

// step 6, second launch: alpha from the nr minima of the launch before (every workgroup forms it itself), the step alpha d,
// clamped as in step 5.  The component that set alpha (its ratio, formed by k_bounds_ratio's expression, equals alpha) ends ON
// its bound: p + ((far - p) / d) d rounds onto the bound's bits, one ulp beyond it (which the clamp brings back) or one ulp short
// of it, depending on the last bit of d -- and one ulp short the variable is on no bound, is not held at the next point, and the
// next fallback is cut at alpha ~ 1e-16: the solve would stop on update_threshold over a rounding.  So that component takes the
// clamp's form whichever way the sum rounds: the bound, and s = bound - p (within an ulp of alpha d).
__global__ void __launch_bounds__(TPB) k_bounds_fallback(const double* __restrict__ cauchy, const double* __restrict__ p_from, double* __restrict__ p_to,
                                                         double* __restrict__ step, const double* __restrict__ lo, const double* __restrict__ hi,
                                                         double t0, int n, const double* __restrict__ ratio, int nr, double* __restrict__ part)
{
#pragma clang fp contract(off)
  __shared__ double red[TPB];
  const int t = threadIdx.x, i = blockIdx.x*TPB + t;
  double r = INFINITY;
  for(int k = t; k < nr; k += TPB) r = fmin(r, ratio[k]);
  red[t] = r;
  __syncthreads();
#pragma unroll
  for(int h = TPB/2; h > 0; h >>= 1)
  {
    if(t < h) red[t] = fmin(red[t], red[t + h]);
    __syncthreads();
  }
  const double alpha = fmin(1.0, red[0]);
  __syncthreads();                             // (block_reduce3 has arrays of its own, but red[0] is read by all first)
  double a = 0.0, c = 0.0, q = 0.0;
  if(i < n)
  {
    const double pi = p_from[i], l = lo[i], u = hi[i];
    const double d = t0*cauchy[i];
    double s = alpha*d;
    double tr = pi + s;
    const double far = d > 0.0 ? u : l;
    if(d != 0.0 && (far - pi)/d == alpha) { tr = far; s = far - pi; c = 1.0; }
    else if(tr < l) { tr = l; s = l - pi; c = 1.0; }
    else if(tr > u) { tr = u; s = u - pi; c = 1.0; }
    p_to[i] = tr; step[i] = s;
    a = fabs(s); q = s*s;
  }
  block_reduce3(a, c, q, part + 3*(size_t)blockIdx.x);
}

thread_local double t_stats[6];

bool hip_ok(hipError_t e, const char* what)
{
  if(e == hipSuccess) return true;
  MSG("bounded device solve: %s failed: %s", what, hipGetErrorString(e));
  (void)hipGetLastError();
  return false;
}

// Between solves the library keeps the device block of the last bounded solve, as robust_prelude.hip keeps its own: the next
// bounded solve of the same size on the same GPU takes it over.  dogleg_amd_release_cache gives it back,
// DOGLEG_AMD_NO_BACKEND_CACHE never keeps it.
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

void bounds_release_cache()
{
  void* p = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_kept_mu);
    p = g_kept.p; g_kept = KeptBlock();
  }
  if(p) dlg_mem_free(p);
}

struct Bounds
{
  const double *lower, *upper; unsigned char* held_out;     // the caller's (host)
  int N, nblk;                       // variables; workgroups of the per-variable kernels = partial triples
  long long nent;                    // entries of J
  void* block; size_t block_bytes; int device;              // ONE device allocation: the arrays below, the doubles first
  double *lo_dev, *hi_dev;           // [N] (a NULL array: infinities)
  double *part, *ratio;              // [3 nblk], [nblk]
  double* out_dev;                   // [NOUT]
  int* ri_dev;                       // sparse: this solve's Jt_rowidx
  unsigned char* held_dev[2];        // per slot
  double* out_host;                  // page-locked [NOUT]
  double nheld[2];                   // per slot: held variables at its last evaluation
  long evaluations, clipped, fallbacks, held_steps;
  std::vector<hipEvent_t> tm;        // DOGLEG_AMD_TIMING: pairs of events around the feature's launches
  std::vector<hipEvent_t> tm_mask;   // ... those around the mask pass (part of the total)
};

namespace {
struct Timed
{
  Driver* d; Bounds* B; hipStream_t st; bool mask; hipEvent_t t0 = nullptr, t1 = nullptr;
  Timed(Driver* d_, hipStream_t st_, bool mask_ = false) : d(d_), B(d_->bounds), st(st_), mask(mask_)
  { if(d->timing && hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess) (void)hipEventRecord(t0, st); }
  ~Timed()
  {
    std::vector<hipEvent_t>& v = mask ? B->tm_mask : B->tm;
    if(t1) { (void)hipEventRecord(t1, st); v.push_back(t0); v.push_back(t1); }
    else if(t0) (void)hipEventDestroy(t0);
  }
};
// the three scalars of the launch sequence before, on the host (the one wait)
bool fetch_out(Driver* d, hipStream_t st, const char* what)
{
  Bounds* B = d->bounds;
  return hip_ok(hipMemcpyAsync(B->out_host, B->out_dev, sizeof(double)*3, hipMemcpyDeviceToHost, st), what) &&
         hip_ok(hipStreamSynchronize(st), what);
}
}

bool bounds_args_ok(const dogleg_amd_batch_bounds_t* bounds, const dogleg_amd_batch_loss_t* loss, const double* weights, const double* p,
                    unsigned int Nstate)
{
  const char* who = "dogleg_amd_optimize_device2_bounded";
  if(!bounds) { MSG("%s: a NULL bounds", who); return false; }
  if(!p || Nstate == 0) { MSG("%s: a NULL p or no variables", who); return false; }
  if(weights && !loss) { MSG("%s: weights without a loss", who); return false; }
  for(unsigned int i = 0; i < Nstate; i++)
  {
    const double l = bounds->lower ? bounds->lower[i] : -INFINITY, u = bounds->upper ? bounds->upper[i] : INFINITY;
    if(!(l <= u)) { MSG("%s: variable %u has a NaN bound or lower > upper (%g, %g)", who, i, l, u); return false; }
  }
  return true;
}

Bounds* bounds_create(const dogleg_amd_batch_bounds_t* bounds)
{
  Bounds* B = new (std::nothrow) Bounds();
  if(!B) return nullptr;
  B->lower = bounds->lower; B->upper = bounds->upper; B->held_out = bounds->held;
  B->N = B->nblk = 0; B->nent = 0;
  B->block = nullptr; B->block_bytes = 0; B->device = -1;
  B->lo_dev = B->hi_dev = B->part = B->ratio = B->out_dev = nullptr; B->ri_dev = nullptr;
  B->held_dev[0] = B->held_dev[1] = nullptr; B->out_host = nullptr;
  B->nheld[0] = B->nheld[1] = 0.0;
  B->evaluations = B->clipped = B->fallbacks = B->held_steps = 0;
  return B;
}

// step 1, on the host, in front of the upload of p
void bounds_clamp_start(const Driver* d, double* p)
{
  const Bounds* B = d->bounds;
  for(int i = 0; i < d->pub.Nstate; i++)
  {
    if(B->lower && p[i] < B->lower[i]) p[i] = B->lower[i];
    if(B->upper && p[i] > B->upper[i]) p[i] = B->upper[i];
  }
}

bool bounds_set_up(Driver* d)
{
  Bounds* B = d->bounds;
  const size_t N = (size_t)d->pub.Nstate;
  const bool sparse = d->pub.solve_type == DOGLEG_SPARSE;
  B->N = (int)N;
  B->nblk = (int)((N + TPB - 1)/TPB);
  B->nent = sparse ? (long long)d->nnz : (long long)d->pub.Nmeasurements*(long long)N;
  const size_t nd = 2*N + 4*(size_t)B->nblk + NOUT;
  const size_t held_bytes = (N + 7) & ~(size_t)7;
  B->block_bytes = sizeof(double)*nd + (sparse ? sizeof(int)*(((size_t)d->nnz + 1) & ~(size_t)1) : 0) + 2*held_bytes;
  B->device = dlg_backend_device(d->be);
  B->block = block_take(B->block_bytes, B->device);
  if(!B->block) { MSG("out of device memory"); return false; }
  double* q = (double*)B->block;
  B->lo_dev = q; q += N; B->hi_dev = q; q += N;
  B->part = q; q += 3*(size_t)B->nblk; B->ratio = q; q += B->nblk;
  B->out_dev = q; q += NOUT;
  unsigned char* bytes = (unsigned char*)q;
  if(sparse) { B->ri_dev = (int*)bytes; bytes += sizeof(int)*(((size_t)d->nnz + 1) & ~(size_t)1); }
  B->held_dev[0] = bytes; B->held_dev[1] = bytes + held_bytes;
  B->out_host = (double*)pinned_take(sizeof(double)*NOUT);
  if(!B->out_host) B->out_host = (double*)dlg_host_alloc(sizeof(double)*NOUT);
  if(!B->out_host) { MSG("out of (pinned) host memory"); return false; }
  // (a NULL array: infinities, so that the kernels have one form)
  std::vector<double> inf(N);
  for(int k = 0; k < 2; k++)
  {
    const double* src = k == 0 ? B->lower : B->upper;
    if(!src) { for(size_t i = 0; i < N; i++) inf[i] = k == 0 ? -INFINITY : INFINITY; src = inf.data(); }
    if(!be_ok(dlg_mem_upload(k == 0 ? B->lo_dev : B->hi_dev, src, sizeof(double)*N), "upload of the bounds")) return false;
  }
  if(!be_ok(dlg_mem_zero(B->held_dev[0], 2*held_bytes), "clearing the held bytes")) return false;
  if(sparse && !be_ok(dlg_mem_upload(B->ri_dev, d->dev_ri, sizeof(int)*(size_t)d->nnz), "upload of Jt_rowidx")) return false;
  return true;
}

// steps 2 and 3 behind dlg_point_eval of slot s: the held bytes, g_F, the masked J, and what the backend kept of the unmasked g
bool bounds_hold_mask(Driver* d, int s, double* absmax)
{
  Bounds* B = d->bounds;
  hipStream_t st = (hipStream_t)dlg_backend_get_stream(d->be);
  double* g = (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_JTX);
  const double* p = (const double*)dlg_point_device_ptr(d->be, s, DLG_VEC_P);
  double* J = (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_J_OWN);
  if(!g || !p || !J) { MSG("bounded device solve: the slot's vectors are missing"); return false; }
  {
    Timed tm(d, st);
    hipLaunchKernelGGL(k_bounds_hold, dim3((unsigned)B->nblk), dim3(TPB), 0, st, p, g, (const double*)B->lo_dev, (const double*)B->hi_dev,
                       B->held_dev[s], B->N, B->part);
    hipLaunchKernelGGL(k_bounds_reduce, dim3(1), dim3(TPB), 0, st, (const double*)B->part, B->nblk, B->out_dev);
  }
  {
    Timed tm(d, st, true);
    const long long per = (long long)TPB*MASK_ITERS;
    const unsigned grid = (unsigned)((B->nent + per - 1)/per);
    if(grid > 0)
    {
      if(d->pub.solve_type == DOGLEG_SPARSE)
        hipLaunchKernelGGL(k_bounds_mask_sparse, dim3(grid), dim3(TPB), 0, st, J, (const int*)B->ri_dev, (const unsigned char*)B->held_dev[s],
                           B->nent, B->N, (const double*)(B->out_dev + 1));
      else
        hipLaunchKernelGGL(k_bounds_mask_dense, dim3(grid), dim3(TPB), 0, st, J, (const unsigned char*)B->held_dev[s], B->nent, B->N,
                           (const double*)(B->out_dev + 1));
    }
  }
  if(!hip_ok(hipGetLastError(), "the hold and mask launches") || !fetch_out(d, st, "the read-back of the held set's scalars")) return false;
  B->evaluations++;
  B->nheld[s] = B->out_host[1];
  *absmax = B->out_host[0];
  return be_ok(dlg_point_bind_held(d->be, s, B->held_dev[s], B->out_host[2]), "binding the held variables");
}

void bounds_note_step(Driver* d, int from) { if(d->bounds->nheld[from] > 0.0) d->bounds->held_steps++; }

// step 5 behind a step into slot `to`: *clamped components, max |s'| and |s'|^2 of the step as it stands afterwards
bool bounds_clip(Driver* d, int from, int to, double* clamped, double* smax, double* n2)
{
  Bounds* B = d->bounds;
  hipStream_t st = (hipStream_t)dlg_backend_get_stream(d->be);
  const double* pf = (const double*)dlg_point_device_ptr(d->be, from, DLG_VEC_P);
  double* pt = (double*)dlg_point_device_ptr(d->be, to, DLG_VEC_P);
  double* step = (double*)dlg_point_device_ptr(d->be, to, DLG_VEC_STEP);
  {
    Timed tm(d, st);
    hipLaunchKernelGGL(k_bounds_clip, dim3((unsigned)B->nblk), dim3(TPB), 0, st, pf, pt, step, (const double*)B->lo_dev, (const double*)B->hi_dev,
                       B->N, B->part);
    hipLaunchKernelGGL(k_bounds_reduce, dim3(1), dim3(TPB), 0, st, (const double*)B->part, B->nblk, B->out_dev);
  }
  if(!hip_ok(hipGetLastError(), "the clip launches") || !fetch_out(d, st, "the read-back of the clip's scalars")) return false;
  *smax = B->out_host[0]; *clamped = B->out_host[1]; *n2 = B->out_host[2];
  if(*clamped > 0.0) B->clipped++;
  return true;
}

// step 6: the Cauchy step of slot `from`, cut at the trust region (t0) and at the first bound, into slot `to`
bool bounds_fallback(Driver* d, int from, int to, double t0, double* smax, double* n2)
{
  Bounds* B = d->bounds;
  hipStream_t st = (hipStream_t)dlg_backend_get_stream(d->be);
  const double* cauchy = (const double*)dlg_point_device_ptr(d->be, from, DLG_VEC_CAUCHY);
  const double* pf = (const double*)dlg_point_device_ptr(d->be, from, DLG_VEC_P);
  double* pt = (double*)dlg_point_device_ptr(d->be, to, DLG_VEC_P);
  double* step = (double*)dlg_point_device_ptr(d->be, to, DLG_VEC_STEP);
  B->fallbacks++;
  {
    Timed tm(d, st);
    hipLaunchKernelGGL(k_bounds_ratio, dim3((unsigned)B->nblk), dim3(TPB), 0, st, cauchy, pf, (const double*)B->lo_dev, (const double*)B->hi_dev,
                       t0, B->N, B->ratio);
    hipLaunchKernelGGL(k_bounds_fallback, dim3((unsigned)B->nblk), dim3(TPB), 0, st, cauchy, pf, pt, step, (const double*)B->lo_dev,
                       (const double*)B->hi_dev, t0, B->N, (const double*)B->ratio, B->nblk, B->part);
    hipLaunchKernelGGL(k_bounds_reduce, dim3(1), dim3(TPB), 0, st, (const double*)B->part, B->nblk, B->out_dev);
  }
  if(!hip_ok(hipGetLastError(), "the fallback launches") || !fetch_out(d, st, "the read-back of the fallback's scalars")) return false;
  *smax = B->out_host[0]; *n2 = B->out_host[2];
  return true;
}

// the end of a solve: step 8 (the held bytes of slot s to the caller) and the record dogleg_amd_bounded_last_stats reads
bool bounds_finish(Driver* d, int s)
{
  Bounds* B = d->bounds;
  if(B->held_out && !be_ok(dlg_mem_download(B->held_out, B->held_dev[s], (size_t)B->N), "download of the held set")) return false;
  double ms = 0.0, ms_mask = 0.0;
  for(int k = 0; k < 2; k++)
  {
    const std::vector<hipEvent_t>& v = k == 0 ? B->tm : B->tm_mask;
    for(size_t i = 0; i + 1 < v.size(); i += 2)
    {
      float one = 0.f;
      if(hipEventSynchronize(v[i + 1]) == hipSuccess && hipEventElapsedTime(&one, v[i], v[i + 1]) == hipSuccess) (k == 0 ? ms : ms_mask) += one;
    }
  }
  ms += ms_mask;
  t_stats[5] = ms_mask;
  t_stats[0] = (double)B->evaluations; t_stats[1] = (double)B->clipped; t_stats[2] = (double)B->fallbacks;
  t_stats[3] = (double)B->held_steps; t_stats[4] = ms;
  return true;
}

void bounds_destroy(Driver* d)
{
  Bounds* B = d->bounds;
  if(!B) return;
  // (the backend reads the held bytes at its next factorisation: not after this)
  if(d->be) { (void)hipStreamSynchronize((hipStream_t)dlg_backend_get_stream(d->be)); (void)dlg_point_bind_held(d->be, 0, nullptr, 0.0); (void)dlg_point_bind_held(d->be, 1, nullptr, 0.0); }
  for(hipEvent_t e : B->tm) (void)hipEventDestroy(e);
  for(hipEvent_t e : B->tm_mask) (void)hipEventDestroy(e);
  if(B->block) block_give(B->block, B->block_bytes, B->device, !d->failed);
  if(B->out_host) pinned_give(B->out_host, sizeof(double)*NOUT);
  delete B;
  d->bounds = nullptr;
}

extern "C" int dogleg_amd_bounded_last_stats(double* out, int n)
{
  int k = 0;
  for(; k < n && k < 6 && out; k++) out[k] = t_stats[k];
  return k;
}
