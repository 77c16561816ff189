// numeric_device.hip -- numeric Jacobians for a single problem whose model comes as values only (dogleg.h: dogleg_amd_numeric_*),
// sparse and dense.  An adapter in front of dogleg_optimize_device2 and its kin, none of which changes:
// dogleg_amd_numeric_callback is a dogleg_callback_device_t that writes K copies of p (k_numeric_perturb_coloured), calls the
// caller's values model once for all of them, and forms x and J in the buffers it was handed from the copies' x
// (k_numeric_jacobian_sparse / k_numeric_jacobian_dense).  Two launches and one call of the model per invocation whatever the
// sizes are, everything on the stream it is given, no synchronisation, allocation or copy.  The variables are perturbed by
// colour (numeric_plan.h: the colouring of the Jacobian check), so K = C + 1 or 2 C + 1, not Nstate + 1.  The step rule is
// include/dogleg_numeric_step.h; this file is compiled with -ffp-contract=off (build.py) on top of that header's pragma.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>
#include "../../include/dogleg.h"
#include "../../include/dogleg_numeric_step.h"
#include "numeric_plan.h"

void dlg_set_error(const char* fmt, ...);

#define NDMSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)

namespace {

constexpr int ND_THREADS = 256;
constexpr unsigned ND_MAX_GRID = 256*8;         // memory-bound kernels: at most 8 blocks per CU, the rest by grid stride

// ---- the sparse Jacobian kernel's tile.  None of this is measured; the reasoning:
//  * ND_TR = 64 measurement rows per tile: the read of a tile is one segment of 64 doubles per copy, 512 bytes, four whole
//    128-byte lines and one wavefront's worth, so a wavefront stages one copy's segment per load instruction.  With ~15 entries
//    a row a tile holds ~960 entries of J, four passes of the 256 lanes.
//  * the LDS image holds one row of ND_S doubles per staged copy: slot 0 is copy 0, slots 1 .. nc the plus copies of the chunk's
//    colours, slots 1 + nc .. 2 nc their minus copies (central).  ND_S = ND_TR + 1 = 65, ODD, for the entry walk: lane t reads
//    image[slot(colour of t)][row of t], address slot * ND_S + row.  Neighbouring lanes are neighbouring entries: the same row
//    or the next, and within one row all colours differ.  A 64-bit read is served in groups of 32 lanes over 32 double-wide
//    bank slots (address mod 32).  With ND_S odd, slot * ND_S mod 32 takes 32 different values for 32 consecutive slots, so the
//    entries of one row never collide with each other however many the group holds; with ND_S = 64 every lane of a row would
//    hit ONE bank slot, a 15-way conflict on the block-arrowhead patterns.  Two lanes of DIFFERENT rows r, r' collide only when
//    (slot - slot') * 65 = r' - r mod 32, at most a two-way conflict for the two or three rows a group spans.  The staging
//    writes go to consecutive addresses and cannot conflict.
//  * ND_SLOTS = 63 staged copies at most, 63 * 65 * 8 = 32 760 bytes, beside 260 bytes of staged colptr: four workgroups of four
//    wavefronts a CU out of its 160 KiB, four wavefronts a SIMD, which a kernel that only loads, divides and stores needs to
//    cover the latency of its loads.  Only the slots a pattern needs are asked for at the launch: 16 (forward) or 31 (central)
//    on the 15-colour block-arrowhead patterns, 16 120 bytes at most.  A pattern with more colours than a chunk holds, (ND_SLOTS
//    - 1) / 2 = 31 central or 62 forward, loops over chunks of colours: each pass stages copy 0 and the chunk's copies and
//    writes the entries whose colour lies in the chunk.  It is the same code path with one more trip of the loop; every entry is
//    written exactly once because its colour lies in exactly one chunk.
constexpr int ND_TR = 64;
constexpr int ND_S = ND_TR + 1;
constexpr int ND_SLOTS = 63;

// ---- the dense Jacobian kernel's tile: ND_DTR rows x ND_DTV variables of J, filled column-wise from the segments
// x[1 + j][r0 .. r0 + 32) and read out row-wise.  32 x 32 because 32 doubles are two whole 128-byte lines on both sides: the
// reads along r and the stores along j.  Row stride ND_DS = 33, odd: the fill's 16-lane write groups (16 consecutive r, one j)
// land on 16 different double-wide bank slots, and the read-out's 32-lane groups read 32 consecutive doubles of one row (a
// narrower last tile: at most two rows, shifted by one double a row, no slot hit more than twice).  8 448 bytes of LDS.
constexpr int ND_DTR = 32;
constexpr int ND_DTV = 32;
constexpr int ND_DS = ND_DTV + 1;

// The K copies of p and the divisors; one thread per double of the copies [K][N], consecutive loads and stores.  Copy 0 is p,
// copy 1 + c has every variable of colour c at its plus point, copy 1 + C + c (central) at its minus point: entry (k, j)
// evaluates the step rule only where k is a copy of colour[j].  The threads of copy 0 write the divisors.  colour == nullptr:
// the dense problem, colour[j] = j.
__global__ void __launch_bounds__(ND_THREADS)
k_numeric_perturb_coloured(int N, int K, int C, int scheme, double delta_rel, double delta_abs, const double* __restrict__ p,
                           const double* __restrict__ lower, const double* __restrict__ upper, const int* __restrict__ colour,
                           double* __restrict__ pc, double* __restrict__ div)
{
  const size_t total = (size_t)K*(size_t)N;
  for(size_t idx = (size_t)blockIdx.x*ND_THREADS + threadIdx.x; idx < total; idx += (size_t)gridDim.x*ND_THREADS)
  {
    const int k = (int)(idx/(size_t)N);
    const int j = (int)(idx - (size_t)k*N);
    const double pj = p[j];
    double v = pj;
    const int cj = colour ? colour[j] : j;
    const int which = k == 0 ? 0 : (k - 1 == cj ? 1 : (k - 1 - C == cj ? 2 : -1));    // divisor / plus / minus point / p itself
    if(which >= 0)
    {
      double tp, tm, d;
      dogleg_numeric_step(scheme, pj, lower ? lower[j] : -INFINITY, upper ? upper[j] : INFINITY, delta_rel, delta_abs, &tp, &tm, &d);
      if(which == 0) div[j] = d;
      if(which == 1) v = tp;
      if(which == 2) v = tm;
    }
    pc[idx] = v;
  }
}

// x and the values of Jt in pattern order from the copies' x.  A workgroup takes tiles of ND_TR measurement rows: it stages
// colptr[r0 .. r0 + rows] and, chunk of colours by chunk, the segments xc[k][r0 .. r0 + rows) of the chunk's copies -- one
// contiguous segment a copy -- and its lanes then walk the tile's entries, the ONE span colptr[r0] .. colptr[r0 + rows] of J:
// consecutive lanes are consecutive t.  A lane finds its row by bisection in the staged colptr (empty rows: the search keeps
// cp[lo] <= t < cp[hi], so it ends on the row that holds t), reads its colour and variable contiguously, the divisor by gather
// (an Nstate-sized array, L2-resident), the two x from LDS, and stores J[t].  The lanes that stage copy 0 in the first chunk
// write x.  t is an int because colptr is; every offset it scales into is a size_t.
__global__ void __launch_bounds__(ND_THREADS)
k_numeric_jacobian_sparse(int M, int C, int central, int chunk, const int* __restrict__ colptr, const int* __restrict__ rowidx,
                          const int* __restrict__ entry_colour, const double* __restrict__ xc, const double* __restrict__ div,
                          double* __restrict__ x, double* __restrict__ J)
{
  extern __shared__ double image[];              // [slots][ND_S]
  __shared__ int cp[ND_TR + 1];
  const int ntiles = (M + ND_TR - 1)/ND_TR;
  for(int tile = blockIdx.x; tile < ntiles; tile += gridDim.x)
  {
    const int r0 = tile*ND_TR;
    const int rows = min(ND_TR, M - r0);
    for(int i = threadIdx.x; i <= rows; i += ND_THREADS) cp[i] = colptr[r0 + i];
    for(int c0 = 0; c0 < C; c0 += chunk)
    {
      const int nc = min(chunk, C - c0);
      const int nslots = 1 + (central ? 2*nc : nc);
      for(int e = threadIdx.x; e < nslots*rows; e += ND_THREADS)
      {
        const int s = e/rows, r = e - s*rows;
        const int k = s == 0 ? 0 : (s <= nc ? c0 + s : C + c0 + s - nc);           // copy 0 | 1 + c0 + (s - 1) | 1 + C + c0 + (s - 1 - nc)
        const double v = xc[(size_t)k*(size_t)M + (size_t)(r0 + r)];
        image[s*ND_S + r] = v;
        if(s == 0 && c0 == 0) x[r0 + r] = v;
      }
      __syncthreads();
      const int t1 = cp[rows];
      for(int t = cp[0] + (int)threadIdx.x; t < t1; t += ND_THREADS)
      {
        const int c = entry_colour[t] - c0;
        if(c < 0 || c >= nc) continue;
        int lo = 0, hi = rows;
        while(hi - lo > 1) { const int mid = (lo + hi) >> 1; if(cp[mid] <= t) lo = mid; else hi = mid; }
        const double d = div[rowidx[t]];
        const double xp = image[(1 + c)*ND_S + lo];
        const double xm = central ? image[(1 + nc + c)*ND_S + lo] : image[lo];
        J[(size_t)t] = d == 0.0 ? 0.0 : (xp - xm)/d;
      }
      __syncthreads();
    }
  }
}

// x and J[M][N] row-major of a dense problem.  A workgroup takes tiles of ND_DTR rows x ND_DTV variables.  Fill: lane (r, jg)
// reads the segments x+[j][r0 + r] and x-[j][r0 + r] for j = j0 + jg, j0 + jg + 8, ..., contiguous along r, and puts the
// quotient at tile[r][j - j0].  Read-out row-wise: each row of the tile is a segment of tv doubles of J, stored by consecutive
// lanes, so any Nstate works.  The tiles of the first variable block write x.
__global__ void __launch_bounds__(ND_THREADS)
k_numeric_jacobian_dense(int N, int M, int central, const double* __restrict__ xc, const double* __restrict__ div,
                         double* __restrict__ x, double* __restrict__ J)
{
  __shared__ double tile[ND_DTR*ND_DS];
  const int ntr = (M + ND_DTR - 1)/ND_DTR, ntv = (N + ND_DTV - 1)/ND_DTV;
  const size_t work = (size_t)ntr*(size_t)ntv;
  const int r = threadIdx.x % ND_DTR, jg = threadIdx.x / ND_DTR;
  constexpr int JG = ND_THREADS/ND_DTR;
  for(size_t w = blockIdx.x; w < work; w += gridDim.x)
  {
    const int tr = (int)(w/(size_t)ntv), tv0 = (int)(w - (size_t)tr*ntv);
    const int r0 = tr*ND_DTR, j0 = tv0*ND_DTV;
    const int rows = min(ND_DTR, M - r0), tv = min(ND_DTV, N - j0);
    if(r < rows)
    {
      const size_t row = (size_t)(r0 + r);
      const double x0 = xc[row];
      if(jg == 0 && j0 == 0) x[row] = x0;
      for(int jj = jg; jj < tv; jj += JG)
      {
        const int j = j0 + jj;
        const double xp = xc[(size_t)(1 + j)*(size_t)M + row];
        const double xm = central ? xc[(size_t)(1 + N + j)*(size_t)M + row] : x0;
        const double d = div[j];
        tile[r*ND_DS + jj] = d == 0.0 ? 0.0 : (xp - xm)/d;
      }
    }
    __syncthreads();
    for(int e = threadIdx.x; e < rows*tv; e += ND_THREADS)
    {
      const int rr = e/tv, jj = e - rr*tv;
      J[(size_t)(r0 + rr)*(size_t)N + (size_t)(j0 + jj)] = tile[rr*ND_DS + jj];
    }
    __syncthreads();
  }
}

unsigned nd_grid_for(size_t items)
{
  const size_t blocks = (items + ND_THREADS - 1)/ND_THREADS;
  return (unsigned)(blocks < 1 ? 1 : (blocks > ND_MAX_GRID ? ND_MAX_GRID : blocks));
}

struct NdTimedCall { hipEvent_t ev[4]; };       // before the copies | before f | behind f | behind J
constexpr size_t ND_MAX_PENDING = 4096;         // timed invocations kept until dogleg_amd_numeric_stats reads them

} // namespace

struct dogleg_amd_numeric
{
  int N, M, nnz, C, K, scheme, chunk;
  bool dense;
  double delta_rel, delta_abs;
  dogleg_callback_device_values_t* f;
  void* cookie;
  int device;
  double* d_pc;          // [K][N]
  double* d_xc;          // [K][M]
  double* d_div;         // [N]
  double* d_bounds;      // host bounds copied: lower | upper, each [N] where given
  int* d_index;          // sparse: colour [N] | colptr [M + 1] | rowidx [nnz] | entry colour [nnz]
  const int *colour, *colptr, *rowidx, *entry_colour;
  const double* lower;   // device, or nullptr
  const double* upper;
  double invocations, f_calls, copies, launches, ms_f, ms_lib;
  std::vector<NdTimedCall> pending;
};

namespace {

bool nd_refuse(const char* who, const char* why)
{
  dlg_set_error("%s: %s", who, why); NDMSG("%s: %s", who, why);
  return false;
}

bool nd_check_options(const char* who, unsigned N, dogleg_callback_device_values_t* f, const dogleg_amd_numeric_options_t* opt)
{
  if(!f) return nd_refuse(who, "f is NULL");
  if(!opt) return true;
  if(!(opt->delta_rel >= 0.0) || !(opt->delta_abs >= 0.0)) return nd_refuse(who, "delta_rel and delta_abs must not be negative or NaN");
  if(!opt->bounds_on_device)
    for(size_t i = 0; i < (size_t)N; i++)
    {
      const double lo = opt->lower ? opt->lower[i] : -INFINITY, hi = opt->upper ? opt->upper[i] : INFINITY;
      if(!(lo <= hi))
      {
        dlg_set_error("%s: lower > upper", who);
        NDMSG("%s: variable %zu: lower %g > upper %g (or a NaN)", who, i, lo, hi);
        return false;
      }
    }
  return true;
}

void nd_harvest(dogleg_amd_numeric* h)
{
  if(h->pending.empty()) return;
  (void)hipEventSynchronize(h->pending.back().ev[3]);
  for(NdTimedCall& c : h->pending)
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

int dogleg_amd_numeric_plan(unsigned Nstate, unsigned Nmeas, unsigned NJnnz, const int* Jt_colptr, const int* Jt_rowidx,
                            int scheme, int* colour, int* copies, double* device_bytes)
{
  const char* who = "dogleg_amd_numeric_plan";
  NumericPlan P;
  char err[512];
  if(numeric_plan(P, Nstate, Nmeas, NJnnz, Jt_colptr, Jt_rowidx, scheme, false, err, sizeof(err)))
  { nd_refuse(who, err); return -1; }
  if(colour)
    for(int j = 0; j < P.N; j++) colour[j] = P.dense ? j : P.colour[j];
  if(copies) *copies = P.K;
  if(device_bytes) *device_bytes = P.device_bytes;
  return P.C;
}

void dogleg_amd_numeric_destroy(struct dogleg_amd_numeric* h)
{
  if(!h) return;
  int cur = -1;
  const bool sw = h->device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != h->device && hipSetDevice(h->device) == hipSuccess;
  nd_harvest(h);
  if(h->d_pc) (void)hipFree(h->d_pc);
  if(h->d_xc) (void)hipFree(h->d_xc);
  if(h->d_div) (void)hipFree(h->d_div);
  if(h->d_bounds) (void)hipFree(h->d_bounds);
  if(h->d_index) (void)hipFree(h->d_index);
  if(sw) (void)hipSetDevice(cur);
  (void)hipGetLastError();
  delete h;
}

struct dogleg_amd_numeric* dogleg_amd_numeric_create(unsigned Nstate, unsigned Nmeas, unsigned NJnnz,
                                                     const int* Jt_colptr, const int* Jt_rowidx,
                                                     dogleg_callback_device_values_t* f, void* cookie,
                                                     const dogleg_amd_numeric_options_t* opt)
{
  const char* who = "dogleg_amd_numeric_create";
  const int scheme = opt ? opt->scheme : DOGLEG_AMD_NUMERIC_FORWARD;
  NumericPlan P;
  char err[512];
  if(numeric_plan(P, Nstate, Nmeas, NJnnz, Jt_colptr, Jt_rowidx, scheme, true, err, sizeof(err)))
  { nd_refuse(who, err); return nullptr; }
  if(!nd_check_options(who, Nstate, f, opt)) return nullptr;
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    (void)hipGetLastError();
    dlg_set_error("%s: no HIP device", who); NDMSG("%s: no HIP device (there is no CPU fallback)", who);
    return nullptr;
  }
  dogleg_amd_numeric* h = new (std::nothrow) dogleg_amd_numeric();
  if(!h) return nullptr;
  h->N = P.N; h->M = P.M; h->nnz = P.nnz; h->C = P.C; h->K = P.K; h->scheme = scheme; h->dense = P.dense;
  h->chunk = scheme == DOGLEG_AMD_NUMERIC_CENTRAL ? (ND_SLOTS - 1)/2 : ND_SLOTS - 1;
  const double dflt = scheme == DOGLEG_AMD_NUMERIC_CENTRAL ? DOGLEG_NUMERIC_DELTA_CENTRAL : DOGLEG_NUMERIC_DELTA_FORWARD;
  const bool defaults = !opt || (opt->delta_rel <= 0.0 && opt->delta_abs <= 0.0);
  h->delta_rel = defaults ? dflt : opt->delta_rel; h->delta_abs = defaults ? dflt : opt->delta_abs;
  h->f = f; h->cookie = cookie; h->device = -1;
  h->d_pc = h->d_xc = h->d_div = h->d_bounds = nullptr; h->d_index = nullptr;
  h->colour = h->colptr = h->rowidx = h->entry_colour = nullptr; h->lower = h->upper = nullptr;
  h->invocations = h->f_calls = h->copies = h->launches = h->ms_f = h->ms_lib = 0.0;
  const bool host_lo = opt && !opt->bounds_on_device && opt->lower, host_hi = opt && !opt->bounds_on_device && opt->upper;
  const size_t N = (size_t)P.N, M = (size_t)P.M, nnz = (size_t)P.nnz, K = (size_t)P.K;
  const size_t vec = sizeof(double)*N, pc_bytes = K*vec, xc_bytes = sizeof(double)*K*M;
  const size_t bounds_bytes = vec*((host_lo ? 1 : 0) + (host_hi ? 1 : 0));
  const size_t index_ints = P.dense ? 0 : N + (M + 1) + 2*nnz;
  bool ok = hipGetDevice(&h->device) == hipSuccess;
  ok = ok && hipMalloc((void**)&h->d_pc, pc_bytes) == hipSuccess && hipMalloc((void**)&h->d_xc, xc_bytes) == hipSuccess &&
       hipMalloc((void**)&h->d_div, vec) == hipSuccess && (bounds_bytes == 0 || hipMalloc((void**)&h->d_bounds, bounds_bytes) == hipSuccess) &&
       (index_ints == 0 || hipMalloc((void**)&h->d_index, sizeof(int)*index_ints) == hipSuccess);
  if(!ok)
  {
    (void)hipGetLastError();
    dlg_set_error("%s: cannot allocate %.3g bytes of device memory", who, P.device_bytes + (double)bounds_bytes);
    NDMSG("%s: C = %d colours, K = %d copies of %d + %d doubles (the longest row holds %d variables) need %.3g bytes of device "
          "memory: the allocation failed", who, P.C, P.K, P.N, P.M, P.longest_row, P.device_bytes + (double)bounds_bytes);
    dogleg_amd_numeric_destroy(h);
    return nullptr;
  }
  if(!P.dense)
  {
    int* q = h->d_index;
    ok = ok && hipMemcpy(q, P.colour.data(), sizeof(int)*N, hipMemcpyHostToDevice) == hipSuccess; h->colour = q; q += N;
    ok = ok && hipMemcpy(q, Jt_colptr, sizeof(int)*(M + 1), hipMemcpyHostToDevice) == hipSuccess; h->colptr = q; q += M + 1;
    ok = ok && hipMemcpy(q, Jt_rowidx, sizeof(int)*nnz, hipMemcpyHostToDevice) == hipSuccess; h->rowidx = q; q += nnz;
    ok = ok && hipMemcpy(q, P.entry_colour.data(), sizeof(int)*nnz, hipMemcpyHostToDevice) == hipSuccess; h->entry_colour = q;
  }
  if(opt && opt->bounds_on_device) { h->lower = opt->lower; h->upper = opt->upper; }
  else
  {
    double* q = h->d_bounds;
    if(host_lo) { ok = ok && hipMemcpy(q, opt->lower, vec, hipMemcpyHostToDevice) == hipSuccess; h->lower = q; q += N; }
    if(host_hi) { ok = ok && hipMemcpy(q, opt->upper, vec, hipMemcpyHostToDevice) == hipSuccess; h->upper = q; }
  }
  if(!ok)
  {
    dlg_set_error("%s: the upload of the pattern or the bounds failed", who); NDMSG("%s: the upload of the pattern or the bounds failed", who);
    (void)hipGetLastError();
    dogleg_amd_numeric_destroy(h);
    return nullptr;
  }
  return h;
}

void dogleg_amd_numeric_callback(const double* p_dev, double* x_dev, double* J_dev, void* hip_stream, void* cookie)
{
  dogleg_amd_numeric* h = (dogleg_amd_numeric*)cookie;
  hipStream_t st = (hipStream_t)hip_stream;
  h->invocations += 1.0;
  const int N = h->N, M = h->M, K = h->K, C = h->C;
  const int central = h->scheme == DOGLEG_AMD_NUMERIC_CENTRAL ? 1 : 0;
  NdTimedCall T;
  bool timed = getenv("DOGLEG_AMD_NUMERIC_TIMING") != nullptr && h->pending.size() < ND_MAX_PENDING;
  if(timed)
    for(int i = 0; i < 4; i++)
      if(hipEventCreate(&T.ev[i]) != hipSuccess) { for(int k = 0; k < i; k++) (void)hipEventDestroy(T.ev[k]); (void)hipGetLastError(); timed = false; break; }
  if(timed) (void)hipEventRecord(T.ev[0], st);
  hipLaunchKernelGGL(k_numeric_perturb_coloured, dim3(nd_grid_for((size_t)K*(size_t)N)), dim3(ND_THREADS), 0, st, N, K, C, h->scheme,
                     h->delta_rel, h->delta_abs, p_dev, h->lower, h->upper, h->colour, h->d_pc, h->d_div);
  if(timed) (void)hipEventRecord(T.ev[1], st);
  h->f(h->d_pc, h->d_xc, (unsigned int)K, hip_stream, h->cookie);
  if(timed) (void)hipEventRecord(T.ev[2], st);
  if(h->dense)
  {
    const size_t work = (size_t)((M + ND_DTR - 1)/ND_DTR)*(size_t)((N + ND_DTV - 1)/ND_DTV);
    hipLaunchKernelGGL(k_numeric_jacobian_dense, dim3((unsigned)(work > ND_MAX_GRID ? ND_MAX_GRID : work)), dim3(ND_THREADS), 0, st,
                       N, M, central, h->d_xc, h->d_div, x_dev, J_dev);
  }
  else
  {
    const int ntiles = (M + ND_TR - 1)/ND_TR;
    const int nc = C < h->chunk ? C : h->chunk;
    const size_t lds = sizeof(double)*(size_t)ND_S*(size_t)(1 + (central ? 2*nc : nc));
    hipLaunchKernelGGL(k_numeric_jacobian_sparse, dim3((unsigned)(ntiles > (int)ND_MAX_GRID ? (int)ND_MAX_GRID : ntiles)),
                       dim3(ND_THREADS), lds, st, M, C, central, h->chunk, h->colptr, h->rowidx, h->entry_colour, h->d_xc, h->d_div,
                       x_dev, J_dev);
  }
  if(timed) { (void)hipEventRecord(T.ev[3], st); h->pending.push_back(T); }
  h->f_calls += 1.0; h->copies += (double)K; h->launches += 2.0;
}

int dogleg_amd_numeric_stats(struct dogleg_amd_numeric* h, double* out, int n)
{
  if(!h || !out || n <= 0) return 0;
  nd_harvest(h);
  const double v[6] = {h->invocations, h->f_calls, h->copies, h->launches, h->ms_f, h->ms_lib};
  const int m = n < 6 ? n : 6;
  for(int i = 0; i < m; i++) out[i] = v[i];
  return m;
}

int dogleg_amd_numeric_buffers(struct dogleg_amd_numeric* h, const double** p_copies_dev, const double** x_copies_dev,
                               const double** divisor_dev)
{
  if(!h) return -1;
  if(p_copies_dev) *p_copies_dev = h->d_pc;
  if(x_copies_dev) *x_copies_dev = h->d_xc;
  if(divisor_dev) *divisor_dev = h->d_div;
  return h->K;
}

} // extern "C"
