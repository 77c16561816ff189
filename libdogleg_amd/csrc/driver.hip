// driver.hip -- host trust-region driver behind the dogleg.h API.
//
// Restates the reference's control flow (dogleg.c:1172-1476 takeStepFrom /
// evaluateStep_adjustTrustRegion / runOptimizer, dogleg.c:1633-1818 entry
// points) on the host; all vector/matrix arithmetic is delegated to the HIP
// backend through dlg_backend.h.  Comparison senses, the lambda schedule, the
// un-applied terminal step and the cached-retry behaviour follow SURVEY.md 8a.
//
// Host memory handed to user callbacks (x, J, Jt arrays) is pinned
// (hipHostMalloc) so the per-evaluation upload is a straight DMA.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <new>
#include <chrono>
#include <string>
#include <vector>
#include <mutex>
#include <future>
#include <time.h>
#include "../../include/dogleg.h"
#include "../../include/dlg_backend.h"
#include "../../include/dlg_trace.h"
#include "dense_batch.h"
#include "gradcheck.h"
#include "gradcheck_plan.h"

#define MSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)
#define VERBOSE(c, ...) do { if((c)->pub.parameters->debug && !(c)->pub.parameters->debug_vnlog) MSG(__VA_ARGS__); } while(0)

namespace {

constexpr double LAMBDA_INITIAL = 1e-10;       // dogleg.c:138

const dogleg_parameters2_t k_defaults = []{
  dogleg_parameters2_t q;
  memset(&q, 0, sizeof(q));
  q.max_iterations                 = 100;      // dogleg.c:117-128
  q.trustregion0                   = 1.0e3;
  q.trustregion_decrease_factor    = 0.1;
  q.trustregion_decrease_threshold = 0.25;
  q.trustregion_increase_factor    = 2;
  q.trustregion_increase_threshold = 0.75;
  q.Jt_x_threshold                 = 1e-8;
  q.update_threshold               = 1e-8;
  q.trustregion_threshold          = 1e-8;
  return q;
}();
dogleg_parameters2_t g_params = k_defaults;    // the legacy process-global set (dogleg.c:131)

thread_local dlg_trace_t* t_trace = nullptr;

// ---- multi-GPU behind dogleg.h (include/dogleg.h, "multi-GPU"): one process -- or, in the single-GPU
// tests, one host thread -- per rank calls dogleg_optimize* with the same arguments; the communicator a
// solve uses is the calling thread's (dogleg_amd_set_communicator / _set_allreduce) or comes from the
// environment (DOGLEG_AMD_WORLD_SIZE ...: a re-linked libdogleg program under a launcher, no source change).
struct Comm
{
  int rank = 0, nranks = 1, device = -1;
  bool have_id = false; unsigned char id[128];
  dlg_allreduce_fn fn = nullptr; void* cookie = nullptr;
  bool set = false;
};
thread_local Comm t_comm;
// the environment contract: the RCCL communicator is made once per process and adopted by every solve
struct EnvComm { bool tried = false, ok = false; int rank = 0, nranks = 1, device = -1; dlg_backend_t* holder = nullptr; };
EnvComm g_env_comm;

struct Driver
{
  dogleg_solverContext_t pub;                  // MUST be first: the API hands out &pub
  dlg_backend_t* be;
  dogleg_operatingPoint_t* pts[2];             // slot id == index
  unsigned int nnz;
  bool pattern_set;
  cholmod_sparse jt[2];
  cholmod_dense  gn_dense[2];
  cholmod_factor* factor_handle;               // opaque handle handed out as ctx->factorization (heap: never a by-value
                                               // cholmod_factor, only its public fields n / minor are written)
  void* pinned[2][8];
  size_t pinned_bytes[2][8];
  int   npinned[2];
  int   be_flags;                              // the flags the backend was created with
  // trial record under construction
  dlg_trial_t cur;
  int ncallbacks;
  bool check_pattern;
  int *pat_p, *pat_i;
  bool pattern_owned;                          // device solve: Jt->p / Jt->i of the points are copies (a returned context), not the caller's arrays
  bool be_reused;                              // the backend served an earlier solve (take_parked)
  bool expect_gn;                              // the last step needed the Gauss-Newton step: issue it with the Cauchy step
  bool tail_out;                               // the expected improvement of the step just taken is still on its way (dlg_step_tail)
  // device callback: the model's kernels for the trial point and the first pass over its J went onto the stream from inside
  // the step (between_fn, dlg_backend_set_between) -- early_slot: the slot whose callback ran there (-1: none)
  int early_slot; bool no_between;
  std::future<int>* pat_check;                 // the comparison of the caller's pattern with the taken-over backend's, running beside the first evaluation
  bool failed;                                 // a backend op failed during the solve: the backend is not kept
  bool sharded;                                // this solve is one rank of several (subtree partition / row shard + all-reduces)
  int rank, nranks, row0, row1;                // its rank; dense: the contiguous rows it holds
  const int* part_rows; int part_nrows;        // sparse: the measurement rows the partition gave this rank (dlg_partition_rows)
  double *x_loc, *J_loc;                       // page-locked staging of the rank's rows of x / values of Jt (host callback)
  double *x_full_dev, *J_full_dev;             // sparse device callback on a rank: it evaluates ALL rows here, the rank's are gathered
  // device-side evaluation (dogleg_optimize_device2): the model runs on the GPU, x / J never cross PCIe
  dogleg_callback_device_t* f_device;
  const int *dev_cp, *dev_ri;                  // the caller's pattern (host), valid during the call
  // DOGLEG_AMD_TIMING=1: where the wall time of run_optimizer goes (host clock around the driver's own calls)
  bool timing;
  double tm_ms[8]; int tm_n[8];
};
enum { TM_PATTERN, TM_CALLBACK, TM_UPLOAD, TM_EVAL, TM_STEP, TM_TRACE, TM_COUNT };
thread_local double t_last_tm_ms[TM_COUNT + 1]; thread_local int t_last_tm_n[TM_COUNT + 1];      // dogleg_amd_last_solve_timing
const char* const k_tm_names[TM_COUNT] = { "pattern (symbolic phase or comparison with the parked one)", "model callback (host: evaluation; device: enqueue)",
                                           "inputs to the backend (upload / bind / gather)", "dlg_point_eval (K1 [+ K4, leaf level ahead], norms fetched)",
                                           "dlg_take_step / dlg_step (K3 .. K8, p_new fetched)", "trace / vnlog records (test harness, debug)" };
struct Tick
{
  Driver* d; int k; std::chrono::steady_clock::time_point t0;
  Tick(Driver* d_, int k_) : d(d_), k(k_) { if(d->timing) t0 = std::chrono::steady_clock::now(); }
  ~Tick() { if(d->timing) { d->tm_ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); d->tm_n[k]++; } }
};

// ---- what outlives a solve (the reference allocates and frees everything per solve, dogleg.c:1479-1562,
// 1694-1750; there a solve takes seconds -- here the set-up WAS the solve: 90 of the 100 ms of a 5-trial
// device-callback solve of config #4).  Between dogleg_optimize* calls the library keeps
//   * ONE idle backend (device buffers, streams, the uploaded pattern and schedules, hipFuncSetAttribute'd
//     kernels): the next solve of the same shape takes it over (dlg_backend_reset); a sparse solve whose
//     pattern is the one it was set up for skips the symbolic phase and every upload;
//   * the page-locked host buffers of the operating points (hipHostMalloc of 2 x 190 MB costs tens of ms).
// DOGLEG_AMD_NO_BACKEND_CACHE=1 turns both off; dogleg_amd_release_cache() frees them.
struct ParkedBackend { dlg_backend_t* be = nullptr; int type = 0, N = 0, M = 0, nnz = 0, flags = 0, device = 0; unsigned long long env = 0; };
// (a backend reads its DOGLEG_AMD_* knobs when it is created: one made under other knobs is not taken over)
extern "C" char** environ;
unsigned long long env_knobs_hash()
{
  unsigned long long h = 1469598103934665603ull;
  for(char** e = environ; e && *e; e++)
    if(!strncmp(*e, "DOGLEG_AMD_", 11) || !strncmp(*e, "DLG_", 4))
    {
      unsigned long long g = 1469598103934665603ull;
      for(const char* c = *e; *c; c++) { g ^= (unsigned char)*c; g *= 1099511628211ull; }
      h += g;                               // order-independent
    }
  return h;
}
struct PinnedBuf { void* p; size_t bytes; };
std::mutex g_cache_mu;
ParkedBackend g_parked;
std::vector<PinnedBuf> g_pinned_pool;
size_t g_pinned_pool_bytes = 0;
constexpr size_t PINNED_POOL_CAP = (size_t)4 << 30;
bool cache_on() { static const bool on = getenv("DOGLEG_AMD_NO_BACKEND_CACHE") == nullptr; return on; }

dlg_backend_t* take_parked(int type, int N, int M, int nnz, int flags, int device)
{
  // (device -1 = the calling thread's current GPU, as dlg_backend_create resolves it: a backend parked on
  // another GPU is not this solve's -- a device callback would get pointers and a stream of the wrong device)
  if(device < 0 && hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lk(g_cache_mu);
  ParkedBackend& P = g_parked;
  if(!P.be || P.type != type || P.N != N || P.M != M || P.nnz != nnz || P.flags != flags || P.device != device ||
     P.env != env_knobs_hash()) return nullptr;
  dlg_backend_t* be = P.be;
  P.be = nullptr;
  return be;
}
void park_backend(dlg_backend_t* be, int type, int N, int M, int nnz, int flags)
{
  if(!be) return;
  dlg_backend_t* old = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    old = g_parked.be;
    g_parked.be = be; g_parked.type = type; g_parked.N = N; g_parked.M = M; g_parked.nnz = nnz; g_parked.flags = flags;
    g_parked.device = dlg_backend_device(be); g_parked.env = env_knobs_hash();
  }
  if(old) dlg_backend_destroy(old);
}
void* pinned_take(size_t bytes)
{
  std::lock_guard<std::mutex> lk(g_cache_mu);
  for(size_t i = 0; i < g_pinned_pool.size(); i++)
    if(g_pinned_pool[i].bytes == bytes)
    {
      void* p = g_pinned_pool[i].p;
      g_pinned_pool_bytes -= bytes;
      g_pinned_pool[i] = g_pinned_pool.back(); g_pinned_pool.pop_back();
      return p;
    }
  return nullptr;
}
void pinned_give(void* p, size_t bytes)
{
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if(cache_on() && g_pinned_pool_bytes + bytes <= PINNED_POOL_CAP && g_pinned_pool.size() < 64)
    { g_pinned_pool.push_back({p, bytes}); g_pinned_pool_bytes += bytes; return; }
  }
  (void)hipHostFree(p);
}

inline Driver* D(dogleg_solverContext_t* ctx) { return reinterpret_cast<Driver*>(ctx); }
inline int slot_of(const Driver* d, const dogleg_operatingPoint_t* pt) { return pt == d->pts[0] ? 0 : 1; }

bool be_ok(int rc, const char* what)
{
  if(rc == DLG_OK) return true;
  MSG("%s failed: %s", what, dlg_last_error());
  return false;
}

void* pinned_alloc(Driver* d, int s, size_t bytes)
{
  void* p = nullptr;
  if(bytes == 0) bytes = 8;
  // (a buffer of an earlier solve: the large ones -- x, the arrays of Jt / J -- are written in full by the
  // callback before anything reads them; the small ones are cleared as a fresh allocation is)
  if(cache_on() && (p = pinned_take(bytes)) != nullptr) { if(bytes <= ((size_t)8 << 20)) memset(p, 0, bytes); }
  else
  {
    if(hipHostMalloc(&p, bytes) != hipSuccess) return nullptr;
    memset(p, 0, bytes);
  }
  d->pinned_bytes[s][d->npinned[s]] = bytes;
  d->pinned[s][d->npinned[s]++] = p;
  return p;
}

// ---- vnlog record (dogleg.c:42-113) ---------------------------------------
void vnlog_legend()
{
  printf("# iteration step_accepted norm2x_before norm2x_after step_len_cauchy step_len_gauss_newton "
         "step_len_interpolated k_cauchy_to_gn step_len step_type step_direction_change_deg "
         "expected_improvement observed_improvement rho trustregion_before trustregion_after\n");
}
void vn(double v) { if(std::isnan(v)) printf("- "); else printf("%g ", v); }
void vnlog_record(const Driver* d, int iteration, int accepted_flag, double len_interp)
{
  const dlg_trial_t& t = d->cur;
  static const char* names[] = { "cauchy", "gaussnewton", "interpolated" };
  printf("%d %d ", iteration, accepted_flag);
  vn(t.norm2x_before); vn(t.norm2x_after);
  vn(sqrt(t.norm2_cauchy)); vn(sqrt(t.norm2_gn));
  vn(len_interp); vn(t.k_cauchy_to_gn);
  vn(sqrt(t.norm2_step));
  printf("%s ", names[t.step_type]);
  printf("- ");                                   // direction change: never available
  vn(t.expected_improvement); vn(t.observed_improvement); vn(t.rho);
  vn(t.trustregion_before); vn(t.trustregion_after);
  printf("\n");
  fflush(stdout);
}

void cur_reset(Driver* d)
{
  memset(&d->cur, 0, sizeof(d->cur));
  d->cur.norm2x_after = d->cur.norm2_cauchy = d->cur.norm2_gn = d->cur.k_cauchy_to_gn = NAN;
  d->cur.observed_improvement = d->cur.rho = d->cur.trustregion_after = NAN;
}
void emit(Driver* d, int iteration, int accepted)
{
  Tick tt(d, TM_TRACE);
  d->cur.iteration = iteration;
  d->cur.accepted  = accepted;
  d->cur.lambda    = d->pub.lambda;
  if(d->pub.parameters->debug_vnlog)
  {
    // the terminal record prints the un-clamped expected improvement in the
    // reference; it is not retained here (trace keeps -1 as the driver sees it)
    vnlog_record(d, iteration, accepted ? 1 : 0,
                 d->cur.step_type == DLG_STEP_INTERPOLATED ? sqrt(d->cur.norm2_step) : NAN);
  }
  dlg_trace_t* tr = t_trace;
  if(tr)
  {
    if(tr->ntrials < tr->capacity)
    {
      const int N = d->pub.Nstate;
      tr->trials[tr->ntrials] = d->cur;
      if(tr->p_trial) memcpy(&tr->p_trial[(size_t)tr->ntrials*N], d->pub.afterStep->p, sizeof(double)*(size_t)N);
      if(tr->step)
        dlg_point_download(d->be, slot_of(d, d->pub.afterStep), DLG_VEC_STEP,
                           &tr->step[(size_t)tr->ntrials*N], (size_t)N);
    }
    tr->ntrials++;
  }
  cur_reset(d);
}

// ---- operating points ------------------------------------------------------
// dogleg.c:1479-1562, with the callback-visible arrays pinned
dogleg_operatingPoint_t* alloc_point(Driver* d, int s)
{
  dogleg_operatingPoint_t* pt = (dogleg_operatingPoint_t*)calloc(1, sizeof(*pt));
  if(!pt) return nullptr;
  const size_t N = (size_t)d->pub.Nstate, M = (size_t)d->pub.Nmeasurements;
  const dogleg_solve_type_t type = d->pub.solve_type;
  pt->p            = (double*)pinned_alloc(d, s, sizeof(double)*N);
  pt->Jt_x         = (double*)pinned_alloc(d, s, sizeof(double)*N);
  pt->updateCauchy = (double*)calloc(N, sizeof(double));
  pt->step_to_here = (double*)calloc(N, sizeof(double));
  double* gn       = (double*)calloc(N, sizeof(double));
  if(!pt->p || !pt->Jt_x || !pt->updateCauchy || !pt->step_to_here || !gn) return nullptr;
  if(type != DOGLEG_DENSE_PRODUCTS)
  { pt->x = (double*)pinned_alloc(d, s, sizeof(double)*M); if(!pt->x) return nullptr; }
  if(type == DOGLEG_SPARSE)
  {
    cholmod_sparse* A = &d->jt[s];
    memset(A, 0, sizeof(*A));
    A->nrow = N; A->ncol = M; A->nzmax = d->nnz;
    if(d->f_device)
    {
      // the values stay on the device and the pattern never travels from here: during the solve Jt->p / Jt->i
      // ARE the caller's arrays (copying 64 MB per point costs 10 ms each on config #4); a context that is
      // handed back gets copies of its own then (own_pattern_copies)
      A->p = const_cast<int*>(d->dev_cp);
      A->i = const_cast<int*>(d->dev_ri);
    }
    else
    {
      A->p = pinned_alloc(d, s, sizeof(int)*(M + 1));
      A->i = pinned_alloc(d, s, sizeof(int)*(size_t)d->nnz);
      A->x = pinned_alloc(d, s, sizeof(double)*(size_t)d->nnz);
      if(!A->p || !A->i || !A->x) return nullptr;
    }
    A->stype = 0; A->itype = CHOLMOD_INT; A->xtype = CHOLMOD_REAL; A->dtype = CHOLMOD_DOUBLE;
    A->sorted = 1; A->packed = 1;
    pt->Jt = A;
    cholmod_dense* g = &d->gn_dense[s];
    memset(g, 0, sizeof(*g));
    g->nrow = N; g->ncol = 1; g->nzmax = N; g->d = N; g->x = gn;
    g->xtype = CHOLMOD_REAL; g->dtype = CHOLMOD_DOUBLE;
    pt->updateGN_cholmoddense = g;
  }
  else
  {
    if(type == DOGLEG_DENSE)
    {
      if(!d->f_device) { pt->J_dense = (double*)pinned_alloc(d, s, sizeof(double)*M*N); if(!pt->J_dense) return nullptr; }
    }
    else
    {
      const size_t sz = d->pub.parameters->JtJ_packed ? N*(N+1)/2 : N*N;
      pt->JtJ = (double*)pinned_alloc(d, s, sizeof(double)*sz);
      if(!pt->JtJ) return nullptr;
    }
    pt->updateGN_dense = gn;
  }
  return pt;
}
double* gn_host(Driver* d, dogleg_operatingPoint_t* pt)
{
  return d->pub.solve_type == DOGLEG_SPARSE ? (double*)pt->updateGN_cholmoddense->x : pt->updateGN_dense;
}
void free_point(Driver* d, int s)
{
  dogleg_operatingPoint_t* pt = d->pts[s];
  if(pt)
  {
    free(pt->updateCauchy); free(pt->step_to_here);
    free(d->pub.solve_type == DOGLEG_SPARSE ? d->gn_dense[s].x : (void*)pt->updateGN_dense);
    if(d->f_device && d->pub.solve_type == DOGLEG_SPARSE && d->pattern_owned) { free(d->jt[s].p); free(d->jt[s].i); }
    free(pt);
  }
  for(int i = 0; i < d->npinned[s]; i++) pinned_give(d->pinned[s][i], d->pinned_bytes[s][i]);
  d->npinned[s] = 0;
  d->pts[s] = nullptr;
}

// the first evaluation of a sparse solve: the symbolic phase -- unless the backend was taken over from an
// earlier solve and is set up for this very pattern
bool set_pattern(Driver* d, const int* cp, const int* ri)
{
  if(d->be_reused)
  {
    if(dlg_sparse_pattern_matches(d->be, cp, ri)) return true;
    if(!be_ok(dlg_sparse_drop_pattern(d->be), "dropping the previous solve's pattern")) return false;
  }
  return be_ok(dlg_sparse_set_pattern(d->be, cp, ri), "sparse symbolic analysis");
}

// sparse, one rank of several: the rows the subtree partition gave this rank (known once the pattern is set)
// and the page-locked staging for them
bool rank_rows(Driver* d, const int* cp)
{
  if(!d->sharded || d->pub.solve_type != DOGLEG_SPARSE || d->part_rows) return true;
  if(!be_ok(dlg_partition_rows(d->be, &d->part_nrows, &d->part_rows), "partition rows")) return false;
  if(!d->part_rows) { static const int none = 0; d->part_rows = &none; }
  if(d->f_device) return true;
  size_t nv = 0;
  for(int i = 0; i < d->part_nrows; i++) nv += (size_t)(cp[d->part_rows[i] + 1] - cp[d->part_rows[i]]);
  d->x_loc = (double*)dlg_host_alloc(sizeof(double)*(size_t)(d->part_nrows ? d->part_nrows : 1));
  d->J_loc = (double*)dlg_host_alloc(sizeof(double)*(nv ? nv : 1));
  if(!d->x_loc || !d->J_loc) { MSG("out of (pinned) host memory"); return false; }
  return true;
}

// dogleg.c:1004-1083
bool eval_point(bool* converged, dogleg_operatingPoint_t* pt, Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  const int s = slot_of(d, pt);
  pt->norm2_x = -1.;
  memset(pt->dummy_bits, 0, sizeof(pt->dummy_bits));
  d->ncallbacks++;
  double norm2x = 0, absmax = 0;
  if(d->f_device)
  {
    // dogleg.c:1016-1022 with the model on the device: the callback writes x and the Jacobian
    // values straight into the slot's HBM buffers, ordered on the backend's stream
    if(ctx->solve_type == DOGLEG_SPARSE && !d->pattern_set)
    {
      Tick tk(d, TM_PATTERN);
      if(d->be_reused && !d->sharded && !d->check_pattern && getenv("DOGLEG_AMD_NO_PATTERN_OVERLAP") == nullptr)
      {
        // A backend taken over from the previous solve: whether its pattern is the caller's is 64 MB of comparison on
        // config #4 (1 ms of a 5 ms solve).  It runs on a thread of its own beside the first evaluation, which is made with
        // the backend's schedules -- if the patterns turn out to differ (below), that evaluation is thrown away: the callback's
        // x and J stay where they are, the pattern is analysed and the evaluation made again.  (Same shape, so every index the
        // stale schedules hold is inside the arrays.)
        dlg_backend_t* be = d->be; const int* cp = d->dev_cp; const int* ri = d->dev_ri;
        // (a thread that cannot be started throws: then the comparison is made in line, as without the overlap)
        try { d->pat_check = new std::future<int>(std::async(std::launch::async, [be, cp, ri] { return dlg_sparse_pattern_matches(be, cp, ri); })); }
        catch(...) { d->pat_check = nullptr; }
        if(!d->pat_check && !set_pattern(d, d->dev_cp, d->dev_ri)) return false;
      }
      else if(!set_pattern(d, d->dev_cp, d->dev_ri)) return false;
      d->pattern_set = true;
    }
    if(!rank_rows(d, d->dev_cp)) return false;
    const double* p_dev = (const double*)dlg_point_device_ptr(d->be, s, DLG_VEC_P);
    double* x_dev = (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_X_OWN);
    double* J_dev = (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_J_OWN);
    if(d->sharded && ctx->solve_type == DOGLEG_SPARSE)
    {
      // one rank of several: the callback evaluates ALL rows (its contract does not know about ranks) into
      // buffers of the full size, the rank's rows are gathered on the device
      if(!d->x_full_dev)
      {
        d->x_full_dev = (double*)dlg_mem_alloc(sizeof(double)*(size_t)ctx->Nmeasurements);
        d->J_full_dev = (double*)dlg_mem_alloc(sizeof(double)*(size_t)d->nnz);
        if(!d->x_full_dev || !d->J_full_dev) { MSG("out of device memory"); return false; }
      }
      { Tick tk(d, TM_CALLBACK); (*d->f_device)(p_dev, d->x_full_dev, d->J_full_dev, dlg_backend_get_stream(d->be), ctx->cookie); }
      Tick tu(d, TM_UPLOAD);
      if(!be_ok(dlg_point_gather_device(d->be, s, d->x_full_dev, d->J_full_dev, d->dev_cp), "gather of the rank's rows")) return false;
    }
    else
    {
      // (the callback of this point may have run already -- between_fn, from inside the step that made the point; a step
      // that was made again behind it moved the point: then it runs again)
      const bool early_cb = d->early_slot == s && !dlg_backend_between_redone(d->be);
      d->early_slot = -1;
      if(!early_cb) { Tick tk(d, TM_CALLBACK); (*d->f_device)(p_dev, x_dev, J_dev, dlg_backend_get_stream(d->be), ctx->cookie); }
      // (dense on a rank: its rows are a contiguous slice of what the callback wrote)
      const size_t r0 = d->sharded ? (size_t)d->row0 : 0;
      Tick tu(d, TM_UPLOAD);
      if(!be_ok(dlg_point_bind_device(d->be, s, x_dev + r0, J_dev + r0*(size_t)ctx->Nstate), "bind")) return false;
    }
    if(ctx->solve_type == DOGLEG_SPARSE) dlg_backend_set_speculation(d->be, d->expect_gn);
    // the model lives on the device: nothing on the host waits for p_new, and the expected improvement of a step is needed as
    // rho's denominator behind the evaluation of its trial point (dogleg.c:1410-1427; the `< 0` stop of 1403-1408 is made
    // there too, run_optimizer) -- its pass over J, if it needs one, runs beside this evaluation
    if((ctx->solve_type == DOGLEG_SPARSE || ctx->solve_type == DOGLEG_DENSE) && !d->sharded) dlg_backend_set_defer_tail(d->be, 1);
    int rc_eval;
    { Tick te(d, TM_EVAL); rc_eval = dlg_point_eval(d->be, s, &norm2x, &absmax); }
    if(d->pat_check)
    {
      int same;
      { Tick tk(d, TM_PATTERN); same = d->pat_check->get(); delete d->pat_check; d->pat_check = nullptr; }
      if(!same)
      {
        // another pattern of the same shape: what was just evaluated is void
        { Tick tk(d, TM_PATTERN);
          if(!be_ok(dlg_sparse_drop_pattern(d->be), "dropping the previous solve's pattern")) return false;
          if(!be_ok(dlg_sparse_set_pattern(d->be, d->dev_cp, d->dev_ri), "sparse symbolic analysis")) return false; }
        { Tick tu(d, TM_UPLOAD); if(!be_ok(dlg_point_bind_device(d->be, s, x_dev, J_dev), "bind")) return false; }
        dlg_backend_set_speculation(d->be, d->expect_gn);
        dlg_backend_set_defer_tail(d->be, 1);
        Tick te(d, TM_EVAL);
        rc_eval = dlg_point_eval(d->be, s, &norm2x, &absmax);
      }
    }
    if(!be_ok(rc_eval, "Jt*x")) return false;
    pt->norm2_x = norm2x;
    pt->have_x = pt->have_J = pt->have_Jtx = true;
  }
  else if(ctx->solve_type == DOGLEG_SPARSE)
  {
    { Tick tk(d, TM_CALLBACK); (*ctx->f)(pt->p, pt->x, pt->Jt, ctx->cookie); }
    const int* cp = (const int*)pt->Jt->p; const int* ri = (const int*)pt->Jt->i;
    if(!d->pattern_set)
    {
      Tick tk(d, TM_PATTERN);
      if(!set_pattern(d, cp, ri)) return false;
      d->pattern_set = true;
      if(d->check_pattern)
      {
        d->pat_p = (int*)malloc(sizeof(int)*((size_t)ctx->Nmeasurements + 1));
        d->pat_i = (int*)malloc(sizeof(int)*(size_t)d->nnz);
        memcpy(d->pat_p, cp, sizeof(int)*((size_t)ctx->Nmeasurements + 1));
        memcpy(d->pat_i, ri, sizeof(int)*(size_t)d->nnz);
      }
    }
    else if(d->check_pattern &&
            (memcmp(d->pat_p, cp, sizeof(int)*((size_t)ctx->Nmeasurements + 1)) ||
             memcmp(d->pat_i, ri, sizeof(int)*(size_t)d->nnz)))
    { MSG("the sparsity pattern of Jt changed between evaluations; it must stay fixed (reference dogleg.c:648-649)"); return false; }
    if(!rank_rows(d, cp)) return false;
    if(d->sharded)
    {
      // one rank of several: the callback evaluated all rows (its contract does not know about ranks); the
      // rank's rows -- those the subtree partition gave it, in that order -- go to the device
      const double* Jv = (const double*)pt->Jt->x;
      size_t q = 0;
      for(int i = 0; i < d->part_nrows; i++)
      {
        const int r = d->part_rows[i];
        d->x_loc[i] = pt->x[r];
        const size_t n = (size_t)(cp[r+1] - cp[r]);
        memcpy(d->J_loc + q, Jv + cp[r], sizeof(double)*n);
        q += n;
      }
      Tick tu(d, TM_UPLOAD);
      if(!be_ok(dlg_point_upload(d->be, s, d->x_loc, d->J_loc), "upload")) return false;
    }
    else
    { Tick tu(d, TM_UPLOAD); if(!be_ok(dlg_point_upload(d->be, s, pt->x, (const double*)pt->Jt->x), "upload")) return false; }
    // once steps need the Gauss-Newton step an accepted point is factorised next: its JtJ is assembled
    // beside Jt*x (an unused assembly -- a rejected point -- is simply dropped; no number changes)
    dlg_backend_set_speculation(d->be, d->expect_gn);
    { Tick te(d, TM_EVAL); if(!be_ok(dlg_point_eval(d->be, s, &norm2x, &absmax), "Jt*x")) return false; }
    pt->norm2_x = norm2x;
    pt->have_x = pt->have_J = pt->have_Jtx = true;
  }
  else if(ctx->solve_type == DOGLEG_DENSE)
  {
    { Tick tk(d, TM_CALLBACK); (*ctx->f_dense)(pt->p, pt->x, pt->J_dense, ctx->cookie); }
    // (a rank of several: its contiguous rows of what the callback wrote)
    const size_t r0 = d->sharded ? (size_t)d->row0 : 0;
    { Tick tu(d, TM_UPLOAD); if(!be_ok(dlg_point_upload(d->be, s, pt->x + r0, pt->J_dense + r0*(size_t)ctx->Nstate), "upload")) return false; }
    Tick te(d, TM_EVAL);
    if(!be_ok(dlg_point_eval(d->be, s, &norm2x, &absmax), "Jt*x")) return false;
    pt->norm2_x = norm2x;
    pt->have_x = pt->have_J = pt->have_Jtx = true;
  }
  else
  {
    { Tick tk(d, TM_CALLBACK); (*ctx->f_dense_products)(pt->p, &pt->norm2_x, pt->Jt_x, pt->JtJ, ctx->cookie); }
    { Tick tu(d, TM_UPLOAD); if(!be_ok(dlg_point_upload_products(d->be, s, pt->norm2_x, pt->Jt_x, pt->JtJ), "upload")) return false; }
    Tick te(d, TM_EVAL);
    if(!be_ok(dlg_point_eval(d->be, s, &norm2x, &absmax), "gradient norm")) return false;
    pt->have_Jtx = pt->have_JtJ = true;
  }
  // dogleg.c:1073-1082: converged unless some |Jt_x[i]| exceeds the threshold
  *converged = !(absmax > ctx->parameters->Jt_x_threshold);
  if(*converged) VERBOSE(d, "gradient below threshold everywhere: done");
  return true;
}

// dogleg.c:529-617
bool compute_cauchy(dogleg_operatingPoint_t* pt, Driver* d)
{
  if(!pt->have_updateCauchy)
  {
    if(!pt->have_Jtx) { MSG("Cauchy step needs Jt_x, which is missing"); return false; }
    double n2 = 0;
    if(!be_ok(dlg_cauchy(d->be, slot_of(d, pt), &n2), "Cauchy step")) return false;
    pt->norm2_updateCauchy = n2;
    pt->have_updateCauchy = true;
    VERBOSE(d, "cauchy step length %.6g", sqrt(n2));
  }
  d->cur.norm2_cauchy = pt->norm2_updateCauchy;
  return true;
}

// ctx->factorization of a sparse solve (dogleg.h:185-190; the reference gets it from
// cholmod_analyze, dogleg.c:650-654): an opaque, zero-filled cholmod_factor of which only the public
// fields n and minor are maintained (minor == n <=> the last factorisation succeeded, dogleg.c:667).
// The factor itself lives on the device; dogleg_amd_backend(ctx) + dlg_solve_with_factor use it.
bool publish_factor_handle(Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(ctx->solve_type != DOGLEG_SPARSE || ctx->factorization) return true;
  if(!d->factor_handle) d->factor_handle = (cholmod_factor*)calloc(1, sizeof(cholmod_factor));
  if(!d->factor_handle) { MSG("out of memory"); return false; }
  d->factor_handle->n = (size_t)ctx->Nstate; d->factor_handle->minor = 0;
  ctx->factorization = d->factor_handle;
  return true;
}
void factor_handle_ok(Driver* d)
{
  if(d->pub.solve_type == DOGLEG_SPARSE && d->factor_handle) d->factor_handle->minor = d->factor_handle->n;
}

bool factorize(dogleg_operatingPoint_t* pt, Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(pt->have_factorization) return true;                      // dogleg.c:637
  if(ctx->solve_type == DOGLEG_DENSE_PRODUCTS ? !pt->have_JtJ : !pt->have_J)
  { MSG("factorization needs J (or JtJ), which is missing"); return false; }
  if(!publish_factor_handle(d)) return false;                  // dogleg.c:650-654
  while(true)
  {
    int ok = 0;
    if(!be_ok(dlg_factorize(d->be, slot_of(d, pt), ctx->lambda, &ok), "factorization")) return false;
    if(ok) break;
    ctx->lambda = (ctx->lambda == 0.0) ? LAMBDA_INITIAL : ctx->lambda*10.0;   // dogleg.c:671-672, 812-813
    if(!std::isfinite(ctx->lambda)) { MSG("lambda overflowed while regularising a singular JtJ"); return false; }
    VERBOSE(d, "singular JtJ: adding %g I from now on", ctx->lambda);
  }
  factor_handle_ok(d);
  pt->have_factorization = true;
  return true;
}

// dogleg.c:822-908
bool compute_gn(dogleg_operatingPoint_t* pt, Driver* d)
{
  if(!pt->have_updateGN)
  {
    if(!pt->have_Jtx) { MSG("GN step needs Jt_x, which is missing"); return false; }
    double n2 = 0;
    if(!pt->have_factorization)
    {
      // factorisation (with the lambda loop, dogleg.c:656-677 / 806-815) and solve in one backend op:
      // one host synchronisation per attempt
      dogleg_solverContext_t* ctx = &d->pub;
      if(ctx->solve_type == DOGLEG_DENSE_PRODUCTS ? !pt->have_JtJ : !pt->have_J)
      { MSG("factorization needs J (or JtJ), which is missing"); return false; }
      if(!publish_factor_handle(d)) return false;                // dogleg.c:650-654
      const double lambda_before = ctx->lambda;
      if(!be_ok(dlg_gauss_newton(d->be, slot_of(d, pt), &ctx->lambda, &n2), "factorization + GN solve")) return false;
      if(ctx->lambda != lambda_before) VERBOSE(d, "singular JtJ: adding %g I from now on", ctx->lambda);
      factor_handle_ok(d);
      pt->have_factorization = true;
    }
    else if(!be_ok(dlg_solve_gn(d->be, slot_of(d, pt), &n2), "GN solve")) return false;
    pt->norm2_updateGN = n2;
    pt->have_updateGN = true;
    VERBOSE(d, "gn step length %.6g", sqrt(n2));
  }
  d->cur.norm2_gn = pt->norm2_updateGN;
  return true;
}

// A device-side model: the evaluation of the trial point (dogleg.c:1410, computeCallbackOperatingPoint) needs nothing of the
// step but p_new, which is final on the device in stream order -- its kernels, and the backend's first pass over the new
// Jacobian, go onto the stream from INSIDE the step, in front of the host's wait for the step's scalars
// (dlg_backend_set_between); eval_point then finds them there.  A step that ends the solve (dogleg.c:1289-1296) has
// evaluated one point for nothing: it is not counted and never looked at.
struct BetweenArgs { Driver* d; int slot; };
void driver_between(void* c)
{
  BetweenArgs* a = static_cast<BetweenArgs*>(c);
  Driver* d = a->d;
  const int s = a->slot;
  const double* p_dev = (const double*)dlg_point_device_ptr(d->be, s, DLG_VEC_P);
  double* x_dev = (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_X_OWN);
  double* J_dev = (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_J_OWN);
  { Tick tk(d, TM_CALLBACK); (*d->f_device)(p_dev, x_dev, J_dev, dlg_backend_get_stream(d->be), d->pub.cookie); }
  d->early_slot = s;
  if(d->pub.solve_type == DOGLEG_SPARSE)
  {
    int done = 0;
    dlg_backend_set_speculation(d->be, d->expect_gn);
    (void)dlg_point_eval_early(d->be, s, x_dev, J_dev, &done);
  }
}
bool between_ok(const Driver* d)
{
  return d->f_device && !d->sharded && !d->no_between && !d->pat_check &&
         (d->pub.solve_type == DOGLEG_DENSE || (d->pub.solve_type == DOGLEG_SPARSE && d->pattern_set));
}

// dogleg.c:1172-1297.  The step vector stays on the device (slot `to`); p_new
// comes back because the user callback needs it.
bool take_step(double* expectedImprovement, dogleg_operatingPoint_t* to,
               dogleg_operatingPoint_t* from, double trustregion, Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  Tick tstep(d, TM_STEP);
  VERBOSE(d, "taking step with trustregion %.6g", trustregion);
  d->cur.trustregion_before = trustregion;
  d->cur.norm2x_before      = from->norm2_x;
  const int sf = slot_of(d, from), st = slot_of(d, to);

  // The reference computes the Cauchy step, and the Gauss-Newton step only if the Cauchy step ends
  // inside the trust region (dogleg.c:1186-1211).  Once a step has needed both, the whole of
  // takeStepFrom for a fresh point -- both steps, the choice between them (same comparisons, made
  // on the device), the step, its expected improvement, p_new -- is ONE backend op behind one host
  // synchronisation; the values are the same, and a Gauss-Newton step the reference would not have
  // computed is discarded by the backend: neither cached nor reported, and lambda keeps its value.
  int kind;
  double n2 = 0, k = NAN, amax = 0;
  const bool fresh = !from->have_updateCauchy && !from->have_updateGN && !from->have_factorization;
  if(d->expect_gn && fresh)
  {
    if(!from->have_Jtx) { MSG("Cauchy step needs Jt_x, which is missing"); return false; }
    if(ctx->solve_type == DOGLEG_DENSE_PRODUCTS ? !from->have_JtJ : !from->have_J)
    { MSG("factorization needs J (or JtJ), which is missing"); return false; }
    double o[7];
    const double lambda_before = ctx->lambda;
    BetweenArgs ba{d, st};
    if(between_ok(d)) dlg_backend_set_between(d->be, driver_between, &ba);
    if(!be_ok(dlg_take_step(d->be, sf, st, trustregion, &ctx->lambda, o, to->p), "step")) return false;
    if(ctx->lambda != lambda_before) VERBOSE(d, "singular JtJ: adding %g I from now on", ctx->lambda);
    from->norm2_updateCauchy = o[0]; from->have_updateCauchy = true;
    d->cur.norm2_cauchy = o[0];
    VERBOSE(d, "cauchy step length %.6g", sqrt(o[0]));
    kind = (int)o[2]; n2 = o[3]; k = o[4]; amax = o[5]; *expectedImprovement = o[6];
    d->tail_out = dlg_step_tail_pending(d->be) != 0;          // (dlg_backend_set_defer_tail: run_optimizer fetches it behind the evaluation)
    if(kind != DLG_KIND_CAUCHY_TO_EDGE)
    {
      // (on the Cauchy branch the backend dropped its speculative factor and GN step and left
      // lambda alone: dogleg.c:1192-1211 never gets to compute_updateGN)
      if(!publish_factor_handle(d)) return false;                // dogleg.c:650-654
      factor_handle_ok(d);
      from->norm2_updateGN = o[1]; from->have_updateGN = true; from->have_factorization = true;
      d->cur.norm2_gn = o[1]; VERBOSE(d, "gn step length %.6g", sqrt(o[1]));
    }
    d->cur.step_type = (kind == DLG_KIND_CAUCHY_TO_EDGE) ? DLG_STEP_CAUCHY : (kind == DLG_KIND_GAUSSNEWTON ? DLG_STEP_GAUSSNEWTON : DLG_STEP_INTERPOLATED);
    from->didStepToEdgeOfTrustRegion = (kind != DLG_KIND_GAUSSNEWTON);
    d->expect_gn = (kind != DLG_KIND_CAUCHY_TO_EDGE);
  }
  else
  {
  if(!compute_cauchy(from, d)) return false;
  if(from->norm2_updateCauchy >= trustregion*trustregion)
  {
    kind = DLG_KIND_CAUCHY_TO_EDGE;
    d->cur.step_type = DLG_STEP_CAUCHY;
    from->didStepToEdgeOfTrustRegion = true;
    d->expect_gn = false;
  }
  else
  {
    if(!compute_gn(from, d)) return false;
    d->expect_gn = true;
    if(from->norm2_updateGN <= trustregion*trustregion)
    {
      kind = DLG_KIND_GAUSSNEWTON;
      d->cur.step_type = DLG_STEP_GAUSSNEWTON;
      from->didStepToEdgeOfTrustRegion = false;
    }
    else
    {
      kind = DLG_KIND_INTERPOLATED;
      d->cur.step_type = DLG_STEP_INTERPOLATED;
      from->didStepToEdgeOfTrustRegion = true;
    }
  }
  // step, its expected improvement and p_new: one backend op, one host synchronisation
  BetweenArgs ba{d, st};
  if(between_ok(d)) dlg_backend_set_between(d->be, driver_between, &ba);
  if(!be_ok(dlg_step(d->be, sf, st, kind, trustregion, &n2, &k, &amax, expectedImprovement, to->p), "step")) return false;
  d->tail_out = dlg_step_tail_pending(d->be) != 0;      // (dlg_backend_set_defer_tail: run_optimizer fetches it behind the evaluation)
  }
  to->norm2_step_to_here = n2;
  d->cur.norm2_step = n2;
  d->cur.k_cauchy_to_gn = k;
  d->cur.did_step_to_edge = from->didStepToEdgeOfTrustRegion;
  if(kind == DLG_KIND_INTERPOLATED) VERBOSE(d, "k_cauchy_to_gn %.6g, norm %.6g", k, sqrt(n2));

  // the diagnostics record the computed value, also for the terminal step whose return value is
  // replaced by -1 below (dogleg.c:1267-1269 comes before 1289-1296)
  d->cur.expected_improvement = *expectedImprovement;

  // dogleg.c:1289-1296: every |step_i| <= update_threshold -> signal termination
  if(!(amax > ctx->parameters->update_threshold))
  {
    if(d->tail_out)
    {
      // (no evaluation follows: the record of the terminal step still carries the computed value)
      d->tail_out = false;
      if(!be_ok(dlg_step_tail(d->be, expectedImprovement), "expected improvement")) return false;
      d->cur.expected_improvement = *expectedImprovement;
    }
    VERBOSE(d, "update small enough: done");
    *expectedImprovement = -1.0;
  }
  return true;
}

// dogleg.c:1303-1356
bool evaluate_step(bool* accept, double* trustregion, const dogleg_operatingPoint_t* before,
                   const dogleg_operatingPoint_t* after, double expectedImprovement, Driver* d)
{
  const dogleg_parameters2_t* prm = d->pub.parameters;
  const double observed = before->norm2_x - after->norm2_x;
  const double rho = observed / expectedImprovement;
  VERBOSE(d, "observed/expected improvement: %.6g/%.6g. rho = %.6g", observed, expectedImprovement, rho);
  d->cur.observed_improvement = observed;
  d->cur.rho = rho;
  if(rho < prm->trustregion_decrease_threshold)
  {
    if(!before->didStepToEdgeOfTrustRegion)
    {
      if(!before->have_updateGN) { MSG("internal error: GN step missing when shrinking the trust region"); return false; }
      *trustregion = sqrt(before->norm2_updateGN);
    }
    *trustregion *= prm->trustregion_decrease_factor;
  }
  else if(rho > prm->trustregion_increase_threshold && before->didStepToEdgeOfTrustRegion)
    *trustregion *= prm->trustregion_increase_factor;
  d->cur.trustregion_after = *trustregion;
  *accept = (rho > 0.0);
  return true;
}

// dogleg.c:1359-1476
int run_optimizer(Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  double trustregion = ctx->parameters->trustregion0;
  int stepCount = 0;
  cur_reset(d);

  bool converged;
  if(!eval_point(&converged, ctx->beforeStep, d)) return -1;
  if(converged) return stepCount;
  VERBOSE(d, "initial operating point has norm2_x %.6g", ctx->beforeStep->norm2_x);

  while(stepCount < ctx->parameters->max_iterations)
  {
    VERBOSE(d, "================= step %d", stepCount);
    while(true)
    {
      ctx->afterStep->have_step_to_here = false;
      double expectedImprovement;
      if(!take_step(&expectedImprovement, ctx->afterStep, ctx->beforeStep, trustregion, d)) return -1;
      ctx->afterStep->have_step_to_here = true;

      if(expectedImprovement < 0.0)                 // dogleg.c:1403-1408: step NOT applied
      { emit(d, stepCount, 2); return stepCount; }

      bool afterZeroGradient;
      if(!eval_point(&afterZeroGradient, ctx->afterStep, d)) return -1;
      VERBOSE(d, "evaluated operating point with norm2_x %.6g", ctx->afterStep->norm2_x);
      d->cur.norm2x_after = ctx->afterStep->norm2_x;
      if(d->tail_out)
      {
        d->tail_out = false;
        Tick tt(d, TM_STEP);
        if(!be_ok(dlg_step_tail(d->be, &expectedImprovement), "expected improvement")) return -1;
        d->cur.expected_improvement = expectedImprovement;
        // dogleg.c:1403-1408, made where the value is first at hand: the reference tests it in FRONT of the evaluation and
        // stops with the step not applied; here the trial point has been evaluated meanwhile (one callback more than the
        // reference makes) and is discarded -- evaluate_step must never divide by a negative expected improvement
        if(expectedImprovement < 0.0) { emit(d, stepCount, 2); return stepCount; }
      }

      bool accept;
      if(!evaluate_step(&accept, &trustregion, ctx->beforeStep, ctx->afterStep, expectedImprovement, d))
        return -1;

      if(accept)
      {
        VERBOSE(d, "accepted step");
        emit(d, stepCount, 1);
        stepCount++;
        dogleg_operatingPoint_t* t = ctx->afterStep;
        ctx->afterStep = ctx->beforeStep;
        ctx->beforeStep = t;
        if(afterZeroGradient) { VERBOSE(d, "gradient low enough after an improving step: done"); return stepCount; }
        break;
      }
      VERBOSE(d, "rejected step");
      emit(d, stepCount, 0);
      if(trustregion < ctx->parameters->trustregion_threshold)
      { VERBOSE(d, "trust region below threshold: giving up"); return stepCount; }
    }
  }
  if(stepCount == ctx->parameters->max_iterations) VERBOSE(d, "iteration limit reached");
  return stepCount;
}

// bring the host mirrors of a point up to date (returnContext contract,
// SURVEY.md 3.4): Jt_x, updateCauchy, updateGN, step_to_here
void sync_point_to_host(Driver* d, dogleg_operatingPoint_t* pt)
{
  const int s = slot_of(d, pt);
  const size_t N = (size_t)d->pub.Nstate;
  if(pt->have_Jtx && d->pub.solve_type != DOGLEG_DENSE_PRODUCTS)
    dlg_point_download(d->be, s, DLG_VEC_JTX, pt->Jt_x, N);
  if(pt->have_updateCauchy) dlg_point_download(d->be, s, DLG_VEC_CAUCHY, pt->updateCauchy, N);
  if(pt->have_updateGN)     dlg_point_download(d->be, s, DLG_VEC_GN, gn_host(d, pt), N);
  dlg_point_download(d->be, s, DLG_VEC_STEP, pt->step_to_here, N);
  if(d->f_device && pt->have_x) dlg_point_download(d->be, s, DLG_VEC_X, pt->x, (size_t)d->pub.Nmeasurements);
}

// a device solve whose context outlives the call: the points' Jt->p / Jt->i must not point into the caller's arrays
bool own_pattern_copies(Driver* d)
{
  if(d->pattern_owned) return true;
  const size_t M = (size_t)d->pub.Nmeasurements;
  int* cp[2] = {nullptr, nullptr}; int* ri[2] = {nullptr, nullptr};
  for(int s = 0; s < 2; s++)
  {
    cp[s] = (int*)malloc(sizeof(int)*(M + 1));
    ri[s] = (int*)malloc(sizeof(int)*(size_t)(d->nnz ? d->nnz : 1));
    if(!cp[s] || !ri[s]) { for(int k = 0; k <= s; k++) { free(cp[k]); free(ri[k]); } return false; }
    memcpy(cp[s], d->dev_cp, sizeof(int)*(M + 1));
    memcpy(ri[s], d->dev_ri, sizeof(int)*(size_t)d->nnz);
  }
  for(int s = 0; s < 2; s++) { d->jt[s].p = cp[s]; d->jt[s].i = ri[s]; }
  d->pattern_owned = true;
  d->dev_cp = d->dev_ri = nullptr;
  return true;
}

void destroy(Driver* d)
{
  if(!d) return;
  if(d->pat_check) { (void)d->pat_check->get(); delete d->pat_check; d->pat_check = nullptr; }      // (it reads the backend's pattern)
  free_point(d, 0); free_point(d, 1);
  if(d->pub.solve_type != DOGLEG_SPARSE) free(d->pub.factorization_dense);
  if(d->x_full_dev) dlg_mem_free(d->x_full_dev);
  if(d->J_full_dev) dlg_mem_free(d->J_full_dev);
  if(d->x_loc) dlg_host_free(d->x_loc);
  if(d->J_loc) dlg_host_free(d->J_loc);
  if(d->be)
  {
    // (a backend that is one rank of several holds its communicator and partition: not kept)
    if(cache_on() && !d->sharded && !d->failed && dlg_backend_reset(d->be) == DLG_OK)
      park_backend(d->be, (int)d->pub.solve_type, d->pub.Nstate, d->pub.Nmeasurements, (int)d->nnz, d->be_flags);
    else dlg_backend_destroy(d->be);
  }
  free(d->factor_handle);
  free(d->pat_p); free(d->pat_i);
  free(d);
}

// ---- the id file of the environment contract.  144 bytes: the 128-byte RCCL id, the tag "DLGAMD01", and the
// 64-bit FNV-1a hash of the launch's run id (DOGLEG_AMD_RUN_ID, else TORCHELASTIC_RUN_ID, else empty).  A reader takes
// only a complete file whose run id is its own: a file an earlier launch left at the path under another run id is
// skipped (under the SAME run id -- or none -- the path has to be fresh for each launch; rank 0 removes what it finds
// before it makes the id, which narrows that window, it cannot close it).  Written as tmp + rename: never seen half.
unsigned long long run_id_hash(const char* run_id)
{
  unsigned long long g = 1469598103934665603ull;
  for(const char* c = run_id ? run_id : ""; *c; c++) { g ^= (unsigned char)*c; g *= 1099511628211ull; }
  return g;
}
const char* env_run_id()
{
  const char* r = getenv("DOGLEG_AMD_RUN_ID");
  if(!r) r = getenv("TORCHELASTIC_RUN_ID");
  return r ? r : "";
}
constexpr size_t ID_FILE_BYTES = 144;
} // namespace
extern "C" int dogleg_amd_id_file_publish(const char* path, const void* id128, const char* run_id)
{
  if(!path || !id128) { MSG("dogleg_amd_id_file_publish: bad arguments"); return -1; }
  unsigned char rec[ID_FILE_BYTES];
  memcpy(rec, id128, 128); memcpy(rec + 128, "DLGAMD01", 8);
  const unsigned long long h = run_id_hash(run_id);
  memcpy(rec + 136, &h, 8);
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if(!f || fwrite(rec, 1, ID_FILE_BYTES, f) != ID_FILE_BYTES) { MSG("cannot write %s", tmp.c_str()); if(f) fclose(f); return -1; }
  if(fclose(f) != 0) { MSG("cannot write %s", tmp.c_str()); return -1; }
  if(rename(tmp.c_str(), path) != 0) { MSG("cannot rename %s to %s", tmp.c_str(), path); return -1; }
  return 0;
}
extern "C" int dogleg_amd_id_file_wait(const char* path, void* id128_out, const char* run_id, int timeout_ms)
{
  if(!path || !id128_out) { MSG("dogleg_amd_id_file_wait: bad arguments"); return -1; }
  const unsigned long long want = run_id_hash(run_id);
  const auto t0 = std::chrono::steady_clock::now();
  for(;;)
  {
    unsigned char rec[ID_FILE_BYTES + 1];
    FILE* f = fopen(path, "rb");
    if(f)
    {
      const size_t n = fread(rec, 1, sizeof(rec), f);
      fclose(f);
      unsigned long long h = 0;
      if(n == ID_FILE_BYTES) memcpy(&h, rec + 136, 8);
      if(n == ID_FILE_BYTES && !memcmp(rec + 128, "DLGAMD01", 8) && h == want) { memcpy(id128_out, rec, 128); return 0; }
    }
    if(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() >= (double)timeout_ms) break;
    struct timespec ts = {0, 20000000}; nanosleep(&ts, nullptr);
  }
  MSG("no RCCL id of this launch in %s after %d ms", path, timeout_ms);
  return -1;
}
namespace {

// DOGLEG_AMD_WORLD_SIZE (> 1), DOGLEG_AMD_RANK, DOGLEG_AMD_LOCAL_RANK (the GPU; default: the rank),
// DOGLEG_AMD_RCCL_ID_FILE: rank 0 writes the RCCL id there (dogleg_amd_id_file_publish), the others wait for it
// (dogleg_amd_id_file_wait, two minutes; DOGLEG_AMD_RUN_ID names the launch).  The communicator is made once per
// process -- a backend that only holds it -- and shared by every solve; solves may start on several threads.
std::mutex g_env_comm_mu;
bool env_communicator(Comm* cm)
{
  std::lock_guard<std::mutex> lk(g_env_comm_mu);
  EnvComm& E = g_env_comm;
  if(!E.tried)
  {
    E.tried = true;
    const char* ws = getenv("DOGLEG_AMD_WORLD_SIZE");
    const int n = ws ? atoi(ws) : 1;
    if(n > 1 || (ws && getenv("DOGLEG_AMD_FORCE_COMM")))
    {
      const char* rk = getenv("DOGLEG_AMD_RANK"); const char* lr = getenv("DOGLEG_AMD_LOCAL_RANK");
      const char* idf = getenv("DOGLEG_AMD_RCCL_ID_FILE");
      if(!rk || !idf) { MSG("DOGLEG_AMD_WORLD_SIZE=%d needs DOGLEG_AMD_RANK and DOGLEG_AMD_RCCL_ID_FILE", n); return false; }
      E.rank = atoi(rk); E.nranks = n; E.device = lr ? atoi(lr) : E.rank;
      if(E.rank < 0 || E.rank >= n) { MSG("DOGLEG_AMD_RANK=%d of %d", E.rank, n); return false; }
      unsigned char id[128];
      if(E.rank == 0)
      {
        (void)remove(idf);                          // (what an earlier launch left there)
        if(dlg_rccl_unique_id(id) != DLG_OK) { MSG("RCCL id: %s", dlg_last_error()); return false; }
        if(dogleg_amd_id_file_publish(idf, id, env_run_id()) != 0) return false;
      }
      else if(dogleg_amd_id_file_wait(idf, id, env_run_id(), 120000) != 0) return false;
      // (a backend with nothing in it but the communicator: dlg_backend_share_rccl hands it to the solves)
      if(dlg_backend_create(&E.holder, DLG_DENSE_PRODUCTS, 1, 0, 0, 0, E.device) != DLG_OK ||
         dlg_backend_init_rccl(E.holder, E.rank, E.nranks, id) != DLG_OK)
      { MSG("cannot make the process's RCCL communicator: %s", dlg_last_error()); return false; }
      E.ok = true;
    }
  }
  if(E.tried && !E.ok && getenv("DOGLEG_AMD_WORLD_SIZE") && atoi(getenv("DOGLEG_AMD_WORLD_SIZE")) > 1) return false;
  if(E.ok) { cm->rank = E.rank; cm->nranks = E.nranks; cm->device = E.device; cm->set = true; }
  return true;
}

// dogleg.c:1633-1753
double optimize(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                dogleg_callback_t* f, dogleg_callback_dense_t* f_dense,
                dogleg_callback_dense_products_t* f_products, void* cookie,
                const dogleg_parameters2_t* parameters, dogleg_solverContext_t** returnContext,
                dogleg_callback_device_t* f_device = nullptr, const int* dev_cp = nullptr,
                const int* dev_ri = nullptr)
{
  Driver* d = (Driver*)calloc(1, sizeof(Driver));
  if(!d) { MSG("out of memory"); return -1.0; }
  d->f_device = f_device; d->dev_cp = dev_cp; d->dev_ri = dev_ri;
  d->early_slot = -1; d->no_between = getenv("DOGLEG_AMD_NO_BETWEEN") != nullptr;
  dogleg_solverContext_t* ctx = &d->pub;
  ctx->cookie = cookie;
  ctx->lambda = 0.0;
  ctx->Nstate = (int)Nstate;
  ctx->Nmeasurements = (int)Nmeas;
  ctx->parameters = parameters ? parameters : &g_params;
  d->nnz = NJnnz;
  const char* chk = getenv("DOGLEG_AMD_CHECK_PATTERN");
  d->check_pattern = chk && chk[0] == '1';

  if(f_device)
  {
    // ctx->f stays NULL: the device callback has another signature and lives in the driver
    if(NJnnz > 0)
    {
      ctx->solve_type = DOGLEG_SPARSE;
      if(!dev_cp || !dev_ri) { MSG("a sparse device solve needs the pattern of Jt"); free(d); return -1.0; }
      if(dev_cp[0] != 0 || dev_cp[Nmeas] != (int)NJnnz)
      { MSG("the pattern has %d entries, NJnnz says %u", dev_cp[Nmeas], NJnnz); free(d); return -1.0; }
    }
    else ctx->solve_type = DOGLEG_DENSE;
  }
  else if(f)
  {
    ctx->solve_type = DOGLEG_SPARSE; ctx->f = f;
    if(NJnnz == 0) { MSG("sparse solves need NJnnz > 0"); free(d); return -1.0; }
  }
  else if(f_dense)
  {
    ctx->solve_type = DOGLEG_DENSE; ctx->f_dense = f_dense;
    if(NJnnz > 0) { MSG("dense solves need NJnnz == 0"); free(d); return -1.0; }
  }
  else if(f_products)
  {
    ctx->solve_type = DOGLEG_DENSE_PRODUCTS; ctx->f_dense_products = f_products;
    if(NJnnz > 0) { MSG("dense solves need NJnnz == 0"); free(d); return -1.0; }
  }
  else { MSG("exactly one of the callbacks must be given"); free(d); return -1.0; }

  if(ctx->parameters->debug_vnlog) vnlog_legend();
  // DOGLEG_AMD_TIMING=1: wall time of the phases of a solve on stderr (where an end-to-end call spends its time)
  const bool timing = getenv("DOGLEG_AMD_TIMING") != nullptr;
  d->timing = timing;
  const auto t_begin = std::chrono::steady_clock::now();
  auto t_last = t_begin;
  auto lap = [&](const char* what) {
    if(!timing) return;
    const auto now = std::chrono::steady_clock::now();
    MSG("timing: %-34s %8.2f ms", what, std::chrono::duration<double, std::milli>(now - t_last).count());
    t_last = now; };

  int flags = 0;
  if(ctx->parameters->JtJ_packed) flags |= DLG_FLAG_JTJ_PACKED;
  if(ctx->parameters->JtJ_upper)  flags |= DLG_FLAG_JTJ_UPPER;
  // this solve's communicator: the calling thread's, else the environment's, else none (one GPU)
  Comm cm = t_comm;
  if(!cm.set && !env_communicator(&cm)) { free(d); return -1.0; }
  d->be_flags = flags;
  if(cache_on() && !cm.set) d->be = take_parked((int)ctx->solve_type, (int)Nstate, (int)Nmeas, (int)NJnnz, flags, cm.device);
  if(d->be) { d->be_reused = true; lap("backend taken over from the previous solve"); }
  else
  {
    if(dlg_backend_create(&d->be, (int)ctx->solve_type, (int)Nstate, (int)Nmeas, (int)NJnnz, flags, cm.device) != DLG_OK)
    { MSG("cannot create the GPU backend: %s", dlg_last_error()); free(d); return -1.0; }
    lap("backend create (device buffers)");
  }
  d->rank = cm.rank; d->nranks = cm.nranks; d->row0 = 0; d->row1 = (int)Nmeas;
  if(cm.set && ctx->solve_type != DOGLEG_DENSE_PRODUCTS)
  {
    // Measurement rows are the sharded unit (dogleg.c:253-260, 269-278, 712-714).  Sparse: the subtree
    // partition of the elimination tree; dense: contiguous rows, JtJ summed.  (dense-products: the
    // callback has already summed over the rows -- every rank does the same work: replicas.)
    bool ok = true;
    if(ctx->solve_type == DOGLEG_SPARSE) ok = be_ok(dlg_backend_set_partition(d->be, cm.rank, cm.nranks), "subtree partition");
    else
    {
      d->row0 = (int)((long)Nmeas*cm.rank/cm.nranks); d->row1 = (int)((long)Nmeas*(cm.rank + 1)/cm.nranks);
      ok = be_ok(dlg_backend_set_shard(d->be, d->row0, d->row1, nullptr, nullptr), "row shard");
    }
    if(ok && g_env_comm.ok && g_env_comm.holder && !cm.have_id && !cm.fn)
      ok = be_ok(dlg_backend_share_rccl(d->be, g_env_comm.holder), "RCCL communicator of the process");
    else if(ok && cm.have_id) ok = be_ok(dlg_backend_init_rccl(d->be, cm.rank, cm.nranks, cm.id), "RCCL communicator");
    else if(ok && cm.fn)      ok = be_ok(dlg_backend_set_allreduce(d->be, cm.fn, cm.cookie), "all-reduce hook");
    else if(ok) { MSG("a communicator of %d ranks needs an RCCL id or an all-reduce hook", cm.nranks); ok = false; }
    if(!ok) { destroy(d); return -1.0; }
    d->sharded = true;
    lap("communicator");
  }

  if(ctx->solve_type != DOGLEG_SPARSE)
  {
    const size_t N = Nstate;
    const size_t sz = (ctx->solve_type == DOGLEG_DENSE || ctx->parameters->JtJ_packed) ? N*(N+1)/2 : N*N;
    ctx->factorization_dense = (double*)calloc(sz, sizeof(double));          // dogleg.c:1707-1725
    if(!ctx->factorization_dense) { MSG("out of memory"); destroy(d); return -1.0; }
  }
  d->pts[0] = alloc_point(d, 0);
  d->pts[1] = alloc_point(d, 1);
  if(!d->pts[0] || !d->pts[1]) { MSG("out of (pinned) host memory"); destroy(d); return -1.0; }
  ctx->beforeStep = d->pts[0];
  ctx->afterStep  = d->pts[1];
  lap("operating points (pinned host)");

  memcpy(ctx->beforeStep->p, p, sizeof(double)*Nstate);
  if(!be_ok(dlg_point_set_p(d->be, 0, ctx->beforeStep->p), "upload of p")) { destroy(d); return -1.0; }

  dlg_trace_t* tr = t_trace;
  if(tr) { tr->ntrials = 0; tr->ncallbacks = 0; tr->nstate = (int)Nstate; }

  const auto t_run = std::chrono::steady_clock::now();
  const int numsteps = run_optimizer(d);
  if(timing)
  {
    // where run_optimizer's wall time went: the driver's own calls, host clock (one line for all of it hid 6 ms)
    const double run_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_run).count();
    double acc = 0;
    for(int k = 0; k < TM_COUNT; k++)
    {
      if(d->tm_n[k]) MSG("timing:   %-62s %8.3f ms in %2d calls (%7.3f ms each)", k_tm_names[k], d->tm_ms[k], d->tm_n[k], d->tm_ms[k]/d->tm_n[k]);
      acc += d->tm_ms[k];
    }
    MSG("timing:   %-62s %8.3f ms", "host logic between them (trust region, bookkeeping)", run_ms - acc);
    for(int k = 0; k < TM_COUNT; k++) { t_last_tm_ms[k] = d->tm_ms[k]; t_last_tm_n[k] = d->tm_n[k]; }
    t_last_tm_ms[TM_COUNT] = run_ms; t_last_tm_n[TM_COUNT] = 1;
  }
  lap("run_optimizer (incl. symbolic phase)");
  const double norm2_x = ctx->beforeStep->norm2_x;
  if(tr) tr->ncallbacks = d->ncallbacks;
  if(numsteps < 0)
  {
    MSG("the solve failed");
    d->failed = true;
    destroy(d);
    return -1.0;
  }
  memcpy(p, ctx->beforeStep->p, sizeof(double)*Nstate);        // dogleg.c:1745
  VERBOSE(d, "success: %d iterations", numsteps);

  if(returnContext)
  {
    if(d->f_device && ctx->solve_type == DOGLEG_SPARSE && !own_pattern_copies(d)) { MSG("out of memory"); destroy(d); return -1.0; }
    sync_point_to_host(d, ctx->beforeStep);
    if(ctx->solve_type != DOGLEG_SPARSE && ctx->beforeStep->have_factorization)
    {
      const size_t N = Nstate;
      const size_t sz = (ctx->solve_type == DOGLEG_DENSE || ctx->parameters->JtJ_packed) ? N*(N+1)/2 : N*N;
      dlg_factor_download_dense(d->be, ctx->factorization_dense, sz);
    }
    *returnContext = ctx;
  }
  else destroy(d);
  lap("teardown");
  return norm2_x;
}

} // namespace

// ============================================================ public API ====
extern "C" {

void dlg_set_trace(void* tr) { t_trace = (dlg_trace_t*)tr; }

void dogleg_getDefaultParameters(dogleg_parameters2_t* parameters) { *parameters = k_defaults; }

// dogleg.c:140-181
void dogleg_setDebug(int debug)
{
  if(debug == 0)                       { g_params.debug = false; g_params.debug_vnlog = false; }
  else if(debug & DOGLEG_DEBUG_VNLOG)  { g_params.debug = false; g_params.debug_vnlog = true;  }
  else                                 { g_params.debug = true;  g_params.debug_vnlog = false; }
}
void dogleg_setInitialTrustregion(double t) { g_params.trustregion0 = t; }
void dogleg_setThresholds(double Jt_x, double update, double trustregion)
{
  if(Jt_x > 0.0)        g_params.Jt_x_threshold        = Jt_x;
  if(update > 0.0)      g_params.update_threshold      = update;
  if(trustregion > 0.0) g_params.trustregion_threshold = trustregion;
}
void dogleg_setMaxIterations(int n) { g_params.max_iterations = n; }
void dogleg_setTrustregionUpdateParameters(double downFactor, double downThreshold,
                                           double upFactor, double upThreshold)
{
  g_params.trustregion_decrease_factor    = downFactor;
  g_params.trustregion_decrease_threshold = downThreshold;
  g_params.trustregion_increase_factor    = upFactor;
  g_params.trustregion_increase_threshold = upThreshold;
}

double dogleg_optimize2(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                        dogleg_callback_t* f, void* cookie,
                        const dogleg_parameters2_t* parameters,
                        dogleg_solverContext_t** returnContext)
{
  if(NJnnz == 0) { MSG("NJnnz must be > 0, got %u", NJnnz); return -1.0; }      // dogleg.c:1762-1766
  return optimize(p, Nstate, Nmeas, NJnnz, f, nullptr, nullptr, cookie, parameters, returnContext);
}
double dogleg_optimize(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                       dogleg_callback_t* f, void* cookie, dogleg_solverContext_t** returnContext)
{
  return dogleg_optimize2(p, Nstate, Nmeas, NJnnz, f, cookie, nullptr, returnContext);
}
double dogleg_optimize_dense2(double* p, unsigned int Nstate, unsigned int Nmeas,
                              dogleg_callback_dense_t* f, void* cookie,
                              const dogleg_parameters2_t* parameters,
                              dogleg_solverContext_t** returnContext)
{
  return optimize(p, Nstate, Nmeas, 0, nullptr, f, nullptr, cookie, parameters, returnContext);
}
double dogleg_optimize_dense(double* p, unsigned int Nstate, unsigned int Nmeas,
                             dogleg_callback_dense_t* f, void* cookie,
                             dogleg_solverContext_t** returnContext)
{
  return dogleg_optimize_dense2(p, Nstate, Nmeas, f, cookie, nullptr, returnContext);
}
double dogleg_optimize_device2(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                               const int* Jt_colptr, const int* Jt_rowidx,
                               dogleg_callback_device_t* f, void* cookie,
                               const dogleg_parameters2_t* parameters,
                               dogleg_solverContext_t** returnContext)
{
  if(!f) { MSG("dogleg_optimize_device2 needs a device callback"); return -1.0; }
  return optimize(p, Nstate, Nmeas, NJnnz, nullptr, nullptr, nullptr, cookie, parameters, returnContext,
                  f, Jt_colptr, Jt_rowidx);
}
double dogleg_optimize_dense_products(double* p, unsigned int Nstate,
                                      dogleg_callback_dense_products_t* f, void* cookie,
                                      const dogleg_parameters2_t* parameters,
                                      dogleg_solverContext_t** returnContext)
{
  return optimize(p, Nstate, 0, 0, nullptr, nullptr, f, cookie, parameters, returnContext);
}

// dogleg.h:304-310: make sure the factor of JtJ at `point` is held
bool dogleg_computeJtJfactorization(dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  Driver* d = D(ctx);
  if(!factorize(point, d)) return false;
  if(ctx->solve_type != DOGLEG_SPARSE)
  {
    const size_t N = (size_t)ctx->Nstate;
    const size_t sz = (ctx->solve_type == DOGLEG_DENSE || ctx->parameters->JtJ_packed) ? N*(N+1)/2 : N*N;
    if(dlg_factor_download_dense(d->be, ctx->factorization_dense, sz) != DLG_OK) return false;
  }
  return true;
}

// ---- outliers (dogleg.h; reference dogleg.c:2294-3149).  The leverage blocks come from the device (dlg_backend.h:
// dlg_feature_leverage); what is left here is the host logic around them.
} // extern "C"
namespace {
bool outlier_ready(dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx, const char* who)
{
  if(!point || !ctx) { MSG("%s(): no point or context", who); return false; }
  if(!point->have_x) { MSG("%s() needs x, but it isn't available", who); return false; }
  if(!point->have_J) { MSG("%s() needs J, but it isn't available", who); return false; }
  if(ctx->solve_type == DOGLEG_DENSE_PRODUCTS) { MSG("%s() is not available with DENSE_PRODUCTS: there is no J", who); return false; }
  return dogleg_computeJtJfactorization(point, ctx);
}
// a backend call that needs the factor of the point's slot: if the factor held is another slot's, factorise again and retry
template <class F> bool with_point_factor(dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx, const char* what, F call)
{
  int rc = call();
  if(rc == DLG_ERR_STATE)
  {
    point->have_factorization = false;
    if(!dogleg_computeJtJfactorization(point, ctx)) return false;
    rc = call();
  }
  return be_ok(rc, what);
}
// *scale <= 0: Nn / (4 (Nstate + 1) |x|^2 / (Nn - Nstate - 1)), Nn the measurements that are not outliers
void outlier_scale(double* scale, const dogleg_solverContext_t* ctx, int NoutlierFeatures, int featureSize, double norm2_x)
{
  if(*scale > 0.0) return;
  const int nn = ctx->Nmeasurements - NoutlierFeatures*featureSize;
  *scale = (double)nn / (4.0*((double)(ctx->Nstate + 1)*norm2_x/(double)(nn - ctx->Nstate - 1)));
}
} // namespace
extern "C" {

bool dogleg_getOutliernessFactors(double* factors, double* scale, int featureSize, int Nfeatures,
                                  int NoutlierFeatures, dogleg_operatingPoint_t* point,
                                  dogleg_solverContext_t* ctx)
{
  if(featureSize <= 1) featureSize = 1;
  if(featureSize > 2) { MSG("dogleg_getOutliernessFactors(): featureSize > 2 is not implemented (got %d)", featureSize); return false; }
  if(!factors || !scale || Nfeatures < 0) { MSG("dogleg_getOutliernessFactors(): bad arguments"); return false; }
  if(!outlier_ready(point, ctx, "dogleg_getOutliernessFactors")) return false;
  if((long)Nfeatures*featureSize > (long)ctx->Nmeasurements)
  { MSG("dogleg_getOutliernessFactors(): %d features of size %d exceed %d measurements", Nfeatures, featureSize, ctx->Nmeasurements); return false; }
  outlier_scale(scale, ctx, NoutlierFeatures, featureSize, point->norm2_x);
  Driver* d = D(ctx);
  const double sc = *scale;
  return with_point_factor(point, ctx, "outlierness factors",
                           [&]{ return dlg_outlierness_factors(d->be, slot_of(d, point), featureSize, Nfeatures, sc, factors); });
}

bool dogleg_markOutliers(struct dogleg_outliers_t* markedOutliers, double* scale, int* Noutliers,
                         double (getConfidence)(int i_feature_exclude), int featureSize, int Nfeatures,
                         dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  if(featureSize <= 1) featureSize = 1;
  if(!markedOutliers || !Noutliers || !getConfidence || Nfeatures < 0) { MSG("dogleg_markOutliers(): bad arguments"); return false; }
  std::vector<double> factors((size_t)Nfeatures);
  if(!dogleg_getOutliernessFactors(factors.data(), scale, featureSize, Nfeatures, *Noutliers, point, ctx)) return false;
  // candidates have a factor of at least 1; one is an outlier if leaving it out costs little confidence
  const double confidence0 = getConfidence(-1);
  if(confidence0 < 0.0) return false;
  Driver* d = D(ctx);
  VERBOSE(d, "Initial confidence: %g", confidence0);
  bool markedAny = false;
  *Noutliers = 0;
  for(int i = 0; i < Nfeatures; i++)
  {
    if(markedOutliers[i].marked) { (*Noutliers)++; continue; }
    if(factors[i] < 1.0) continue;
    const double confidence = getConfidence(i);
    if(confidence < 0.0) return false;
    const double drop = 1.0 - confidence/confidence0;
    if(drop < 0.05)
    {
      markedOutliers[i].marked = 1;
      markedAny = true;
      (*Noutliers)++;
      VERBOSE(d, "Feature %d has outlierness factor %f. Culling produces a confidence: %g. relative loss: %g... YES an outlier; confidence drops little",
              i, factors[i], confidence, drop);
    }
    else
      VERBOSE(d, "Feature %d has outlierness factor %f. Culling produces a confidence: %g. relative loss: %g... NOT an outlier: confidence drops too much",
              i, factors[i], confidence, drop);
  }
  return markedAny;
}

void dogleg_reportOutliers(double (getConfidence)(int i_feature_exclude), double* scale, int featureSize,
                           int Nfeatures, int Noutliers, dogleg_operatingPoint_t* point,
                           dogleg_solverContext_t* ctx)
{
  if(featureSize <= 1) featureSize = 1;
  if(!getConfidence || Nfeatures < 0) { MSG("dogleg_reportOutliers(): bad arguments"); return; }
  std::vector<double> factors((size_t)Nfeatures, 0.0);
  (void)dogleg_getOutliernessFactors(factors.data(), scale, featureSize, Nfeatures, Noutliers, point, ctx);   // (a failure is reported, not fatal)
  MSG("## Outlier statistics");
  MSG("# i_feature outlier_factor confidence_drop_relative_if_removed");
  const double confidence_full = getConfidence(-1);
  for(int i = 0; i < Nfeatures; i++)
  {
    const double confidence = getConfidence(i);
    MSG("%5d %9.3g %9.3g", i, factors[i], 1.0 - confidence/confidence_full);
  }
}

double dogleg_getOutliernessTrace_newFeature_sparse(const double* JqueryFeature, int istateActive,
                                                    int NstateActive, int featureSize, int NoutlierFeatures,
                                                    dogleg_operatingPoint_t* point,
                                                    dogleg_solverContext_t* ctx)
{
  const char* who = "dogleg_getOutliernessTrace_newFeature_sparse";
  if(point && !point->have_x) { MSG("%s() needs x, but it isn't available", who); return -1.0; }
  if(point && !point->have_J) { MSG("%s() needs J, but it isn't available", who); return -1.0; }
  if(featureSize != 2) { MSG("%s(): only featureSize 2 is implemented (got %d)", who, featureSize); return -1.0; }
  if(!JqueryFeature || NstateActive < 1) { MSG("%s(): bad arguments", who); return -1.0; }
  if(!outlier_ready(point, ctx, who)) return -1.0;
  Driver* d = D(ctx);
  double A[3];
  if(!with_point_factor(point, ctx, "leverage of a query feature",
                        [&]{ return dlg_leverage_query(d->be, slot_of(d, point), JqueryFeature, istateActive, NstateActive, 2, A); }))
    return -1.0;
  // Mq = I + A; tr Mq^-1 = tr(Mq) / det(Mq)
  const double m00 = 1.0 + A[0], m01 = A[1], m11 = 1.0 + A[2];
  const double trace_inv = (m00 + m11)/(m00*m11 - m01*m01);
  double scale = -1.0;
  outlier_scale(&scale, ctx, NoutlierFeatures, featureSize, point->norm2_x);
  return scale*(2.0 - trace_inv);
}

// ---- extension (not in the reference): covariance blocks from the factor held on the device (dlg_backend.h:
// dlg_covariance_blocks).  What the reference's users get from cholmod_solve on ctx->factorization with unit right-hand sides.
} // extern "C"
namespace {
bool cov_ready(dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx, const char* who)
{
  if(!point || !ctx) { MSG("%s(): no point or context", who); return false; }
  const Driver* d = D(ctx);
  if(d->sharded && d->nranks > 1) { MSG("%s() works on one rank only (this context has %d)", who, d->nranks); return false; }
  return dogleg_computeJtJfactorization(point, ctx);
}
} // namespace
extern "C" {

int dogleg_amd_covariance_blocks(double* out, int nreq, const int* r0, const int* nr, const int* c0, const int* nc,
                                 dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  const char* who = "dogleg_amd_covariance_blocks";
  if(nreq < 0 || (nreq > 0 && (!out || !r0 || !nr || !c0 || !nc))) { MSG("%s(): bad arguments", who); return -1; }
  if(!cov_ready(point, ctx, who)) return -1;
  Driver* d = D(ctx);
  return with_point_factor(point, ctx, "covariance blocks",
                           [&]{ return dlg_covariance_blocks(d->be, slot_of(d, point), nreq, r0, nr, c0, nc, out); }) ? 0 : -1;
}

int dogleg_amd_marginal_variances(double* var, dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  const char* who = "dogleg_amd_marginal_variances";
  if(!var) { MSG("%s(): bad arguments", who); return -1; }
  if(!cov_ready(point, ctx, who)) return -1;
  Driver* d = D(ctx);
  return with_point_factor(point, ctx, "marginal variances",
                           [&]{ return dlg_marginal_variances(d->be, slot_of(d, point), var); }) ? 0 : -1;
}

int dogleg_amd_covariance_entries(double* out, long n, const int* row, const int* col,
                                  dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  const char* who = "dogleg_amd_covariance_entries";
  if(n < 0 || (n > 0 && (!out || !row || !col))) { MSG("%s(): bad arguments", who); return -1; }
  if(!cov_ready(point, ctx, who)) return -1;
  Driver* d = D(ctx);
  return with_point_factor(point, ctx, "covariance entries",
                           [&]{ return dlg_covariance_entries(d->be, slot_of(d, point), n, row, col, out); }) ? 0 : -1;
}

int dogleg_amd_query_covariance(double* out, int nq, const int* qrow, const int* rowptr, const int* var,
                                const double* val, int Nobservations,
                                dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  const char* who = "dogleg_amd_query_covariance";
  if(nq < 0 || (nq > 0 && (!out || !qrow || !rowptr || !var || !val))) { MSG("%s(): bad arguments", who); return -1; }
  if(!cov_ready(point, ctx, who)) return -1;
  Driver* d = D(ctx);
  return with_point_factor(point, ctx, "query covariance",
                           [&]{ return dlg_query_covariance(d->be, slot_of(d, point), nq, qrow, rowptr, var, val, Nobservations, out); }) ? 0 : -1;
}

// ---- extension (not in the reference): multi-GPU.  See include/dogleg.h.
int dogleg_amd_set_communicator(int rank, int nranks, int device, const void* rccl_unique_id128)
{
  if(nranks < 1 || rank < 0 || rank >= nranks || !rccl_unique_id128) { MSG("dogleg_amd_set_communicator: bad arguments"); return -1; }
  Comm c; c.rank = rank; c.nranks = nranks; c.device = device; c.have_id = true; memcpy(c.id, rccl_unique_id128, 128); c.set = true;
  t_comm = c;
  return 0;
}
int dogleg_amd_set_allreduce(int rank, int nranks, int device, dogleg_amd_allreduce_t fn, void* cookie)
{
  if(nranks < 1 || rank < 0 || rank >= nranks || !fn) { MSG("dogleg_amd_set_allreduce: bad arguments"); return -1; }
  Comm c; c.rank = rank; c.nranks = nranks; c.device = device; c.fn = fn; c.cookie = cookie; c.set = true;
  t_comm = c;
  return 0;
}
void dogleg_amd_clear_communicator(void) { t_comm = Comm(); }

// ---- extension (not in the reference): a batch of small dense problems, the dog-leg loop on the device (dense_batch.hip)
int dogleg_amd_optimize_dense_batch(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                    dogleg_callback_device_batch_t* f, void* cookie,
                                    const dogleg_parameters2_t* parameters, dogleg_amd_batch_result_t* results)
{
  const char* who = "dogleg_amd_optimize_dense_batch";
  if(!p || !f || !results) { MSG("%s: p, the callback and results must be given", who); return -1; }
  if(B == 0 || Nstate == 0 || Nmeas == 0) { MSG("%s: B = %u, Nstate = %u, Nmeas = %u: none may be 0", who, B, Nstate, Nmeas); return -1; }
  if(Nstate > DOGLEG_AMD_BATCH_MAX_NSTATE)
  {
    MSG("%s: Nstate = %u, the batch kernels take at most %d variables (larger problems: a loop over dogleg_optimize_dense2)", who,
        Nstate, DOGLEG_AMD_BATCH_MAX_NSTATE);
    return -1;
  }
  if(B > 0x7fffffffu/4 || Nmeas > 0x7fffffffu/(Nstate + 1))
  { MSG("%s: B = %u problems of %u x %u: beyond the index range of the batch kernels", who, B, Nmeas, Nstate); return -1; }
  const char* ws = getenv("DOGLEG_AMD_WORLD_SIZE");
  if(t_comm.set || (ws && atoi(ws) > 1))
  { MSG("%s: one rank only (a communicator is set: dogleg_amd_clear_communicator)", who); return -1; }
  return dlg_dense_batch_run(p, B, Nstate, Nmeas, f, cookie, parameters ? parameters : &g_params, results);
}
int dogleg_amd_batch_last_stats(double* out, int n) { return out ? dlg_dense_batch_last_stats(out, n) : 0; }
int dogleg_amd_dense_batch_uncertainty(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                       dogleg_callback_device_batch_t* f, void* cookie,
                                       double* lambda, double* covariance, double* variances, double* factors,
                                       double* scale, int featureSize, int* status)
{
  const char* who = "dogleg_amd_dense_batch_uncertainty";
  if(!p || !f || !status) { MSG("%s: p, the callback and status must be given", who); return -1; }
  if(B == 0 || Nstate == 0 || Nmeas == 0) { MSG("%s: B = %u, Nstate = %u, Nmeas = %u: none may be 0", who, B, Nstate, Nmeas); return -1; }
  if(Nstate > DOGLEG_AMD_BATCH_MAX_NSTATE)
  {
    MSG("%s: Nstate = %u, the batch kernels take at most %d variables (larger problems: a loop over dogleg_optimize_dense2)", who,
        Nstate, DOGLEG_AMD_BATCH_MAX_NSTATE);
    return -1;
  }
  if(B > 0x7fffffffu/4 || Nmeas > 0x7fffffffu/(Nstate + 1))
  { MSG("%s: B = %u problems of %u x %u: beyond the index range of the batch kernels", who, B, Nmeas, Nstate); return -1; }
  if(featureSize > 2) { MSG("%s: featureSize = %d: only 1 and 2 are supported", who, featureSize); return -1; }
  const int fs = featureSize <= 1 ? 1 : 2;
  if(!covariance && !variances && !factors) { MSG("%s: none of covariance, variances, factors is asked for", who); return -1; }
  if(factors && !scale) { MSG("%s: factors need scale", who); return -1; }
  if(factors && Nmeas/(unsigned int)fs == 0) { MSG("%s: Nmeas = %u holds no feature of size %d", who, Nmeas, fs); return -1; }
  if(factors && Nmeas <= Nstate + 1)
    for(unsigned int b = 0; b < B; b++)
      if(!(scale[b] > 0.0))
      {
        MSG("%s: scale[%u] <= 0 is to be computed, which needs Nmeas > Nstate + 1 (%u, %u)", who, b, Nmeas, Nstate);
        return -1;
      }
  const char* ws = getenv("DOGLEG_AMD_WORLD_SIZE");
  if(t_comm.set || (ws && atoi(ws) > 1))
  { MSG("%s: one rank only (a communicator is set: dogleg_amd_clear_communicator)", who); return -1; }
  return dlg_dense_batch_uncertainty_run(p, B, Nstate, Nmeas, f, cookie, lambda, covariance, variances, factors, scale, fs, status);
}
int dogleg_amd_batch_uncertainty_last_stats(double* out, int n) { return out ? dlg_dense_batch_uncertainty_last_stats(out, n) : 0; }

// ---- extension (not in the reference): the Jacobian of a device callback against central differences (gradcheck.hip)
namespace {
constexpr double GRADTEST_DELTA = 1e-6;             // dogleg.c:352
bool one_rank_only(const char* who)
{
  const char* ws = getenv("DOGLEG_AMD_WORLD_SIZE");
  if(!t_comm.set && !(ws && atoi(ws) > 1)) return true;
  MSG("%s: one rank only (a communicator is set: dogleg_amd_clear_communicator)", who);
  return false;
}
// the pattern arguments of a device callback's entry points: NJnnz == 0 with NULL pointers is dense
bool device_pattern_ok(const char* who, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz, const int* colptr,
                       const int* rowidx)
{
  if(Nstate > 0x7fffffffu || Nmeas > 0x7fffffffu - 1 || NJnnz > 0x7fffffffu)
  { MSG("%s: Nstate = %u, Nmeas = %u, NJnnz = %u: beyond the index range", who, Nstate, Nmeas, NJnnz); return false; }
  if(NJnnz == 0)
  {
    if(colptr || rowidx) { MSG("%s: NJnnz = 0 selects the dense path, which takes no pattern", who); return false; }
    return true;
  }
  if(!colptr || !rowidx) { MSG("%s: NJnnz = %u needs Jt_colptr and Jt_rowidx", who, NJnnz); return false; }
  char err[512];
  if(gradcheck_check_pattern((int)Nstate, (int)Nmeas, (long)NJnnz, colptr, rowidx, err, sizeof(err)))
  { MSG("%s: %s", who, err); return false; }
  return true;
}
bool tolerances_ok(const char* who, double rtol, double atol)
{
  if(rtol >= 0.0 && atol >= 0.0) return true;
  MSG("%s: rtol = %g, atol = %g: both must be given and non-negative", who, rtol, atol);
  return false;
}
} // namespace
int dogleg_amd_jacobian_colouring(unsigned Nstate, unsigned Nmeas, const int* Jt_colptr, const int* Jt_rowidx, int* colour)
{
  const char* who = "dogleg_amd_jacobian_colouring";
  if(!colour || Nstate == 0 || Nmeas == 0 || Nstate > 0x7fffffffu || Nmeas > 0x7fffffffu - 1)
  { MSG("%s: Nstate = %u, Nmeas = %u and colour must be given", who, Nstate, Nmeas); return -1; }
  char err[512];
  if(gradcheck_check_pattern((int)Nstate, (int)Nmeas, -1, Jt_colptr, Jt_rowidx, err, sizeof(err)))
  { MSG("%s: %s", who, err); return -1; }
  return gradcheck_colour((int)Nstate, (int)Nmeas, Jt_colptr, Jt_rowidx, colour);
}
int dogleg_amd_check_jacobian_device(const double* p0, unsigned Nstate, unsigned Nmeas, unsigned NJnnz,
                                     const int* Jt_colptr, const int* Jt_rowidx, dogleg_callback_device_t* f, void* cookie,
                                     double delta, double rtol, double atol, int flags,
                                     dogleg_amd_jacobian_report_t* report, double* var_error,
                                     dogleg_amd_jacobian_entry_t* bad, int max_bad)
{
  const char* who = "dogleg_amd_check_jacobian_device";
  if(!p0 || !f || !report) { MSG("%s: p0, the callback and report must be given", who); return -1; }
  if(Nstate == 0 || Nmeas == 0) { MSG("%s: Nstate = %u, Nmeas = %u: neither may be 0", who, Nstate, Nmeas); return -1; }
  if(!tolerances_ok(who, rtol, atol) || !device_pattern_ok(who, Nstate, Nmeas, NJnnz, Jt_colptr, Jt_rowidx)) return -1;
  if(!one_rank_only(who)) return -1;
  return dlg_gradcheck_run(p0, Nstate, Nmeas, NJnnz, Jt_colptr, Jt_rowidx, f, cookie, delta > 0.0 ? delta : GRADTEST_DELTA,
                           rtol, atol, flags, report, var_error, bad, max_bad);
}
int dogleg_amd_check_jacobian_device_batch(const double* p0, unsigned B, unsigned Nstate, unsigned Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           double delta, double rtol, double atol, dogleg_amd_jacobian_report_t* reports,
                                           dogleg_amd_jacobian_entry_t* bad, int max_bad, long long* nbad_total)
{
  const char* who = "dogleg_amd_check_jacobian_device_batch";
  if(!p0 || !f || !reports) { MSG("%s: p0, the callback and reports must be given", who); return -1; }
  if(B == 0 || Nstate == 0 || Nmeas == 0) { MSG("%s: B = %u, Nstate = %u, Nmeas = %u: none may be 0", who, B, Nstate, Nmeas); return -1; }
  if(Nstate > DOGLEG_AMD_BATCH_MAX_NSTATE)
  {
    MSG("%s: Nstate = %u, a batch takes at most %d variables (larger problems: dogleg_amd_check_jacobian_device)", who, Nstate,
        DOGLEG_AMD_BATCH_MAX_NSTATE);
    return -1;
  }
  if(B > 0x7fffffffu/4 || Nmeas > 0x7fffffffu/(Nstate + 1))
  { MSG("%s: B = %u problems of %u x %u: beyond the index range of the batch kernels", who, B, Nmeas, Nstate); return -1; }
  if(!tolerances_ok(who, rtol, atol) || !one_rank_only(who)) return -1;
  return dlg_gradcheck_batch_run(p0, B, Nstate, Nmeas, f, cookie, delta > 0.0 ? delta : GRADTEST_DELTA, rtol, atol, reports, bad,
                                 max_bad, nbad_total);
}
void dogleg_amd_testGradient_device(unsigned var, const double* p0, unsigned Nstate, unsigned Nmeas, unsigned NJnnz,
                                    const int* Jt_colptr, const int* Jt_rowidx, dogleg_callback_device_t* f, void* cookie)
{
  const char* who = "dogleg_amd_testGradient_device";
  if(!p0 || !f || Nmeas == 0 || var >= Nstate) { MSG("%s: bad arguments", who); return; }
  if(!device_pattern_ok(who, Nstate, Nmeas, NJnnz, Jt_colptr, Jt_rowidx) || !one_rank_only(who)) return;
  std::vector<double> table(2*(size_t)Nmeas);
  if(dlg_gradcheck_table(var, p0, Nstate, Nmeas, NJnnz, Jt_colptr, Jt_rowidx, f, cookie, GRADTEST_DELTA, table.data())) return;
  // the table of dogleg_testGradient (gradtest.cpp: report)
  printf("# ivar imeasurement gradient_reported gradient_observed error error_relative\n");
  for(unsigned int m = 0; m < Nmeas; m++)
  {
    const double rep = table[2*(size_t)m], observed = table[2*(size_t)m + 1];
    const double sum = fabs(rep) + fabs(observed), err = fabs(rep - observed);
    printf("%d %d %.6g %.6g %.6g %.6g\n", (int)var, (int)m, rep, observed, err, sum == 0.0 ? 0.0 : err/(sum/2.0));
  }
  fflush(stdout);
}
int dogleg_amd_check_jacobian_last_stats(double* out, int n) { return out ? dlg_gradcheck_last_stats(out, n) : 0; }
// what the library keeps between solves (the idle backend with its device memory, page-locked host buffers)
void dogleg_amd_release_cache(void)
{
  dlg_backend_t* be = nullptr;
  std::vector<PinnedBuf> pool;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    be = g_parked.be; g_parked.be = nullptr;
    pool.swap(g_pinned_pool); g_pinned_pool_bytes = 0;
  }
  if(be) dlg_backend_destroy(be);
  for(const PinnedBuf& b : pool) (void)hipHostFree(b.p);
  dlg_dense_batch_release();
}
// where the calling thread's last solve spent its wall time (DOGLEG_AMD_TIMING=1 must have been set for it): milliseconds and
// calls of {pattern, model callback, inputs to the backend, dlg_point_eval, dlg_take_step / dlg_step, trace records,
// run_optimizer as a whole} -- everything but the second entry is the library's share of a trial (tools/e2e_bench.py)
int dogleg_amd_last_solve_timing(double* ms7, int* calls7)
{
  for(int k = 0; k <= TM_COUNT; k++) { if(ms7) ms7[k] = t_last_tm_ms[k]; if(calls7) calls7[k] = t_last_tm_n[k]; }
  return TM_COUNT + 1;
}
int dogleg_amd_rccl_unique_id(void* out128) { return dlg_rccl_unique_id(out128) == DLG_OK ? 0 : -1; }
int dogleg_amd_rank(const dogleg_solverContext_t* ctx, int* nranks)
{
  const Driver* d = reinterpret_cast<const Driver*>(ctx);
  if(!d) return -1;
  if(nranks) *nranks = d->sharded ? d->nranks : 1;
  return d->sharded ? d->rank : 0;
}

// extension (not in the reference): the device backend behind a returned context, for
// dlg_solve_with_factor / dlg_point_download on the resident factor and vectors
dlg_backend_t* dogleg_amd_backend(dogleg_solverContext_t* ctx) { return ctx ? D(ctx)->be : nullptr; }
int dogleg_amd_point_slot(dogleg_solverContext_t* ctx, const dogleg_operatingPoint_t* point)
{ return (ctx && point) ? slot_of(D(ctx), point) : -1; }

void dogleg_freeContext(dogleg_solverContext_t** ctx)
{
  if(!ctx || !*ctx) return;
  destroy(D(*ctx));
  *ctx = nullptr;
}

} // extern "C"
