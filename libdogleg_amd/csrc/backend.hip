// backend.hip -- the backend's lifecycle behind the C-ABI in include/dlg_backend.h: create / destroy / reset, the setters,
// profiling, RCCL and the sums over the ranks, downloads and raw memory.  The per-step path (operating points, K1 .. K8,
// dlg_step / dlg_take_step / dlg_run_steps) is in step.hip.  The entry points that use the factor held after a solve
// (solves with it, leverage, covariance, query covariance, the selected inverse) are in factor_users.hip; what they ask of
// the backend's state first, dlg_factor_user_begin, is here.
#include "dlg_internal.h"

// ------------------------------------------------------------------ errors --
static thread_local char g_err[1024] = "";
#include <chrono>
#include <atomic>
#include <mutex>
namespace {
constexpr int DLG_TURN_DEV = 64;
std::mutex g_turn_mu;
std::atomic<int> g_turn_live[DLG_TURN_DEV];
hipEvent_t g_turn_ev[DLG_TURN_DEV];
dlg_backend* g_turn_owner[DLG_TURN_DEV];
}
DlgRegionTurn::DlgRegionTurn(dlg_backend* b_) : b(b_), on(false)
{
  const int d = b->device & (DLG_TURN_DEV - 1);
  if(g_turn_live[d].load(std::memory_order_relaxed) <= 1 || !b->ev_region) return;
  on = true;
  g_turn_mu.lock();
  // (the launch before this one on the device, if it was another backend's: over before this one goes out)
  if(g_turn_owner[d] && g_turn_owner[d] != b && g_turn_ev[d]) (void)hipEventSynchronize(g_turn_ev[d]);
}
DlgRegionTurn::~DlgRegionTurn()
{
  if(!on) return;
  const int d = b->device & (DLG_TURN_DEV - 1);
  if(hipEventRecord(b->ev_region, b->stream) == hipSuccess) { g_turn_ev[d] = b->ev_region; g_turn_owner[d] = b; }
  g_turn_mu.unlock();
}
static void turn_register(dlg_backend* b) { g_turn_live[b->device & (DLG_TURN_DEV - 1)].fetch_add(1); }
static void turn_unregister(dlg_backend* b)
{
  const int d = b->device & (DLG_TURN_DEV - 1);
  std::lock_guard<std::mutex> lk(g_turn_mu);
  if(g_turn_owner[d] == b) { if(g_turn_ev[d]) (void)hipEventSynchronize(g_turn_ev[d]); g_turn_owner[d] = nullptr; g_turn_ev[d] = nullptr; }
  g_turn_live[d].fetch_sub(1);
}
void dlg_set_error(const char* fmt, ...)
{
  va_list ap; va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* dlg_last_error(void) { return g_err; }

extern "C" int dlg_device_count(void)
{
  int n = 0;
  if(hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int dlg_fetch_scalars(dlg_backend* b, int n)
{
  // (always the whole block, 128 bytes: the hand-off status word of the one-launch regions rides in it)
  (void)n;
  DLG_HIP(hipMemcpyAsync(b->h_scal, b->d_scal, sizeof(double)*(size_t)dlg_backend::NSCAL, hipMemcpyDeviceToHost,
                         b->stream));
  DLG_HIP(hipStreamSynchronize(b->stream));
  b->sync_mark++;
  dlg_resolve_pending(b);
  if(b->profiling) dlg_prof_resolve(b);
  return dlg_check_handoff(b);
}
// A wait inside a one-launch region (sparse factorisation / backward solve, dense potrf / trsv) gave up:
// whatever that launch computed is not to be used.  The status word is cleared for the next attempt.
int dlg_check_handoff(dlg_backend* b)
{
  const int st = *reinterpret_cast<const int*>(b->h_scal + (dlg_backend::NSCAL - 2));
  if(st == 0) return DLG_OK;
  *reinterpret_cast<int*>(b->h_scal + (dlg_backend::NSCAL - 2)) = 0;
  (void)hipMemsetAsync(b->d_scal + (dlg_backend::NSCAL - 2), 0, sizeof(double), b->stream);
  b->factor_slot = -1;
  for(int s = 0; s < 2; s++) b->slot[s].have_gn = false;
  dlg_set_error("a hand-off between workgroups timed out (status 0x%x:%s%s%s%s%s): the GPU is shared with work that keeps "
                "the waiting workgroups' partners off the chip, or a launch failed", st,
                (st & DLG_HANDOFF_FACTOR) ? " sparse factorisation" : "", (st & DLG_HANDOFF_SOLVE) ? " sparse backward solve" : "",
                (st & DLG_HANDOFF_POTRF) ? " dense potrf" : "", (st & DLG_HANDOFF_TRSV) ? " dense trsv" : "",
                (st & DLG_HANDOFF_TRSM) ? " dense potrf step" : "");
  return DLG_ERR_STATE;
}

// ---------------------------------------------------------------- profiling --
static hipEvent_t prof_event(dlg_backend* b)
{
  hipEvent_t e = nullptr;
  if(!b->prof_pool.empty()) { e = b->prof_pool.back(); b->prof_pool.pop_back(); return e; }
  if(hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
// (only the phases whose kernels look at the pivot flag: the assembly of a retried attempt runs in full)
static bool prof_is_cond(const dlg_backend* b, int id)
{ return b->prof_cond && (id == DLG_PROF_K5_FACTOR || id == DLG_PROF_K6_SOLVE || id == DLG_PROF_K3K8_NORM2JV); }
hipEvent_t dlg_prof_begin(dlg_backend* b)
{
  hipEvent_t e = prof_event(b);
  if(e) (void)hipEventRecord(e, b->stream);
  return e;
}
void dlg_prof_end(dlg_backend* b, int id, hipEvent_t start)
{
  hipEvent_t e = prof_event(b);
  if(!e) { b->prof_pool.push_back(start); return; }
  (void)hipEventRecord(e, b->stream);
  b->prof_pending.push_back({start, e, id, prof_is_cond(b, id), b->prof_cont});
}
bool dlg_prof_pair(dlg_backend* b, int id, hipEvent_t* e0, hipEvent_t* e1)
{
  if(!(b->prof_mask >> id & 1u) || !b->ext_events) return false;
  if(b->prof_tick[id]++ % b->prof_every != 0) return false;
  *e0 = prof_event(b); *e1 = prof_event(b);
  if(!*e0 || !*e1) { if(*e0) b->prof_pool.push_back(*e0); if(*e1) b->prof_pool.push_back(*e1); return false; }
  b->prof_pending.push_back({*e0, *e1, id, prof_is_cond(b, id)});
  return true;
}
void dlg_prof_resolve(dlg_backend* b)
{
  for(auto& pp : b->prof_pending)
  {
    float ms = 0;
    (void)hipEventSynchronize(pp.b);          // (a phase on the second stream may still be running)
    if(hipEventElapsedTime(&ms, pp.a, pp.b) == hipSuccess)
    {
      // (cont: the second part of a phase that was counted with its first part -- a factorisation enqueued in two pieces)
      if(pp.cond) { b->prof_att_ms[pp.id] += ms; b->prof_att_n[pp.id] += pp.cont ? 0 : 1; }
      else        { b->prof_ms[pp.id] += ms; b->prof_n[pp.id] += pp.cont ? 0 : 1; }
    }
    b->prof_pool.push_back(pp.a); b->prof_pool.push_back(pp.b);
  }
  b->prof_pending.clear();
}
// the outcome of the attempt the conditionally timed launches belong to is known
void dlg_prof_commit(dlg_backend* b, bool attempt_succeeded)
{
  for(int i = 0; i < DLG_PROF_COUNT; i++)
  {
    if(attempt_succeeded) { b->prof_ms[i] += b->prof_att_ms[i]; b->prof_n[i] += b->prof_att_n[i]; }
    else                  { b->prof_early_ms[i] += b->prof_att_ms[i]; b->prof_early_n[i] += b->prof_att_n[i]; }
    b->prof_att_ms[i] = 0; b->prof_att_n[i] = 0;
  }
}
extern "C" int dlg_backend_set_profiling(dlg_backend_t* b, int on)
{
  if(!b) return DLG_ERR_ARG;
  DLG_HIP(hipStreamSynchronize(b->stream));
  dlg_prof_resolve(b);
  for(int i = 0; i < DLG_PROF_COUNT; i++) { b->prof_ms[i] = 0; b->prof_n[i] = 0; b->prof_att_ms[i] = 0; b->prof_att_n[i] = 0; b->prof_early_ms[i] = 0; b->prof_early_n[i] = 0; }
  const int every = (on >> 16) & 0xff, sel = on & 0xffff;
  b->profiling = sel != 0;
  b->prof_mask = sel == 0 ? 0u : (sel == 1 ? ~0u : (unsigned)sel >> 1);
  b->prof_every = every > 0 ? every : 1;
  for(int i = 0; i < DLG_PROF_COUNT; i++) b->prof_tick[i] = 0;
  return DLG_OK;
}
extern "C" int dlg_backend_get_profile(dlg_backend_t* b, double* ms_total, long* launches, int n)
{
  if(!b) return DLG_ERR_ARG;
  DLG_HIP(hipStreamSynchronize(b->stream));
  dlg_prof_resolve(b);
  dlg_prof_commit(b, true);                  // (an attempt nobody reported on: its launches ran in full)
  for(int i = 0; i < n && i < DLG_PROF_COUNT; i++)
  { if(ms_total) ms_total[i] = b->prof_ms[i]; if(launches) launches[i] = b->prof_n[i]; }
  return DLG_OK;
}
// the launches that returned early behind a failed factorisation (the lambda path), kept out of dlg_backend_get_profile
extern "C" int dlg_backend_get_profile_early(dlg_backend_t* b, double* ms_total, long* launches, int n)
{
  if(!b) return DLG_ERR_ARG;
  DLG_HIP(hipStreamSynchronize(b->stream));
  dlg_prof_resolve(b);
  for(int i = 0; i < n && i < DLG_PROF_COUNT; i++)
  { if(ms_total) ms_total[i] = b->prof_early_ms[i]; if(launches) launches[i] = b->prof_early_n[i]; }
  return DLG_OK;
}

size_t dlg_j_doubles(const dlg_backend* b)
{
  const size_t N = (size_t)b->N;
  switch(b->type)
  {
  case DLG_DENSE:  return (size_t)b->M*N;
  case DLG_SPARSE: return (size_t)b->nnz;
  default:         return (b->flags & DLG_FLAG_JTJ_PACKED) ? N*(N+1)/2 : N*N;
  }
}

// ---------------------------------------------------------------- lifecycle --
static void rccl_release(dlg_backend* b);
extern "C" int dlg_backend_create(dlg_backend_t** out, int solve_type, int Nstate, int Nmeas,
                                  int NJnnz, int flags, int device)
{
  if(!out || Nstate <= 0 || Nmeas < 0 || solve_type < 0 || solve_type > 2)
  { dlg_set_error("dlg_backend_create: bad arguments"); return DLG_ERR_ARG; }
  if(solve_type == DLG_SPARSE && NJnnz <= 0)
  { dlg_set_error("sparse backend needs NJnnz > 0"); return DLG_ERR_ARG; }
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
  {
    dlg_set_error("no HIP device available: libdogleg_amd has no CPU fallback");
    return DLG_ERR_NODEVICE;
  }
  if(device >= 0) DLG_HIP(hipSetDevice(device));
  else            DLG_HIP(hipGetDevice(&device));

  dlg_backend* b = new (std::nothrow) dlg_backend();
  if(!b) { dlg_set_error("out of host memory"); return DLG_ERR_NOMEM; }
  b->type = solve_type; b->N = Nstate; b->M = Nmeas; b->nnz = NJnnz; b->flags = flags;
  b->device = device;
  b->row0 = 0; b->row1 = Nmeas; b->mloc = Nmeas;
  *out = nullptr;

  auto fail = [&](int rc) { dlg_backend_destroy(b); return rc; };
#define TRY_HIP(call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { \
    dlg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
    return fail(DLG_ERR_HIP); } } while(0)

  TRY_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
  b->own_stream = true;
  TRY_HIP(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
  TRY_HIP(hipEventCreateWithFlags(&b->ev_step, hipEventDisableTiming));
  TRY_HIP(hipEventCreateWithFlags(&b->ev_copy, hipEventDisableTiming));
  TRY_HIP(hipStreamCreateWithFlags(&b->aux_stream, hipStreamNonBlocking));
  TRY_HIP(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
  TRY_HIP(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
  TRY_HIP(hipEventCreateWithFlags(&b->ev_region, hipEventDisableTiming));
  turn_register(b); b->turn_registered = true;
  TRY_HIP(hipMalloc(&b->d_join, sizeof(int)*2));
  TRY_HIP(hipMemsetAsync(b->d_join, 0, sizeof(int)*2, b->stream));
  b->overlap = getenv("DOGLEG_AMD_NO_OVERLAP") == nullptr;
  b->fuse_eval = getenv("DOGLEG_AMD_NO_FUSED_EVAL") == nullptr;
  TRY_HIP(hipMalloc(&b->d_scal, sizeof(double)*dlg_backend::NSCAL));
  TRY_HIP(hipMemsetAsync(b->d_scal, 0, sizeof(double)*dlg_backend::NSCAL, b->stream));
  TRY_HIP(hipHostMalloc(&b->h_scal, sizeof(double)*dlg_backend::NSCAL));
  TRY_HIP(hipHostMalloc(&b->h_part, sizeof(double)*dlg_backend::HPART_CAP));
  b->host_finals = getenv("DOGLEG_AMD_DEVICE_FINALS") == nullptr;
  {
    dlg_backend::Knobs& k = b->knobs;
    k.potrf_steps = getenv("DOGLEG_AMD_POTRF_STEPS") != nullptr;
    k.trsv_steps = getenv("DOGLEG_AMD_TRSV_STEPS") != nullptr;
    k.no_abandon = getenv("DOGLEG_AMD_NO_ABANDON") != nullptr;
    k.ei_jpass = getenv("DOGLEG_AMD_EI_JPASS") != nullptr;
    k.no_between = getenv("DOGLEG_AMD_NO_BETWEEN") != nullptr;
    k.no_k8_predict = getenv("DOGLEG_AMD_NO_K8_PREDICT") != nullptr;
    // test hook of the driver's `expected improvement < 0` stop (dogleg.c:1403-1408; exact arithmetic never gets there: the
    // value is a positive definite form of Jt x for all three kinds of step): the n-th value this backend hands out is negated
    if(const char* e = getenv("DOGLEG_AMD_DEBUG_EI_FLIP")) b->ei_flip = atoi(e);
    // test hook of the hand-off time-outs: the waits of the one-launch regions look for an epoch that never
    // comes and give up after a few hundred polls
    if(getenv("DOGLEG_AMD_DEBUG_HANDOFF_TIMEOUT")) { b->handoff_skew = 1; b->handoff_spins = 256; }
    (void)hipDeviceGetAttribute(&b->ncu, hipDeviceAttributeMultiprocessorCount, device);
    if(b->ncu <= 0) b->ncu = 256;
  }
  TRY_HIP(hipHostMalloc(&b->h_vec, sizeof(double)*(size_t)Nstate));
  TRY_HIP(hipMalloc(&b->d_work, sizeof(double)*(size_t)Nstate));
  const size_t N = (size_t)Nstate, M = (size_t)Nmeas;
  for(int s = 0; s < 2; s++)
  {
    DlgSlot& S = b->slot[s];
    TRY_HIP(hipMalloc(&S.p,      sizeof(double)*N));
    TRY_HIP(hipMalloc(&S.Jt_x,   sizeof(double)*(N + 8)));      // (+ room for |x|^2 behind the vector: the sum over the ranks is made in place, dlg_point_eval)
    TRY_HIP(hipMalloc(&S.cauchy, sizeof(double)*N));
    TRY_HIP(hipMalloc(&S.gn,     sizeof(double)*(N + 8)));      // (+ room for a scalar behind the vector: sparse_solve, fold_scalar)
    TRY_HIP(hipMalloc(&S.step,   sizeof(double)*N));
    TRY_HIP(hipMemsetAsync(S.p, 0, sizeof(double)*N, b->stream));
    TRY_HIP(hipMemsetAsync(S.step, 0, sizeof(double)*N, b->stream));
    if(solve_type != DLG_DENSE_PRODUCTS && M > 0) TRY_HIP(hipMalloc(&S.x, sizeof(double)*M));
    TRY_HIP(hipMalloc(&S.J, sizeof(double)*dlg_j_doubles(b)));
  }
#undef TRY_HIP
  int rc = (solve_type == DLG_SPARSE) ? sparse_create(b) : dense_create(b);
  if(rc != DLG_OK) return fail(rc);
  if(hipStreamSynchronize(b->stream) != hipSuccess)
  { dlg_set_error("stream sync failed during create"); return fail(DLG_ERR_HIP); }
  *out = b;
  return DLG_OK;
}

extern "C" void dlg_backend_destroy(dlg_backend_t* b)
{
  if(!b) return;
  if(b->stream) (void)hipStreamSynchronize(b->stream);
  if(b->type == DLG_SPARSE) sparse_destroy(b); else dense_destroy(b);
  rccl_release(b);
  for(int s = 0; s < 2; s++)
  {
    DlgSlot& S = b->slot[s];
    double* v[] = { S.p, S.x, S.J, S.Jt_x, S.cauchy, S.gn, S.step };
    for(double* q : v) if(q) (void)hipFree(q);
  }
  if(b->d_scal) (void)hipFree(b->d_scal);
  if(b->h_scal) (void)hipHostFree(b->h_scal);
  if(b->h_part) (void)hipHostFree(b->h_part);
  if(b->h_tail) (void)hipHostFree(b->h_tail);
  if(b->h_vec)  (void)hipHostFree(b->h_vec);
  if(b->d_part) (void)hipFree(b->d_part);
  if(b->d_gnpart) (void)hipFree(b->d_gnpart);
  if(b->d_work) (void)hipFree(b->d_work);
  if(b->solve_scr.p) (void)hipFree(b->solve_scr.p);
  if(b->lev_scr.p) (void)hipFree(b->lev_scr.p);
  if(b->cov) { for(int i = 0; i < COV_NPLAN; i++) cov_plan_release(b->cov[i]); delete[] b->cov; }
  selinv_release(b);
  if(b->d_red)  (void)hipFree(b->d_red);
  for(auto& pp : b->prof_pending) { (void)hipEventDestroy(pp.a); (void)hipEventDestroy(pp.b); }
  for(hipEvent_t e : b->prof_pool) (void)hipEventDestroy(e);
  if(b->copy_stream) { (void)hipStreamSynchronize(b->copy_stream); (void)hipStreamDestroy(b->copy_stream); b->copy_stream = nullptr; }
  if(b->aux_stream) { (void)hipStreamSynchronize(b->aux_stream); (void)hipStreamDestroy(b->aux_stream); b->aux_stream = nullptr; }
  if(b->ev_fork) { (void)hipEventDestroy(b->ev_fork); b->ev_fork = nullptr; }
  if(b->ev_join) { (void)hipEventDestroy(b->ev_join); b->ev_join = nullptr; }
  if(b->turn_registered) { turn_unregister(b); b->turn_registered = false; }
  if(b->ev_region) { (void)hipEventDestroy(b->ev_region); b->ev_region = nullptr; }
  if(b->d_join) { (void)hipFree(b->d_join); b->d_join = nullptr; }
  if(b->ev_step) { (void)hipEventDestroy(b->ev_step); b->ev_step = nullptr; }
  if(b->ev_copy) { (void)hipEventDestroy(b->ev_copy); b->ev_copy = nullptr; }
  if(b->ev_fetch) { (void)hipEventDestroy(b->ev_fetch); b->ev_fetch = nullptr; }
  if(b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

// One backend, one solve after another (the driver parks a backend between dogleg_optimize* calls instead
// of destroying it: device buffers, the uploaded pattern and schedules, streams and events all stay).  What
// belongs to the previous solve -- operating points, the held factor, bound inputs -- is forgotten.
extern "C" int dlg_backend_reset(dlg_backend_t* b)
{
  if(!b) return DLG_ERR_ARG;
  DLG_HIP(hipStreamSynchronize(b->stream));
  if(b->aux_stream) DLG_HIP(hipStreamSynchronize(b->aux_stream));
  if(b->copy_stream) DLG_HIP(hipStreamSynchronize(b->copy_stream));
  dlg_resolve_pending(b);
  for(int s = 0; s < 2; s++)
  {
    DlgSlot& S = b->slot[s];
    S.x_bound = S.J_bound = nullptr; S.held = nullptr;
    S.have_inputs = S.have_Jtx = S.have_cauchy = S.have_gn = false;
    S.norm2_x = S.norm2_cauchy = S.norm2_gn = S.norm2_jtx = 0;
    // (step_to_here of the first point of a solve is read by nobody, but a returned context downloads it)
    DLG_HIP(hipMemsetAsync(S.step, 0, sizeof(double)*(size_t)b->N, b->stream));
  }
  b->factor_slot = -1; b->speculate = false; b->presolve = false; b->pre_slot = -1; b->pre_held = -1; b->pre_hint_valid = false; b->pre_hint_input = false; b->pre_rejected = false; b->pre_split = false;
  b->want_fork = b->fork_recorded = false; b->fork_gate = nullptr;
  b->join_pending = 0;
  b->fold_scalar = b->fold_result = nullptr; b->fold_cauchy_out = nullptr;
  b->h_part_used = 0; b->pending.clear();
  b->between_fn = nullptr; b->between_cookie = nullptr; b->between_armed = b->between_ran = b->between_redone = false; b->early_slot = -1; b->ident_predict = false;
  if(b->tail_pending) DLG_HIP(hipStreamSynchronize(b->stream));
  b->tail_pending = false; b->defer_tail = false;
  b->ei_count = 0; b->p_side_pending = false;      // (the test hook counts the values of ONE solve; the copy stream was waited for above)
  DLG_HIP(hipMemsetAsync(b->d_scal, 0, sizeof(double)*dlg_backend::NSCAL, b->stream));
  if(b->type == DLG_SPARSE) sparse_reset(b);
  selinv_release(b);
  DLG_HIP(hipStreamSynchronize(b->stream));
  return DLG_OK;
}

extern "C" int dlg_backend_set_stream(dlg_backend_t* b, void* hip_stream)
{
  if(!b) return DLG_ERR_ARG;
  if(b->stream) DLG_HIP(hipStreamSynchronize(b->stream));
  if(b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
  b->stream = (hipStream_t)hip_stream;
  b->own_stream = false;
  return DLG_OK;
}
extern "C" void* dlg_backend_get_stream(dlg_backend_t* b) { return b ? (void*)b->stream : nullptr; }
extern "C" int dlg_backend_device(dlg_backend_t* b) { return b ? b->device : -1; }

extern "C" int dlg_backend_set_shard(dlg_backend_t* b, int row0, int row1, dlg_allreduce_fn fn,
                                     void* cookie)
{
  if(!b || row0 < 0 || row1 < row0 || row1 > b->M)
  { dlg_set_error("dlg_backend_set_shard: bad row range"); return DLG_ERR_ARG; }
  if(b->type == DLG_DENSE_PRODUCTS)
  { dlg_set_error("dense-products has no measurement rows to shard"); return DLG_ERR_ARG; }
  if(b->type == DLG_SPARSE && b->sym)
  { dlg_set_error("set the shard before dlg_sparse_set_pattern"); return DLG_ERR_STATE; }
  b->row0 = row0; b->row1 = row1; b->mloc = row1 - row0;
  b->allreduce = fn; b->allreduce_cookie = fn ? cookie : nullptr;      // (fn == NULL: no hook -- RCCL, or a single rank again)
  b->host_finals = b->sharded() ? false : getenv("DOGLEG_AMD_DEVICE_FINALS") == nullptr;   // sums over the ranks act on device scalars: they must be final on the device
  return DLG_OK;
}

extern "C" int dlg_backend_set_speculation(dlg_backend_t* b, int on)
{
  if(!b) return DLG_ERR_ARG;
  b->speculate = on != 0;
  b->presolve = b->speculate && getenv("DOGLEG_AMD_NO_PRESOLVE") == nullptr;
  return DLG_OK;
}

// dlg_take_step / dlg_step return without the expected improvement (NaN in its place) and, for a page-locked p_new_host,
// possibly without p_new: both are complete when dlg_step_tail returns.  The reference uses the value only after the
// NEXT evaluation (dogleg.c:1427; "done" is decided on max|step|, 1289-1296): the pass over J that forms |J step|^2 runs
// while the host is on its way back and enqueues what comes next (the model's kernels, the next evaluation) instead of
// in front of the synchronisation the host decides behind.  Until dlg_step_tail the caller must leave J of the slot the
// step was taken from alone (binding other arrays to the slot is fine: the bound ones are only read).
extern "C" int dlg_backend_set_defer_tail(dlg_backend_t* b, int on)
{
  if(!b) return DLG_ERR_ARG;
  b->defer_tail = on != 0;
  return DLG_OK;
}
// the held variables of a slot: the assembly's hooks (sparse_assemble.hip: k_held_diag_sparse; kernels_dense.hip: k_held_diag_dense) read the bytes
extern "C" int dlg_point_bind_held(dlg_backend_t* b, int s, const unsigned char* held_dev, double norm2_Jtx)
{
  DLG_CHECK(dlg_check_slot(b, s));
  if(held_dev && (b->type == DLG_DENSE_PRODUCTS || b->sharded() || b->part_nranks > 1))
  { dlg_set_error("dlg_point_bind_held: one rank, sparse or dense only"); return DLG_ERR_STATE; }
  DlgSlot& S = b->slot[s];
  S.held = held_dev;
  if(!held_dev) return DLG_OK;
  if(!S.have_Jtx) { dlg_set_error("dlg_point_bind_held: slot %d has not been evaluated", s); return DLG_ERR_STATE; }
  S.norm2_jtx = norm2_Jtx;
  // (whatever was formed from the unmasked point is not this point's)
  S.have_cauchy = S.have_gn = false; S.ident_ok = false;
  if(b->factor_slot == s) b->factor_slot = -1;
  if(b->type == DLG_SPARSE) sparse_spec_invalidate(b, s);
  return DLG_OK;
}
extern "C" int dlg_backend_set_between(dlg_backend_t* b, dlg_between_fn fn, void* cookie)
{
  if(!b) return DLG_ERR_ARG;
  b->between_fn = fn; b->between_cookie = fn ? cookie : nullptr;
  return DLG_OK;
}
extern "C" int dlg_backend_between_redone(dlg_backend_t* b) { return (b && b->between_redone) ? 1 : 0; }
extern "C" int dlg_backend_ei_source(dlg_backend_t* b, int* from_solved_system, double* pivot_ratio)
{
  if(!b) return DLG_ERR_ARG;
  if(from_solved_system) *from_solved_system = b->ei_from_system ? 1 : 0;
  if(pivot_ratio) *pivot_ratio = b->pivot_ratio;
  return DLG_OK;
}

// MEASUREMENT ONLY: the per-rank compute time of a partitioned step on ONE device, for a scaling projection where no
// multi-GPU node is at hand (bench.py --logical-ranks).  Every sum over the ranks is skipped, so a rank sees only its
// own contributions: the caller adds a lambda that keeps the partial top of the tree positive definite, and uses
// nothing but the clocks.
extern "C" int dlg_backend_set_noop_comm(dlg_backend_t* b, int on)
{
  if(!b) return DLG_ERR_ARG;
  b->noop_comm = on != 0;
  if(b->noop_comm) b->host_finals = false;
  return DLG_OK;
}
extern "C" int dlg_backend_set_allreduce(dlg_backend_t* b, dlg_allreduce_fn fn, void* cookie)
{
  if(!b) return DLG_ERR_ARG;
  b->allreduce = fn; b->allreduce_cookie = cookie;
  if(b->sharded()) b->host_finals = false;
  return DLG_OK;
}

extern "C" int dlg_backend_set_partition(dlg_backend_t* b, int rank, int nranks)
{
  if(!b || nranks < 1 || rank < 0 || rank >= nranks)
  { dlg_set_error("dlg_backend_set_partition: bad rank %d of %d", rank, nranks); return DLG_ERR_ARG; }
  if(b->type != DLG_SPARSE)
  { dlg_set_error("the subtree partition is a property of the sparse path (dense: dlg_backend_set_shard)"); return DLG_ERR_ARG; }
  if(b->sym) { dlg_set_error("set the partition before dlg_sparse_set_pattern"); return DLG_ERR_STATE; }
  b->part_rank = rank; b->part_nranks = nranks; b->part_requested = true;
  return DLG_OK;
}

// ---- RCCL, loaded on demand: the library itself does not depend on librccl.so ----------------
#include <dlfcn.h>
#include <mutex>
namespace {
struct dlg_nccl_id { char internal[128]; };        // ncclUniqueId
struct RcclApi
{
  void* lib = nullptr;
  int (*GetUniqueId)(dlg_nccl_id*) = nullptr;
  int (*CommInitRank)(void**, int, dlg_nccl_id, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mu;
int rccl_load()
{
  std::lock_guard<std::mutex> lk(g_rccl_mu);       // backends on several threads may ask at once
  if(g_rccl.lib) return DLG_OK;
  const char* names[] = { "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so" };
  void* h = nullptr;
  for(const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if(h) break; }
  if(!h) { dlg_set_error("cannot load librccl.so: %s", dlerror()); return DLG_ERR_COMM; }
  RcclApi a; a.lib = h;
  a.GetUniqueId  = (int (*)(dlg_nccl_id*))dlsym(h, "ncclGetUniqueId");
  a.CommInitRank = (int (*)(void**, int, dlg_nccl_id, int))dlsym(h, "ncclCommInitRank");
  a.AllReduce    = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(h, "ncclAllReduce");
  a.CommDestroy  = (int (*)(void*))dlsym(h, "ncclCommDestroy");
  a.GetErrorString = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
  a.CommCount    = (int (*)(void*, int*))dlsym(h, "ncclCommCount");
  if(!a.GetUniqueId || !a.CommInitRank || !a.AllReduce || !a.CommDestroy)
  { dlg_set_error("librccl.so lacks the NCCL entry points"); dlclose(h); return DLG_ERR_COMM; }
  g_rccl = a;
  return DLG_OK;
}
const char* rccl_err(int rc) { return g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error"; }
constexpr int DLG_NCCL_FLOAT64 = 8, DLG_NCCL_SUM = 0;
}

extern "C" int dlg_rccl_unique_id(void* out128)
{
  if(!out128) return DLG_ERR_ARG;
  DLG_CHECK(rccl_load());
  dlg_nccl_id id;
  const int rc = g_rccl.GetUniqueId(&id);
  if(rc != 0) { dlg_set_error("ncclGetUniqueId: %s", rccl_err(rc)); return DLG_ERR_COMM; }
  memcpy(out128, &id, sizeof(id));
  return DLG_OK;
}
extern "C" int dlg_backend_init_rccl(dlg_backend_t* b, int rank, int nranks, const void* unique_id128)
{
  if(!b || !unique_id128 || nranks < 1 || rank < 0 || rank >= nranks)
  { dlg_set_error("dlg_backend_init_rccl: bad arguments"); return DLG_ERR_ARG; }
  if(b->rccl_comm) { dlg_set_error("the backend already has a communicator"); return DLG_ERR_STATE; }
  DLG_CHECK(rccl_load());
  DLG_HIP(hipSetDevice(b->device));
  dlg_nccl_id id; memcpy(&id, unique_id128, sizeof(id));
  void* comm = nullptr;
  const int rc = g_rccl.CommInitRank(&comm, nranks, id, rank);
  if(rc != 0) { dlg_set_error("ncclCommInitRank(rank %d of %d): %s", rank, nranks, rccl_err(rc)); return DLG_ERR_COMM; }
  b->rccl_comm = comm; b->rccl_owned = true;
  b->host_finals = false;
  return DLG_OK;
}
extern "C" int dlg_backend_set_rccl(dlg_backend_t* b, void* nccl_comm)
{
  if(!b || !nccl_comm) { dlg_set_error("dlg_backend_set_rccl: bad arguments"); return DLG_ERR_ARG; }
  DLG_CHECK(rccl_load());
  rccl_release(b);                                  // a communicator the backend made itself is not leaked
  b->rccl_comm = nccl_comm; b->rccl_owned = false;
  b->host_finals = false;
  return DLG_OK;
}
// the communicator of another backend of this process (which keeps owning it and must outlive b)
extern "C" int dlg_backend_share_rccl(dlg_backend_t* b, dlg_backend_t* owner)
{
  if(!b || !owner || !owner->rccl_comm) { dlg_set_error("dlg_backend_share_rccl: the owner has no communicator"); return DLG_ERR_ARG; }
  return dlg_backend_set_rccl(b, owner->rccl_comm);
}
extern "C" int dlg_backend_comm_size(dlg_backend_t* b, int* nranks)
{
  if(!b || !nranks) return DLG_ERR_ARG;
  *nranks = 1;
  if(b->rccl_comm && g_rccl.CommCount)
  {
    const int rc = g_rccl.CommCount(b->rccl_comm, nranks);
    if(rc != 0) { dlg_set_error("ncclCommCount: %s", rccl_err(rc)); return DLG_ERR_COMM; }
  }
  return DLG_OK;
}
extern "C" int dlg_backend_has_rccl(dlg_backend_t* b) { return (b && b->rccl_comm) ? 1 : 0; }
static void rccl_release(dlg_backend* b)
{
  if(b->rccl_comm && b->rccl_owned && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(b->rccl_comm);
  b->rccl_comm = nullptr;
}

// sum-all-reduce `count` doubles at device address buf across ranks (no-op single rank): RCCL on the
// backend's stream -- nothing for the host to wait for --, or the caller's hook behind a synchronisation
int dlg_allreduce_dev(dlg_backend* b, double* buf, size_t count)
{
  if(b->noop_comm) return DLG_OK;
  if(b->rccl_comm)
  {
    const int rc = g_rccl.AllReduce(buf, buf, count, DLG_NCCL_FLOAT64, DLG_NCCL_SUM, b->rccl_comm, b->stream);
    if(rc != 0) { dlg_set_error("ncclAllReduce(%zu doubles): %s", count, rccl_err(rc)); return DLG_ERR_COMM; }
    return DLG_OK;
  }
  if(!b->allreduce) return DLG_OK;
  DLG_HIP(hipStreamSynchronize(b->stream));
  if(b->allreduce(buf, count, b->allreduce_cookie) != 0)
  { dlg_set_error("all-reduce hook failed"); return DLG_ERR_COMM; }
  return DLG_OK;
}

extern "C" int dlg_sparse_set_pattern(dlg_backend_t* b, const int* colptr, const int* rowidx)
{
  if(!b || b->type != DLG_SPARSE || !colptr || !rowidx)
  { dlg_set_error("dlg_sparse_set_pattern: bad arguments"); return DLG_ERR_ARG; }
  return sparse_set_pattern(b, colptr, rowidx);
}

// measurement only: enqueue-to-completion time of `iters` all-reduces of `count` doubles each on the backend's stream,
// through whatever communicator the backend holds (RCCL at world size 1 on a one-GPU box: the floor of what a
// collective costs the step -- tools/rccl_floor.py, tools/scaling_projection.py).  us_each = average, microseconds.
extern "C" int dlg_backend_time_allreduce(dlg_backend_t* b, size_t count, int iters, double* us_each)
{
  if(!b || count == 0 || iters <= 0 || !us_each) { dlg_set_error("dlg_backend_time_allreduce: bad arguments"); return DLG_ERR_ARG; }
  double* buf = nullptr;
  DLG_HIP(hipMalloc(&buf, sizeof(double)*count));
  DLG_HIP(hipMemsetAsync(buf, 0, sizeof(double)*count, b->stream));
  hipEvent_t e0, e1;
  DLG_HIP(hipEventCreate(&e0)); DLG_HIP(hipEventCreate(&e1));
  int rc = DLG_OK;
  for(int i = 0; i < 3 && rc == DLG_OK; i++) rc = dlg_allreduce_dev(b, buf, count);          // warm-up
  DLG_HIP(hipStreamSynchronize(b->stream));
  const auto t0 = std::chrono::steady_clock::now();
  DLG_HIP(hipEventRecord(e0, b->stream));
  for(int i = 0; i < iters && rc == DLG_OK; i++) rc = dlg_allreduce_dev(b, buf, count);
  DLG_HIP(hipEventRecord(e1, b->stream));
  DLG_HIP(hipStreamSynchronize(b->stream));
  const double wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(buf);
  // (back to back on one stream: the larger of the device time between the events and the host's wall time)
  *us_each = std::max((double)ms*1e3, wall_us)/iters;
  return rc;
}

int dlg_check_slot(dlg_backend* b, int s)
{
  if(!b || s < 0 || s > 1) { dlg_set_error("bad backend/slot"); return DLG_ERR_ARG; }
  return DLG_OK;
}

// ------------------------------------- the users of the held factor (factor_users.hip)
// What every entry point that works with the factor held for slot s asks once, behind its own argument checks: a valid
// backend and slot, no other ranks where the call has no multi-GPU form, nothing enqueued ahead for a step that has not
// been taken (dlg_step_unprepare), the inputs it reads (DLG_NEEDS_J: the slot's Jacobian on the device), the factor of this
// slot, and the pattern the plans are built against.  DLG_ERR_ARG for the handle, DLG_ERR_STATE for everything else.
int dlg_factor_user_begin(dlg_backend* b, int s, const char* who, unsigned needs)
{
  DLG_CHECK(dlg_check_slot(b, s));
  if(((needs & DLG_NEEDS_UNSHARDED) && b->sharded()) || ((needs & DLG_NEEDS_UNPARTITIONED) && b->part_nranks > 1))
  { dlg_set_error("%s is not available on a sharded or partitioned backend", who); return DLG_ERR_STATE; }
  DLG_CHECK(dlg_step_unprepare(b));
  if((needs & DLG_NEEDS_J) && b->type == DLG_DENSE_PRODUCTS) { dlg_set_error("%s needs J: a dense-products backend keeps none", who); return DLG_ERR_STATE; }
  if((needs & DLG_NEEDS_J) && !b->slot[s].have_inputs) { dlg_set_error("%s needs x and J of slot %d", who, s); return DLG_ERR_STATE; }
  if(b->factor_slot != s) { dlg_set_error("%s: no factorization of slot %d is held", who, s); return DLG_ERR_STATE; }
  if((needs & DLG_NEEDS_PATTERN) && b->type == DLG_SPARSE && !b->sym) { dlg_set_error("%s: no sparse pattern", who); return DLG_ERR_STATE; }
  // (the held factor's merged leaves as every user reads them: L_below stored, once per held factor -- sparse_factor.hip.
  // Every reader of those rows in sparse_multi.hip and sparse_selinv.hip runs behind this prelude; the one that can be
  // reached without it, sparse_solve with a right-hand side of its own, asks for the rows itself.)
  if(b->type == DLG_SPARSE) DLG_CHECK(sparse_leaf_rows_materialize(b));
  return DLG_OK;
}

// ---------------------------------------------------------------- downloads --
static double* slot_vec(dlg_backend* b, int s, int which, size_t* n)
{
  DlgSlot& S = b->slot[s];
  *n = (size_t)b->N;
  switch(which)
  {
  case DLG_VEC_P:      return S.p;
  case DLG_VEC_X:      *n = (size_t)b->M; return const_cast<double*>(S.xin());
  case DLG_VEC_JTX:    return S.Jt_x;
  case DLG_VEC_CAUCHY: return S.cauchy;
  case DLG_VEC_GN:     return S.gn;
  case DLG_VEC_STEP:   return S.step;
  case DLG_VEC_J:      *n = dlg_j_doubles(b); return const_cast<double*>(S.Jin());
  case DLG_VEC_X_OWN:  *n = (size_t)b->M; return S.x;
  case DLG_VEC_J_OWN:  *n = dlg_j_doubles(b); return S.J;
  default:             return nullptr;
  }
}
extern "C" int dlg_point_download(dlg_backend_t* b, int s, int which, double* host, size_t n)
{
  DLG_CHECK(dlg_check_slot(b, s));
  size_t have = 0;
  double* src = slot_vec(b, s, which, &have);
  if(!src) { dlg_set_error("nothing to download for vector %d", which); return DLG_ERR_ARG; }
  if(n > have) n = have;
  DLG_HIP(hipMemcpyAsync(host, src, sizeof(double)*n, hipMemcpyDeviceToHost, b->stream));
  DLG_HIP(hipStreamSynchronize(b->stream));
  return DLG_OK;
}
extern "C" void* dlg_point_device_ptr(dlg_backend_t* b, int s, int which)
{
  if(!b || s < 0 || s > 1) return nullptr;
  size_t n;
  return slot_vec(b, s, which, &n);
}

// ------------------------------------------------------------ raw memory ----
extern "C" void* dlg_mem_alloc(size_t bytes)
{
  void* p = nullptr;
  if(hipMalloc(&p, bytes ? bytes : 8) != hipSuccess) { dlg_set_error("hipMalloc(%zu) failed", bytes); return nullptr; }
  return p;
}
extern "C" void dlg_mem_free(void* dev) { if(dev) (void)hipFree(dev); }
extern "C" void* dlg_host_alloc(size_t bytes)
{
  void* p = nullptr;
  if(hipHostMalloc(&p, bytes ? bytes : 8) != hipSuccess) { dlg_set_error("hipHostMalloc(%zu) failed", bytes); return nullptr; }
  return p;
}
extern "C" void dlg_host_free(void* host) { if(host) (void)hipHostFree(host); }
extern "C" int dlg_mem_upload(void* dev, const void* host, size_t bytes)
{ DLG_HIP(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice)); return DLG_OK; }
extern "C" int dlg_mem_download(void* host, const void* dev, size_t bytes)
{ DLG_HIP(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost)); return DLG_OK; }
extern "C" int dlg_mem_zero(void* dev, size_t bytes)
{ DLG_HIP(hipMemset(dev, 0, bytes)); return DLG_OK; }
extern "C" int dlg_device_sync(void) { DLG_HIP(hipDeviceSynchronize()); return DLG_OK; }
