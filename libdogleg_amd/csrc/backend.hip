// backend.hip -- implementation of the C-ABI in include/dlg_backend.h: context
// lifecycle, operating-point slots, and the per-op orchestration that strings
// the HIP kernels together.  No CPU arithmetic happens here: every op is a
// kernel sequence on b->stream followed by one small D2H of result scalars.
// The entry points that use the factor held after a solve (solves with it, leverage,
// covariance, query covariance, the selected inverse) are in factor_users.hip; what
// they ask of the backend's state first, dlg_factor_user_begin, is here.
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

static size_t j_doubles(const dlg_backend* b)
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
    TRY_HIP(hipMalloc(&S.J, sizeof(double)*j_doubles(b)));
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
    S.x_bound = S.J_bound = nullptr;
    S.have_inputs = S.have_Jtx = S.have_cauchy = S.have_gn = false;
    S.norm2_x = S.norm2_cauchy = S.norm2_gn = S.norm2_jtx = 0;
    // (step_to_here of the first point of a solve is read by nobody, but a returned context downloads it)
    DLG_HIP(hipMemsetAsync(S.step, 0, sizeof(double)*(size_t)b->N, b->stream));
  }
  b->factor_slot = -1; b->speculate = false; b->presolve = false; b->pre_slot = -1; b->pre_held = -1; b->pre_hint_valid = false; b->pre_hint_input = false; b->pre_rejected = false; b->pre_split = false;
  b->want_fork = b->fork_recorded = false; b->fork_gate = nullptr;
  b->join_pending = 0;
  b->fold_scalar = b->fold_result = nullptr; b->fold_cauchy_out = nullptr;
  b->fold_p_src = nullptr; b->p_copied = false; b->scal_copied = false; b->fold_scal = 0;
  b->h_part_used = 0; b->pending.clear();
  b->between_fn = nullptr; b->between_cookie = nullptr; b->between_armed = b->between_ran = b->between_redone = false; b->early_slot = -1; b->ident_predict = false;
  if(b->tail_pending) DLG_HIP(hipStreamSynchronize(b->stream));
  b->tail_pending = false; b->defer_tail = false; b->tail_mode = false; b->fold_scal_k7 = 0;
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
extern "C" int dlg_backend_set_between(dlg_backend_t* b, dlg_between_fn fn, void* cookie)
{
  if(!b) return DLG_ERR_ARG;
  b->between_fn = fn; b->between_cookie = fn ? cookie : nullptr;
  return DLG_OK;
}
extern "C" int dlg_backend_between_redone(dlg_backend_t* b) { return (b && b->between_redone) ? 1 : 0; }
// what a between function enqueued is void: the step is made again (another lambda), p_new changes
static void between_drop(dlg_backend* b)
{
  if(!b->between_ran) return;
  b->between_ran = false; b->between_redone = true;
  if(b->early_slot >= 0 && b->type == DLG_SPARSE) sparse_spec_invalidate(b, b->early_slot);
  b->early_slot = -1;
}
// The first pass over the next point's J, enqueued from a between function: what dlg_point_eval launches first (K1 + K4 in
// one kernel, the Jt*x record sums behind it) with the inputs given -- the slot's bound inputs are not touched: the
// caller binds them when its turn comes, dlg_point_eval then recognises them
extern "C" int dlg_point_eval_early(dlg_backend_t* b, int s, const double* x_dev, const double* J_dev, int* done)
{
  if(done) *done = 0;
  if(!b || s < 0 || s > 1 || !x_dev || !J_dev) { dlg_set_error("dlg_point_eval_early: bad arguments"); return DLG_ERR_ARG; }
  if(b->type != DLG_SPARSE || !b->sym || !b->speculate || !b->fuse_eval || b->sharded() || b->part_nranks > 1 || b->pre_slot >= 0) return DLG_OK;
  DlgSlot& S = b->slot[s];
  const double* ox = S.x_bound; const double* oJ = S.J_bound;
  S.x_bound = x_dev; S.J_bound = J_dev;
  int fused = 0;
  const int rc = sparse_eval_assemble(b, s, &fused);
  S.x_bound = ox; S.J_bound = oJ;
  DLG_CHECK(rc);
  if(fused) { b->early_slot = s; b->early_x = x_dev; b->early_J = J_dev; }
  if(done) *done = fused;
  return DLG_OK;
}
// Before anything overwrites what a tail that is still out reads (the step vector, p_new, J of its slot): the tail is a
// launch on the backend's own stream, so whatever is enqueued there is behind it already.
static double ei_out(dlg_backend* b, double v)
{
  if(b->ei_flip > 0 && ++b->ei_count == b->ei_flip) return -fabs(v);
  return v;
}
// ... p_new of such a step travels on the copy stream behind the step kernel's event (dlg_take_step): what writes the
// slot's p or the caller's buffer next waits for it here (long over by then: the copy starts when the step kernel ends)
static int tail_guard(dlg_backend* b)
{
  if(b->p_side_pending) { b->p_side_pending = false; DLG_HIP(hipEventSynchronize(b->ev_copy)); }
  return DLG_OK;
}
extern "C" int dlg_step_tail(dlg_backend_t* b, double* expected_improvement)
{
  if(!b) return DLG_ERR_ARG;
  if(b->tail_pending)
  {
    if(b->tail_mark == b->sync_mark && !(b->tail_ident && b->tail_no_fold)) DLG_HIP(hipStreamSynchronize(b->stream));      // (nobody has waited for anything behind K8 yet -- and K8 carries something: sums or p_new)
    double v = 0.0;
    if(b->tail_ident) v = b->tail_nJs;                                // (from the solved system: that K8 returned at once)
    else for(int i = 0; i < b->tail_nb; i++) v += b->h_tail[i];     // in index order, as dlg_resolve_pending adds them
    b->tail_value = ei_out(b, -2.0*b->tail_inner - v);               // dogleg.c:1107-1109
    b->ei_from_system = b->tail_ident;
    b->tail_pending = false; b->tail_ident = false;
  }
  DLG_CHECK(tail_guard(b));                                          // (p_new on the copy stream)
  if(expected_improvement) *expected_improvement = b->tail_value;
  return DLG_OK;
}
extern "C" int dlg_step_tail_pending(dlg_backend_t* b) { return (b && b->tail_pending) ? 1 : 0; }
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
static int allreduce(dlg_backend* b, double* buf, size_t count)
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
int dlg_allreduce_dev(dlg_backend* b, double* buf, size_t count) { return allreduce(b, buf, count); }

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
  for(int i = 0; i < 3 && rc == DLG_OK; i++) rc = allreduce(b, buf, count);          // warm-up
  DLG_HIP(hipStreamSynchronize(b->stream));
  const auto t0 = std::chrono::steady_clock::now();
  DLG_HIP(hipEventRecord(e0, b->stream));
  for(int i = 0; i < iters && rc == DLG_OK; i++) rc = allreduce(b, buf, count);
  DLG_HIP(hipEventRecord(e1, b->stream));
  DLG_HIP(hipStreamSynchronize(b->stream));
  const double wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(buf);
  // (back to back on one stream: the larger of the device time between the events and the host's wall time)
  *us_each = std::max((double)ms*1e3, wall_us)/iters;
  return rc;
}

// ------------------------------------------------------------------ inputs --
static int step_unprepare(dlg_backend* b);
static int check_slot(dlg_backend* b, int s)
{
  if(!b || s < 0 || s > 1) { dlg_set_error("bad backend/slot"); return DLG_ERR_ARG; }
  return DLG_OK;
}
static void invalidate(DlgSlot& S)
{
  S.have_Jtx = S.have_cauchy = S.have_gn = false;
  S.ident_ok = false;
}

// |J step|^2 without a pass over J.  The Cauchy step is a = kappa g with kappa = -|g|^2 / |J g|^2 (dogleg.c:605): |J a|^2 =
// kappa^2 |J g|^2, K3's own scalar.  The Gauss-Newton step b solves (JtJ + lambda I) b = -g, so
// |J b|^2 = b' JtJ b = -<g, b> - lambda |b|^2 and <J a, J b> = a' JtJ b = -<a, g> - lambda <a, b> = -kappa |g|^2 - lambda <a, b>;
// the interpolated step is (1 - k) a + k b (dogleg.c:964-987).  The error of the last two against the pass over J is b' r
// with r the residual of the solve, i.e. eps * cond(JtJ + lambda I) along b relative to <g, b> -- first order in the
// factor's backward error, where computeExpectedImprovement's pass over J (dogleg.c:1085-1165) has a second-order one.  The
// caller uses them only where the step kernel's estimate of that error is small (k_part_take_step, dlg_backend::
// IDENT_ERR_MAX): the value is then within about 2e-12 (relative) of the exact one.  (lambda > 0: -<g, b> and
// lambda |b|^2 may cancel in |J b|^2 alone, but not in the expected improvement, which carries -2 <g, step> beside it.)
static double ident_norm2_Jstep(int kind, double k, double trustregion, double g2, double Jg2, double n2c, double g_dot_gn,
                                double lambda, double n2g, double a_dot_gn)
{
  const double kappa = -g2/Jg2;
  const double Ja2 = kappa*kappa*Jg2;
  const double Jb2 = -g_dot_gn - lambda*n2g, JaJb = -kappa*g2 - lambda*a_dot_gn;
  switch(kind)
  {
  case DLG_KIND_CAUCHY_TO_EDGE: { const double sc = trustregion/sqrt(n2c); return sc*sc*Ja2; }      // dogleg.c:1204-1207
  case DLG_KIND_GAUSSNEWTON:    return Jb2;
  default:                      return (1.0 - k)*(1.0 - k)*Ja2 + 2.0*k*(1.0 - k)*JaJb + k*k*Jb2;
  }
}

static int tail_guard(dlg_backend* b);
extern "C" int dlg_point_set_p(dlg_backend_t* b, int s, const double* p_host)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(tail_guard(b));
  DLG_HIP(hipMemcpyAsync(b->slot[s].p, p_host, sizeof(double)*(size_t)b->N, hipMemcpyHostToDevice,
                         b->stream));
  DLG_HIP(hipStreamSynchronize(b->stream));     // p_host may be pageable / reused
  return DLG_OK;
}

extern "C" int dlg_point_upload(dlg_backend_t* b, int s, const double* x_host, const double* J_host)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  if(b->type == DLG_DENSE_PRODUCTS) { dlg_set_error("use dlg_point_upload_products"); return DLG_ERR_ARG; }
  DLG_CHECK(tail_guard(b));                     // (a K8 behind the decision point may still be reading this slot's J)
  DlgSlot& S = b->slot[s];
  S.x_bound = S.J_bound = nullptr;
  if(b->early_slot == s) b->early_slot = -1;
  // a sharded rank uploads only its own rows: x[row0:row1] and the J entries of those rows
  const size_t mloc = (size_t)dlg_mloc(b);
  if(mloc > 0)
    DLG_HIP(hipMemcpyAsync(S.x, x_host, sizeof(double)*mloc, hipMemcpyHostToDevice, b->stream));
  const size_t jn = (b->type == DLG_DENSE) ? mloc*(size_t)b->N : sparse_local_nnz(b);
  if(jn > 0)
    DLG_HIP(hipMemcpyAsync(S.J, J_host, sizeof(double)*jn, hipMemcpyHostToDevice, b->stream));
  S.have_inputs = true;
  invalidate(S);
  if(b->factor_slot == s) b->factor_slot = -1;
  if(b->type == DLG_SPARSE) sparse_spec_invalidate(b, s);
  return DLG_OK;
}

extern "C" int dlg_point_upload_products(dlg_backend_t* b, int s, double norm2x, const double* Jtx_host,
                                         const double* JtJ_host)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  if(b->type != DLG_DENSE_PRODUCTS) { dlg_set_error("not a dense-products backend"); return DLG_ERR_ARG; }
  DlgSlot& S = b->slot[s];
  S.x_bound = S.J_bound = nullptr;
  DLG_HIP(hipMemcpyAsync(S.Jt_x, Jtx_host, sizeof(double)*(size_t)b->N, hipMemcpyHostToDevice, b->stream));
  DLG_HIP(hipMemcpyAsync(S.J, JtJ_host, sizeof(double)*j_doubles(b), hipMemcpyHostToDevice, b->stream));
  S.norm2_x = norm2x;
  S.have_inputs = true;
  invalidate(S);
  if(b->factor_slot == s) b->factor_slot = -1;
  return DLG_OK;
}

extern "C" int dlg_point_bind_device(dlg_backend_t* b, int s, const double* x_dev, const double* J_dev)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  DlgSlot& S = b->slot[s];
  S.x_bound = x_dev; S.J_bound = J_dev;
  S.have_inputs = true;
  invalidate(S);
  if(b->factor_slot == s) b->factor_slot = -1;
  // (inputs whose first pass is on the stream already -- dlg_point_eval_early -- keep it)
  const bool early = b->early_slot == s && b->early_x == x_dev && b->early_J == J_dev;
  if(b->early_slot == s && !early) b->early_slot = -1;
  if(b->type == DLG_SPARSE && !early) sparse_spec_invalidate(b, s);
  return DLG_OK;
}

static int cauchy_fork_begin(dlg_backend* b);
// what step_prepare enqueued is not going to be used: the factor it displaced is the held one again
static int step_unprepare(dlg_backend* b)
{
  if(b->pre_slot < 0) return DLG_OK;
  b->pre_slot = -1;
  b->want_fork = b->fork_recorded = false; b->fork_gate = nullptr;
  const int held = b->pre_held;
  b->pre_held = -1;
  if(b->type != DLG_SPARSE) return DLG_OK;
  // (a rejected trial point, dogleg.c:1455-1468: whatever of its K5 + K6 has not started yet is not worth starting --
  // the retry from the cached vectors of the other point, README.pod:49, is behind them on this stream)
  if(!b->knobs.no_abandon) DLG_CHECK(sparse_abandon_enqueued(b));
  b->pre_split = false;
  // ... and the next trial point is expected to go the same way (rejections come in runs while the trust region
  // shrinks, dogleg.c:1455-1468): its evaluation enqueues nothing ahead -- a retry then costs what the reference's
  // does, K7 + K8 + the evaluation -- until a step is taken from a fresh point again (dlg_take_step)
  b->pre_rejected = true;
  if(held < 0) { sparse_release_held(b); return DLG_OK; }
  bool restored = false;
  DLG_CHECK(sparse_restore_factor(b, &restored, b->knobs.no_abandon));      // (the abandon re-armed the pivot flag)
  b->factor_slot = restored ? held : -1;
  return DLG_OK;
}
// K5 + K6 of slot s enqueued ahead of the caller's decision to step from it (dlg_point_eval, one-pass form:
// the panels are the ones assembled beside Jt*x), at the lambda of the last factorisation.  dlg_take_step
// picks them up if it is called for this slot at this lambda (pre_slot / pre_lambda); any other use of the
// slot factorises again.  Nothing is fetched here: the pivot flag comes back with the step's scalars.
static int step_prepare(dlg_backend* b, int s)
{
  DlgSlot& S = b->slot[s];
  // the lambda the next step is expected to ask for: the one the last step ended with (the reference's lambda is
  // sticky, dogleg.c:138, 671-672) -- or, for a caller that was seen to start over from its own value, the one it passed
  const double lam = b->pre_hint_valid ? b->pre_hint : sparse_current_lambda(b);
  // (a factorisation that would ask the host about its diagonal first -- lambda = 0 on a backend that has broken down there
  // before -- is not enqueued ahead: dlg_take_step's loop makes it, and most likely goes on to the next lambda at once)
  if(sparse_would_look(b, lam)) return DLG_OK;
  b->pre_held = (b->factor_slot >= 0 && b->factor_slot != s) ? b->factor_slot : -1;
  sparse_hold_factor(b);
  b->factor_slot = -1;
  S.have_Jtx = true;                                           // (enqueued: the panels carry it as their right-hand side)
  DLG_CHECK(cauchy_fork_begin(b));
  int good = 0;
  DlgProfCond pc(b);
  // Only what covers the host's round trip goes onto the stream now -- the leaf level (88 us on config #4 against ~45 us
  // until the host has its norms and ~15 us until it is back) --; dlg_take_step enqueues the levels above and the solve
  // behind it, back to back.  A rejected point (step_unprepare) then has one kernel to abandon, not K5 + K6.
  b->defer_factor_sync = true; b->factor_ahead = true;
  const int rc = sparse_factorize(b, s, lam, &good);
  b->defer_factor_sync = false; b->factor_ahead = false;
  if(rc != DLG_OK) b->want_fork = false;
  DLG_CHECK(rc);
  b->pre_split = sparse_factor_pending(b);
  if(!b->pre_split)
  {
    DlgProfScope ps(b, DLG_PROF_K6_SOLVE);
    DLG_CHECK(sparse_solve(b, S.Jt_x, S.gn));
  }
  b->pre_slot = s; b->pre_lambda = lam;
  return DLG_OK;
}

// ---------------------------------------------------------------------- K1 --
extern "C" int dlg_point_eval(dlg_backend_t* b, int s, double* norm2_x, double* Jtx_absmax)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  DlgSlot& S = b->slot[s];
  if(!S.have_inputs) { dlg_set_error("dlg_point_eval: no inputs uploaded for slot %d", s); return DLG_ERR_STATE; }
  if(b->type == DLG_DENSE_PRODUCTS)
  {
    // the callback already reduced over the measurements (dogleg.c:1057-1068)
    DLG_CHECK(k_norm2_absmax(b, S.Jt_x, b->N, b->d_scal + 2));
    DLG_CHECK(dlg_fetch_scalars(b, 4));
  }
  else
  {
    const int mloc = dlg_mloc(b);
    // the caller expects to factorise this point: JtJ is assembled in the same pass over J that forms
    // Jt*x (sparse_eval_assemble) or, where that schedule is not available, on the second stream meanwhile
    int fused = 0;
    // (the pass over J may be on the stream already: dlg_point_eval_early from inside the step before)
    const bool early = b->type == DLG_SPARSE && b->early_slot == s && b->early_x == S.xin() && b->early_J == S.Jin() && b->speculate && b->fuse_eval &&
                       sparse_spec_is(b, s, S.Jin());
    if(b->early_slot == s) b->early_slot = -1;
    if(early) fused = 1;
    else if(b->type == DLG_SPARSE && b->speculate && b->fuse_eval) DLG_CHECK(sparse_eval_assemble(b, s, &fused));
    if(!fused)
    {
      if(b->type == DLG_SPARSE && b->speculate && b->overlap) DLG_CHECK(sparse_assemble_speculative(b, s));
      DlgProfScope ps(b, DLG_PROF_K1_JTX);
      if(b->type == DLG_SPARSE) DLG_CHECK(sparse_eval(b, s)); else DLG_CHECK(dense_eval(b, s));
    }
    DlgProfScope pv(b, DLG_PROF_VEC);
    // norm2_x over the local rows (one-pass evaluation: together with the norms of Jt_x, one launch)
    const bool pair = fused && mloc > 0 && !b->sharded();
    // (a rank of several: |x|^2 of its rows goes straight behind its share of Jt*x -- [Jt_x | |x|^2] is summed over the
    // ranks in place, one collective, no staging copies: rounds 1 - 4 copied N doubles into a reduce buffer and back around
    // the all-reduce, two 1.2 MB copies on the critical stream of every evaluation of config #4)
    double* n2x_dev = b->sharded() ? S.Jt_x + b->N : b->d_scal;
    if(pair) { /* below */ }
    else if(mloc > 0) DLG_CHECK(k_norm2_absmax(b, S.xin(), mloc, n2x_dev));
    else         DLG_HIP(hipMemsetAsync(n2x_dev, 0, 2*sizeof(double), b->stream));
    if(b->sharded())
    {
      DLG_CHECK(allreduce(b, S.Jt_x, (size_t)b->N + 1));
      DLG_HIP(hipMemcpyAsync(b->d_scal, S.Jt_x + b->N, sizeof(double), hipMemcpyDeviceToDevice, b->stream));
    }
    bool norms_on_host = false;
    // The partial-sum stages of JtJ and the norm kernel the host waits for leave the critical stream where the
    // factorisation of this point is going to follow at once (step_prepare): the main stream goes from Jt*x
    // straight to the augmented row and the leaf level, the second stream does norms and stages meanwhile.
    const bool ahead = b->presolve && !b->pre_rejected;
    const bool side = pair && fused && ahead && b->host_finals && b->part_nranks <= 1 && sparse_fin_side_ok(b);
    struct SideGuard { dlg_backend* b; ~SideGuard() { (void)sparse_fin_side_end(b); } } side_guard{b};     // (an error on the way: the main stream is b->stream again)
    if(side) DLG_CHECK(sparse_fin_side_begin(b));
    if(pair)
    {
      // (the event the host waits for rides on the norm kernel where that is the last thing the host reads)
      if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
      b->attach_stop = b->ext_events ? b->ev_fetch : nullptr; b->stop_attached = false;
      const int rcn = k_norm2_absmax_pair(b, S.Jt_x, b->N, b->d_scal + 2, S.xin(), mloc, b->d_scal, &norms_on_host);
      b->attach_stop = nullptr;
      DLG_CHECK(rcn);
    }
    else     DLG_CHECK(k_norm2_absmax(b, S.Jt_x, b->N, b->d_scal + 2));
    if(fused)
    {
      // the scalars go to the host first; the partial-sum stages of JtJ run while the host gets them
      if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
      // (the workgroups of the norm kernel wrote their partial sums to page-locked host memory and the host
      // adds them: nothing to copy then -- the event alone is the point the host waits for)
      if(!norms_on_host) DLG_HIP(hipMemcpyAsync(b->h_scal, b->d_scal, sizeof(double)*4, hipMemcpyDeviceToHost, b->stream));
      if(!(norms_on_host && b->stop_attached)) DLG_HIP(hipEventRecord(b->ev_fetch, b->stream));
      b->stop_attached = false;
      DLG_CHECK(sparse_assemble_finish(b));
      if(side) DLG_CHECK(sparse_fin_side_end(b));
      // the factorisation and the Gauss-Newton solve follow at once (dlg_take_step finds them enqueued): the
      // chip works on them while the host fetches the norms and decides
      if(ahead && !b->sharded() && b->part_nranks <= 1) DLG_CHECK(step_prepare(b, s));
      DLG_HIP(hipEventSynchronize(b->ev_fetch));
      b->sync_mark++;       // (the host has waited for something enqueued behind everything that was on the main stream before this call)
      dlg_resolve_pending(b);
    }
    else DLG_CHECK(dlg_fetch_scalars(b, 4));
    S.norm2_x = b->h_scal[0];
  }
  S.have_Jtx = true;
  S.norm2_jtx = b->h_scal[2];
  // (values that are not numbers may have reached the panels: no partial clear relies on what they hold)
  if(b->type == DLG_SPARSE && !(std::isfinite(S.norm2_x) && std::isfinite(S.norm2_jtx) && std::isfinite(b->h_scal[3]))) sparse_mark_unclean(b);
  if(norm2_x) *norm2_x = S.norm2_x;
  if(Jtx_absmax) *Jtx_absmax = b->h_scal[3];
  return DLG_OK;
}

// |J v|^2 into dev scalar `out` (all-reduced over ranks)
static int norm2_Jv(dlg_backend* b, int s, const double* v, double* out, const double* kind_if_factor_failed = nullptr)
{
  DlgProfScope ps(b, DLG_PROF_K3K8_NORM2JV);
  switch(b->type)
  {
  case DLG_SPARSE:  DLG_CHECK(sparse_norm2_Jv(b, s, v, out, kind_if_factor_failed)); break;
  case DLG_DENSE:   DLG_CHECK(dense_norm2_Jv(b, s, v, out)); break;
  default:          return products_quadform(b, s, v, out);
  }
  return allreduce(b, out, 1);
}

// ---------------------------------------------------------------------- K3 --
// launches only: sc[1] = |J g|^2, sc[2] = |cauchy|^2 (device scalars)
static int cauchy_enqueue(dlg_backend* b, int s, double* sc)
{
  DlgSlot& S = b->slot[s];
  DLG_CHECK(norm2_Jv(b, s, S.Jt_x, sc + 1));
  DLG_CHECK(k_cauchy_finish(b, S.Jt_x, S.norm2_jtx, sc + 1, S.cauchy, b->N, sc + 2));    // |g|^2: from dlg_point_eval
  return DLG_OK;
}
// The Cauchy step beside the factorisation (K3 || K5): the caller sets want_fork before the
// factorisation is enqueued, the factorisation records ev_fork where its latency-bound phase
// begins (or never: then the fork is here, behind it), the Cauchy kernels go to aux_stream behind
// that event and the main stream waits for them before anything reads the Cauchy step.
static int cauchy_fork_begin(dlg_backend* b)
{
  // (one communicator: its collectives stay on ONE stream.  Subtree partition: the pass over J forks off, its
  // scalar is summed over the ranks with the solution on the main stream -- cauchy_fork_enqueue; the other
  // sharded forms keep the Cauchy step in line)
  const bool part = b->type == DLG_SPARSE && b->part_nranks > 1;
  b->want_fork = b->overlap && b->aux_stream && (!b->sharded() || part);
  b->fork_recorded = false; b->fork_gate = nullptr;
  return DLG_OK;
}
// holds the second stream until the one-launch region of the factorisation is on the chip (dlg_fork_gate)
__global__ void k_gate_wait(const int* gate, int epoch, int* status = nullptr)
{
  if(threadIdx.x != 0) return;
  int spins = 0;
  while(__hip_atomic_load(gate, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch)
  {
    __builtin_amdgcn_s_sleep(8);
    if(++spins > (1 << 21))
    {
      // (a launch that never comes.  status == NULL: go on, it is only timing; else the wait ORDERS work and the
      // caller must not use what follows: reported like a hand-off that timed out)
      if(status) atomicOr(status, DLG_HANDOFF_FACTOR);
      break;
    }
  }
}
__global__ void k_raise_word(int* word, int epoch)
{
  if(threadIdx.x == 0) __hip_atomic_store(word, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
int dlg_gate_wait(dlg_backend* b, hipStream_t st, const int* gate, int epoch, bool report)
{
  hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, st, gate, epoch,
                     report ? reinterpret_cast<int*>(b->d_scal + (dlg_backend::NSCAL - 2)) : (int*)nullptr);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}
static int cauchy_fork_enqueue(dlg_backend* b, int s, double* sc)
{
  if(!b->want_fork) return cauchy_enqueue(b, s, sc);
  int* gate = b->fork_recorded ? b->fork_gate : nullptr;
  const int gate_epoch = b->fork_gate_epoch;
  b->fork_gate = nullptr;
  if(!b->fork_recorded) DLG_HIP(hipEventRecord(b->ev_fork, b->stream));
  b->want_fork = false; b->fork_recorded = false;
  if(gate) hipLaunchKernelGGL(k_gate_wait, dim3(1), dim3(64), 0, b->aux_stream, (const int*)gate, gate_epoch, (int*)nullptr);
  else     DLG_HIP(hipStreamWaitEvent(b->aux_stream, b->ev_fork, 0));
  hipStream_t main_stream = b->stream;
  b->stream = b->aux_stream;
  int rc;
  if(b->sharded())
  {
    // the rank's share of |J g|^2 only; its sum over the ranks rides with the solution (sparse_solve), the rest
    // of the Cauchy step follows there (cauchy_deferred_finish)
    DlgProfScope ps(b, DLG_PROF_K3K8_NORM2JV);
    rc = sparse_norm2_Jv(b, s, b->slot[s].Jt_x, sc + 1);
    b->fold_scalar = sc + 1; b->fold_result = nullptr; b->fold_cauchy_out = sc + 2;
  }
  else rc = cauchy_enqueue(b, s, sc);
  // The panel buffer the factorisation of this step swapped out (the previous factor: nobody's any more once the step is
  // being taken) is cleared HERE, on the second stream behind the Cauchy step -- behind the fork, so behind everything the
  // main stream had enqueued before the factorisation's one-launch region; in front of the join, so in front of the step
  // kernels and of the next assembly on the main stream.  Behind the step kernel (step_finish) the clear sat between a
  // step and the next evaluation's pass over J: 8 us of the critical queue, 13 with the gap in front of it.
  if(rc == DLG_OK && b->type == DLG_SPARSE && !b->sharded() && b->part_nranks <= 1) rc = sparse_zero_spare(b, main_stream);
  b->stream = main_stream;
  DLG_CHECK(rc);
  if(b->d_join && !b->sharded())
  {
    // (no event: the word goes up behind the Cauchy step, k_negate_interp1 polls it)
    hipLaunchKernelGGL(k_raise_word, dim3(1), dim3(64), 0, b->aux_stream, b->d_join, ++b->join_epoch);
    DLG_LAUNCH_CHECK();
    b->join_pending = b->join_epoch;
  }
  else
  {
    DLG_HIP(hipEventRecord(b->ev_join, b->aux_stream));
    DLG_HIP(hipStreamWaitEvent(b->stream, b->ev_join, 0));
  }
  if(b->type == DLG_SPARSE) DLG_CHECK(sparse_touch_factor(b, b->aux_stream));     // (behind the join: a hint nobody waits for)
  return DLG_OK;
}

// behind the solve that carried the Cauchy step's scalar through its sum over the ranks
static int cauchy_deferred_finish(dlg_backend* b, int s)
{
  if(!b->fold_cauchy_out) return DLG_OK;
  double* out = b->fold_cauchy_out;
  b->fold_cauchy_out = nullptr;
  const double* jg2 = b->fold_result;
  if(!jg2)
  {
    // (the solve had no sum over the ranks to offer: the scalar gets its own)
    double* own = const_cast<double*>(b->fold_scalar);
    b->fold_scalar = nullptr;
    if(!own) { dlg_set_error("internal error: the Cauchy step's scalar was lost"); return DLG_ERR_STATE; }
    DLG_CHECK(dlg_allreduce_dev(b, own, 1));
    jg2 = own;
  }
  b->fold_result = nullptr;
  DlgSlot& S = b->slot[s];
  return k_cauchy_finish(b, S.Jt_x, S.norm2_jtx, jg2, S.cauchy, b->N, out);
}

extern "C" int dlg_cauchy(dlg_backend_t* b, int s, double* norm2_updateCauchy)
{
  DLG_CHECK(check_slot(b, s));
  DlgSlot& S = b->slot[s];
  if(!S.have_Jtx) { dlg_set_error("dlg_cauchy needs Jt_x (reference dogleg.c:551-555)"); return DLG_ERR_STATE; }
  if(!S.have_cauchy)
  {
    DLG_CHECK(cauchy_enqueue(b, s, b->d_scal));
    DLG_CHECK(dlg_fetch_scalars(b, 3));
    S.norm2_cauchy = b->h_scal[2];
    S.Jg2 = b->sharded() ? 0.0 : b->h_scal[1];       // (|J Jt_x|^2: ident_norm2_Jstep; a rank of several holds a partial sum there)
    S.have_cauchy = true;
  }
  if(norm2_updateCauchy) *norm2_updateCauchy = S.norm2_cauchy;
  return DLG_OK;
}

// ----------------------------------------------------------------- K4 + K5 --
extern "C" int dlg_factorize(dlg_backend_t* b, int s, double lambda, int* ok)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  DlgSlot& S = b->slot[s];
  if(!S.have_inputs) { dlg_set_error("dlg_factorize: slot %d has no J/JtJ", s); return DLG_ERR_STATE; }
  int good = 0;
  switch(b->type)
  {
  case DLG_SPARSE: DLG_CHECK(sparse_factorize(b, s, lambda, &good)); break;
  case DLG_DENSE:  DLG_CHECK(dense_factorize(b, s, lambda, &good)); break;
  default:         DLG_CHECK(products_factorize(b, s, lambda, &good)); break;
  }
  if(b->profiling) dlg_prof_resolve(b);
  b->factor_slot = good ? s : -1;
  if(b->factor_doomed) b->factor_doomed = false;            // (sparse_factorize noted the breakdown itself)
  else if(!good && b->type == DLG_SPARSE) (void)sparse_note_breakdown(b);
  if(ok) *ok = good;
  return DLG_OK;
}

// ---------------------------------------------------------------------- K6 --
extern "C" int dlg_solve_gn(dlg_backend_t* b, int s, double* norm2_updateGN)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  DlgSlot& S = b->slot[s];
  if(!S.have_Jtx) { dlg_set_error("dlg_solve_gn needs Jt_x"); return DLG_ERR_STATE; }
  if(b->factor_slot != s) { dlg_set_error("dlg_solve_gn: no factorization of slot %d is held", s); return DLG_ERR_STATE; }
  if(!S.have_gn)
  {
    {
      DlgProfScope ps(b, DLG_PROF_K6_SOLVE);
      if(b->type == DLG_SPARSE) DLG_CHECK(sparse_solve(b, S.Jt_x, S.gn));
      else                      DLG_CHECK(dense_solve(b, S.Jt_x, S.gn));
    }
    DLG_CHECK(k_negate_norm2(b, S.gn, b->N, b->d_scal));      // dogleg.c:862-865
    DLG_CHECK(dlg_fetch_scalars(b, 1));
    S.norm2_gn = b->h_scal[0];
    S.have_gn = true; S.ident_ok = false;
  }
  if(norm2_updateGN) *norm2_updateGN = S.norm2_gn;
  return DLG_OK;
}

// ------------------------------------------------------------- K4+K5+K6 ----
// The reference's compute_updateGN (dogleg.c:822-908) starts with the factorisation
// (dogleg.c:825 -> 634-820, including the lambda loop 656-677 / 806-815) and solves right after it.
// Fused here so that one attempt costs ONE host synchronisation: the factorisation is enqueued,
// the solve is enqueued behind it, and the pivot flag is read together with |gn|^2 (a failed
// factorisation replaces its bad pivots by 1, so the speculative solve cannot fault).
static int gauss_newton_impl(dlg_backend_t* b, int s, double* lambda_io, double* norm2_updateGN,
                            bool with_cauchy, double* norm2_updateCauchy)
{
  DLG_CHECK(check_slot(b, s));
  DLG_CHECK(step_unprepare(b));
  if(!lambda_io) { dlg_set_error("dlg_gauss_newton: lambda_io is NULL"); return DLG_ERR_ARG; }
  DlgSlot& S = b->slot[s];
  if(!S.have_inputs) { dlg_set_error("dlg_gauss_newton: slot %d has no J/JtJ", s); return DLG_ERR_STATE; }
  if(!S.have_Jtx) { dlg_set_error("dlg_gauss_newton needs Jt_x"); return DLG_ERR_STATE; }
  bool cauchy_pending = false;
  if(b->factor_slot == s && S.have_gn)                       // both cached (dogleg.c:637, 825)
  {
    if(with_cauchy) DLG_CHECK(dlg_cauchy(b, s, norm2_updateCauchy));
    if(norm2_updateGN) *norm2_updateGN = S.norm2_gn;
    return DLG_OK;
  }
  double lam = *lambda_io;
  for(;;)
  {
    int good = 0, rc;
    // the Cauchy step rides along (its scalars come back with the same synchronisation), on the
    // second stream beside the factorisation
    const bool do_cauchy = with_cauchy && !S.have_cauchy && !cauchy_pending;
    if(do_cauchy) DLG_CHECK(cauchy_fork_begin(b));
    if(b->factor_slot != s)
    {
      DlgProfCond pc(b);
      b->defer_factor_sync = true;
      switch(b->type)
      {
      case DLG_SPARSE: rc = sparse_factorize(b, s, lam, &good); break;
      case DLG_DENSE:  rc = dense_factorize(b, s, lam, &good); break;
      default:         rc = products_factorize(b, s, lam, &good); break;
      }
      b->defer_factor_sync = false;
      if(rc != DLG_OK) b->want_fork = false;
      DLG_CHECK(rc);
      if(b->factor_doomed)
      {
        // (found doomed at the diagonal, in front of every launch -- sparse_factorize: the next lambda at once)
        b->factor_doomed = false; b->want_fork = false; b->factor_slot = -1;
        if(b->profiling) { dlg_prof_resolve(b); dlg_prof_commit(b, false); }
        lam = (lam == 0.0) ? 1e-10 : lam*10.0;                    // dogleg.c:138, 671-672, 812-813
        if(!(lam < 1e300)) { dlg_set_error("lambda overflowed while regularising a singular JtJ"); return DLG_ERR_STATE; }
        continue;
      }
    }
    if(do_cauchy)
    {
      DLG_CHECK(cauchy_fork_enqueue(b, s, b->d_scal + 4));
      cauchy_pending = true;
    }
    {
      DlgProfCond pc(b);
      DlgProfScope ps(b, DLG_PROF_K6_SOLVE);
      if(b->type == DLG_SPARSE) DLG_CHECK(sparse_solve(b, S.Jt_x, S.gn));
      else                      DLG_CHECK(dense_solve(b, S.Jt_x, S.gn));
    }
    DLG_CHECK(cauchy_deferred_finish(b, s));
    DLG_CHECK(k_negate_norm2(b, S.gn, b->N, b->d_scal));      // dogleg.c:862-865
    DLG_CHECK(dlg_fetch_scalars(b, dlg_backend::NSCAL));      // the one synchronisation (the sparse pivot flag rides in the last slot)
    if(b->profiling) dlg_prof_resolve(b);
    if(cauchy_pending && !S.have_cauchy) { S.norm2_cauchy = b->h_scal[6]; S.Jg2 = b->sharded() ? 0.0 : b->h_scal[5]; S.have_cauchy = true; }
    good = (b->factor_slot == s) ? 1 : (b->type == DLG_SPARSE ? sparse_factor_ok(b) : dense_factor_ok(b));
    if(b->profiling) dlg_prof_commit(b, good != 0);
    if(good) break;
    if(b->type == DLG_SPARSE && !sparse_note_breakdown(b)) sparse_mark_unclean(b);          // (a factorisation that broke down: full clears next -- unless nothing of it ran)
    b->factor_slot = -1;
    if(b->tail_pending) { DLG_CHECK(tail_guard(b)); b->tail_pending = false; }     // (that attempt's K8 returned at its first look at the pivot flag)
    lam = (lam == 0.0) ? 1e-10 : lam*10.0;                    // dogleg.c:138, 671-672, 812-813
    if(!(lam < 1e300)) { dlg_set_error("lambda overflowed while regularising a singular JtJ"); return DLG_ERR_STATE; }
  }
  b->factor_slot = s;
  S.norm2_gn = b->h_scal[0];
  S.have_gn = true; S.ident_ok = false;        // (<Jt x, gn> is formed by dlg_take_step only)
  *lambda_io = lam;
  if(norm2_updateGN) *norm2_updateGN = S.norm2_gn;
  if(with_cauchy && norm2_updateCauchy) *norm2_updateCauchy = S.norm2_cauchy;
  return DLG_OK;
}
extern "C" int dlg_gauss_newton(dlg_backend_t* b, int s, double* lambda_io, double* norm2_updateGN)
{ return gauss_newton_impl(b, s, lambda_io, norm2_updateGN, false, nullptr); }
// K3 + K4 + K5 + K6 behind one synchronisation: the Cauchy step (dogleg.c:529-617) is issued in
// front of the Gauss-Newton work of dlg_gauss_newton.  For callers that expect to need both (the
// driver does once a step has left the trust region's edge behind).
extern "C" int dlg_cauchy_gauss_newton(dlg_backend_t* b, int s, double* lambda_io, double* norm2_updateCauchy,
                                       double* norm2_updateGN)
{ return gauss_newton_impl(b, s, lambda_io, norm2_updateGN, true, norm2_updateCauchy); }

// ---------------------------------------------------------------------- K7 --
// launches the step kernel (its scalars land in d_scal[0..2]); nscal = how many to fetch
static int make_step_enqueue(dlg_backend* b, int from, int to, int kind, double trustregion, int* nscal)
{
  DlgSlot& F = b->slot[from];
  DlgSlot& T = b->slot[to];
  DlgProfScope ps(b, DLG_PROF_K7_STEP);
  switch(kind)
  {
  case DLG_KIND_CAUCHY_TO_EDGE:
    if(!F.have_cauchy) { dlg_set_error("cauchy step not computed"); return DLG_ERR_STATE; }
    DLG_CHECK(k_scaled_step(b, F.cauchy, trustregion / sqrt(F.norm2_cauchy), F.p, T.step, T.p, b->N,
                            b->d_scal));                          // dogleg.c:1204-1207
    *nscal = 1;
    break;
  case DLG_KIND_GAUSSNEWTON:
    if(!F.have_gn) { dlg_set_error("GN step not computed"); return DLG_ERR_STATE; }
    DLG_CHECK(k_scaled_step(b, F.gn, 1.0, F.p, T.step, T.p, b->N, b->d_scal));   // dogleg.c:1231
    *nscal = 1;
    break;
  case DLG_KIND_INTERPOLATED:
    if(!F.have_cauchy || !F.have_gn) { dlg_set_error("interpolation needs cauchy and GN"); return DLG_ERR_STATE; }
    DLG_CHECK(k_interpolate(b, F.cauchy, F.gn, F.norm2_cauchy, trustregion, F.p, T.step, T.p, b->N,
                            b->d_scal));
    *nscal = 3;
    break;
  default:
    dlg_set_error("dlg_make_step: unknown kind %d", kind);
    return DLG_ERR_ARG;
  }
  return DLG_OK;
}
static void make_step_read(dlg_backend* b, int from, int kind, double* n2, double* kk, double* amax)
{
  DlgSlot& F = b->slot[from];
  *kk = NAN;
  switch(kind)
  {
  case DLG_KIND_CAUCHY_TO_EDGE: *n2 = F.norm2_cauchy; *amax = b->h_scal[0]; break;   // unscaled: dogleg.c:1200
  case DLG_KIND_GAUSSNEWTON:    *n2 = F.norm2_gn;     *amax = b->h_scal[0]; break;
  default:                      *n2 = b->h_scal[0]; *kk = b->h_scal[1]; *amax = b->h_scal[2]; break;
  }
}
// scalars and (optionally) p_new back to the host behind ONE synchronisation
static int step_finish(dlg_backend* b, int to, int nscal, double* p_new_host)
{
  DlgSlot& T = b->slot[to];
  // (unless the step's last kernel has written them to the page-locked h_scal itself: sparse_norm2_Jv)
  bool attached = b->stop_attached && b->scal_copied && !p_new_host;      // (the step's last kernel carries ev_fetch)
  b->stop_attached = false;
  if(!b->scal_copied) DLG_HIP(hipMemcpyAsync(b->h_scal, b->d_scal, sizeof(double)*(size_t)nscal, hipMemcpyDeviceToHost, b->stream));
  b->scal_copied = false;
  bool pinned = true;
  if(p_new_host)
  {
    // page-locked destination (the driver's operating points, dlg_host_alloc): straight DMA;
    // pageable: through the backend's pinned staging vector
    hipPointerAttribute_t attr;
    pinned = hipPointerGetAttributes(&attr, p_new_host) == hipSuccess && attr.type == hipMemoryTypeHost;
    if(!pinned) (void)hipGetLastError();
    double* dst = pinned ? p_new_host : b->h_vec;
    DLG_HIP(hipMemcpyAsync(dst, T.p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->stream));
  }
  // The host only waits for what it reads.  Behind that point the stream clears the panel buffer a
  // factorisation left behind (sparse_zero_spare): the GPU does it while the host digests the step and
  // evaluates the next point, and that point's assembly finds the buffer zeroed.
  if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
  if(!attached) DLG_HIP(hipEventRecord(b->ev_fetch, b->stream));
  if(b->type == DLG_SPARSE) DLG_CHECK(sparse_zero_spare(b));
  // (the caller's work for the stream that needs no scalar of this step: dlg_backend_set_between)
  if(b->between_armed && b->between_fn)
  {
    b->between_armed = false; b->between_ran = true;
    dlg_between_fn fn = b->between_fn; void* ck = b->between_cookie;
    b->between_fn = nullptr; b->between_cookie = nullptr;
    fn(ck);
  }
  DLG_HIP(hipEventSynchronize(b->ev_fetch));
  b->sync_mark++;
  dlg_resolve_pending(b);
  if(p_new_host && !pinned) memcpy(p_new_host, b->h_vec, sizeof(double)*(size_t)b->N);
  return nscal >= dlg_backend::NSCAL ? dlg_check_handoff(b) : DLG_OK;
}
extern "C" int dlg_make_step(dlg_backend_t* b, int from, int to, int kind, double trustregion,
                             double* norm2_step, double* k_cauchy_to_gn, double* step_absmax,
                             double* p_new_host)
{
  DLG_CHECK(check_slot(b, from)); DLG_CHECK(check_slot(b, to));
  if(from == to) { dlg_set_error("dlg_make_step: from == to"); return DLG_ERR_ARG; }
  // (a step from the cached vectors of `from` after the trial point was rejected: what dlg_point_eval enqueued for
  // the trial point is dropped and the factor it displaced is the held one again BEFORE step_finish clears the
  // spare panel buffer -- which is where the displaced factor lives)
  DLG_CHECK(step_unprepare(b));
  DLG_CHECK(tail_guard(b)); b->tail_pending = false;
  double n2 = 0, kk = NAN, amax = 0;
  int nscal = 0;
  DLG_CHECK(make_step_enqueue(b, from, to, kind, trustregion, &nscal));
  DLG_CHECK(step_finish(b, to, nscal, p_new_host));
  make_step_read(b, from, kind, &n2, &kk, &amax);
  if(norm2_step) *norm2_step = n2;
  if(k_cauchy_to_gn) *k_cauchy_to_gn = kk;
  if(step_absmax) *step_absmax = amax;
  return DLG_OK;
}

// ---------------------------------------------------------------------- K8 --
static int expected_improvement_enqueue(dlg_backend* b, int from, int to, double* sc)
{
  DlgSlot& F = b->slot[from];
  DlgSlot& T = b->slot[to];
  if(!F.have_Jtx) { dlg_set_error("expected improvement needs Jt_x"); return DLG_ERR_STATE; }
  DLG_CHECK(k_inner(b, F.Jt_x, T.step, b->N, sc));
  DLG_CHECK(norm2_Jv(b, from, T.step, sc + 1));
  return DLG_OK;
}
extern "C" int dlg_expected_improvement(dlg_backend_t* b, int from, int to, double* out)
{
  DLG_CHECK(check_slot(b, from)); DLG_CHECK(check_slot(b, to));
  DLG_CHECK(expected_improvement_enqueue(b, from, to, b->d_scal));
  DLG_CHECK(dlg_fetch_scalars(b, 2));
  if(out) { *out = ei_out(b, -2.0*b->h_scal[0] - b->h_scal[1]); b->tail_value = *out; b->ei_from_system = false; }              // dogleg.c:1107-1109
  return DLG_OK;
}
// K7 + K8 behind one synchronisation: the step (dlg_make_step), its expected improvement
// (dlg_expected_improvement, dogleg.c:1258-1269 computes it right after the step) and p_new
extern "C" int dlg_step(dlg_backend_t* b, int from, int to, int kind, double trustregion,
                        double* norm2_step, double* k_cauchy_to_gn, double* step_absmax,
                        double* expected_improvement, double* p_new_host)
{
  DLG_CHECK(check_slot(b, from)); DLG_CHECK(check_slot(b, to));
  if(from == to) { dlg_set_error("dlg_step: from == to"); return DLG_ERR_ARG; }
  DLG_CHECK(step_unprepare(b));                 // (as in dlg_make_step: the driver's retry after a rejected trial point)
  DLG_CHECK(tail_guard(b)); b->tail_pending = false;
  b->between_armed = b->between_fn != nullptr; b->between_ran = false; b->between_redone = false;      // dlg_backend_set_between
  struct BetweenGuard { dlg_backend* b; ~BetweenGuard() { b->between_armed = false; b->between_fn = nullptr; } } between_guard{b};
  double n2 = 0, kk = NAN, amax = 0;
  int nscal = 0;
  // The deferred form (dlg_backend_set_defer_tail): the host waits for the kernel that forms <Jt x, step> -- every scalar of the
  // step reaches it through page-locked partial sums, nothing is copied on the main stream
  hipPointerAttribute_t pa;
  const bool pin = p_new_host && hipPointerGetAttributes(&pa, p_new_host) == hipSuccess && pa.type == hipMemoryTypeHost && pa.devicePointer;
  if(p_new_host && !pin) (void)hipGetLastError();
  const int chunks = b->type == DLG_SPARSE ? sparse_norm2_chunks(b) : (b->type == DLG_DENSE ? dense_norm2_chunks(b) : 0);
  const bool defer = b->defer_tail && expected_improvement && b->host_finals && b->h_part && !b->sharded() && (!p_new_host || pin) &&
                     !(b->prof_mask >> DLG_PROF_K3K8_NORM2JV & 1u) && !(b->prof_mask >> DLG_PROF_K7_STEP & 1u) && b->ext_events &&
                     chunks > 0 && b->slot[from].have_Jtx && b->h_part_used + 4096 <= dlg_backend::HPART_CAP &&      // (room for the step's partial sums: 4 x 1024 at most)
                     dlg_tail_partials(b, chunks) != nullptr;
  // The expected improvement from the solved system (ident_norm2_Jstep): a step from the cached vectors of a point whose
  // dlg_take_step left <Jt x, gn> and the factor's verdict behind -- or the Cauchy step, which needs K3's scalar only --
  // has no pass over J at all: step, <Jt x, step>, one synchronisation.  In the deferred form p_new travels on the copy
  // stream behind that kernel's event and dlg_step_tail hands the value out (it is complete, the copy may not be).
  {
    DlgSlot& F = b->slot[from];
    const bool ident = expected_improvement && !b->knobs.ei_jpass && b->host_finals && !b->sharded() && b->part_nranks <= 1 &&
                       b->type != DLG_DENSE_PRODUCTS && F.have_Jtx && F.have_cauchy && F.Jg2 > 0.0 &&
                       (kind == DLG_KIND_CAUCHY_TO_EDGE || (F.ident_ok && F.have_gn));
    if(ident)
    {
      const bool deferred = defer && (!p_new_host || b->copy_stream);
      b->kout_host = deferred;
      const int rcm = make_step_enqueue(b, from, to, kind, trustregion, &nscal);
      b->kout_host = false;
      DLG_CHECK(rcm);
      if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
      if(deferred) { b->attach_stop = b->ev_fetch; b->stop_attached = false; }
      const int rci = k_inner(b, F.Jt_x, b->slot[to].step, b->N, b->d_scal + 4);
      const bool attached = deferred && b->stop_attached;
      b->attach_stop = nullptr; b->stop_attached = false;
      DLG_CHECK(rci);
      if(attached)
      {
        if(p_new_host)
        {
          DLG_HIP(hipStreamWaitEvent(b->copy_stream, b->ev_fetch, 0));
          DLG_HIP(hipMemcpyAsync(p_new_host, b->slot[to].p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->copy_stream));
          DLG_HIP(hipEventRecord(b->ev_copy, b->copy_stream));
          b->p_side_pending = true;
        }
        b->stop_attached = true; b->scal_copied = true;          // (nothing to copy: every scalar is a sum of page-locked partials)
        DLG_CHECK(step_finish(b, to, 0, nullptr));
      }
      else
      {
        if(deferred)
        {
          // (no room for the partial sums in page-locked memory: the in-line form; an interpolation whose partial sums DID
          // find room has written k to the page-locked block itself)
          b->scal_copied = false;
          bool k_on_host = false;
          for(const dlg_backend::PendingFinal& f : b->pending) if(f.dst == 0 && f.stride == 2) k_on_host = true;
          if(k_on_host && kind == DLG_KIND_INTERPOLATED)
          {
            DLG_HIP(hipMemcpyAsync(b->h_scal + 2, b->d_scal + 2, sizeof(double)*4, hipMemcpyDeviceToHost, b->stream));
            b->scal_copied = true;
          }
        }
        DLG_CHECK(step_finish(b, to, 6, p_new_host));
      }
      make_step_read(b, from, kind, &n2, &kk, &amax);
      if(norm2_step) *norm2_step = n2;
      if(k_cauchy_to_gn) *k_cauchy_to_gn = kk;
      if(step_absmax) *step_absmax = amax;
      const double nJs = ident_norm2_Jstep(kind, kk, trustregion, F.norm2_jtx, F.Jg2, F.norm2_cauchy, F.g_dot_gn, F.ident_lam, F.norm2_gn, F.a_dot_gn);
      if(attached)
      {
        b->tail_pending = true; b->tail_ident = true; b->tail_nJs = nJs; b->tail_no_fold = true;
        b->tail_inner = b->h_scal[4]; b->tail_mark = b->sync_mark;
        *expected_improvement = NAN;                             // (dlg_step_tail has it, and p_new complete)
        return DLG_OK;
      }
      *expected_improvement = ei_out(b, -2.0*b->h_scal[4] - nJs);
      b->tail_value = *expected_improvement; b->ei_from_system = true;
      return DLG_OK;
    }
  }
  // K8 behind the decision point (dlg_backend_set_defer_tail), as in dlg_take_step: the host waits for the kernel that
  // forms <Jt x, step> -- every scalar of the step reaches it through page-locked partial sums, nothing is copied --,
  // the pass over J and p_new follow on the stream, dlg_step_tail has the value
  {
    if(defer)
    {
      DlgSlot& F = b->slot[from];
      DlgSlot& T = b->slot[to];
      b->kout_host = true;
      const int rcm = make_step_enqueue(b, from, to, kind, trustregion, &nscal);
      b->kout_host = false;
      DLG_CHECK(rcm);
      if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
      b->attach_stop = b->ev_fetch; b->stop_attached = false;
      const int rci = k_inner(b, F.Jt_x, T.step, b->N, b->d_scal + 4);
      const bool attached = b->stop_attached;
      b->attach_stop = nullptr; b->stop_attached = false;
      DLG_CHECK(rci);
      if(attached)
      {
        if(pin) { b->fold_p_src = T.p; b->fold_p_dst = (double*)pa.devicePointer; }
        b->tail_mode = true; b->fold_scal = 0;
        const int rct = b->type == DLG_SPARSE ? sparse_norm2_Jv(b, from, T.step, b->d_scal + 5, nullptr) : dense_norm2_Jv(b, from, T.step, b->d_scal + 5);
        b->tail_mode = false;
        b->fold_p_src = nullptr; b->p_copied = false;
        DLG_CHECK(rct);
        b->tail_pending = true;
        b->stop_attached = true; b->scal_copied = true;          // (nothing to copy: every scalar is a sum of page-locked partials)
        DLG_CHECK(step_finish(b, to, 0, nullptr));
        b->tail_mark = b->sync_mark;
        b->tail_inner = b->h_scal[4];
        make_step_read(b, from, kind, &n2, &kk, &amax);
        if(norm2_step) *norm2_step = n2;
        if(k_cauchy_to_gn) *k_cauchy_to_gn = kk;
        if(step_absmax) *step_absmax = amax;
        *expected_improvement = NAN;                             // (dlg_step_tail has it)
        return DLG_OK;
      }
      // (the sum <Jt x, step> found no room for its partial sums in page-locked memory -- k_inner ran with a second stage on
      // the device instead and took no event along: the step is formed, the rest follows in the in-line form, as in dlg_take_step)
      b->stop_attached = false; b->scal_copied = false;
      DLG_CHECK(norm2_Jv(b, from, T.step, b->d_scal + 5));
      // (kout_host: an interpolation whose partial sums DID find room has written k to the page-locked block itself)
      bool k_on_host = false;
      for(const dlg_backend::PendingFinal& f : b->pending) if(f.dst == 0 && f.stride == 2) k_on_host = true;
      if(k_on_host && kind == DLG_KIND_INTERPOLATED)
      {
        DLG_HIP(hipMemcpyAsync(b->h_scal + 2, b->d_scal + 2, sizeof(double)*4, hipMemcpyDeviceToHost, b->stream));
        b->scal_copied = true;
      }
      DLG_CHECK(step_finish(b, to, 6, p_new_host));
      make_step_read(b, from, kind, &n2, &kk, &amax);
      if(norm2_step) *norm2_step = n2;
      if(k_cauchy_to_gn) *k_cauchy_to_gn = kk;
      if(step_absmax) *step_absmax = amax;
      *expected_improvement = ei_out(b, -2.0*b->h_scal[4] - b->h_scal[5]); b->tail_value = *expected_improvement; b->ei_from_system = false;
      return DLG_OK;
    }
  }
  DLG_CHECK(make_step_enqueue(b, from, to, kind, trustregion, &nscal));
  // p_new is final here: it travels to the host on the side stream while K8 runs (a page-locked
  // destination; a pageable one goes through step_finish's staging copy afterwards)
  bool side_copy = false;
  if(p_new_host && b->copy_stream)
  {
    hipPointerAttribute_t attr;
    const bool pinned = hipPointerGetAttributes(&attr, p_new_host) == hipSuccess && attr.type == hipMemoryTypeHost;
    if(!pinned) (void)hipGetLastError();
    if(pinned)
    {
      DLG_HIP(hipEventRecord(b->ev_step, b->stream));
      DLG_HIP(hipStreamWaitEvent(b->copy_stream, b->ev_step, 0));
      DLG_HIP(hipMemcpyAsync(p_new_host, b->slot[to].p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->copy_stream));
      DLG_HIP(hipEventRecord(b->ev_copy, b->copy_stream));
      side_copy = true;
    }
  }
  DLG_CHECK(expected_improvement_enqueue(b, from, to, b->d_scal + 4));
  DLG_CHECK(step_finish(b, to, 6, side_copy ? nullptr : p_new_host));
  if(side_copy) DLG_HIP(hipEventSynchronize(b->ev_copy));
  make_step_read(b, from, kind, &n2, &kk, &amax);
  if(norm2_step) *norm2_step = n2;
  if(k_cauchy_to_gn) *k_cauchy_to_gn = kk;
  if(step_absmax) *step_absmax = amax;
  if(expected_improvement) { *expected_improvement = ei_out(b, -2.0*b->h_scal[4] - b->h_scal[5]); b->tail_value = *expected_improvement; b->ei_from_system = false; }
  return DLG_OK;
}

// ------------------------------------------------ K3 .. K8, one round trip ----
// takeStepFrom (dogleg.c:1172-1297) for a point with nothing cached, behind ONE host synchronisation:
// Cauchy step, factorise + solve (lambda loop as in dlg_gauss_newton), the choice between the three
// kinds of step made on the device (k_take_step), the step, its expected improvement, p_new.
// out = {|cauchy|^2, |gn|^2, kind, |step|^2 as the reference reports it, k_cauchy_to_gn, max|step|,
// expected improvement}.  The Gauss-Newton step is computed speculatively (for callers that expect
// to need it: the driver, once a step has needed it); when the Cauchy step turns out to be the one
// taken it is discarded together with its factorisation and *lambda_io is left alone, as in the
// reference, which does not factorise on that branch (|gn|^2 is then reported as NaN).
extern "C" int dlg_take_step(dlg_backend_t* b, int from, int to, double trustregion, double* lambda_io,
                             double* out7, double* p_new_host)
{
  DLG_CHECK(check_slot(b, from)); DLG_CHECK(check_slot(b, to));
  if(from == to) { dlg_set_error("dlg_take_step: from == to"); return DLG_ERR_ARG; }
  if(!lambda_io || !out7) { dlg_set_error("dlg_take_step: NULL argument"); return DLG_ERR_ARG; }
  DlgSlot& F = b->slot[from];
  DlgSlot& T = b->slot[to];
  if(!F.have_inputs) { dlg_set_error("dlg_take_step: slot %d has no J/JtJ", from); return DLG_ERR_STATE; }
  if(!F.have_Jtx) { dlg_set_error("dlg_take_step needs Jt_x"); return DLG_ERR_STATE; }
  if(!b->d_gnpart) DLG_HIP(hipMalloc(&b->d_gnpart, sizeof(double)*4096));      // |gn|^2 partials, then the pivots' partial minima / maxima (k_negate_interp1)
  double lam = *lambda_io;
  bool side_copy = false, ident_used = false, k8_omitted = false;
  double ident_nJs = 0.0;
  // (the factorisation and the solve enqueued by dlg_point_eval -- step_prepare -- are this step's if the
  // lambda is the one they were formed at; they are used once)
  const double lam_in = lam;
  if(b->pre_slot == from && b->pre_lambda != lam) b->pre_hint_input = true;      // (the guess was wrong: this caller does not keep lambda)
  const bool prepared_here = b->pre_slot == from && b->pre_lambda == lam;
  bool pre_split = prepared_here && b->pre_split;          // (the prepared factorisation stopped behind its leaf level: the rest is enqueued here)
  if(prepared_here) { b->pre_slot = -1; b->pre_held = -1; b->pre_split = false; if(b->type == DLG_SPARSE) sparse_release_held(b); } else DLG_CHECK(step_unprepare(b));
  bool prepared = prepared_here;
  b->pre_rejected = false;                     // (a step from a fresh point: the point before it was accepted)
  DLG_CHECK(tail_guard(b));
  b->tail_pending = false;
  b->between_armed = b->between_fn != nullptr; b->between_ran = false; b->between_redone = false;      // dlg_backend_set_between
  struct BetweenGuard { dlg_backend* b; ~BetweenGuard() { b->between_armed = false; b->between_fn = nullptr; } } between_guard{b};
  // Where p_new goes: a page-locked destination is written by the step's pass over J itself (K8, a slice per workgroup)
  hipPointerAttribute_t p_attr;
  const bool p_pinned = p_new_host && b->copy_stream && hipPointerGetAttributes(&p_attr, p_new_host) == hipSuccess && p_attr.type == hipMemoryTypeHost;
  if(p_new_host && b->copy_stream && !p_pinned) (void)hipGetLastError();
  const bool p_foldable = p_pinned && b->host_finals && !b->sharded() && p_attr.devicePointer;
  // K8 behind the decision point (dlg_backend_set_defer_tail): the step kernel is what the host waits for
  const int tail_chunks = b->type == DLG_SPARSE ? sparse_norm2_chunks(b) : (b->type == DLG_DENSE ? dense_norm2_chunks(b) : 0);
  bool defer = b->defer_tail && b->host_finals && !b->sharded() &&
                     (!p_new_host || p_foldable) && !(b->prof_mask >> DLG_PROF_K3K8_NORM2JV & 1u) &&
                     tail_chunks > 0 && dlg_tail_partials(b, tail_chunks) != nullptr;
  // (the dense pass over J takes p_new along only in that form)
  bool p_fold = p_foldable && (b->type == DLG_SPARSE || (b->type == DLG_DENSE && defer));
  // The expected improvement from the solved system instead of a pass over J (ident_norm2_Jstep): one rank, the host adds the
  // partial sums; the sparse backward solve leaves the factor's pivots' minima / maxima per supernode for the step kernel
  const bool ident_try = !b->knobs.ei_jpass && b->host_finals && !b->sharded() && b->part_nranks <= 1 && b->type != DLG_DENSE_PRODUCTS &&
                         (!F.have_cauchy || F.Jg2 > 0.0);
  int ident_nmm = 0; long ident_stride = 2;
  const double* ident_mm = (ident_try && b->type == DLG_SPARSE) ? sparse_pivot_minmax(b, &ident_nmm) : nullptr;
  if(ident_try && b->type == DLG_DENSE && b->G) { ident_mm = b->G; ident_nmm = b->N; ident_stride = (long)b->N + 1; }      // (the diagonal of the dense factor)
  b->ident_launched = false;
  for(;;)
  {
    int good = 0, rc;
    double* n2c_dev = b->d_scal + 6;
    const bool do_cauchy = !F.have_cauchy;
    if(do_cauchy) { if(!prepared) DLG_CHECK(cauchy_fork_begin(b)); }
    else
    {
      b->want_fork = b->fork_recorded = false; b->fork_gate = nullptr;
      DLG_HIP(hipMemcpyAsync(n2c_dev, &F.norm2_cauchy, sizeof(double), hipMemcpyHostToDevice, b->stream));
    }
    if(prepared)
    {
      // K5 is on the stream already -- or its leaf level is, and the levels above follow here
      if(pre_split)
      {
        DlgProfCond pc(b);
        bool was = false;
        const int rcr = sparse_factorize_rest(b, &was);
        if(rcr != DLG_OK) b->want_fork = false;
        DLG_CHECK(rcr);
      }
    }
    else if(b->factor_slot != from)
    {
      DlgProfCond pc(b);
      b->defer_factor_sync = true;
      switch(b->type)
      {
      case DLG_SPARSE: rc = sparse_factorize(b, from, lam, &good); break;
      case DLG_DENSE:  rc = dense_factorize(b, from, lam, &good); break;
      default:         rc = products_factorize(b, from, lam, &good); break;
      }
      b->defer_factor_sync = false;
      if(rc != DLG_OK) b->want_fork = false;
      DLG_CHECK(rc);
      if(b->factor_doomed)
      {
        // (found doomed at the diagonal, in front of every launch -- sparse_factorize: the next lambda at once)
        b->factor_doomed = false; b->want_fork = false; b->factor_slot = -1;
        if(b->profiling) { dlg_prof_resolve(b); dlg_prof_commit(b, false); }
        lam = (lam == 0.0) ? 1e-10 : lam*10.0;                    // dogleg.c:138, 671-672, 812-813
        if(!(lam < 1e300)) { dlg_set_error("lambda overflowed while regularising a singular JtJ"); return DLG_ERR_STATE; }
        continue;
      }
    }
    if(do_cauchy) DLG_CHECK(cauchy_fork_enqueue(b, from, b->d_scal + 4));     // K3 beside K5 (second stream)
    if(!prepared || pre_split)
    {
      DlgProfCond pc(b);
      DlgProfScope ps(b, DLG_PROF_K6_SOLVE);
      if(b->type == DLG_SPARSE) DLG_CHECK(sparse_solve(b, F.Jt_x, F.gn));
      else                      DLG_CHECK(dense_solve(b, F.Jt_x, F.gn));
    }
    prepared = false; pre_split = false;
    DLG_CHECK(cauchy_deferred_finish(b, from));
    int nbg = 0;
    if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
    {
      DlgProfScope ps(b, DLG_PROF_K7_STEP);
      DLG_CHECK(k_negate_interp1(b, F.gn, F.cauchy, b->N, b->d_gnpart, &nbg, ident_mm, ident_nmm, ident_stride));      // dogleg.c:862-865, 964-972
      if(defer)
      {
        // (the last kernel on the main stream: it takes the scalars to the host and carries the event the host waits for)
        b->fold_scal_k7 = dlg_backend::NSCAL;
        b->attach_stop = (b->ext_events && !(b->prof_mask >> DLG_PROF_K7_STEP & 1u)) ? b->ev_fetch : nullptr; b->stop_attached = false;
      }
      const int rc7 = k_take_step(b, F.cauchy, F.gn, b->d_gnpart, nbg, n2c_dev, trustregion, F.p, T.step, T.p, b->N,
                                  b->d_scal, b->d_scal + 8, F.Jt_x, b->d_scal + 11,
                                  ident_try ? b->d_scal + dlg_backend::GB_SLOT : (double*)nullptr,
                                  ident_try ? b->d_scal + dlg_backend::IDENT_SLOT : (double*)nullptr,
                                  ident_mm != nullptr, true, dlg_backend::IDENT_RATIO_MAX, F.norm2_jtx, dlg_backend::IDENT_ERR_MAX);
      b->fold_scal_k7 = 0; b->attach_stop = nullptr;
      DLG_CHECK(rc7);
    }
    side_copy = false;
    b->fold_p_src = nullptr; b->p_copied = false;
    if(defer && !b->scal_copied)
    {
      // (the step kernel could not take the scalars along -- no room left for its partial sums in page-locked memory --:
      // this step in the in-line form, K8 in front of the synchronisation)
      defer = false;
      p_fold = p_foldable && b->type == DLG_SPARSE;
      b->stop_attached = false;
    }
    if(defer)
    {
      // K8 right behind the step kernel on the same stream -- but the host is already on its way back when it runs: its
      // partial sums and p_new land in page-locked memory, the event rides on the launch (dlg_step_tail waits for it).
      // (On the second stream beside the next evaluation it gained nothing: that evaluation's pass over J is bound by HBM
      // as K8 is -- 131 + 0 us against 98 + 38 -- and the wait for the event between the queues cost 18 us.)
      const bool k7_attached = b->stop_attached;
      // p_new: on the copy stream behind the step kernel's own event (the one the host listens to: no event more on the main
      // stream) -- the pass over J, which may return at once (k8_skip), does not have to carry 8 N bytes over PCIe on the
      // critical queue (1.2 MB, ~25 us on config #4); dlg_step_tail / tail_guard wait for the copy
      const bool p_side = p_fold && k7_attached && b->copy_stream;
      if(p_side)
      {
        DLG_HIP(hipStreamWaitEvent(b->copy_stream, b->ev_fetch, 0));
        DLG_HIP(hipMemcpyAsync(p_new_host, T.p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->copy_stream));
        DLG_HIP(hipEventRecord(b->ev_copy, b->copy_stream));
        b->p_side_pending = true;
      }
      else if(p_fold) { b->fold_p_src = T.p; b->fold_p_dst = (double*)p_attr.devicePointer; }
      b->tail_no_fold = p_side || !p_fold;
      // No event of its own (a launch somebody listens to holds the next dispatch back by ~5 us): the evaluation that
      // follows is waited for on this stream behind it -- dlg_step_tail only waits itself if nothing was (sync_mark).
      b->tail_mode = true; b->fold_scal = 0; b->attach_stop = nullptr; b->stop_attached = false;
      // The pass over J is not even launched where the step kernel is expected to let it return at once -- the last step of
      // this backend did (ident_predict), lambda is 0 again, and the launch would carry nothing else (p_new is on the copy
      // stream): a launch that returns at once is still 5 - 6 us on the critical queue.  The device's word is the judge: if
      // it says the pass is needed after all, it is launched behind the wait (below), late but the same pass.
      k8_omitted = b->ident_launched && b->ident_predict && b->tail_no_fold && !b->knobs.no_k8_predict;
      int rct = DLG_OK;
      if(!k8_omitted)
      {
        b->k8_skip = b->ident_launched ? b->d_scal + dlg_backend::IDENT_SLOT : nullptr;
        rct = b->type == DLG_SPARSE ? sparse_norm2_Jv(b, from, T.step, b->d_scal + 12, b->d_scal + 8)
                                    : dense_norm2_Jv(b, from, T.step, b->d_scal + 12);
      }
      b->tail_mode = false; b->k8_skip = nullptr;
      b->fold_p_src = nullptr; b->p_copied = false;
      DLG_CHECK(rct);
      b->tail_pending = true;
      b->stop_attached = k7_attached; b->scal_copied = true;
      DLG_CHECK(step_finish(b, to, dlg_backend::NSCAL, nullptr));
      b->tail_mark = b->sync_mark;              // (that wait was for the step kernel, in front of K8)
      b->tail_inner = b->h_scal[11];
    }
    else
    {
    if(p_new_host && b->copy_stream)
    {
      const hipPointerAttribute_t& attr = p_attr;
      const bool pinned = p_pinned;
      if(p_fold)
      {
        // page-locked destination: the step's last kernel (K8) writes p_new there itself, a slice per
        // workgroup -- no event between the step kernel and K8 for a copy on the side stream to wait on
        b->fold_p_src = T.p; b->fold_p_dst = (double*)attr.devicePointer;
      }
      else if(pinned)
      {
        DLG_HIP(hipEventRecord(b->ev_step, b->stream));
        DLG_HIP(hipStreamWaitEvent(b->copy_stream, b->ev_step, 0));
        DLG_HIP(hipMemcpyAsync(p_new_host, T.p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->copy_stream));
        DLG_HIP(hipEventRecord(b->ev_copy, b->copy_stream));
        side_copy = true;
      }
    }
    b->fold_scal = dlg_backend::NSCAL;       // (the last kernel of the step: it takes the scalars to the host with it)
    b->attach_stop = (b->ext_events && !side_copy && !(b->prof_mask >> DLG_PROF_K3K8_NORM2JV & 1u)) ? b->ev_fetch : nullptr; b->stop_attached = false;   // ... and the event the host waits for
    int rc8;
    b->k8_skip = b->ident_launched ? b->d_scal + dlg_backend::IDENT_SLOT : nullptr;
    { DlgProfCond pc(b); rc8 = norm2_Jv(b, from, T.step, b->d_scal + 12, b->d_scal + 8); }   // the other half of the expected improvement (returns early behind a failed factorisation unless the step is the Cauchy step)
    b->attach_stop = nullptr; b->k8_skip = nullptr;
    b->fold_scal = 0;
    const bool p_done = b->p_copied;
    b->fold_p_src = nullptr; b->p_copied = false;
    DLG_CHECK(rc8);
    DLG_CHECK(step_finish(b, to, dlg_backend::NSCAL, (side_copy || p_done) ? nullptr : p_new_host));   // the one synchronisation
    if(side_copy) DLG_HIP(hipEventSynchronize(b->ev_copy));
    }
    if(b->profiling) dlg_prof_resolve(b);
    if(!F.have_cauchy) { F.norm2_cauchy = b->h_scal[6]; F.Jg2 = b->h_scal[5]; F.have_cauchy = true; }
    // the step kernel let the pass over J return at once: |J step|^2 from the solved system
    ident_used = b->ident_launched && b->h_scal[dlg_backend::IDENT_SLOT] != 0.0 && F.Jg2 > 0.0;
    if(b->ident_launched && !ident_used && b->h_scal[dlg_backend::IDENT_SLOT] != 0.0)
    { dlg_set_error("internal error: the expected improvement's pass over J was skipped without |J Jt_x|^2 at hand"); return DLG_ERR_STATE; }
    if(ident_used)
      ident_nJs = ident_norm2_Jstep((int)b->h_scal[8], b->h_scal[9], trustregion, F.norm2_jtx, F.Jg2, F.norm2_cauchy, b->h_scal[dlg_backend::GB_SLOT],
                                    lam, b->h_scal[10], F.norm2_cauchy - b->h_scal[dlg_backend::IDENT_SLOT + 4]);
    if(defer) { b->tail_ident = ident_used; b->tail_nJs = ident_nJs; }
    if(b->ident_launched) b->ident_predict = ident_used;
    if(defer && k8_omitted && !ident_used)
    {
      // (the step kernel wants the pass over J after all -- another pivot range than last time: behind the wait, in the
      // tail's own form; dlg_step_tail waits for it)
      b->tail_mode = true; b->fold_scal = 0; b->attach_stop = nullptr; b->stop_attached = false; b->k8_skip = nullptr;
      const int rcl = b->type == DLG_SPARSE ? sparse_norm2_Jv(b, from, T.step, b->d_scal + 12, b->d_scal + 8)
                                            : dense_norm2_Jv(b, from, T.step, b->d_scal + 12);
      b->tail_mode = false;
      DLG_CHECK(rcl);
      b->tail_mark = b->sync_mark;
    }
    k8_omitted = false;
    if((int)b->h_scal[8] == DLG_KIND_CAUCHY_TO_EDGE)
    {
      // The Cauchy step was the one taken: the reference never factorises on this branch
      // (dogleg.c:1192-1211), so the speculative Gauss-Newton work is dropped -- no cached factor,
      // no cached GN step, and above all no change of the (sticky) lambda, whether or not the
      // speculative factorisation succeeded.
      b->factor_slot = -1;
      F.have_gn = false;
      out7[0] = F.norm2_cauchy; out7[1] = NAN; out7[2] = (double)DLG_KIND_CAUCHY_TO_EDGE;
      out7[3] = F.norm2_cauchy;                                 // unscaled: dogleg.c:1200
      out7[4] = NAN;
      out7[5] = b->h_scal[2];
      out7[6] = defer ? NAN : ei_out(b, -2.0*b->h_scal[11] - (ident_used ? ident_nJs : b->h_scal[12]));             // dogleg.c:1107-1109 (NaN: dlg_step_tail has it)
      if(!defer) { b->tail_value = out7[6]; b->ei_from_system = ident_used; }
      if(b->profiling) dlg_prof_commit(b, b->type == DLG_SPARSE ? sparse_factor_ok(b) : dense_factor_ok(b));
      return DLG_OK;
    }
    good = (b->factor_slot == from) ? 1 : (b->type == DLG_SPARSE ? sparse_factor_ok(b) : dense_factor_ok(b));
    if(b->profiling) dlg_prof_commit(b, good != 0);
    if(good) break;
    if(b->type == DLG_SPARSE && !sparse_note_breakdown(b)) sparse_mark_unclean(b);          // (a factorisation that broke down: full clears next -- unless nothing of it ran)
    b->factor_slot = -1;
    between_drop(b);                                          // (the step is made again: what the caller enqueued behind it is void)
    lam = (lam == 0.0) ? 1e-10 : lam*10.0;                    // dogleg.c:138, 671-672, 812-813
    if(!(lam < 1e300)) { dlg_set_error("lambda overflowed while regularising a singular JtJ"); return DLG_ERR_STATE; }
  }
  b->factor_slot = from;
  F.norm2_gn = b->h_scal[10];
  F.have_gn = true;
  *lambda_io = lam;
  b->pre_hint = b->pre_hint_input ? lam_in : lam; b->pre_hint_valid = true;
  const int kind = (int)b->h_scal[8];
  out7[0] = F.norm2_cauchy; out7[1] = F.norm2_gn; out7[2] = (double)kind;
  out7[3] = (kind == DLG_KIND_CAUCHY_TO_EDGE) ? F.norm2_cauchy : (kind == DLG_KIND_GAUSSNEWTON ? F.norm2_gn : b->h_scal[0]);
  out7[4] = b->h_scal[9];
  out7[5] = b->h_scal[2];
  out7[6] = defer ? NAN : ei_out(b, -2.0*b->h_scal[11] - (ident_used ? ident_nJs : b->h_scal[12]));               // dogleg.c:1107-1109 (NaN: dlg_step_tail has it)
  if(!defer) { b->tail_value = out7[6]; b->ei_from_system = ident_used; }
  b->pivot_ratio = b->ident_launched ? b->h_scal[dlg_backend::IDENT_SLOT + 1] : NAN;
  // (a retry from the cached vectors of this point, dlg_step, takes the same route: <Jt x, gn> and the factor's verdict)
  F.g_dot_gn = b->h_scal[dlg_backend::GB_SLOT];
  F.ident_ok = b->ident_launched && ident_mm != nullptr && b->h_scal[dlg_backend::IDENT_SLOT] == 1.0;      // (the factor's verdict, not the Cauchy step's)
  F.ident_lam = lam; F.a_dot_gn = F.norm2_cauchy - b->h_scal[dlg_backend::IDENT_SLOT + 4];
  return DLG_OK;
}

// ---- the hot path of one trial step, nsteps times: what driver.hip does for a fresh operating point once steps
// need the Gauss-Newton step -- inputs bound (here: resident copies of (x, J), rotated), dlg_point_eval,
// dlg_take_step from lambda0 -- as ONE C call, so that a timed loop carries the host overhead of the C driver
// and not that of an interpreter calling the three entry points (bench.py).  Same entry points, same two host
// synchronisations per step.  out9 (may be NULL) = {|x|^2, |cauchy|^2, |gn|^2, k, |step|^2, expected
// improvement, max|Jt x|, max|step|, lambda} of the last step; *kind_out its kind of step.
extern "C" int dlg_run_steps(dlg_backend_t* b, int from, int to, int nsteps, int ncopy, const double* const* x_dev,
                             const double* const* J_dev, int first_copy, double trustregion, double lambda0,
                             double* out9, int* kind_out)
{
  DLG_CHECK(check_slot(b, from)); DLG_CHECK(check_slot(b, to));
  if(nsteps < 0 || ncopy < 1 || !x_dev || !J_dev) { dlg_set_error("dlg_run_steps: bad arguments"); return DLG_ERR_ARG; }
  double n2x = 0, gmax = 0, lam = lambda0, tail = 0, o[7] = {0, 0, 0, 0, 0, 0, 0};
  // (as the driver's device-callback solves do, driver.hip take_step: the next point's first pass over J goes onto the
  // stream from inside the step, in front of the host's wait for the step's scalars -- dlg_backend_set_between)
  struct Next { dlg_backend* b; int slot; const double* x; const double* J; };
  auto next_fn = [](void* c) { Next* n = static_cast<Next*>(c); int done = 0; (void)dlg_point_eval_early(n->b, n->slot, n->x, n->J, &done); };
  for(int i = 0; i < nsteps; i++)
  {
    const int c = (first_copy + i) % ncopy;
    DLG_CHECK(dlg_point_bind_device(b, from, x_dev[c], J_dev[c]));
    DLG_CHECK(dlg_point_eval(b, from, &n2x, &gmax));
    Next nx{b, from, x_dev[(c + 1) % ncopy], J_dev[(c + 1) % ncopy]};
    if(i + 1 < nsteps && b->defer_tail && !b->knobs.no_between) DLG_CHECK(dlg_backend_set_between(b, next_fn, &nx));
    // (dlg_backend_set_defer_tail: the expected improvement of the step before is fetched where the driver needs it --
    // behind the evaluation of the trial point, dogleg.c:1410-1427; its pass over J ran beside that evaluation)
    DLG_CHECK(dlg_step_tail(b, &tail));
    lam = lambda0;
    DLG_CHECK(dlg_take_step(b, from, to, trustregion, &lam, o, b->h_vec));      // p_new travels to the host (page-locked), as for the driver
  }
  if(b->defer_tail && nsteps > 0) { DLG_CHECK(dlg_step_tail(b, &tail)); if(std::isnan(o[6])) o[6] = tail; }
  if(out9) { out9[0] = n2x; out9[1] = o[0]; out9[2] = o[1]; out9[3] = o[4]; out9[4] = o[3]; out9[5] = o[6]; out9[6] = gmax; out9[7] = o[5]; out9[8] = lam; }
  if(kind_out) *kind_out = (int)o[2];
  return DLG_OK;
}

// ------------------------------------- the users of the held factor (factor_users.hip)
// What every entry point that works with the factor held for slot s asks once, behind its own argument checks: a valid
// backend and slot, no other ranks where the call has no multi-GPU form, nothing enqueued ahead for a step that has not
// been taken (step_unprepare), the inputs it reads (DLG_NEEDS_J: the slot's Jacobian on the device), the factor of this
// slot, and the pattern the plans are built against.  DLG_ERR_ARG for the handle, DLG_ERR_STATE for everything else.
int dlg_factor_user_begin(dlg_backend* b, int s, const char* who, unsigned needs)
{
  DLG_CHECK(check_slot(b, s));
  if(((needs & DLG_NEEDS_UNSHARDED) && b->sharded()) || ((needs & DLG_NEEDS_UNPARTITIONED) && b->part_nranks > 1))
  { dlg_set_error("%s is not available on a sharded or partitioned backend", who); return DLG_ERR_STATE; }
  DLG_CHECK(step_unprepare(b));
  if((needs & DLG_NEEDS_J) && b->type == DLG_DENSE_PRODUCTS) { dlg_set_error("%s needs J: a dense-products backend keeps none", who); return DLG_ERR_STATE; }
  if((needs & DLG_NEEDS_J) && !b->slot[s].have_inputs) { dlg_set_error("%s needs x and J of slot %d", who, s); return DLG_ERR_STATE; }
  if(b->factor_slot != s) { dlg_set_error("%s: no factorization of slot %d is held", who, s); return DLG_ERR_STATE; }
  if((needs & DLG_NEEDS_PATTERN) && b->type == DLG_SPARSE && !b->sym) { dlg_set_error("%s: no sparse pattern", who); return DLG_ERR_STATE; }
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
  case DLG_VEC_J:      *n = j_doubles(b); return const_cast<double*>(S.Jin());
  case DLG_VEC_X_OWN:  *n = (size_t)b->M; return S.x;
  case DLG_VEC_J_OWN:  *n = j_doubles(b); return S.J;
  default:             return nullptr;
  }
}
extern "C" int dlg_point_download(dlg_backend_t* b, int s, int which, double* host, size_t n)
{
  DLG_CHECK(check_slot(b, s));
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
