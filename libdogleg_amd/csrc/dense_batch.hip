// dense_batch.hip -- the host side of the batch solver: what is kept between calls (the cache), and one call path per kind of
// request of dense_batch.h -- the solve (solve_locked: the rounds), and the uncertainty and query calls (evaluate_at: one
// callback and ONE launch; with the fit of the ..._fit entry points, whose weights and held set travel with the inputs).  Each
// path serves the J and the products form, host arrays and the caller's device arrays; the solve and the evaluation calls also
// the model form, which has no callback and no evaluation buffer.  The
// kernels and what they compute: dense_batch_kernels.hip; their arguments and launchers: dense_batch_dev.h.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <mutex>
#include <vector>
#include "dense_batch.h"
#include "dense_batch_dev.h"

void dlg_set_error(const char* fmt, ...);

#define BMSG(...) do { fprintf(stderr, "libdogleg_amd: " __VA_ARGS__); fputc('\n', stderr); } while(0)

namespace {

// ---- what is kept between calls ----
struct BatchCache
{
  int device = -1;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  int* h_counter = nullptr;
  void* d_eval = nullptr; size_t eval_bytes = 0;      // x, J of the trial points; products form: norm2x | xtJ | JtJ
  void* d_state = nullptr; size_t state_bytes = 0;    // everything else
  void* h_stage = nullptr; size_t stage_bytes = 0;    // page-locked: what the uncertainty call uploads and reads back
};
std::mutex g_mu;
BatchCache g_cache;
thread_local double t_stats[3] = {0.0, 0.0, 0.0};
thread_local double t_unc_stats[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

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
    if(K.h_stage) (void)hipHostFree(K.h_stage);
    for(hipEvent_t& e : K.ev) if(e) (void)hipEventDestroy(e);
    if(K.stream) (void)hipStreamDestroy(K.stream);
    if(sw) (void)hipSetDevice(cur);
  }
  K = BatchCache();
}
// a public call: under the lock, and without a cache where the environment says so
template <class Fn> int locked_call(Fn fn)
{
  std::lock_guard<std::mutex> lk(g_mu);
  const int rc = fn();
  if(getenv("DOGLEG_AMD_NO_BACKEND_CACHE")) release_locked();
  return rc;
}

#define BHIP(call) \
  do { hipError_t e__ = (call); \
       if(e__ != hipSuccess) { dlg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
                               BMSG("%s: %s -> %s", who, #call, hipGetErrorString(e__)); (void)hipGetLastError(); return -1; } } while(0)

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// the device, the stream and the page-locked counter of the cache
int cache_open(const char* who)
{
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
  return 0;
}
// the two device buffers of the cache, grown to eval_bytes and state_bytes (M == 0: the products form, for the message)
bool cache_ensure(const char* who, unsigned int B, unsigned int N, unsigned int M, size_t eval_bytes, size_t state_bytes)
{
  BatchCache& K = g_cache;
  auto ensure = [&](void** ptr, size_t* have, size_t want) -> bool {
    if(*have >= want) return true;
    if(*ptr) { (void)hipFree(*ptr); *ptr = nullptr; *have = 0; }
    if(hipMalloc(ptr, want) != hipSuccess)
    {
      (void)hipGetLastError(); *ptr = nullptr;
      dlg_set_error("%s: cannot allocate %zu bytes of device memory", who, want);
      if(M) BMSG("%s: B = %u problems of %u x %u need %zu + %zu bytes of device memory: the allocation of %zu failed", who, B, M, N,
                 eval_bytes, state_bytes, want);
      else  BMSG("%s: B = %u problems of %u variables need %zu bytes of callback output + %zu bytes of state in device memory: "
                 "the allocation of %zu failed", who, B, N, eval_bytes, state_bytes, want);
      return false;
    }
    *have = want;
    return true;
  };
  return ensure(&K.d_eval, &K.eval_bytes, eval_bytes) && ensure(&K.d_state, &K.state_bytes, state_bytes);
}
// the page-locked staging buffer of the host-pointer uncertainty and query calls, grown to io_bytes
bool stage_ensure(const char* who, unsigned int B, unsigned int N, unsigned int M, size_t io_bytes)
{
  BatchCache& K = g_cache;
  if(K.stage_bytes >= io_bytes) return true;
  if(K.h_stage) { (void)hipHostFree(K.h_stage); K.h_stage = nullptr; K.stage_bytes = 0; }
  if(hipHostMalloc(&K.h_stage, io_bytes) != hipSuccess)
  {
    (void)hipGetLastError(); K.h_stage = nullptr;
    dlg_set_error("%s: cannot allocate %zu bytes of page-locked memory", who, io_bytes);
    BMSG("%s: B = %u problems of %u x %u need %zu bytes of page-locked host memory: the allocation failed", who, B, M, N, io_bytes);
    return false;
  }
  K.stage_bytes = io_bytes;
  return true;
}
// segments of a buffer, each aligned to 256 bytes: off = add(bytes)
struct Segments
{
  size_t bytes = 0;
  size_t add(size_t n) { const size_t off = bytes; bytes += align256(n); return off; }
};

// ---- what every call path shares ----
// the callback of a call and what it writes: the J form (fJ: x, J of Nmeas = M rows) or the products form (fP: norm2x,
// xtJ, JtJ; M is 0 there), or the model form (model: no callback, nothing written: the rows are formed inside the sweep)
struct BatchForm
{
  dogleg_callback_device_batch_t* fJ;
  dogleg_callback_device_batch_products_t* fP;
  bool unpacked;               // products: JtJ as N x N
  const dogleg_amd_batch_model_t* model;
  const dogleg_amd_batch_camera_t* camera;     // the model form on a camera record's data (model: its model), or nullptr
  bool products() const { return fP != nullptr; }
  unsigned int S(unsigned int N) const { return unpacked ? N*N : N*(N + 1)/2; }
};
// the evaluation buffer of a call, what the callback writes for B problems: x | J, or norm2x | xtJ | JtJ
struct EvalBuffer
{
  double doubles;              // its size in doubles: B * M * (N + 1) can pass 2^64 bytes, so a call is refused on this
  size_t bytes;
  size_t second, third;        // where J, or xtJ and JtJ, begin
};
EvalBuffer eval_buffer(const BatchForm& F, unsigned int B, unsigned int N, unsigned int M)
{
  EvalBuffer E;
  Segments S;
  if(F.model)
  {
    // the model form: an empty buffer
    E.doubles = 0.0; E.second = 0; E.third = 0;
  }
  else if(F.products())
  {
    E.doubles = (double)B*(1.0 + N + F.S(N));
    S.add(sizeof(double)*(size_t)B); E.second = S.add(sizeof(double)*(size_t)B*N); E.third = S.add(sizeof(double)*(size_t)B*F.S(N));
  }
  else
  {
    E.doubles = (double)B*(double)M*((double)N + 1.0);
    S.add(sizeof(double)*(size_t)B*M); E.second = S.add(sizeof(double)*(size_t)B*M*N); E.third = 0;
  }
  E.bytes = S.bytes;
  return E;
}
// x / J / P of a kernel's argument (BatchDev, UncDev), the buffer at d_eval.  P stays empty in the J form (the launchers tell the
// forms apart by it); x and J are not read in the products form
template <class Dev> void point_at_eval(Dev& A, const BatchForm& F, const EvalBuffer& E, void* d_eval)
{
  char* q = (char*)d_eval;
  A.x = (double*)q; A.J = (double*)(q + (F.products() ? 0 : E.second));
  A.P = ProductsDev{nullptr, nullptr, nullptr, 0};
  if(F.products()) A.P = ProductsDev{(double*)q, (double*)(q + E.second), (double*)(q + E.third), F.unpacked ? 1 : 0};
}
// the caller's callback at the points p of the problems whose live byte is set, into the buffer A points at, on st
template <class Dev> void invoke_callback(const BatchForm& F, const double* p, const Dev& A, const unsigned char* live,
                                          unsigned int B, hipStream_t st, void* cookie)
{
  if(F.products())
    F.fP(p, const_cast<double*>(A.P.n2x), const_cast<double*>(A.P.xtJ), const_cast<double*>(A.P.JtJ), live, B, (void*)st, cookie);
  else
    F.fJ(p, const_cast<double*>(A.x), const_cast<double*>(A.J), live, B, (void*)st, cookie);
}
// whether a call fits, from the arithmetic alone: the evaluation buffer, state_d doubles of state and, for a query call, q's Jq
// and out
bool fits(const char* who, const BatchForm& F, unsigned int B, unsigned int N, unsigned int M, const EvalBuffer& E, double state_d,
          const DlgBatchQuery* q = nullptr)
{
  const double rows_d = q ? (double)B*(double)q->Nq*(double)q->Qrows : 0.0;
  const double Jq_d = rows_d*N*8.0, out_d = q ? rows_d*q->Qrows*8.0 : 0.0;
  const double need = (E.doubles + state_d)*8.0 + Jq_d + out_d;
  if(!(need > 1.0e15)) return true;
  dlg_set_error("%s: %.3g bytes of device memory", who, need);
  if(q)                 BMSG("%s: B = %u problems of %u variables with %u queries of %u rows need %.3g bytes of device memory (%.3g of "
                             "them for Jq, %.3g for out)", who, B, N, q->Nq, q->Qrows, need, Jq_d, out_d);
  else if(F.products()) BMSG("%s: B = %u problems of %u variables need %.3g bytes of device memory", who, B, N, need);
  else                  BMSG("%s: B = %u problems of %u x %u need %.3g bytes of device memory", who, B, M, N, need);
  return false;
}
// DOGLEG_AMD_BATCH_TIMING: the time of the callback and of the library's launch behind it, between three marks on the stream
struct BatchTimer
{
  bool on = false;
  double ms_callback = 0.0, ms_library = 0.0;
  int start(const char* who)
  {
    on = getenv("DOGLEG_AMD_BATCH_TIMING") != nullptr;
    if(on) for(hipEvent_t& e : g_cache.ev) if(!e) BHIP(hipEventCreate(&e));
    return 0;
  }
  int mark(const char* who, int k, hipStream_t st)
  {
    if(on) BHIP(hipEventRecord(g_cache.ev[k], st));
    return 0;
  }
  // behind a synchronisation: adds what lies between the marks
  int read(const char* who)
  {
    if(!on) return 0;
    float a = 0.f, c = 0.f;
    BHIP(hipEventElapsedTime(&a, g_cache.ev[0], g_cache.ev[1])); BHIP(hipEventElapsedTime(&c, g_cache.ev[1], g_cache.ev[2]));
    ms_callback += a; ms_library += c;
    return 0;
  }
};

// the kernels' records of a call's (checked) model and of the camera record it may lie in; empty without a model.  A camera
// record of doubles without calibration is the model form itself: its raw is the model's y
void model_records(const dogleg_amd_batch_model_t* m, const dogleg_amd_batch_camera_t* cam, int likelihood, ModelDev& Md, CameraDev& Cd)
{
  Md = ModelDev{0, 0, 0, 0, nullptr, nullptr, nullptr};
  Cd = CameraDev{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  if(!m) return;
  Md = ModelDev{m->kind, (int)m->width, m->t_per_problem ? 1 : 0, likelihood, m->y, m->t, m->scale};
  if(!cam) return;
  if(!cam->offset && cam->dtype == DOGLEG_AMD_DATA_F64) { Md.y = (const double*)cam->raw; return; }
  Cd = CameraDev{cam->raw, cam->offset, cam->gain_inv, cam->readvar, cam->origin, cam->dtype, (int)cam->sensor_width,
                 (int)(cam->sensor_width - m->width), (int)(cam->sensor_height - m->height), cam->offset ? 1 : 0};
}

// ---- the solve ----
const char* solve_who(const DlgBatchSolve& a)
{
  static const char* const names[5][2] = {
    {"dogleg_amd_optimize_dense_products_batch_bounded", "dogleg_amd_optimize_dense_products_batch_bounded_device"},
    {"dogleg_amd_optimize_dense_products_batch", "dogleg_amd_optimize_dense_products_batch_device"},
    {"dogleg_amd_optimize_dense_batch_bounded", "dogleg_amd_optimize_dense_batch_bounded_device"},
    {"dogleg_amd_optimize_dense_batch_robust", "dogleg_amd_optimize_dense_batch_robust_device"},
    {"dogleg_amd_optimize_dense_batch", "dogleg_amd_optimize_dense_batch_device"}};
  if(a.camera) return a.device ? "dogleg_amd_optimize_dense_batch_camera_device" : "dogleg_amd_optimize_dense_batch_camera";
  if(a.model && a.mle) return a.device ? "dogleg_amd_optimize_dense_batch_model_mle_device" : "dogleg_amd_optimize_dense_batch_model_mle";
  if(a.model) return a.device ? "dogleg_amd_optimize_dense_batch_model_device" : "dogleg_amd_optimize_dense_batch_model";
  return names[a.fP ? (a.bounds ? 0 : 1) : a.bounds ? 2 : a.loss ? 3 : 4][a.device ? 1 : 0];
}
// the cache opened and grown for the solve a, and the kernels' argument pointing into it.  The host route keeps the bounds it is
// given behind the state (A.lo, A.hi); the device route reads the caller's arrays
int batch_setup(const char* who, const DlgBatchSolve& a, const BatchForm& F, BatchDev& A)
{
  const unsigned int B = a.B, N = a.N, M = a.M;
  const dogleg_amd_batch_loss_t* loss = a.loss;
  const dogleg_parameters2_t* prm = a.prm;
  const bool room_lo = !a.device && a.bounds && a.bounds->lower, room_hi = !a.device && a.bounds && a.bounds->upper;
  const int nbounds = (room_lo ? 1 : 0) + (room_hi ? 1 : 0);
  const unsigned int fs = loss ? (loss->featureSize <= 1 ? 1u : (unsigned int)loss->featureSize) : 1u;
  const unsigned int NF = loss ? M/fs : 0;
  if(cache_open(who)) return -1;
  BatchCache& K = g_cache;
  const int NP = (int)(N*(N + 1)/2);
  const EvalBuffer E = eval_buffer(F, B, N, M);
  if(!fits(who, F, B, N, M, E, (double)B*(5.0*N + NP + SC_COUNT + 1.0 + NF + (double)nbounds*N))) return -1;
  const size_t vec_bytes = sizeof(double)*(size_t)B*N;
  Segments S;
  const size_t o_before = S.add(vec_bytes), o_trial = S.add(vec_bytes), o_g = S.add(vec_bytes), o_cauchy = S.add(vec_bytes);
  const size_t o_gn = S.add(vec_bytes), o_JtJ = S.add(sizeof(double)*(size_t)B*NP), o_sc = S.add(sizeof(double)*(size_t)B*SC_COUNT);
  const size_t o_st = S.add(sizeof(int)*(size_t)B*ST_COUNT), o_live = S.add(B), o_counter = S.add(256);
  const size_t o_wts = S.add(sizeof(double)*(size_t)B*NF);
  const size_t o_lo = S.add(room_lo ? vec_bytes : 0), o_hi = S.add(room_hi ? vec_bytes : 0);
  if(!cache_ensure(who, B, N, M, E.bytes, S.bytes)) return -1;

  A.B = (int)B; A.N = (int)N; A.M = (int)M; A.NP = NP;
  point_at_eval(A, F, E, K.d_eval);
  char* q = (char*)K.d_state;
  A.p_before = (double*)(q + o_before); A.p_trial = (double*)(q + o_trial); A.g = (double*)(q + o_g);
  A.cauchy = (double*)(q + o_cauchy); A.gn = (double*)(q + o_gn); A.JtJ = (double*)(q + o_JtJ);
  A.sc = (double*)(q + o_sc); A.st = (int*)(q + o_st); A.live = (unsigned char*)(q + o_live); A.counter = (int*)(q + o_counter);
  A.wts = loss ? (double*)(q + o_wts) : nullptr; A.NF = (int)NF; A.robust = loss ? 1 : 0;
  A.lo = room_lo ? (const double*)(q + o_lo) : nullptr; A.hi = room_hi ? (const double*)(q + o_hi) : nullptr;
  A.held = nullptr; A.bounded = 0;
  model_records(a.model, a.camera, a.likelihood, A.Mdl, A.Cam);
  A.L.kind = loss ? loss->kind : DOGLEG_AMD_LOSS_TRIVIAL; A.L.fs = (int)fs;
  A.L.a = loss && loss->kind != DOGLEG_AMD_LOSS_TRIVIAL ? loss->scale : 1.0; A.L.c = A.L.a*A.L.a;
  A.max_iterations = prm->max_iterations; A.trustregion0 = prm->trustregion0;
  A.dec_factor = prm->trustregion_decrease_factor; A.dec_thr = prm->trustregion_decrease_threshold;
  A.inc_factor = prm->trustregion_increase_factor; A.inc_thr = prm->trustregion_increase_threshold;
  A.jtx_thr = prm->Jt_x_threshold; A.upd_thr = prm->update_threshold; A.tr_thr = prm->trustregion_threshold;
  return 0;
}

// the rounds on stream st, from the initial p in A.p_trial and the initial live bytes to the round that leaves no problem
// live: the callback (none in the model form), ONE launch and the 4-byte read-back of the counter per round.  Fills t_stats.
int batch_rounds(const char* who, const BatchForm& F, const BatchDev& A, void* cookie, hipStream_t st)
{
  BatchCache& K = g_cache;
  BatchTimer T;
  if(T.start(who)) return -1;
  // a problem leaves a round finished or with a new trial point; rejected trials shrink the trust region until the
  // threshold stops them, so the rounds are bounded wherever the reference's own loop is.  The cap only keeps a
  // parameter set under which the reference would never return (a decrease factor >= 1) from holding the device.
  const long max_rounds = 1000000;
  long rounds = 0;
  while(true)
  {
    if(rounds >= max_rounds)
    {
      dlg_set_error("%s: %ld rounds", who, rounds); BMSG("%s: still live problems after %ld rounds: giving up", who, rounds);
      return -1;
    }
    BHIP(hipMemsetAsync(A.counter, 0, sizeof(int), st));
    if(T.mark(who, 0, st)) return -1;
    if(!F.model) invoke_callback(F, A.p_trial, A, A.live, (unsigned int)A.B, st, cookie);
    if(T.mark(who, 1, st)) return -1;
    launch_batch_round(st, A);
    BHIP(hipGetLastError());
    if(T.mark(who, 2, st)) return -1;
    BHIP(hipMemcpyAsync(K.h_counter, A.counter, sizeof(int), hipMemcpyDeviceToHost, st));
    BHIP(hipStreamSynchronize(st));
    rounds++;
    if(T.read(who)) return -1;
    if(*K.h_counter == 0) break;
  }
  // (the model form: no callback ran between the first two marks)
  t_stats[0] = (double)rounds; t_stats[1] = F.model ? 0.0 : T.ms_callback; t_stats[2] = T.ms_library;
  return 0;
}

// Both routes: the initial p into the cache (from the host, or by a copy within the device), the live bytes (the mask of the
// device route), the start points clamped into the bounds, the rounds.  Then the host route downloads the state and forms the
// caller's arrays in a loop here; the device route ends in k_batch_finish, which writes them where the caller has them.
// Everything on the caller's stream if one is given.
int solve_locked(const DlgBatchSolve& a)
{
  const BatchForm F{a.fJ, a.fP, a.unpacked, a.model, a.camera};
  const char* who = solve_who(a);
  const unsigned int B = a.B, N = a.N;
  const dogleg_amd_batch_bounds_t* bounds = a.bounds;
  double* const weights = a.loss ? a.weights : nullptr;
  BatchDev A;
  if(batch_setup(who, a, F, A)) return -1;
  hipStream_t st = a.stream ? (hipStream_t)a.stream : g_cache.stream;
  BHIP(hipMemcpyAsync(A.p_trial, a.p, sizeof(double)*(size_t)B*N, a.device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  launch_batch_init(st, A, a.active);
  BHIP(hipGetLastError());
  if(bounds)
  {
    A.bounded = 1;
    if(a.device) { A.lo = bounds->lower; A.hi = bounds->upper; A.held = bounds->held; }      // the caller's arrays, where they lie
    if(!a.device && A.lo) BHIP(hipMemcpyAsync(const_cast<double*>(A.lo), bounds->lower, sizeof(double)*(size_t)B*N, hipMemcpyHostToDevice, st));
    if(!a.device && A.hi) BHIP(hipMemcpyAsync(const_cast<double*>(A.hi), bounds->upper, sizeof(double)*(size_t)B*N, hipMemcpyHostToDevice, st));
    launch_batch_clamp(st, A);
    BHIP(hipGetLastError());
  }
  if(batch_rounds(who, F, A, a.cookie, st)) return -1;
  if(a.device)
  {
    launch_batch_finish(st, A, a.p, a.results, a.lambda, weights);
    BHIP(hipGetLastError());
    BHIP(hipStreamSynchronize(st));
    return 0;
  }
  std::vector<double> sc((size_t)B*SC_COUNT), pb((size_t)B*N);
  std::vector<double> gb(bounds && bounds->held ? (size_t)B*N : 0);
  if(!gb.empty()) BHIP(hipMemcpyAsync(gb.data(), A.g, sizeof(double)*gb.size(), hipMemcpyDeviceToHost, st));
  std::vector<int> sti((size_t)B*ST_COUNT);
  BHIP(hipMemcpyAsync(sc.data(), A.sc, sizeof(double)*sc.size(), hipMemcpyDeviceToHost, st));
  BHIP(hipMemcpyAsync(sti.data(), A.st, sizeof(int)*sti.size(), hipMemcpyDeviceToHost, st));
  BHIP(hipMemcpyAsync(pb.data(), A.p_before, sizeof(double)*pb.size(), hipMemcpyDeviceToHost, st));
  const size_t NF = (size_t)A.NF;
  std::vector<double> wt(weights ? (size_t)B*NF : 0);
  if(weights) BHIP(hipMemcpyAsync(wt.data(), A.wts, sizeof(double)*wt.size(), hipMemcpyDeviceToHost, st));
  BHIP(hipStreamSynchronize(st));
  for(size_t b = 0; b < B; b++)
  {
    dogleg_amd_batch_result_t& R = a.results[b];
    const int status = sti[b*ST_COUNT + ST_STATUS];
    const bool failed = status == DOGLEG_AMD_BATCH_FAILED;
    R.norm2_x = failed ? -1.0 : sc[b*SC_COUNT + SC_N2X];
    R.trustregion = sc[b*SC_COUNT + SC_TR]; R.lambda = sc[b*SC_COUNT + SC_LAMBDA];
    R.iterations = sti[b*ST_COUNT + ST_ITER]; R.evaluations = sti[b*ST_COUNT + ST_EVAL]; R.status = status;
    if(!failed) memcpy(a.p + b*N, pb.data() + b*N, sizeof(double)*N);
    if(weights)
    {
      if(failed) for(size_t f = 0; f < NF; f++) weights[b*NF + f] = std::nan("");
      else       memcpy(weights + b*NF, wt.data() + b*NF, sizeof(double)*NF);
    }
    if(!gb.empty())
      for(size_t i = b*N; i < (b + 1)*N; i++)
        bounds->held[i] = failed ? 0 : held_code(pb[i], gb[i], bounds->lower ? bounds->lower[i] : -INFINITY,
                                                 bounds->upper ? bounds->upper[i] : INFINITY);
  }
  return 0;
}

// ---- the evaluation calls: the uncertainty and the query calls, each by host arrays or by the caller's device arrays.  One
// callback and ONE launch at given points.  What the four share is here; a kind says where its arrays lie and what it launches.
struct EvalCall
{
  const char* who; BatchForm F; unsigned int B, N, M; void* cookie;
  const double* p; double* lambda; int* status; const unsigned char* active; void* stream; bool device;
  // the host route.  stage: the segments of the state buffer and of its page-locked mirror: p first, lambda at o_lam, the status
  // at o_st and whatever the kind adds, inputs before o_st and outputs behind it, so that up: p .. o_st and down: o_lam .. end
  // are one copy each; the live bytes lie behind them.  state_d: their doubles, for the refusal
  Segments stage; size_t o_lam, o_st; double state_d;
  const DlgBatchQuery* query;  // a query call (for the refusal), or nullptr
  // the fit of the ..._fit forms (dense_batch.h), all nullptr without one; the host route stages weights and held at o_wts and
  // o_held (stage_fit), among the inputs in front of o_lam, so that they go up with p and do not come down again
  const dogleg_amd_batch_loss_t* loss; const double* weights; const unsigned char* held;
  size_t o_wts, o_held, wts_bytes, held_bytes;
  bool fit() const { return loss || weights || held; }
  int likelihood;              // of the model form (F.model)
};
template <class Req> EvalCall eval_call(const char* who, const Req& a)
{
  EvalCall c{};
  c.who = who; c.F = BatchForm{a.fJ, a.fP, a.unpacked, a.model, a.camera}; c.likelihood = a.likelihood; c.B = a.B; c.N = a.N; c.M = a.M; c.cookie = a.cookie;
  c.p = a.p; c.lambda = a.lambda; c.status = a.status; c.active = a.active; c.stream = a.stream; c.device = a.device;
  c.loss = a.loss; c.weights = a.weights; c.held = a.held;
  return c;
}
// rows a weight feature of a (checked) loss; 1 without one
unsigned int loss_fs(const dogleg_amd_batch_loss_t* loss)
{
  return loss && loss->featureSize > 1 ? (unsigned int)loss->featureSize : 1u;
}
// the segments of weights and held in the staging buffer: behind the inputs added so far, in front of lambda.  Returns their
// doubles, for the refusal
double stage_fit(EvalCall& c)
{
  c.wts_bytes = c.weights ? sizeof(double)*(size_t)c.B*(c.M/loss_fs(c.loss)) : 0;
  c.held_bytes = c.held ? (size_t)c.B*c.N : 0;
  c.o_wts = c.stage.add(c.wts_bytes); c.o_held = c.stage.add(c.held_bytes);
  return (double)(c.wts_bytes + c.held_bytes)/8.0;
}
// where an array of a kind lies for the kernel: nowhere if the caller has none, at off of the state buffer d on the host route,
// where the caller has it on the device route (d == nullptr)
template <class T> T* placed(char* d, size_t off, T* callers)
{
  return !callers ? nullptr : d ? (T*)(d + off) : callers;
}
// the kernels' argument of a call's fit
FitDev fit_dev(const EvalCall& c, char* d)
{
  FitDev F;
  // (with weights given, kind and scale are not read)
  const bool eval = c.loss && !c.weights && c.loss->kind != DOGLEG_AMD_LOSS_TRIVIAL;
  F.L.kind = eval ? c.loss->kind : DOGLEG_AMD_LOSS_TRIVIAL; F.L.fs = (int)loss_fs(c.loss);
  F.L.a = eval ? c.loss->scale : 1.0; F.L.c = F.L.a*F.L.a;
  F.wts = placed(d, c.o_wts, c.weights); F.held = placed(d, c.o_held, c.held);
  F.fit = c.fit() ? 1 : 0;
  return F;
}
// the kernels' argument of a call's model and its points (d_p: p in device memory), empty without a model
ModelEvalDev model_dev(const EvalCall& c, const double* d_p)
{
  ModelEvalDev E{};
  model_records(c.F.model, c.F.camera, c.likelihood, E.Mdl, E.Cam);
  E.p = c.F.model ? d_p : nullptr;
  return E;
}
// U: the kernel's argument (of a query: its front half), its shape filled in.  bind(d): the kind's own pointers into the
// kernel's argument (placed); gather(h): its inputs into the staging buffer h; launch(st, fit, model): with the call's fit and model as the kernels
// take them (weights and held are staged and placed here, for both kinds); scatter(h): its outputs from h into the caller's arrays.  gather and scatter: the host route only.  Counted into t_unc_stats where they happen: kernel launches,
// synchronisations, copies + fills.
// The device route keeps of the cache x / J (or the products) and at most two small arrays: a zeroed lambda where the caller
// gives none and the live bytes, all 1, where no mask is given (the mask itself is the callback's live_dev otherwise).
// The model form: no callback, an empty x / J buffer (the cache's is neither grown nor read) and no live bytes, which only a
// callback reads; ms_callback is 0
template <class Bind, class Gather, class Launch, class Scatter>
int evaluate_at(const EvalCall& c, UncDev& U, Bind bind, Gather gather, Launch launch, Scatter scatter)
{
  const char* who = c.who;
  const unsigned int B = c.B, N = c.N, M = c.M;
  double* const ts = t_unc_stats;
  for(int k = 0; k < 5; k++) ts[k] = 0.0;
  const EvalBuffer E = eval_buffer(c.F, B, N, M);
  // (the arithmetic needs no device: a call that cannot fit is refused before any device work)
  if(!fits(who, c.F, B, N, M, E, c.device ? 2.0*B : c.state_d, c.query)) return -1;
  if(cache_open(who)) return -1;
  BatchCache& K = g_cache;
  const size_t b_bytes = align256(sizeof(double)*(size_t)B), io_bytes = c.device ? b_bytes : c.stage.bytes;
  const bool model = c.F.model != nullptr;
  if(!cache_ensure(who, B, N, M, E.bytes, io_bytes + (model ? 0 : align256(B))) || (!c.device && !stage_ensure(who, B, N, M, io_bytes))) return -1;
  char* d = (char*)K.d_state; char* h = (char*)K.h_stage;
  unsigned char* own_live = (unsigned char*)(d + io_bytes);
  point_at_eval(U, c.F, E, K.d_eval);
  bind(c.device ? nullptr : d);
  const FitDev fit = fit_dev(c, c.device ? nullptr : d);
  U.lam = c.device ? (c.lambda ? c.lambda : (double*)d) : (double*)(d + c.o_lam);
  U.status = c.device ? c.status : (int*)(d + c.o_st);
  U.active = c.active;
  const double* d_p = c.device ? c.p : (const double*)d;
  const unsigned char* d_live = c.active ? c.active : own_live;
  BatchTimer T;
  if(T.start(who)) return -1;
  hipStream_t st = c.stream ? (hipStream_t)c.stream : K.stream;
  if(c.device)
  {
    if(!c.lambda) { BHIP(hipMemsetAsync(d, 0, sizeof(double)*(size_t)B, st)); ts[2] += 1.0; }
  }
  else
  {
    memcpy(h, c.p, sizeof(double)*(size_t)B*N);
    if(c.lambda) memcpy(h + c.o_lam, c.lambda, sizeof(double)*B); else memset(h + c.o_lam, 0, sizeof(double)*B);
    gather(h);
    if(c.weights) memcpy(h + c.o_wts, c.weights, c.wts_bytes);
    if(c.held) memcpy(h + c.o_held, c.held, c.held_bytes);
    BHIP(hipMemcpyAsync(d, h, c.o_st, hipMemcpyHostToDevice, st)); ts[2] += 1.0;
  }
  if(!c.active && !model) { BHIP(hipMemsetAsync(own_live, 1, B, st)); ts[2] += 1.0; }
  if(T.mark(who, 0, st)) return -1;
  if(!model) invoke_callback(c.F, d_p, U, d_live, B, st, c.cookie);
  if(T.mark(who, 1, st)) return -1;
  launch(st, fit, model_dev(c, d_p));
  BHIP(hipGetLastError()); ts[0] += 1.0;
  if(T.mark(who, 2, st)) return -1;
  if(!c.device) { BHIP(hipMemcpyAsync(h + c.o_lam, d + c.o_lam, io_bytes - c.o_lam, hipMemcpyDeviceToHost, st)); ts[2] += 1.0; }
  BHIP(hipStreamSynchronize(st)); ts[1] += 1.0;
  if(T.read(who)) return -1;
  ts[3] = model ? 0.0 : T.ms_callback; ts[4] = T.ms_library;
  if(c.device) return 0;
  if(c.lambda) memcpy(c.lambda, h + c.o_lam, sizeof(double)*B);
  memcpy(c.status, h + c.o_st, sizeof(int)*B);
  scatter(h);
  return 0;
}

// host layout: p | weights | held | lambda | scale | status | variances | covariance | factors
int unc_locked(const DlgBatchUnc& a)
{
  static const char* const names[2][2][2] = {
    {{"dogleg_amd_dense_batch_uncertainty", "dogleg_amd_dense_batch_uncertainty_device"},
     {"dogleg_amd_dense_products_batch_uncertainty", "dogleg_amd_dense_products_batch_uncertainty_device"}},
    {{"dogleg_amd_dense_batch_uncertainty_fit", "dogleg_amd_dense_batch_uncertainty_fit_device"},
     {"dogleg_amd_dense_products_batch_uncertainty_fit", "dogleg_amd_dense_products_batch_uncertainty_fit_device"}}};
  static const char* const model_names[2] = {"dogleg_amd_dense_batch_model_uncertainty", "dogleg_amd_dense_batch_model_uncertainty_device"};
  static const char* const camera_names[2] = {"dogleg_amd_dense_batch_camera_uncertainty", "dogleg_amd_dense_batch_camera_uncertainty_device"};
  EvalCall c = eval_call(a.camera ? camera_names[a.device ? 1 : 0] : a.model ? model_names[a.device ? 1 : 0] :
                         names[a.loss || a.weights || a.held ? 1 : 0][a.fP ? 1 : 0][a.device ? 1 : 0], a);
  const unsigned int B = a.B, N = a.N, NF = a.M/(unsigned int)a.fs;
  const size_t vec_bytes = sizeof(double)*(size_t)B*N, fac_bytes = sizeof(double)*(size_t)B*NF;
  c.stage.add(vec_bytes);
  const double fit_d = stage_fit(c);
  c.o_lam = c.stage.add(sizeof(double)*(size_t)B);
  const size_t o_scale = c.stage.add(sizeof(double)*(size_t)B);
  c.o_st = c.stage.add(sizeof(int)*(size_t)B);
  const size_t o_var = c.stage.add(a.variances ? vec_bytes : 0), o_cov = c.stage.add(a.covariance ? vec_bytes*N : 0);
  const size_t o_fac = c.stage.add(a.factors ? fac_bytes : 0);
  c.state_d = (double)B*((double)N + 3.0 + (a.variances ? N : 0.0) + (a.covariance ? (double)N*N : 0.0) + (a.factors ? NF : 0.0)) + fit_d;
  UncDev A;
  A.B = (int)B; A.N = (int)N; A.M = (int)a.M; A.NP = (int)(N*(N + 1)/2); A.fs = a.fs; A.NF = (int)NF;
  return evaluate_at(c, A,
    [&](char* d) {
      A.scale = a.factors ? placed(d, o_scale, a.scale) : nullptr;
      A.var = placed(d, o_var, a.variances); A.cov = placed(d, o_cov, a.covariance); A.fac = placed(d, o_fac, a.factors);
    },
    [&](char* h) { if(a.factors) memcpy(h + o_scale, a.scale, sizeof(double)*B); },
    [&](hipStream_t st, const FitDev& fit, const ModelEvalDev& mdl) { launch_batch_uncertainty(st, A, fit, mdl); },
    [&](const char* h) {
      if(a.factors) { memcpy(a.scale, h + o_scale, sizeof(double)*B); memcpy(a.factors, h + o_fac, fac_bytes); }
      if(a.variances) memcpy(a.variances, h + o_var, vec_bytes);
      if(a.covariance) memcpy(a.covariance, h + o_cov, vec_bytes*N);
    });
}

// host layout: p | Jq | weights | held | lambda | status | out
int query_locked(const DlgBatchQuery& a)
{
  static const char* const names[2][2][2] = {
    {{"dogleg_amd_dense_batch_query_covariance", "dogleg_amd_dense_batch_query_covariance_device"},
     {"dogleg_amd_dense_products_batch_query_covariance", "dogleg_amd_dense_products_batch_query_covariance_device"}},
    {{"dogleg_amd_dense_batch_query_covariance_fit", "dogleg_amd_dense_batch_query_covariance_fit_device"},
     {"dogleg_amd_dense_products_batch_query_covariance_fit", "dogleg_amd_dense_products_batch_query_covariance_fit_device"}}};
  static const char* const model_names[2] = {"dogleg_amd_dense_batch_model_query_covariance",
                                             "dogleg_amd_dense_batch_model_query_covariance_device"};
  static const char* const camera_names[2] = {"dogleg_amd_dense_batch_camera_query_covariance",
                                              "dogleg_amd_dense_batch_camera_query_covariance_device"};
  EvalCall c = eval_call(a.camera ? camera_names[a.device ? 1 : 0] : a.model ? model_names[a.device ? 1 : 0] :
                         names[a.loss || a.weights || a.held ? 1 : 0][a.fP ? 1 : 0][a.device ? 1 : 0], a);
  const unsigned int B = a.B, N = a.N;
  const size_t rows = (size_t)B*a.Nq*a.Qrows, Jq_bytes = sizeof(double)*rows*N, out_bytes = sizeof(double)*rows*a.Qrows;
  c.stage.add(sizeof(double)*(size_t)B*N);
  const size_t o_Jq = c.stage.add(Jq_bytes);
  const double fit_d = stage_fit(c);
  c.o_lam = c.stage.add(sizeof(double)*(size_t)B);
  c.o_st = c.stage.add(sizeof(int)*(size_t)B);
  const size_t o_out = c.stage.add(out_bytes);
  c.state_d = (double)B*((double)N + 3.0) + fit_d;
  c.query = &a;
  QueryDev A;
  UncDev& U = A.U;
  U.B = (int)B; U.N = (int)N; U.M = (int)a.M; U.NP = (int)(N*(N + 1)/2); U.fs = 1; U.NF = 0;
  U.scale = nullptr; U.cov = nullptr; U.var = nullptr; U.fac = nullptr;
  A.Nq = (int)a.Nq; A.Q = (int)a.Qrows; A.nobs = a.fP ? -1 : a.Nobservations;
  return evaluate_at(c, U,
    [&](char* d) { A.Jq = placed(d, o_Jq, a.Jq); A.out = placed(d, o_out, a.out); },
    [&](char* h) { memcpy(h + o_Jq, a.Jq, Jq_bytes); },
    [&](hipStream_t st, const FitDev& fit, const ModelEvalDev& mdl) { launch_batch_query(st, A, fit, mdl); },
    [&](const char* h) { memcpy(a.out, h + o_out, out_bytes); });
}

} // namespace

int dlg_dense_batch_solve(const DlgBatchSolve& a) { return locked_call([&] { return solve_locked(a); }); }
int dlg_dense_batch_uncertainty(const DlgBatchUnc& a) { return locked_call([&] { return unc_locked(a); }); }
int dlg_dense_batch_query(const DlgBatchQuery& a) { return locked_call([&] { return query_locked(a); }); }

extern "C" int dlg_batch_device_span_ok(const void* ptr, size_t bytes)
{
  if(!ptr) return 0;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if(hipPointerGetAttributes(&at, ptr) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if(at.type == hipMemoryTypeManaged || at.type == hipMemoryTypeHost) return 1;      // (host: registered / page-locked)
  if(at.type != hipMemoryTypeDevice) return 0;                                       // unregistered host memory, arrays
  int dev = -1;
  if(hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
  if(at.device != dev) return 0;
  hipDeviceptr_t base = nullptr; size_t size = 0;
  if(hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<void*>(ptr)) != hipSuccess) { (void)hipGetLastError(); return 0; }
  const size_t off = (size_t)((const char*)ptr - (const char*)base);
  return off <= size && bytes <= size - off ? 1 : 0;
}
int dlg_dense_batch_uncertainty_last_stats(double* out, int n)
{
  int k = 0;
  for(; k < n && k < 5; k++) out[k] = t_unc_stats[k];
  return k;
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
