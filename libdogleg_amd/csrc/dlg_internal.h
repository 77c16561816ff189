// dlg_internal.h -- shared declarations of the HIP backend (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <cmath>
#include <vector>
#include <string>
#include "../../include/dlg_backend.h"

// ---------------------------------------------------------------- errors ----
void dlg_set_error(const char* fmt, ...);

#define DLG_HIP(call)                                                              \
  do {                                                                             \
    hipError_t e__ = (call);                                                       \
    if(e__ != hipSuccess) {                                                        \
      dlg_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call,                  \
                    hipGetErrorString(e__));                                       \
      return DLG_ERR_HIP;                                                          \
    }                                                                              \
  } while(0)

#define DLG_CHECK(call)                                                            \
  do { int rc__ = (call); if(rc__ != DLG_OK) return rc__; } while(0)

#define DLG_LAUNCH_CHECK()  DLG_HIP(hipGetLastError())

// ------------------------------------------------------------- geometry ----
static inline int dlg_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

struct SparseSym;      // host+device symbolic data of the sparse path (sparse_symbolic.h)

struct DlgSlot
{
  double* p      = nullptr;   // [N]
  double* x      = nullptr;   // [M] (rank-local rows on a sharded rank)
  double* J      = nullptr;   // dense: [M][N]; sparse: values[nnz]; products: JtJ
  double* Jt_x   = nullptr;   // [N]
  double* cauchy = nullptr;   // [N]
  double* gn     = nullptr;   // [N]
  double* step   = nullptr;   // [N] step_to_here
  const double* x_bound = nullptr;   // device-resident inputs (dlg_point_bind_device)
  const double* J_bound = nullptr;
  double  norm2_x = 0, norm2_cauchy = 0, norm2_gn = 0, norm2_jtx = 0;
  // the expected improvement from the solved system (step.hip, ident_norm2_Jstep): |J Jt_x|^2 of the Cauchy step, <Jt_x, gn>,
  // and whether the factor the Gauss-Newton step came from allows it (pivot ratio)
  double  Jg2 = 0, g_dot_gn = 0, a_dot_gn = 0, ident_lam = 0; bool ident_ok = false;      // (ident_norm2_Jstep: <Jt x, gn>, <cauchy, gn>, the lambda gn was solved at)
  bool    have_inputs = false, have_Jtx = false, have_cauchy = false, have_gn = false;
  // a bounded solve (dlg_point_bind_held): a byte a variable, not 0 = held -- J has zeros in those columns and Jt_x in those
  // entries, and the matrix that is factorised gets a diagonal of exactly 1 there; NULL: nothing of it runs
  const unsigned char* held = nullptr;
  const double* xin() const { return x_bound ? x_bound : x; }
  const double* Jin() const { return J_bound ? J_bound : J; }
};

struct DevScratch { double* p = nullptr; size_t cap = 0; };      // a device buffer that only grows (cap in doubles)

struct dlg_backend
{
  int type = 0, N = 0, M = 0, nnz = 0, flags = 0, device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // side stream + events: p_new travels to the host while the expected improvement is computed (dlg_step)
  hipStream_t copy_stream = nullptr;
  hipEvent_t  ev_step = nullptr, ev_copy = nullptr, ev_fetch = nullptr;
  // second compute stream: the Cauchy step (one pass over J, independent of the factorisation) runs
  // beside the latency-bound upper levels of the elimination tree / the potrf chain, which leave
  // most of the chip idle.  The factorisation records ev_fork where that phase begins
  // (want_fork -> fork_recorded), the caller joins with ev_join before the step is formed.
  hipStream_t aux_stream = nullptr;
  hipEvent_t  ev_fork = nullptr, ev_join = nullptr;
  // the join without an event: the second stream raises d_join to join_epoch behind the Cauchy step, the first kernel of the
  // main stream that reads that step (k_negate_interp1) polls the word itself -- a wait for an event of another stream costs
  // the main stream ~6 us between two kernels even when the event is long complete
  int* d_join = nullptr; int join_epoch = 0, join_pending = 0;
  hipEvent_t ev_region = nullptr;    // behind this backend's last one-launch region (DlgRegionTurn)
  bool turn_registered = false;
  bool want_fork = false, fork_recorded = false, overlap = true;
  bool fuse_eval = true;      // ... in the pass that forms Jt*x where the schedule allows (DOGLEG_AMD_NO_FUSED_EVAL: second stream instead)
  bool speculate = false;     // dlg_backend_set_speculation: assemble JtJ beside Jt*x at every dlg_point_eval
  bool presolve = false;      // ... and enqueue K5 + K6 behind it (step_prepare) for dlg_take_step to pick up
  bool pre_rejected = false;  // the last point whose factorisation was enqueued ahead was rejected: the next evaluation enqueues nothing ahead (a step taken from a fresh point clears it)
  bool factor_ahead = false;  // (around sparse_factorize in step_prepare) only what covers the host's round trip: the leaf level
  bool pre_split = false;     // the prepared factorisation stopped behind its leaf level: dlg_take_step enqueues the rest and the solve
  bool prof_cont = false;     // the next timed scope continues a phase that was counted already (a factorisation in two parts)
  int  pre_slot = -1, pre_held = -1; double pre_lambda = 0.0, pre_hint = 0.0; bool pre_hint_valid = false, pre_hint_input = false;   // prepared slot; slot whose factor it displaced
  DlgSlot slot[2];

  // scalar return path: kernels write d_scal, one D2H into pinned h_scal
  double* d_scal = nullptr;
  double* h_scal = nullptr;
  int* fork_gate = nullptr; int fork_gate_epoch = 0;      // dlg_fork_gate
  // The expected improvement's pass over J (K8) behind the host's decision point (dlg_backend_set_defer_tail): the value is
  // first used after the NEXT evaluation (dogleg.c:1427 -- takeStepFrom only needs max|step| to tell "done", 1289-1296), so
  // dlg_take_step's synchronisation rides on the step kernel (StepLaunch::nscal: it takes the scalars to the host), K8 follows on
  // the same stream while the host is on its way back, its partial sums (and p_new) land in page-locked memory and
  // dlg_step_tail adds them up -- behind a wait of its own only if the host has not waited for anything enqueued behind K8
  // since (sync_mark against tail_mark: the evaluation of the trial point is such a wait).  tail_*: between the step call and
  // dlg_step_tail, which may be several C calls later.
  bool defer_tail = false, tail_pending = false;
  int tail_nb = 0;
  double tail_inner = 0.0, tail_value = 0.0;
  double* h_tail = nullptr; int h_tail_cap = 0;
  unsigned long sync_mark = 0, tail_mark = 0;
  bool factor_doomed = false; // sparse_factorize found the factorisation doomed at its look at the diagonal and enqueued nothing else (the lambda loops go on at once)
  // The expected improvement WITHOUT its pass over J (K8): with (JtJ + lambda I) gn = -Jt_x solved, |J step|^2 of all three
  // kinds of step is a combination of N-vector dot products (ident_norm2_Jstep).  The step kernel decides on the device
  // (d_scal[IDENT_SLOT] = 1: the factor allows it, 2: the step is the Cauchy step, which needs no factor, 0: neither;
  // [IDENT_SLOT + 1] = the pivot ratio, [IDENT_SLOT + 4] = <cauchy - gn, cauchy>) and the pass over J that is on the stream
  // behind it returns at once (StepLaunch::skip); the host reads the same word and forms the value, and a retry from the cached
  // vectors (dlg_step) takes the word's 1 along (DlgSlot::ident_ok).  DOGLEG_AMD_EI_JPASS=1: always the pass over J.
  // The factor allows it where its pivot ratio is at most IDENT_RATIO_MAX AND the estimate of the value's relative error,
  // eps (max L_ii)^2 |gn|^2 / -<Jt x, gn>, is at most IDENT_ERR_MAX.  The error is gn' r with r the residual of the solve:
  // eps times cond(JtJ + lambda I) along gn, first order in the backward error of the factor, where the pass over J has
  // a second-order one.  The pivot ratio bounds cond only from below (a factor with unit pivots can have cond 1e14), so it
  // does not bound the error by itself; the estimate came out at no less than about half the measured error on fixtures
  // built to defeat the ratio (tests/exact_ei.py) and at 1e-15 and below on the bundle-adjustment shapes.  With
  // IDENT_ERR_MAX = 1e-12 the value from the solved system is within about 2e-12 of the exact one.
  static constexpr int IDENT_SLOT = 3, GB_SLOT = 13;     // free slots of dlg_take_step's scalar block
  static constexpr double IDENT_RATIO_MAX = 212.0;
  static constexpr double IDENT_ERR_MAX = 1e-12;
  bool ident_predict = false;      // the last step's pass over J was let go by the device: the NEXT dlg_take_step may not launch it at all
  bool ei_from_system = false; double pivot_ratio = NAN;   // dlg_backend_ei_source: how the last value handed out was formed
  int ei_flip = 0, ei_count = 0;                           // DOGLEG_AMD_DEBUG_EI_FLIP (test hook)
  bool tail_ident = false, tail_no_fold = false; double tail_nJs = 0.0;     // (tail_no_fold: the K8 on the stream carries no p_new)
  bool p_side_pending = false;          // p_new of a step behind the decision point is on its way on the copy stream (ev_copy): until dlg_step_tail / the next call that writes p
  // Work the CALLER has for the stream that does not depend on a step's scalars (dlg_backend_set_between): enqueued from
  // inside dlg_take_step / dlg_step, between the step's last launch and the host's wait for it -- the device model's
  // kernels for the trial point, the first pass over the next point's J (dlg_point_eval_early).  The host's turn-round
  // behind the step (event wake-up, scalars, the evaluation's first launch: ~20 us) then hides behind that work.
  dlg_between_fn between_fn = nullptr; void* between_cookie = nullptr; bool between_armed = false, between_ran = false, between_redone = false;
  int early_slot = -1; const double* early_x = nullptr; const double* early_J = nullptr;      // dlg_point_eval_early: what dlg_point_eval finds enqueued
  static constexpr int NSCAL = 16;
  // hand-offs inside the one-launch regions (flags between workgroups): a wait that gives up raises a bit in
  // the status word (slot NSCAL - 2 of the scalar block, so it travels with every fetch of the scalars);
  // the host turns it into DLG_ERR_STATE (dlg_check_handoff).  handoff_skew != 0 (DOGLEG_AMD_DEBUG_HANDOFF_TIMEOUT,
  // read at create time): the waits look for an epoch that never comes -- the test hook of that path.
  int handoff_spins = 0, handoff_skew = 0;
  // environment knobs that steer per-step paths, read ONCE when the backend is created (dlg_backend_create)
  struct Knobs
  {
    bool potrf_steps = false, trsv_steps = false, no_abandon = false, ei_jpass = false, no_between = false, no_k8_predict = false;
    int touch_wg = 512;
  } knobs;
  int ncu = 256;              // compute units of b->device

  // reduction partials
  double* d_part = nullptr;
  size_t  part_cap = 0;       // in doubles
  double* d_gnpart = nullptr; // [4096]: [0, 1024) partials of |gn|^2 kept on the device (dlg_take_step), [2048, 4096) the pivots' partial minima / maxima
  // Reductions whose result only the host reads skip their one-workgroup second stage: the
  // partials are written straight into page-locked host memory and summed (in index order) by
  // dlg_resolve_pending() after the synchronisation that the host needs anyway.  Off when an
  // all-reduce hook wants the results on the device.
  struct PendingFinal { size_t off; int nb, nsum, nmax, dst, stride; };
  static constexpr size_t HPART_CAP = 16384;
  double* h_part = nullptr;
  size_t  h_part_used = 0;
  std::vector<PendingFinal> pending;
  bool    host_finals = true;

  // pinned staging for p_new D2H / uploads of small vectors
  double* h_vec = nullptr;

  // dense / products
  double* G = nullptr;        // N x N column-major, lower triangle = factor
  double* Linv = nullptr;     // inverses of the 64x64 diagonal blocks of the factor
  int* potrf_flag = nullptr; int potrf_epoch = 0; int* trsv_flag = nullptr; double* trsv_y = nullptr; double* trsv_x = nullptr; int trsv_epoch = 0;   // hand-off flags of the one-launch factorisation ([T*T] + 1 for the step form)
  double* slabs = nullptr;    // split-K partial slabs for the SYRK
  size_t  slabs_bytes = 0;
  int*    d_info = nullptr;
  int*    h_info = nullptr;
  bool    defer_factor_sync = false;   // dlg_gauss_newton: the *_factorize calls enqueue only; the pivot
                                       // flag is read after the solve's synchronisation
  double* d_work = nullptr;   // N-vector scratch
  // scratch of the users of the held factor (factor_users.hip: grow): right-hand sides of the solves, and Gram products
  // and forward-solve blocks of the leverage / covariance calls (two: the observation form of the query covariance uses both at once)
  DevScratch solve_scr, lev_scr;
  struct CovPlan* cov = nullptr; int cov_last = -1;          // [COV_NPLAN] plans of the covariance entry points, the last of [0] (requests) and [1] (marginal variances) run
  struct SelInv* selinv = nullptr;                           // the selected inverse and its entry lookup (dlg_covariance_entries)

  // sparse
  SparseSym* sym = nullptr;

  // multi-GPU: measurement rows are the sharded unit.  Contiguous rows [row0, row1) (dense; sparse
  // "row sharding": every rank factors everything, the whole JtJ is summed), or the subtree
  // partition of the sparse path (part_nranks > 1: the rank's rows are chosen by the symbolic phase,
  // only the top of the elimination tree is summed).  Sums over the ranks: RCCL on the backend's
  // stream (rccl_comm: no host in between), or the caller's hook (host-synchronous fallback).
  int row0 = 0, row1 = 0;     // owned measurement rows (contiguous mode)
  int mloc = 0;               // measurement rows held by this rank
  int part_rank = 0, part_nranks = 1;
  bool part_requested = false;          // dlg_backend_set_partition was called (also with nranks == 1)
  dlg_allreduce_fn allreduce = nullptr;
  void* allreduce_cookie = nullptr;
  void* rccl_comm = nullptr;  // ncclComm_t
  bool  rccl_owned = false;
  double* d_red = nullptr;    // fused reduce buffer [Jt_x | norm2_x | ...]
  // subtree partition: the Cauchy step's pass over the rank's rows runs on the second stream beside the
  // factorisation and leaves |J g|^2 of those rows in fold_scalar; the sum over the ranks is made together
  // with the solution's (sparse_solve -> fold_result = where the sum is), k_cauchy_finish follows on the main stream
  const double* fold_scalar = nullptr; const double* fold_result = nullptr; double* fold_cauchy_out = nullptr;
  // measurement only (dlg_backend_set_noop_comm): the backend behaves as one rank of several -- partition, reduce
  // buffers, device-side finals, every collective's place in the stream -- but a sum over the ranks returns at once
  // (the numbers are this rank's partial sums: timing, not results)
  bool noop_comm = false;
  bool sharded() const { return allreduce != nullptr || rccl_comm != nullptr || noop_comm; }

  // optional per-phase timing with HIP events on b->stream (dlg_backend_set_profiling)
  bool profiling = false;
  bool ext_events = true;     // events may ride on launches (DLG_LAUNCH_TIMED, DLG_LAUNCH_LAST)
  int prof_every = 1; unsigned prof_tick[DLG_PROF_COUNT] = {};      // every n-th occurrence of a timed phase carries events
  unsigned prof_mask = 0;     // the phases that are timed (bit = DLG_PROF_*)
  struct ProfPair { hipEvent_t a, b; int id; bool cond; bool cont = false; };
  std::vector<ProfPair> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  double prof_ms[DLG_PROF_COUNT] = {0};
  long   prof_n[DLG_PROF_COUNT] = {0};
  // Launches that return after their first barrier when the factorisation they belong to has failed (the lambda
  // path: the rest of K5, K6, K8) are timed "conditionally" (prof_cond set by the caller around them): their
  // times wait in prof_att_* until the attempt's outcome is known (dlg_prof_commit) and are then counted as
  // full launches (prof_ms / prof_n) or as early returns (prof_early_*) -- a per-launch average over both
  // would report bandwidths no kernel reaches (7 TB/s on config #5).
  bool   prof_cond = false;
  double prof_att_ms[DLG_PROF_COUNT] = {0};   long prof_att_n[DLG_PROF_COUNT] = {0};
  double prof_early_ms[DLG_PROF_COUNT] = {0}; long prof_early_n[DLG_PROF_COUNT] = {0};

  int factor_slot = -1;       // slot whose JtJ the stored factor belongs to (-1: none)
};

// profiling helpers: bracket a phase with events; resolved at the next stream sync
hipEvent_t dlg_prof_begin(dlg_backend* b);
void dlg_prof_end(dlg_backend* b, int id, hipEvent_t start);
void dlg_prof_resolve(dlg_backend* b);
void dlg_prof_commit(dlg_backend* b, bool attempt_succeeded);
struct DlgProfCond       // launches inside the scope return early if the factorisation of this attempt fails
{
  dlg_backend* b; bool was;
  explicit DlgProfCond(dlg_backend* b_) : b(b_), was(b_->prof_cond) { b_->prof_cond = true; }
  ~DlgProfCond() { b->prof_cond = was; }
};
struct DlgProfScope
{
  dlg_backend* b; int id; hipEvent_t e;
  DlgProfScope(dlg_backend* b_, int id_, bool enable = true) : b(b_), id(id_), e((enable && (b_->prof_mask >> id_ & 1u) && b_->prof_tick[id_]++ % b_->prof_every == 0) ? dlg_prof_begin(b_) : nullptr) {}
  ~DlgProfScope() { if(e) dlg_prof_end(b, id, e); }
};
// One kernel as a timed phase: the two events ride on the launch itself (hipExtLaunchKernelGGL: the dispatch's own
// start / end time stamps) -- no event records, i.e. no barrier packets and no idle microseconds, around it.
bool dlg_prof_pair(dlg_backend* b, int id, hipEvent_t* e0, hipEvent_t* e1);
#define DLG_LAUNCH_TIMED(b_, id_, kernel, grid, block, shm, st, ...) \
  do { hipEvent_t dlg_e0 = nullptr, dlg_e1 = nullptr; \
       if(dlg_prof_pair(b_, id_, &dlg_e0, &dlg_e1)) hipExtLaunchKernelGGL(kernel, grid, block, shm, st, dlg_e0, dlg_e1, 0, __VA_ARGS__); \
       else hipLaunchKernelGGL(kernel, grid, block, shm, st, __VA_ARGS__); } while(0)
// The event the host is going to wait for (ev_, or null: a plain launch), attached to the last kernel of what it waits
// for: no record behind the kernel.
#define DLG_LAUNCH_LAST(ev_, kernel, grid, block, shm, st, ...) \
  do { hipEvent_t dlg_ev = (ev_); \
       if(dlg_ev) hipExtLaunchKernelGGL(kernel, grid, block, shm, st, (hipEvent_t)nullptr, dlg_ev, 0, __VA_ARGS__); \
       else hipLaunchKernelGGL(kernel, grid, block, shm, st, __VA_ARGS__); } while(0)
// What a step function (step.hip) asks ONE launch to carry beyond its arguments, and what the launcher did about it.  A
// default-constructed value is a plain launch.  The launcher decides: it takes the event and the scalars along only where
// its partial sums found page-locked room, and says so -- the caller reads the answer here, nothing travels on dlg_backend.
struct StepLaunch
{
  hipEvent_t stop = nullptr;      // the event the host is going to wait for rides on the launch (DLG_LAUNCH_LAST)
  int nscal = 0;                  // the launch copies d_scal[0 .. nscal) to the page-locked h_scal (it is the last one of the step)
  const double* p_src = nullptr; double* p_dst = nullptr;   // ... and p_new to a page-locked destination (its device address), a slice per workgroup
  const double* skip = nullptr;   // device word; not 0: the pass over J returns at once (the step kernel's verdict, IDENT_SLOT)
  bool tail = false;              // K8 behind the decision point: partial sums to h_tail, dlg_step_tail adds them
  bool k_host = false;            // k_interpolate's k straight into the page-locked scalars (nobody fetches device scalars behind this step)
  // filled in by the launcher
  bool attached = false, scal_copied = false, p_copied = false;
  bool ident = false;             // k_take_step: the step kernel was asked for its verdict on the value from the solved system
};

// rows of the measurement vector owned by this rank
static inline int dlg_mloc(const dlg_backend* b) { return b->mloc; }
// sum-all-reduce over ranks of `count` doubles at device address buf (no-op single rank)
int dlg_allreduce_dev(dlg_backend* b, double* buf, size_t count);

// the factorisation calls this where its latency-bound phase begins
static inline void dlg_fork_point(dlg_backend* b)
{
  if(b->want_fork && !b->fork_recorded && hipEventRecord(b->ev_fork, b->stream) == hipSuccess) b->fork_recorded = true;
}

// ... or, where that phase is ONE launch: the word that launch sets to `epoch` once all its workgroups are
// dispatched (no event on the main stream; the second stream holds a waiting kernel in front of its work)
static inline void dlg_fork_gate(dlg_backend* b, int* gate, int epoch)
{
  if(b->want_fork && !b->fork_recorded) { b->fork_gate = gate; b->fork_gate_epoch = epoch; b->fork_recorded = true; }
}

// fetch the first n scalars of d_scal to the host (synchronises the stream)
int dlg_fetch_scalars(dlg_backend* b, int n);
// between backend.hip and step.hip: a valid backend and slot; the doubles of a slot's J; what step_prepare enqueued ahead
// for a step that is not going to be taken is dropped (every entry point that works on other state calls it first)
int dlg_check_slot(dlg_backend* b, int s);
size_t dlg_j_doubles(const dlg_backend* b);
int dlg_step_unprepare(dlg_backend* b);

// what a kernel of a one-launch region needs to report a wait that gave up
struct DlgHandoff { int* status; int spins; int skew; };
enum { DLG_HANDOFF_FACTOR = 1, DLG_HANDOFF_SOLVE = 2, DLG_HANDOFF_POTRF = 4, DLG_HANDOFF_TRSV = 8, DLG_HANDOFF_TRSM = 16 };
static inline DlgHandoff dlg_handoff(const dlg_backend* b, int spins)
{
  DlgHandoff h;
  h.status = reinterpret_cast<int*>(b->d_scal + (dlg_backend::NSCAL - 2));
  h.spins = b->handoff_spins > 0 ? b->handoff_spins : spins; h.skew = b->handoff_skew;
  return h;
}
// One-launch regions (workgroups that wait for each other inside a launch) of DIFFERENT backends on one device take
// turns: two such launches at once can hold each other's CUs with waiting workgroups whose partners find no room --
// every one of them gives up after its 2^21 polls and the step fails with DLG_ERR_STATE (tools/stress_concurrent.py).
// With one backend on the device (one process per GPU: the rule) this is one atomic load.  Around the launch:
//   { DlgRegionTurn turn(b); hipLaunchKernelGGL(...region...); }
struct DlgRegionTurn { dlg_backend* b; bool on; explicit DlgRegionTurn(dlg_backend* b); ~DlgRegionTurn(); };
// after a synchronisation that brought the scalar block to the host: DLG_ERR_STATE if a hand-off timed out
int dlg_check_handoff(dlg_backend* b);

// --------------------------------------------------------- kernels_vec.hip --
// out[0] = sum x[i]^2 ; out[1] = max |x[i]|   (deterministic two-stage)
int k_norm2_absmax(dlg_backend* b, const double* x, int n, double* out2);
// ... of two vectors behind one launch (*on_host: it was one launch, the host adds all four; `stop` then rode on it)
int k_norm2_absmax_pair(dlg_backend* b, const double* x1, int n1, double* out1, const double* x2, int n2, double* out2,
                        bool* on_host = nullptr, hipEvent_t stop = nullptr);
// out[0] = <x,y>
int k_inner(dlg_backend* b, const double* x, const double* y, int n, double* out, StepLaunch& L);
// Cauchy finish: g2 = |g|^2 (host), Jg2 = *Jg2_dev; k = -g2/Jg2;
// cauchy = k*g ; out[0] = k*k*g2
int k_cauchy_finish(dlg_backend* b, const double* g, double g2, const double* Jg2_dev, double* cauchy,
                    int n, double* out);
// step = s * v ; p_new = p + step ; out[0] = max|step|
int k_scaled_step(dlg_backend* b, const double* v, double s, const double* p, double* step,
                  double* p_new, int n, double* out_absmax);
// interpolation (dogleg.c:964-987): out = {norm2_step, k, max|step|}
int k_interpolate(dlg_backend* b, const double* a, const double* bb, double norm2a,
                  double trustregion, const double* p, double* step, double* p_new, int n,
                  double* out3, const StepLaunch& L);
// gn = -u ; out[0] = norm2(gn)
int k_negate_norm2(dlg_backend* b, double* v, int n, double* out);
// step chosen on the device (dogleg.c:1192-1256): out_n2_max[0] = |step|^2, [2] = max|step|; out3 = {kind, k, |gn|^2}
int k_negate_interp1(dlg_backend* b, double* gn, const double* cauchy, int n, double* gnpart, int* nb, const double* mm = nullptr, int nmm = 0, long mm_stride = 2);
int k_take_step(dlg_backend* b, const double* cauchy, const double* gn, const double* gnpart, int nbg,
                const double* n2c_dev, double trustregion, const double* p, double* step, double* p_new, int n,
                double* out_n2_max, double* out3, const double* Jtx, double* out_inner, StepLaunch& L,
                double* out_gb = nullptr, double* ident_out = nullptr, bool have_mm = false, bool ident_gn = false, double ratio_max = 0.0,
                double g2 = 0.0, double err_max = 0.0);
// generic deterministic final reduction of `np` partials (sum) into out[0]
int k_reduce_sum(dlg_backend* b, const double* partials, int np, double* out);
// region of b->h_part for (nsum + nmax) x nb partials whose results go to h_scal[out - d_scal + k*stride],
// or nullptr: the result is wanted on the device / no room -> the caller launches the second stage
double* dlg_host_partials(dlg_backend* b, const double* out, int nb, int nsum, int nmax, int stride);
double* dlg_tail_partials(dlg_backend* b, int nb);      // page-locked room for the partial sums of a K8 behind the decision point (dlg_step_tail adds them)
void dlg_resolve_pending(dlg_backend* b);
int dlg_ensure_partials(dlg_backend* b, size_t ndoubles);

// ------------------------------------------------------- kernels_dense.hip --
int dense_create(dlg_backend* b);
// dense_diag.hip: factor the 64x64 diagonal block at kb and form its inverse (one workgroup)
void dense_launch_potrf_diag(hipStream_t st, double* A, int lda, int kb, int nb, int* info_dev, double* Linv);
// ... and the rows below it in the same launch (flag: one device int, epoch: a value no earlier launch used)
// the whole dense factorisation in one launch (a workgroup per 64 x 64 tile; flags: T*T device ints, T = ceil(n/64))
void dense_launch_potrf_tiles(hipStream_t st, double* A, int lda, int n, int* info_dev, double* Linv, int* flags, int epoch, const DlgHandoff& ho, int* gate = nullptr);
// both triangular solves of (L L') x = rhs in one launch (a workgroup per 64 rows; flags: 2*T device ints; Y: n doubles of scratch)
void dense_launch_trsv_tiles(hipStream_t st, const double* A, int lda, int n, const double* Linv, const double* rhs,
                             double* Yh, double* X, double* Xh, int epoch, const DlgHandoff& ho);
void dense_trsv_arm(hipStream_t st, double* Yh, double* Xh, size_t n_each);
void dense_launch_potrf_diag_trsm(hipStream_t st, double* A, int lda, int kb, int nb, int n, int* info_dev, double* Linv,
                                  int* flag, int epoch, const DlgHandoff& ho);
// dense_diag.hip: the dynamic-LDS limit of a kernel, set once per device -- a function attribute is a property of
// (function, device); `done`: one array per kernel (per instantiation of a template)
constexpr int DLG_MAX_DEV = 64;
void dlg_func_lds_once(bool (&done)[DLG_MAX_DEV], const void* fn, int bytes);
void dense_destroy(dlg_backend* b);
int dense_eval(dlg_backend* b, int slot);                       // K1
int dense_norm2_Jv(dlg_backend* b, int slot, const double* v, double* out_dev, StepLaunch& L); // K3/K8
int dense_factorize(dlg_backend* b, int slot, double lambda, int* ok);          // K4+K5
bool dense_factor_ok(const dlg_backend* b);      // pivot flag of the last factorisation (after a sync)
int dense_solve(dlg_backend* b, const double* rhs, double* out);                // K6 (no negate)
int products_quadform(dlg_backend* b, int slot, const double* v, double* out_dev);
int products_factorize(dlg_backend* b, int slot, double lambda, int* ok);

// ------------------- sparse_host.hip / sparse_assemble.hip / sparse_solve.hip --
int sparse_create(dlg_backend* b);
size_t sparse_local_nnz(const dlg_backend* b);   // J values held by this rank
void sparse_destroy(dlg_backend* b);
void sparse_reset(dlg_backend* b);
int sparse_set_pattern(dlg_backend* b, const int* colptr, const int* rowidx);
int sparse_eval(dlg_backend* b, int slot);                      // K1
int sparse_assemble_speculative(dlg_backend* b, int s);         // K4 beside K1 (second stream, second panel buffer)
int sparse_eval_assemble(dlg_backend* b, int s, int* done);      // K1 + K4 in one pass over J (the assembly kernel forms Jt*x too)
int sparse_assemble_finish(dlg_backend* b);                      // ... the deferred partial-sum stages of that JtJ
int sparse_touch_factor(dlg_backend* b, hipStream_t st);         // second stream: pull the leaf panels into the Infinity Cache
int sparse_zero_spare(dlg_backend* b, hipStream_t ordered_for = nullptr);                           // clear the panel buffer the factorisation left behind (behind the step's fetch)
int sparse_abandon_enqueued(dlg_backend* b);                     // the launches of a factorisation + solve enqueued ahead (step_prepare) return early from here on
void sparse_spec_invalidate(dlg_backend* b, int s);
bool sparse_spec_is(const dlg_backend* b, int s, const double* J);     // the second panel buffer holds slot s's assembly from the values at J
// K3/K8; kind_if_factor_failed (device scalar holding the kind of step, or null): the pass is skipped when the
// factorisation on the stream failed and the step is not the Cauchy step to the edge
int sparse_norm2_Jv(dlg_backend* b, int slot, const double* v, double* out_dev, const double* kind_if_factor_failed, StepLaunch& L);
int sparse_factorize(dlg_backend* b, int slot, double lambda, int* ok);          // K4+K5 (b->factor_ahead: K5 up to the leaf level only, sparse_factorize_rest owes the rest)
int sparse_factorize_rest(dlg_backend* b, bool* was_pending);
bool sparse_factor_pending(const dlg_backend* b);                     // the levels above the leaves of a factorisation enqueued ahead
int sparse_norm2_chunks(const dlg_backend* b);
int dense_norm2_chunks(const dlg_backend* b);
bool sparse_factor_ok(const dlg_backend* b);     // pivot flag of the last factorisation (after a sync)
int sparse_solve(dlg_backend* b, const double* rhs, double* out);                // K6
int sparse_leaf_rows_materialize(dlg_backend* b);       // the current factor's merged leaves: L_below stored where the lean leaf launch left W (idempotent; no pattern: nothing)
void sparse_hold_factor(dlg_backend* b);
bool sparse_would_look(const dlg_backend* b, double lambda);      // sparse_factorize(lambda) would look at the diagonal first (and ask the host at once)
bool sparse_note_breakdown(dlg_backend* b);           // a factorisation broke down (the host knows): sparse_factorize looks at the diagonal first from now on (lambda = 0); true: stopped by that look, the panels are the assembly's still
void sparse_mark_unclean(dlg_backend* b);             // the next clear of either panel buffer is a full one (clear_panels)
// the partial-sum stages of an evaluation-time assembly on the SECOND stream (sparse_assemble.hip, "fin on the side")
bool sparse_fin_side_ok(const dlg_backend* b);
int  sparse_fin_side_begin(dlg_backend* b);      // main: augmented row + flag A; second stream: waits for flag A; b->stream := second stream
int  sparse_fin_side_end(dlg_backend* b);        // second stream: flag B behind the partial-sum stages; b->stream := main stream
int  sparse_fin_side_gate(dlg_backend* b);       // main: wait for flag B if stages are still owed (no-op otherwise)
// one wave that holds stream `st` until *gate == epoch (bounded: it is a matter of ordering work the chip has
// long finished in every measured case; a gate that never opens is reported through the hand-off status word)
int  dlg_gate_wait(dlg_backend* b, hipStream_t st, const int* gate, int epoch, bool report);
void sparse_release_held(dlg_backend* b);
int sparse_restore_factor(dlg_backend* b, bool* restored, bool rearm = true);
double sparse_current_lambda(const dlg_backend* b);                                 // of the last factorisation enqueued
const double* sparse_pivot_minmax(const dlg_backend* b, int* n);                    // [supernode][min, max] of diag(L) left by the last backward solve
// ---- the users of the held factor (factor_users.hip).  What such an entry point needs beyond a factor held for its slot:
// the slot's Jacobian on the device (refuses a dense-products backend and a slot without inputs), a backend that is not
// sharded, one that is not partitioned, a pattern on a sparse backend.  backend.hip: the one place that refuses.
enum { DLG_NEEDS_J = 1, DLG_NEEDS_UNSHARDED = 2, DLG_NEEDS_UNPARTITIONED = 4, DLG_NEEDS_PATTERN = 8 };
int dlg_factor_user_begin(dlg_backend* b, int s, const char* who, unsigned needs);
// how the forward solves of the chunks go (factor_users.hip: factor_route); the value is part of a plan's key
enum FactorRoute { ROUTE_REACH = 0, ROUTE_SWEEP = 1, ROUTE_DENSE = 2 };

// blocked multi-right-hand-side solves (sparse_multi.hip / kernels_dense.hip): MR = 16 right-hand sides
// interleaved [N][MR] (element (variable k, rhs c) at k*MR + c), solved in place, original order
int sparse_multi_width_ok(const dlg_backend* b);
int sparse_multi_rhs();
int sparse_solve_multi(dlg_backend* b, double* d_il);
int dense_solve_multi(dlg_backend* b, double* d_il);
int multi_cols_to_interleaved(dlg_backend* b, const double* d_cols, int ncols, double* d_il);
int multi_interleaved_to_cols(dlg_backend* b, const double* d_il, int ncols, double* d_cols);
int sparse_jt_chunk_interleaved(dlg_backend* b, int s, int row0, int ncols, double* d_il);
int dense_jt_chunk_interleaved(dlg_backend* b, int s, int row0, int ncols, double* d_il);

// leverage blocks A_f = J_f (JtJ + lambda I)^-1 J_f^T of features of fs = 1 or 2 consecutive measurement rows
// (sparse_multi.hip / kernels_dense.hip): a chunk is MR = 16 rows (16 / fs features); every chunk leaves LEV_NP Gram
// products per slot (slots of chunk ch: [slot_ptr[ch], slot_ptr[ch + 1]), slot_ptr == nullptr: slot ch), summed by
// lev_finish in slot order.  Packed per feature: fs 1 {a}, fs 2 {a00, a01, a11}.
constexpr int LEV_NP = 24;
static __host__ __device__ inline int lev_np(int fs) { return fs == 1 ? 16 : 24; }
static __host__ __device__ inline int lev_nt(int fs) { return fs == 1 ? 1 : 3; }
// product p of a chunk: columns (a, c) of the chunk's 16 right-hand sides
static __device__ inline void lev_prod(int fs, int p, int& a, int& c)
{
  if(fs == 1) { a = c = p; return; }
  const int f = p / 3, e = p - 3*f;
  a = 2*f + (e == 2); c = 2*f + (e >= 1);
}
int sparse_leverage_reach(dlg_backend* b, int s, int fs, int nf, double** d_gram, const int** d_slot_ptr, long* visits);
int sparse_leverage_stats(const dlg_backend* b, int fs, long* nchunks, long* visits, int* nsn);
void sparse_leverage_free(SparseSym* Y);
int lev_gram_rows(dlg_backend* b, int s, int row0, int nrows, int fs, const double* d_il, double* d_gram);
int lev_finish(dlg_backend* b, int s, int nf, int fs, const int* d_slot_ptr, const double* d_gram, double scale, int mode, double* d_out);
int dense_leverage_gram(dlg_backend* b, int s, int fs, int nf, double* d_work, size_t work_doubles, double* d_gram);

// ---- covariance blocks Sigma = (JtJ + lambda I)^-1 (factor_users.hip: dlg_covariance_blocks / dlg_marginal_variances).
// A request is the sub-block Sigma[r0 : r0+nr, c0 : c0+nc] whose two ranges hold at most COV_MAXV distinct variables.
// Requests are packed whole into chunks of at most MR = 16 distinct variables (one unit right-hand side each); a chunk
// needs the Gram products (a, c), a <= c, of the columns its requests pair up, at most COV_NP.
constexpr int COV_MAXV = 16;
constexpr int COV_NP = COV_MAXV*(COV_MAXV + 1)/2;
struct CovPack
{
  int nch = 0, maxvar = 0;
  std::vector<int> var;        // [nch * 16] variables of a chunk, original order (-1: none)
  std::vector<int> pptr, prod; // products of chunk ch: prod[pptr[ch] .. pptr[ch + 1]), each a*16 + c
  std::vector<int> req_ch;     // chunk of each request
  std::vector<int> e_ch, e_p;  // per output value: its chunk and the index of its product there
  std::vector<int> kb0;        // dense: per chunk the first tile (of 64 variables) its solve needs
  // query covariance: the chunk's columns are rows crow[ch] .. crow[ch + 1] - 1 of the query CSR (rebased to row 0 and
  // entry 0: qrp [rows + 1], qvar in the caller's variable order)
  std::vector<int> crow, qrp, qvar;
};
// iperm: the permutation of the factor (sparse; null: dense, requests ordered by variable)
int cov_pack_requests(int N, const int* iperm, int nreq, const int* r0, const int* nr, const int* c0,
                      const int* nc, CovPack& K, const char* who);
void cov_pack_marginal(int N, const int* perm, CovPack& K);       // 16 consecutive (permuted) columns per chunk
// a reach plan (sparse_multi.hip): per chunk the supernodes on the paths from its columns to the root as (chunk,
// supernode) pairs sorted by (level, supernode), chunks cut into batches whose update blocks fit the scratch
struct ReachPlan
{
  int nf = -1, nch = 0, npair = 0, nbatch = 0;
  long visits = 0;                  // pairs = supernode visits of all chunks
  int64_t scr_rows = 0;             // update-block rows of the largest batch
  int *pair_sn = nullptr, *pair_ch = nullptr, *cp_ptr = nullptr, *wl = nullptr;
  int64_t* pair_off = nullptr;      // first row of the pair's update block in its batch's scratch
  double *gram = nullptr, *scr = nullptr;
  std::vector<int> wl_ptr;          // [nbatch * nlevels + 1] into wl: the pairs of a batch by level
};
void reach_plan_release(ReachPlan& P);
// a packed request list on the device, kept by the backend for the next call with the same arrays
struct CovPlan
{
  std::vector<int> key;             // route, pattern, N, then the request arrays it was built for
  CovPack K;
  long ne = 0;                      // output values
  double t_plan = 0.0;              // host seconds of the last build
  int *var = nullptr, *kb0 = nullptr, *pcol = nullptr, *pptr = nullptr, *prod = nullptr, *e_ch = nullptr, *e_p = nullptr, *slot_ptr = nullptr;
  int64_t* goff = nullptr;          // first product of a slot in gram
  double *gram = nullptr, *out = nullptr;
  ReachPlan R;                      // sparse, blocked route: slots are the (chunk, supernode) pairs
  // query plans: K.crow / K.qrp on the device, the variables (permuted on the sparse reach route), the values of the call
  int *crow = nullptr, *qrp = nullptr, *qvar = nullptr;
  double* qval = nullptr; long qnnz = 0;
};
// b->cov: the plans of dlg_covariance_blocks, dlg_marginal_variances, dlg_query_covariance and dlg_leverage_query
constexpr int COV_NPLAN = 4;
void cov_plan_release(CovPlan& P);
int cov_plan_build(dlg_backend* b, CovPlan& P, FactorRoute route, int which, int nreq, const int* r0, const int* nr, const int* c0,
                   const int* nc, const char* who);
uint64_t sparse_pattern_key(const dlg_backend* b);
int sparse_cov_reach_plan(dlg_backend* b, CovPlan& P);            // R, goff, slot_ptr, pcol and gram of the reach route
int sparse_cov_reach_run(dlg_backend* b, CovPlan& P);
int cov_plan_stats(const dlg_backend* b, const CovPlan& P, long* nchunks, long* visits, int* nsn);
int cov_unit_il(dlg_backend* b, const CovPlan& P, int ch, double* d_il);
int cov_pick(dlg_backend* b, const CovPlan& P, int ch, const double* d_il);
int cov_finish(dlg_backend* b, const CovPlan& P);
int dense_cov_setup(dlg_backend* b, CovPlan& P);      // P.kb0
int dense_cov_gram(dlg_backend* b, const CovPlan& P, double* d_work, size_t work_doubles);

// ---- query covariance Jq Sigma Jq^T (factor_users.hip: dlg_query_covariance).  A query is 1 .. 16 rows of a CSR over the
// variables; queries are packed whole, in order, into chunks of at most 16 rows (one right-hand side a row); a query of fs
// rows needs the fs (fs + 1) / 2 Gram products of its own rows.  The plan is a CovPlan (K.crow non-empty); route 0: the
// reach of the chunks' variables (sparse), 1: full solves (sparse sweep, and the observation form), 2: dense forward.
constexpr int QCOV_MAXROWS = 16;
int query_pack(int N, int nq, const int* qrow, const int* rowptr, const int* var, CovPack& K, const char* who);
int query_plan_build(dlg_backend* b, CovPlan& P, FactorRoute route, int nq, const int* qrow, const int* rowptr, const int* var,
                     const char* who);
int sparse_query_reach_run(dlg_backend* b, CovPlan& P);
int query_rhs_il(dlg_backend* b, const CovPlan& P, int ch0, int nch, double* d_il);   // Jq^T of chunks ch0 .. (interleaved, original order), chunk q at d_il + q N 16
int query_gram_rows(dlg_backend* b, const CovPlan& P, int ch, const double* d_il);    // products of chunk ch from U = Sigma Jq^T
// the observation form: products of (J[0:nobs] U)^T (J[0:nobs] U) of chunks ch0 .. ch0 + nch - 1 (nch <= QOBS_NC), U of
// chunk ch0 + q at d_U + q N 16; d_part: QOBS_WG * QOBS_NC * 256 doubles of scratch
constexpr int QOBS_NC = 4, QOBS_WG = 1024;
int query_obs_gram(dlg_backend* b, int s, const CovPlan& P, int ch0, int nch, int nobs, const double* d_U, double* d_part);

// ---- the selected inverse: Sigma on the structure of the factor (sparse_selinv.hip: dlg_covariance_entries).  Sparse,
// Sigma is formed on every panel entry of L in one sweep from the root down (Sx, laid out as Lx); dense, the whole of
// Sigma = L^-T L^-1.  Built on first use, released with the pattern, by dlg_backend_reset and with the backend.
struct SelTask { int s, ti, tj, pad; };
struct SelInv
{
  // sparse sweep plan (of the pattern)
  bool sparse_ready = false;
  int ndepth = 0, nprep = 0;
  std::vector<int> tb_ptr, tc_ptr;  // [ndepth + 1] into task: the Sigma_BJ tiles and the Sigma_JJ tiles of a depth
  SelTask *prep = nullptr, *task = nullptr;
  int *par = nullptr, *prel = nullptr; int64_t* foff = nullptr;
  int64_t fsize[2] = {0, 0}, sx_n = 0; int prep_lds = 0;
  double *Sx = nullptr, *Yb = nullptr, *F[2] = {nullptr, nullptr};
  // dense: L^-1 row-major, Sigma (lower, column-major), the forward solve's chunks of 16 unit columns
  int dn = 0, dnch = 0, dper = 0;
  int *dvar = nullptr, *dystart = nullptr;
  double *Linv_rm = nullptr, *Sig = nullptr, *dwork = nullptr;
  // entry lookup of the last request arrays: positions in Sx / Sig
  std::vector<int> qkey;
  long nq = 0;
  int64_t* qpos = nullptr; double* qout = nullptr;
  double t_plan = -1.0;             // host seconds the last call spent on plans (sweep and lookup), 0: all cached
};
void selinv_release(dlg_backend* b);
void selinv_release_sparse(dlg_backend* b);   // what was built against the pattern
int selinv_entries(dlg_backend* b, long n, const int* row, const int* col, double* out_host, const char* who);
int dense_selinv_run(dlg_backend* b, SelInv& X);   // X.Sig = (L L^T)^-1, lower (kernels_dense.hip)
