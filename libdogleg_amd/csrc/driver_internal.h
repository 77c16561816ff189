// driver_internal.h -- what the files of the host driver share (not installed): the Driver behind a
// dogleg_solverContext_t, a solve's communicator, messages, the DOGLEG_AMD_TIMING scopes.
//   driver.hip          the trust-region loop, operating points, dogleg_optimize* (the restatement of dogleg.c)
//   driver_cache.hip    what outlives a solve: the parked backend, the pool of page-locked buffers
//   driver_comm.hip     multi-GPU: the calling thread's / the environment's communicator, attach_communicator
//   driver_records.cpp  vnlog and trace records, the timing report
//   api_extensions.hip  entry points that check their arguments and forward (outliers, covariance, batch, gradcheck)
//   id_file.cpp         the id-file rendezvous of the environment contract
//   robust_prelude.hip  a loss on a device solve: weights, F = sum rho and the sqrt(w) scaling of x and J behind the callback
//   bounds_device.hip   box bounds on a device solve: the held set, g_F and the masked J behind an evaluation, the clipped step
// Everything declared here is hidden: the library exports dogleg.h, dlg_backend.h and dlg_trace.h, nothing of this.
#pragma once
#include <cstdio>
#include <cstddef>
#include <chrono>
#include <future>
#include "../../include/dogleg.h"
#include "../../include/dlg_backend.h"
#include "../../include/dlg_trace.h"
#include "driver_msg.h"

#define VERBOSE(c, ...) do { if((c)->pub.parameters->debug && !(c)->pub.parameters->debug_vnlog) MSG(__VA_ARGS__); } while(0)

#pragma GCC visibility push(hidden)

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

struct Robust;                                 // robust_prelude.hip
struct Bounds;                                 // bounds_device.hip

enum { TM_PATTERN, TM_CALLBACK, TM_UPLOAD, TM_EVAL, TM_STEP, TM_TRACE, TM_COUNT };

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
  Robust* robust;                              // dogleg_amd_optimize_device2_robust: the loss and its device arrays; NULL: least squares, nothing of it runs
  Bounds* bounds;                              // dogleg_amd_optimize_device2_bounded: the box and its device arrays; NULL: no bounds, nothing of it runs
  // DOGLEG_AMD_TIMING=1: where the wall time of run_optimizer goes (host clock around the driver's own calls)
  bool timing;
  double tm_ms[8]; int tm_n[8];
};
struct Tick
{
  Driver* d; int k; std::chrono::steady_clock::time_point t0;
  Tick(Driver* d_, int k_) : d(d_), k(k_) { if(d->timing) t0 = std::chrono::steady_clock::now(); }
  ~Tick() { if(d->timing) { d->tm_ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); d->tm_n[k]++; } }
};

inline Driver* D(dogleg_solverContext_t* ctx) { return reinterpret_cast<Driver*>(ctx); }
inline int slot_of(const Driver* d, const dogleg_operatingPoint_t* pt) { return pt == d->pts[0] ? 0 : 1; }
inline bool be_ok(int rc, const char* what)
{
  if(rc == DLG_OK) return true;
  MSG("%s failed: %s", what, dlg_last_error());
  return false;
}

// ---- driver.hip
extern dogleg_parameters2_t g_params;          // the legacy process-global set (dogleg.c:131)
// doubles in ctx->factorization_dense (dogleg.c:1707-1725): packed for DENSE, as JtJ was given for DENSE_PRODUCTS
size_t dense_factor_size(const dogleg_solverContext_t* ctx);

// ---- driver_cache.hip
bool cache_on();
dlg_backend_t* take_parked(int type, int N, int M, int nnz, int flags, int device);
void park_backend(dlg_backend_t* be, int type, int N, int M, int nnz, int flags);
void* pinned_take(size_t bytes);
void pinned_give(void* p, size_t bytes);

// ---- driver_comm.hip
// this solve's communicator: the calling thread's, else the environment's, else none (one GPU); false: a message was printed
bool solve_communicator(Comm* cm);
// makes d->be one rank of cm (no-op without a communicator, and for dense-products); false: a message was printed
bool attach_communicator(Driver* d, const Comm& cm);
// entry points that run on one GPU only: false, with a message, if the caller has a communicator
bool one_rank_only(const char* who);

// ---- driver_records.cpp
void vnlog_legend();
void cur_reset(Driver* d);
void emit(Driver* d, int iteration, int accepted);        // closes the trial record d->cur: vnlog line, trace entry
void trace_begin(int Nstate);
void trace_end(const Driver* d);
// DOGLEG_AMD_TIMING: run_optimizer's wall time by TM_* on stderr, kept for dogleg_amd_last_solve_timing
void timing_report(const Driver* d, double run_ms);

// ---- robust_prelude.hip: a loss on a device solve.  One rank, device callback only.
// the checks of the entry point that need no device; false: a message was printed
bool robust_loss_ok(const dogleg_amd_batch_loss_t* loss, unsigned int Nmeas, unsigned int NJnnz, const int* Jt_colptr);
// the record of a solve (host only; the device arrays come with robust_set_up, behind the backend)
Robust* robust_create(const dogleg_amd_batch_loss_t* loss);
bool robust_set_up(Driver* d);
// behind the callback that wrote x and J of slot s, on the backend's stream: weights, F, x and J times sqrt(w)
void robust_enqueue(Driver* d, int s, double* x, double* J);
// F of the last prelude of slot s, once the host has it (waits for the 8-byte copy behind that prelude)
bool robust_F(Driver* d, int s, double* F);
bool robust_weights(Driver* d, int s, double* weights_host);
void robust_destroy(Driver* d);
void robust_release_cache();                   // dogleg_amd_release_cache: the device block kept between robust solves

// ---- bounds_device.hip: box bounds on a device solve.  One rank, device callback only.
// the checks of the entry point that need no device (a NULL bounds, weights without a loss, a NaN bound, lower > upper); false: a message was printed
bool bounds_args_ok(const dogleg_amd_batch_bounds_t* bounds, const dogleg_amd_batch_loss_t* loss, const double* weights, const double* p,
                    unsigned int Nstate);
Bounds* bounds_create(const dogleg_amd_batch_bounds_t* bounds);
void bounds_clamp_start(const Driver* d, double* p);      // step 1, on the host
bool bounds_set_up(Driver* d);
// behind dlg_point_eval of slot s: held bytes, g_F in place, the held columns of J zeroed, the backend told; *absmax = |g_F|_inf
bool bounds_hold_mask(Driver* d, int s, double* absmax);
void bounds_note_step(Driver* d, int from);               // a step is taken from slot `from` (counts the ones with a held variable)
// behind a step into slot `to`: clamp p and the step in place; clamped components, max |s'|, |s'|^2
bool bounds_clip(Driver* d, int from, int to, double* clamped, double* smax, double* n2);
// the Cauchy step of `from` times t0, cut at the first bound, into slot `to`
bool bounds_fallback(Driver* d, int from, int to, double t0, double* smax, double* n2);
bool bounds_finish(Driver* d, int s);                     // held of slot s to the caller, the stats record
void bounds_destroy(Driver* d);
void bounds_release_cache();                   // dogleg_amd_release_cache: the device block kept between bounded solves

#pragma GCC visibility pop
