// driver_records.cpp -- what a solve writes down beside its result: the vnlog record (dogleg.c:42-113), the trace a
// test attaches (dlg_trace.h), the DOGLEG_AMD_TIMING breakdown.
#include <cmath>
#include <cstring>
#include "driver_internal.h"

namespace {

thread_local dlg_trace_t* t_trace = nullptr;
thread_local double t_last_tm_ms[TM_COUNT + 1]; thread_local int t_last_tm_n[TM_COUNT + 1];      // dogleg_amd_last_solve_timing
const char* const k_tm_names[TM_COUNT] = { "pattern (symbolic phase or comparison with the parked one)", "model callback (host: evaluation; device: enqueue)",
                                           "inputs to the backend (upload / bind / gather)", "dlg_point_eval (K1 [+ K4, leaf level ahead], norms fetched)",
                                           "dlg_take_step / dlg_step (K3 .. K8, p_new fetched)", "trace / vnlog records (test harness, debug)" };

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

} // namespace

void vnlog_legend()
{
  printf("# iteration step_accepted norm2x_before norm2x_after step_len_cauchy step_len_gauss_newton "
         "step_len_interpolated k_cauchy_to_gn step_len step_type step_direction_change_deg "
         "expected_improvement observed_improvement rho trustregion_before trustregion_after\n");
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

void trace_begin(int Nstate)
{
  if(dlg_trace_t* tr = t_trace) { tr->ntrials = 0; tr->ncallbacks = 0; tr->nstate = Nstate; }
}
void trace_end(const Driver* d)
{
  if(dlg_trace_t* tr = t_trace) tr->ncallbacks = d->ncallbacks;
}

void timing_report(const Driver* d, double run_ms)
{
  // where run_optimizer's wall time went: the driver's own calls, host clock (one line for all of it hid 6 ms)
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

extern "C" {

void dlg_set_trace(void* tr) { t_trace = (dlg_trace_t*)tr; }

// where the calling thread's last solve spent its wall time (DOGLEG_AMD_TIMING=1 must have been set for it): milliseconds and
// calls of {pattern, model callback, inputs to the backend, dlg_point_eval, dlg_take_step / dlg_step, trace records,
// run_optimizer as a whole} -- everything but the second entry is the library's share of a trial (tools/e2e_bench.py)
int dogleg_amd_last_solve_timing(double* ms7, int* calls7)
{
  for(int k = 0; k <= TM_COUNT; k++) { if(ms7) ms7[k] = t_last_tm_ms[k]; if(calls7) calls7[k] = t_last_tm_n[k]; }
  return TM_COUNT + 1;
}

} // extern "C"
