// step.hip -- the per-step path of the C-ABI in include/dlg_backend.h: operating-point inputs and their evaluation (K1),
// the Cauchy step (K3), factorisation and Gauss-Newton solve (K4 - K6) with the reference's lambda loop, the step (K7), its
// expected improvement (K8), and the fused forms dlg_step / dlg_take_step / dlg_run_steps that put them behind one host
// synchronisation.  Host code only, apart from two one-wave kernels that order the second stream.  A step function tells a
// launcher what a launch carries beyond its arguments with a StepLaunch (dlg_internal.h), never through the backend.
#include "dlg_internal.h"

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
// every expected improvement handed out goes through here (DOGLEG_AMD_DEBUG_EI_FLIP: the n-th one is negated)
static double ei_out(dlg_backend* b, double v)
{
  if(b->ei_flip > 0 && ++b->ei_count == b->ei_flip) return -fabs(v);
  return v;
}
// Before anything overwrites what a tail that is still out reads (the step vector, p_new, J of its slot): the tail is a
// launch on the backend's own stream, so whatever is enqueued there is behind it already.
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

extern "C" int dlg_point_set_p(dlg_backend_t* b, int s, const double* p_host)
{
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(tail_guard(b));
  DLG_HIP(hipMemcpyAsync(b->slot[s].p, p_host, sizeof(double)*(size_t)b->N, hipMemcpyHostToDevice,
                         b->stream));
  DLG_HIP(hipStreamSynchronize(b->stream));     // p_host may be pageable / reused
  return DLG_OK;
}

extern "C" int dlg_point_upload(dlg_backend_t* b, int s, const double* x_host, const double* J_host)
{
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
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
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
  if(b->type != DLG_DENSE_PRODUCTS) { dlg_set_error("not a dense-products backend"); return DLG_ERR_ARG; }
  DlgSlot& S = b->slot[s];
  S.x_bound = S.J_bound = nullptr;
  DLG_HIP(hipMemcpyAsync(S.Jt_x, Jtx_host, sizeof(double)*(size_t)b->N, hipMemcpyHostToDevice, b->stream));
  DLG_HIP(hipMemcpyAsync(S.J, JtJ_host, sizeof(double)*dlg_j_doubles(b), hipMemcpyHostToDevice, b->stream));
  S.norm2_x = norm2x;
  S.have_inputs = true;
  invalidate(S);
  if(b->factor_slot == s) b->factor_slot = -1;
  return DLG_OK;
}

extern "C" int dlg_point_bind_device(dlg_backend_t* b, int s, const double* x_dev, const double* J_dev)
{
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
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
int dlg_step_unprepare(dlg_backend* b)
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
  // behind it, back to back.  A rejected point (dlg_step_unprepare) then has one kernel to abandon, not K5 + K6.
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
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
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
      DLG_CHECK(dlg_allreduce_dev(b, S.Jt_x, (size_t)b->N + 1));
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
      DLG_CHECK(k_norm2_absmax_pair(b, S.Jt_x, b->N, b->d_scal + 2, S.xin(), mloc, b->d_scal, &norms_on_host, b->ext_events ? b->ev_fetch : nullptr));
    }
    else     DLG_CHECK(k_norm2_absmax(b, S.Jt_x, b->N, b->d_scal + 2));
    if(fused)
    {
      // the scalars go to the host first; the partial-sum stages of JtJ run while the host gets them
      if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
      // (the workgroups of the norm kernel wrote their partial sums to page-locked host memory and the host
      // adds them: nothing to copy then -- the event alone is the point the host waits for)
      if(!norms_on_host) DLG_HIP(hipMemcpyAsync(b->h_scal, b->d_scal, sizeof(double)*4, hipMemcpyDeviceToHost, b->stream));
      if(!(norms_on_host && b->ext_events)) DLG_HIP(hipEventRecord(b->ev_fetch, b->stream));      // (else the event rode on the norm kernel)
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
static int norm2_Jv(dlg_backend* b, int s, const double* v, double* out, StepLaunch& L, const double* kind_if_factor_failed = nullptr)
{
  DlgProfScope ps(b, DLG_PROF_K3K8_NORM2JV);
  switch(b->type)
  {
  case DLG_SPARSE:  DLG_CHECK(sparse_norm2_Jv(b, s, v, out, kind_if_factor_failed, L)); break;
  case DLG_DENSE:   DLG_CHECK(dense_norm2_Jv(b, s, v, out, L)); break;
  default:          return products_quadform(b, s, v, out);
  }
  return dlg_allreduce_dev(b, out, 1);
}

// ---------------------------------------------------------------------- K3 --
// launches only: sc[1] = |J g|^2, sc[2] = |cauchy|^2 (device scalars)
static int cauchy_enqueue(dlg_backend* b, int s, double* sc)
{
  DlgSlot& S = b->slot[s];
  StepLaunch plain;
  DLG_CHECK(norm2_Jv(b, s, S.Jt_x, sc + 1, plain));
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
    StepLaunch plain;
    rc = sparse_norm2_Jv(b, s, b->slot[s].Jt_x, sc + 1, nullptr, plain);
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
  DLG_CHECK(dlg_check_slot(b, s));
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
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
  DlgSlot& S = b->slot[s];
  if(!S.have_inputs) { dlg_set_error("dlg_factorize: slot %d has no J/JtJ", s); return DLG_ERR_STATE; }
  // (a Gauss-Newton step this slot still holds came from another factor -- another lambda, perhaps: dlg_solve_gn and
  // dlg_gauss_newton would hand it out again as the cached one)
  S.have_gn = false; S.ident_ok = false;
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
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
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

// ------------------------------------------------- the lambda loop's pieces --
// the reference's schedule: dogleg.c:138, 671-672, 812-813
static int lambda_next(double* lam)
{
  *lam = (*lam == 0.0) ? 1e-10 : *lam*10.0;
  if(!(*lam < 1e300)) { dlg_set_error("lambda overflowed while regularising a singular JtJ"); return DLG_ERR_STATE; }
  return DLG_OK;
}
// One factorisation attempt of slot s at lam goes onto the stream; nothing is fetched (defer_factor_sync: the pivot flag is
// read behind the synchronisation of what follows, factor_verdict).  *doomed: found doomed at the diagonal, in front of
// every launch (sparse_factorize) -- nothing was enqueued, the caller goes on to the next lambda at once.
static int factor_enqueue(dlg_backend* b, int s, double lam, bool* doomed)
{
  DlgProfCond pc(b);
  int good = 0, rc;
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
  *doomed = b->factor_doomed;
  if(!*doomed) return DLG_OK;
  b->factor_doomed = false; b->want_fork = false; b->factor_slot = -1;
  if(b->profiling) { dlg_prof_resolve(b); dlg_prof_commit(b, false); }
  return DLG_OK;
}
// Behind the synchronisation that brought the pivot flag: did the attempt for slot s hold?  One that broke down is noted
// (full clears next -- unless nothing of it ran) and no factor is held.
static bool factor_verdict(dlg_backend* b, int s)
{
  const bool good = b->factor_slot == s || (b->type == DLG_SPARSE ? sparse_factor_ok(b) : dense_factor_ok(b));
  if(b->profiling) dlg_prof_commit(b, good);
  if(good) return true;
  if(b->type == DLG_SPARSE && !sparse_note_breakdown(b)) sparse_mark_unclean(b);
  b->factor_slot = -1;
  return false;
}
// K6 behind a factorisation of this attempt (returns early if that one failed)
static int gn_solve_enqueue(dlg_backend* b, DlgSlot& S)
{
  DlgProfCond pc(b);
  DlgProfScope ps(b, DLG_PROF_K6_SOLVE);
  return b->type == DLG_SPARSE ? sparse_solve(b, S.Jt_x, S.gn) : dense_solve(b, S.Jt_x, S.gn);
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
  DLG_CHECK(dlg_check_slot(b, s));
  DLG_CHECK(dlg_step_unprepare(b));
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
    // the Cauchy step rides along (its scalars come back with the same synchronisation), on the
    // second stream beside the factorisation
    const bool do_cauchy = with_cauchy && !S.have_cauchy && !cauchy_pending;
    if(do_cauchy) DLG_CHECK(cauchy_fork_begin(b));
    if(b->factor_slot != s)
    {
      bool doomed = false;
      DLG_CHECK(factor_enqueue(b, s, lam, &doomed));
      if(doomed) { DLG_CHECK(lambda_next(&lam)); continue; }
    }
    if(do_cauchy)
    {
      DLG_CHECK(cauchy_fork_enqueue(b, s, b->d_scal + 4));
      cauchy_pending = true;
    }
    DLG_CHECK(gn_solve_enqueue(b, S));
    DLG_CHECK(cauchy_deferred_finish(b, s));
    DLG_CHECK(k_negate_norm2(b, S.gn, b->N, b->d_scal));      // dogleg.c:862-865
    DLG_CHECK(dlg_fetch_scalars(b, dlg_backend::NSCAL));      // the one synchronisation (the sparse pivot flag rides in the last slot)
    if(b->profiling) dlg_prof_resolve(b);
    if(cauchy_pending && !S.have_cauchy) { S.norm2_cauchy = b->h_scal[6]; S.Jg2 = b->sharded() ? 0.0 : b->h_scal[5]; S.have_cauchy = true; }
    if(factor_verdict(b, s)) break;
    if(b->tail_pending) { DLG_CHECK(tail_guard(b)); b->tail_pending = false; }     // (that attempt's K8 returned at its first look at the pivot flag)
    DLG_CHECK(lambda_next(&lam));
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

// ------------------------------------------- what the step functions share --
// Where the caller wants p_new: looked up ONCE per C call (hipPointerGetAttributes is ~1 us).  pinned: page-locked host memory,
// a copy engine writes it directly; dev: its device address -- a kernel can write it (K8 takes p_new along); neither: pageable,
// the copy goes through the backend's page-locked h_vec (step_finish).
struct PDest { double* host = nullptr; bool pinned = false; double* dev = nullptr; };
static PDest p_dest(double* p_new_host)
{
  PDest d;
  d.host = p_new_host;
  if(!p_new_host) return d;
  hipPointerAttribute_t attr;
  if(hipPointerGetAttributes(&attr, p_new_host) == hipSuccess && attr.type == hipMemoryTypeHost) { d.pinned = true; d.dev = (double*)attr.devicePointer; }
  else (void)hipGetLastError();
  return d;
}
// p_new of slot `to` to a page-locked destination on the copy stream, behind `after` (an event of the main stream: recorded
// there, or riding on a launch); ev_copy is behind the copy
static int p_copy_side(dlg_backend* b, int to, double* dst, hipEvent_t after)
{
  DLG_HIP(hipStreamWaitEvent(b->copy_stream, after, 0));
  DLG_HIP(hipMemcpyAsync(dst, b->slot[to].p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->copy_stream));
  DLG_HIP(hipEventRecord(b->ev_copy, b->copy_stream));
  return DLG_OK;
}
// the caller's between function (dlg_backend_set_between) is armed for ONE step call, whichever way that call returns
struct BetweenScope
{
  dlg_backend* b;
  explicit BetweenScope(dlg_backend* b_) : b(b_) { b->between_armed = b->between_fn != nullptr; b->between_ran = false; b->between_redone = false; }
  ~BetweenScope() { b->between_armed = false; b->between_fn = nullptr; }
};
// an expected improvement handed out by the call that formed it (dogleg.c:1107-1109): -2 <Jt x, step> - |J step|^2
static double ei_inline(dlg_backend* b, double inner, double norm2_Jstep, bool from_system)
{
  b->tail_value = ei_out(b, -2.0*inner - norm2_Jstep);
  b->ei_from_system = from_system;
  return b->tail_value;
}

// ---------------------------------------------------------------------- K7 --
// launches the step kernel (its scalars land in d_scal[0..2]); nscal = how many to fetch
static int make_step_enqueue(dlg_backend* b, int from, int to, int kind, double trustregion, int* nscal, const StepLaunch& L)
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
                            b->d_scal, L));
    *nscal = 3;
    break;
  default:
    dlg_set_error("dlg_make_step: unknown kind %d", kind);
    return DLG_ERR_ARG;
  }
  return DLG_OK;
}
// the scalars of a step of `kind` from the cached vectors of `from`, once they are on the host, to the caller (returns k)
static double step_scalars_out(dlg_backend* b, int from, int kind, double* norm2_step, double* k_cauchy_to_gn, double* step_absmax)
{
  DlgSlot& F = b->slot[from];
  double n2, kk = NAN, amax;
  switch(kind)
  {
  case DLG_KIND_CAUCHY_TO_EDGE: n2 = F.norm2_cauchy; amax = b->h_scal[0]; break;   // unscaled: dogleg.c:1200
  case DLG_KIND_GAUSSNEWTON:    n2 = F.norm2_gn;     amax = b->h_scal[0]; break;
  default:                      n2 = b->h_scal[0]; kk = b->h_scal[1]; amax = b->h_scal[2]; break;
  }
  if(norm2_step) *norm2_step = n2;
  if(k_cauchy_to_gn) *k_cauchy_to_gn = kk;
  if(step_absmax) *step_absmax = amax;
  return kk;
}
// Scalars and (pd.host: here, not on the copy stream or with K8) p_new back to the host behind ONE synchronisation.
// attached / scal_copied: what the step's last launch reported (StepLaunch) -- it carries ev_fetch; it has written the
// scalars to the page-locked h_scal itself (or every scalar is a sum of page-locked partials: nothing to copy).
static int step_finish(dlg_backend* b, int to, int nscal, const PDest& pd, bool attached, bool scal_copied)
{
  DlgSlot& T = b->slot[to];
  attached = attached && scal_copied && !pd.host;
  if(!scal_copied) DLG_HIP(hipMemcpyAsync(b->h_scal, b->d_scal, sizeof(double)*(size_t)nscal, hipMemcpyDeviceToHost, b->stream));
  // page-locked destination (the driver's operating points, dlg_host_alloc): straight DMA;
  // pageable: through the backend's pinned staging vector
  if(pd.host) DLG_HIP(hipMemcpyAsync(pd.pinned ? pd.host : b->h_vec, T.p, sizeof(double)*(size_t)b->N, hipMemcpyDeviceToHost, b->stream));
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
  if(pd.host && !pd.pinned) memcpy(pd.host, b->h_vec, sizeof(double)*(size_t)b->N);
  return nscal >= dlg_backend::NSCAL ? dlg_check_handoff(b) : DLG_OK;
}
extern "C" int dlg_make_step(dlg_backend_t* b, int from, int to, int kind, double trustregion,
                             double* norm2_step, double* k_cauchy_to_gn, double* step_absmax,
                             double* p_new_host)
{
  DLG_CHECK(dlg_check_slot(b, from)); DLG_CHECK(dlg_check_slot(b, to));
  if(from == to) { dlg_set_error("dlg_make_step: from == to"); return DLG_ERR_ARG; }
  // (a step from the cached vectors of `from` after the trial point was rejected: what dlg_point_eval enqueued for
  // the trial point is dropped and the factor it displaced is the held one again BEFORE step_finish clears the
  // spare panel buffer -- which is where the displaced factor lives)
  DLG_CHECK(dlg_step_unprepare(b));
  DLG_CHECK(tail_guard(b)); b->tail_pending = false;
  int nscal = 0;
  DLG_CHECK(make_step_enqueue(b, from, to, kind, trustregion, &nscal, StepLaunch()));
  DLG_CHECK(step_finish(b, to, nscal, p_dest(p_new_host), false, false));
  step_scalars_out(b, from, kind, norm2_step, k_cauchy_to_gn, step_absmax);
  return DLG_OK;
}

// ---------------------------------------------------------------------- K8 --
static int expected_improvement_enqueue(dlg_backend* b, int from, int to, double* sc)
{
  DlgSlot& F = b->slot[from];
  DlgSlot& T = b->slot[to];
  if(!F.have_Jtx) { dlg_set_error("expected improvement needs Jt_x"); return DLG_ERR_STATE; }
  StepLaunch plain;
  DLG_CHECK(k_inner(b, F.Jt_x, T.step, b->N, sc, plain));
  DLG_CHECK(norm2_Jv(b, from, T.step, sc + 1, plain));
  return DLG_OK;
}
extern "C" int dlg_expected_improvement(dlg_backend_t* b, int from, int to, double* out)
{
  DLG_CHECK(dlg_check_slot(b, from)); DLG_CHECK(dlg_check_slot(b, to));
  DLG_CHECK(expected_improvement_enqueue(b, from, to, b->d_scal));
  DLG_CHECK(dlg_fetch_scalars(b, 2));
  if(out) *out = ei_inline(b, b->h_scal[0], b->h_scal[1], false);
  return DLG_OK;
}
// The step and <Jt x, step> (d_scal[4]) of dlg_step's forms that wait for that sum's kernel (wait): it carries ev_fetch, and
// every scalar of the step reaches the host through page-locked partial sums -- nothing is copied on the main stream.
static int step_inner_enqueue(dlg_backend* b, int from, int to, int kind, double trustregion, bool wait)
{
  int nscal = 0;
  StepLaunch L7, Li;
  L7.k_host = wait;
  DLG_CHECK(make_step_enqueue(b, from, to, kind, trustregion, &nscal, L7));
  if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
  if(wait) Li.stop = b->ev_fetch;
  DLG_CHECK(k_inner(b, b->slot[from].Jt_x, b->slot[to].step, b->N, b->d_scal + 4, Li));
  // The launch always takes the event.  dlg_step asks for this form only with host_finals, h_part, ext_events and
  // h_part_used + 4096 <= HPART_CAP; the step kernel then takes at most 2 x 1024 page-locked partials (k_interpolate; 1024:
  // k_scaled_step) and k_inner at most 1024 (grid_for: MAXB), into d_scal: dlg_host_partials finds room for both.
  if(wait && !Li.attached) { dlg_set_error("internal error: dlg_step's sum <Jt x, step> found no page-locked room behind its own check"); return DLG_ERR_STATE; }
  return DLG_OK;
}
// K7 + K8 behind one synchronisation: the step (dlg_make_step), its expected improvement
// (dlg_expected_improvement, dogleg.c:1258-1269 computes it right after the step) and p_new
extern "C" int dlg_step(dlg_backend_t* b, int from, int to, int kind, double trustregion,
                        double* norm2_step, double* k_cauchy_to_gn, double* step_absmax,
                        double* expected_improvement, double* p_new_host)
{
  DLG_CHECK(dlg_check_slot(b, from)); DLG_CHECK(dlg_check_slot(b, to));
  if(from == to) { dlg_set_error("dlg_step: from == to"); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_step_unprepare(b));                 // (as in dlg_make_step: the driver's retry after a rejected trial point)
  DLG_CHECK(tail_guard(b)); b->tail_pending = false;
  BetweenScope between(b);
  DlgSlot& F = b->slot[from];
  DlgSlot& T = b->slot[to];
  const PDest pd = p_dest(p_new_host);
  // The deferred form (dlg_backend_set_defer_tail): the host waits for the kernel that forms <Jt x, step> -- every scalar of the
  // step reaches it through page-locked partial sums, nothing is copied on the main stream.  (A destination a kernel cannot
  // write -- pageable -- takes the in-line form.)
  const int chunks = b->type == DLG_SPARSE ? sparse_norm2_chunks(b) : (b->type == DLG_DENSE ? dense_norm2_chunks(b) : 0);
  const bool defer = b->defer_tail && expected_improvement && b->host_finals && b->h_part && !b->sharded() && (!p_new_host || pd.dev) &&
                     !(b->prof_mask >> DLG_PROF_K3K8_NORM2JV & 1u) && !(b->prof_mask >> DLG_PROF_K7_STEP & 1u) && b->ext_events &&
                     chunks > 0 && F.have_Jtx && b->h_part_used + 4096 <= dlg_backend::HPART_CAP &&      // (room for the step's partial sums: 4 x 1024 at most)
                     dlg_tail_partials(b, chunks) != nullptr;
  // The expected improvement from the solved system (ident_norm2_Jstep): a step from the cached vectors of a point whose
  // dlg_take_step left <Jt x, gn> and the factor's verdict behind -- or the Cauchy step, which needs K3's scalar only --
  // has no pass over J at all: step, <Jt x, step>, one synchronisation.  In the deferred form p_new travels on the copy
  // stream behind that kernel's event and dlg_step_tail hands the value out (it is complete, the copy may not be).
  const bool ident = expected_improvement && !b->knobs.ei_jpass && b->host_finals && !b->sharded() && b->part_nranks <= 1 &&
                     b->type != DLG_DENSE_PRODUCTS && F.have_Jtx && F.have_cauchy && F.Jg2 > 0.0 &&
                     (kind == DLG_KIND_CAUCHY_TO_EDGE || (F.ident_ok && F.have_gn));
  if(ident)
  {
    const bool deferred = defer && (!p_new_host || b->copy_stream);
    DLG_CHECK(step_inner_enqueue(b, from, to, kind, trustregion, deferred));
    if(deferred)
    {
      if(p_new_host) { DLG_CHECK(p_copy_side(b, to, p_new_host, b->ev_fetch)); b->p_side_pending = true; }
      DLG_CHECK(step_finish(b, to, 0, PDest(), true, true));
    }
    else DLG_CHECK(step_finish(b, to, 6, pd, false, false));
    const double kk = step_scalars_out(b, from, kind, norm2_step, k_cauchy_to_gn, step_absmax);
    const double nJs = ident_norm2_Jstep(kind, kk, trustregion, F.norm2_jtx, F.Jg2, F.norm2_cauchy, F.g_dot_gn, F.ident_lam, F.norm2_gn, F.a_dot_gn);
    if(deferred)
    {
      b->tail_pending = true; b->tail_ident = true; b->tail_nJs = nJs; b->tail_no_fold = true;
      b->tail_inner = b->h_scal[4]; b->tail_mark = b->sync_mark;
      *expected_improvement = NAN;                             // (dlg_step_tail has it, and p_new complete)
    }
    else *expected_improvement = ei_inline(b, b->h_scal[4], nJs, true);
    return DLG_OK;
  }
  // K8 behind the decision point, as in dlg_take_step: the pass over J (no factorisation of this call for it to look at)
  // and p_new, a slice per workgroup, follow the kernel the host waits for on the stream; dlg_step_tail has the value
  if(defer)
  {
    DLG_CHECK(step_inner_enqueue(b, from, to, kind, trustregion, true));
    StepLaunch L8;
    L8.tail = true;
    if(p_new_host) { L8.p_src = T.p; L8.p_dst = pd.dev; }
    DLG_CHECK(b->type == DLG_SPARSE ? sparse_norm2_Jv(b, from, T.step, b->d_scal + 5, nullptr, L8) : dense_norm2_Jv(b, from, T.step, b->d_scal + 5, L8));
    b->tail_pending = true;
    DLG_CHECK(step_finish(b, to, 0, PDest(), true, true));
    b->tail_mark = b->sync_mark;
    b->tail_inner = b->h_scal[4];
    step_scalars_out(b, from, kind, norm2_step, k_cauchy_to_gn, step_absmax);
    *expected_improvement = NAN;                               // (dlg_step_tail has it)
    return DLG_OK;
  }
  // In line: K8 in front of the synchronisation.
  int nscal = 0;
  DLG_CHECK(make_step_enqueue(b, from, to, kind, trustregion, &nscal, StepLaunch()));
  // p_new is final here: it travels to the host on the side stream while K8 runs (a page-locked
  // destination; a pageable one goes through step_finish's staging copy afterwards)
  const bool side_copy = pd.pinned && b->copy_stream;
  if(side_copy)
  {
    DLG_HIP(hipEventRecord(b->ev_step, b->stream));
    DLG_CHECK(p_copy_side(b, to, p_new_host, b->ev_step));
  }
  DLG_CHECK(expected_improvement_enqueue(b, from, to, b->d_scal + 4));
  DLG_CHECK(step_finish(b, to, 6, side_copy ? PDest() : pd, false, false));
  if(side_copy) DLG_HIP(hipEventSynchronize(b->ev_copy));
  step_scalars_out(b, from, kind, norm2_step, k_cauchy_to_gn, step_absmax);
  if(expected_improvement) *expected_improvement = ei_inline(b, b->h_scal[4], b->h_scal[5], false);
  return DLG_OK;
}

// ------------------------------------------------ K3 .. K8, one round trip ----
// K8 of dlg_take_step in the tail's form: its partial sums go to page-locked memory of their own, dlg_step_tail adds them
static int take_step_tail_k8(dlg_backend* b, int from, int to, StepLaunch& L)
{
  L.tail = true;
  return b->type == DLG_SPARSE ? sparse_norm2_Jv(b, from, b->slot[to].step, b->d_scal + 12, b->d_scal + 8, L)
                               : dense_norm2_Jv(b, from, b->slot[to].step, b->d_scal + 12, L);
}
// out7 of dlg_take_step from the scalars on the host.  The Cauchy step: |gn|^2 and k are not reported (the Gauss-Newton
// step was dropped).  The expected improvement (dogleg.c:1107-1109) is NaN where dlg_step_tail has it.
static void take_step_out7(dlg_backend* b, const DlgSlot& F, bool defer, bool ident_used, double ident_nJs, double* out7)
{
  const int kind = (int)b->h_scal[8];
  const bool cauchy = kind == DLG_KIND_CAUCHY_TO_EDGE;
  out7[0] = F.norm2_cauchy; out7[1] = cauchy ? NAN : F.norm2_gn; out7[2] = (double)kind;
  out7[3] = cauchy ? F.norm2_cauchy : (kind == DLG_KIND_GAUSSNEWTON ? F.norm2_gn : b->h_scal[0]);      // (Cauchy: unscaled, dogleg.c:1200)
  out7[4] = cauchy ? NAN : b->h_scal[9];
  out7[5] = b->h_scal[2];
  out7[6] = defer ? NAN : ei_inline(b, b->h_scal[11], ident_used ? ident_nJs : b->h_scal[12], ident_used);
}
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
  DLG_CHECK(dlg_check_slot(b, from)); DLG_CHECK(dlg_check_slot(b, to));
  if(from == to) { dlg_set_error("dlg_take_step: from == to"); return DLG_ERR_ARG; }
  if(!lambda_io || !out7) { dlg_set_error("dlg_take_step: NULL argument"); return DLG_ERR_ARG; }
  DlgSlot& F = b->slot[from];
  DlgSlot& T = b->slot[to];
  if(!F.have_inputs) { dlg_set_error("dlg_take_step: slot %d has no J/JtJ", from); return DLG_ERR_STATE; }
  if(!F.have_Jtx) { dlg_set_error("dlg_take_step needs Jt_x"); return DLG_ERR_STATE; }
  if(!b->d_gnpart) DLG_HIP(hipMalloc(&b->d_gnpart, sizeof(double)*4096));      // |gn|^2 partials, then the pivots' partial minima / maxima (k_negate_interp1)
  double lam = *lambda_io;
  bool ident_launched = false, ident_used = false;
  double ident_nJs = 0.0;
  // (the factorisation and the solve enqueued by dlg_point_eval -- step_prepare -- are this step's if the
  // lambda is the one they were formed at; they are used once)
  const double lam_in = lam;
  if(b->pre_slot == from && b->pre_lambda != lam) b->pre_hint_input = true;      // (the guess was wrong: this caller does not keep lambda)
  const bool prepared_here = b->pre_slot == from && b->pre_lambda == lam;
  bool pre_split = prepared_here && b->pre_split;          // (the prepared factorisation stopped behind its leaf level: the rest is enqueued here)
  if(prepared_here) { b->pre_slot = -1; b->pre_held = -1; b->pre_split = false; if(b->type == DLG_SPARSE) sparse_release_held(b); } else DLG_CHECK(dlg_step_unprepare(b));
  bool prepared = prepared_here;
  b->pre_rejected = false;                     // (a step from a fresh point: the point before it was accepted)
  DLG_CHECK(tail_guard(b));
  b->tail_pending = false;
  BetweenScope between(b);
  // Where p_new goes: a page-locked destination is written by the step's pass over J itself (K8, a slice per workgroup)
  const PDest pd = p_dest(p_new_host);
  const bool p_pinned = pd.pinned && b->copy_stream;
  const bool p_foldable = p_pinned && b->host_finals && !b->sharded() && pd.dev;
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
  for(;;)
  {
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
      bool doomed = false;
      DLG_CHECK(factor_enqueue(b, from, lam, &doomed));
      if(doomed) { DLG_CHECK(lambda_next(&lam)); continue; }
    }
    if(do_cauchy) DLG_CHECK(cauchy_fork_enqueue(b, from, b->d_scal + 4));     // K3 beside K5 (second stream)
    if(!prepared || pre_split) DLG_CHECK(gn_solve_enqueue(b, F));
    prepared = false; pre_split = false;
    DLG_CHECK(cauchy_deferred_finish(b, from));
    int nbg = 0;
    if(!b->ev_fetch) DLG_HIP(hipEventCreateWithFlags(&b->ev_fetch, hipEventDisableTiming));
    StepLaunch L7;
    if(defer)
    {
      // (the last kernel on the main stream: it takes the scalars to the host and carries the event the host waits for)
      L7.nscal = dlg_backend::NSCAL;
      if(b->ext_events && !(b->prof_mask >> DLG_PROF_K7_STEP & 1u)) L7.stop = b->ev_fetch;
    }
    {
      DlgProfScope ps(b, DLG_PROF_K7_STEP);
      DLG_CHECK(k_negate_interp1(b, F.gn, F.cauchy, b->N, b->d_gnpart, &nbg, ident_mm, ident_nmm, ident_stride));      // dogleg.c:862-865, 964-972
      DLG_CHECK(k_take_step(b, F.cauchy, F.gn, b->d_gnpart, nbg, n2c_dev, trustregion, F.p, T.step, T.p, b->N,
                            b->d_scal, b->d_scal + 8, F.Jt_x, b->d_scal + 11, L7,
                            ident_try ? b->d_scal + dlg_backend::GB_SLOT : (double*)nullptr,
                            ident_try ? b->d_scal + dlg_backend::IDENT_SLOT : (double*)nullptr,
                            ident_mm != nullptr, true, dlg_backend::IDENT_RATIO_MAX, F.norm2_jtx, dlg_backend::IDENT_ERR_MAX));
    }
    ident_launched = L7.ident;
    const double* k8_skip = ident_launched ? b->d_scal + dlg_backend::IDENT_SLOT : nullptr;      // (the device's word: the pass over J returns at once)
    bool k8_omitted = false;
    if(defer && !L7.scal_copied)
    {
      // (the step kernel could not take the scalars along -- no room left for its partial sums in page-locked memory --:
      // this step in the in-line form, K8 in front of the synchronisation)
      defer = false;
      p_fold = p_foldable && b->type == DLG_SPARSE;
    }
    if(defer)
    {
      // K8 right behind the step kernel on the same stream -- but the host is already on its way back when it runs: its
      // partial sums and p_new land in page-locked memory, the event rides on the launch (dlg_step_tail waits for it).
      // (On the second stream beside the next evaluation it gained nothing: that evaluation's pass over J is bound by HBM
      // as K8 is -- 131 + 0 us against 98 + 38 -- and the wait for the event between the queues cost 18 us.)
      const bool p_side = p_fold && L7.attached && b->copy_stream;
      // K8's launch gets no event of its own, L8.stop stays null (a launch somebody listens to holds the next dispatch back
      // by ~5 us): the evaluation that follows is waited for on this stream behind it -- dlg_step_tail only waits itself if
      // nothing was (sync_mark).
      StepLaunch L8;
      // p_new: on the copy stream behind the step kernel's own event (the one the host listens to: no event more on the main
      // stream) -- the pass over J, which may return at once (k8_skip), does not have to carry 8 N bytes over PCIe on the
      // critical queue (1.2 MB, ~25 us on config #4); dlg_step_tail / tail_guard wait for the copy
      if(p_side) { DLG_CHECK(p_copy_side(b, to, p_new_host, b->ev_fetch)); b->p_side_pending = true; }
      else if(p_fold) { L8.p_src = T.p; L8.p_dst = pd.dev; }
      b->tail_no_fold = p_side || !p_fold;
      // The pass over J is not even launched where the step kernel is expected to let it return at once -- the last step of
      // this backend did (ident_predict), lambda is 0 again, and the launch would carry nothing else (p_new is on the copy
      // stream): a launch that returns at once is still 5 - 6 us on the critical queue.  The device's word is the judge: if
      // it says the pass is needed after all, it is launched behind the wait (below), late but the same pass.
      k8_omitted = ident_launched && b->ident_predict && b->tail_no_fold && !b->knobs.no_k8_predict;
      L8.skip = k8_skip;
      if(!k8_omitted) DLG_CHECK(take_step_tail_k8(b, from, to, L8));
      b->tail_pending = true;
      DLG_CHECK(step_finish(b, to, dlg_backend::NSCAL, PDest(), L7.attached, true));
      b->tail_mark = b->sync_mark;              // (that wait was for the step kernel, in front of K8)
      b->tail_inner = b->h_scal[11];
    }
    else
    {
      StepLaunch L8;
      bool side_copy = false;
      if(p_fold)
      {
        // page-locked destination: the step's last kernel (K8) writes p_new there itself, a slice per
        // workgroup -- no event between the step kernel and K8 for a copy on the side stream to wait on
        L8.p_src = T.p; L8.p_dst = pd.dev;
      }
      else if(p_pinned)
      {
        DLG_HIP(hipEventRecord(b->ev_step, b->stream));
        DLG_CHECK(p_copy_side(b, to, p_new_host, b->ev_step));
        side_copy = true;
      }
      L8.nscal = dlg_backend::NSCAL;       // (the last kernel of the step: it takes the scalars to the host with it)
      if(b->ext_events && !side_copy && !(b->prof_mask >> DLG_PROF_K3K8_NORM2JV & 1u)) L8.stop = b->ev_fetch;   // ... and the event the host waits for
      L8.skip = k8_skip;
      { DlgProfCond pc(b); DLG_CHECK(norm2_Jv(b, from, T.step, b->d_scal + 12, L8, b->d_scal + 8)); }   // the other half of the expected improvement (returns early behind a failed factorisation unless the step is the Cauchy step)
      DLG_CHECK(step_finish(b, to, dlg_backend::NSCAL, (side_copy || L8.p_copied) ? PDest() : pd, L8.attached, L8.scal_copied));   // the one synchronisation
      if(side_copy) DLG_HIP(hipEventSynchronize(b->ev_copy));
    }
    if(b->profiling) dlg_prof_resolve(b);
    if(!F.have_cauchy) { F.norm2_cauchy = b->h_scal[6]; F.Jg2 = b->h_scal[5]; F.have_cauchy = true; }
    // the step kernel let the pass over J return at once: |J step|^2 from the solved system
    ident_used = ident_launched && b->h_scal[dlg_backend::IDENT_SLOT] != 0.0 && F.Jg2 > 0.0;
    if(ident_launched && !ident_used && b->h_scal[dlg_backend::IDENT_SLOT] != 0.0)
    { dlg_set_error("internal error: the expected improvement's pass over J was skipped without |J Jt_x|^2 at hand"); return DLG_ERR_STATE; }
    if(ident_used)
      ident_nJs = ident_norm2_Jstep((int)b->h_scal[8], b->h_scal[9], trustregion, F.norm2_jtx, F.Jg2, F.norm2_cauchy, b->h_scal[dlg_backend::GB_SLOT],
                                    lam, b->h_scal[10], F.norm2_cauchy - b->h_scal[dlg_backend::IDENT_SLOT + 4]);
    if(defer) { b->tail_ident = ident_used; b->tail_nJs = ident_nJs; }
    if(ident_launched) b->ident_predict = ident_used;
    if(k8_omitted && !ident_used)
    {
      // (the step kernel wants the pass over J after all -- another pivot range than last time: behind the wait, in the
      // tail's own form; dlg_step_tail waits for it)
      StepLaunch L8;
      DLG_CHECK(take_step_tail_k8(b, from, to, L8));
      b->tail_mark = b->sync_mark;
    }
    if((int)b->h_scal[8] == DLG_KIND_CAUCHY_TO_EDGE)
    {
      // The Cauchy step was the one taken: the reference never factorises on this branch
      // (dogleg.c:1192-1211), so the speculative Gauss-Newton work is dropped -- no cached factor,
      // no cached GN step, and above all no change of the (sticky) lambda, whether or not the
      // speculative factorisation succeeded.
      b->factor_slot = -1;
      F.have_gn = false;
      take_step_out7(b, F, defer, ident_used, ident_nJs, out7);
      if(b->profiling) dlg_prof_commit(b, b->type == DLG_SPARSE ? sparse_factor_ok(b) : dense_factor_ok(b));
      return DLG_OK;
    }
    if(factor_verdict(b, from)) break;
    between_drop(b);                                          // (the step is made again: what the caller enqueued behind it is void)
    DLG_CHECK(lambda_next(&lam));
  }
  b->factor_slot = from;
  F.norm2_gn = b->h_scal[10];
  F.have_gn = true;
  *lambda_io = lam;
  b->pre_hint = b->pre_hint_input ? lam_in : lam; b->pre_hint_valid = true;
  take_step_out7(b, F, defer, ident_used, ident_nJs, out7);
  b->pivot_ratio = ident_launched ? b->h_scal[dlg_backend::IDENT_SLOT + 1] : NAN;
  // (a retry from the cached vectors of this point, dlg_step, takes the same route: <Jt x, gn> and the factor's verdict)
  F.g_dot_gn = b->h_scal[dlg_backend::GB_SLOT];
  F.ident_ok = ident_launched && ident_mm != nullptr && b->h_scal[dlg_backend::IDENT_SLOT] == 1.0;      // (the factor's verdict, not the Cauchy step's)
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
  DLG_CHECK(dlg_check_slot(b, from)); DLG_CHECK(dlg_check_slot(b, to));
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
