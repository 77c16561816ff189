// driver.hip -- host trust-region driver behind the dogleg.h API.
//
// Restates the reference's control flow (dogleg.c:1004-1083 computeCallbackOperatingPoint, dogleg.c:1172-1476
// takeStepFrom / evaluateStep_adjustTrustRegion / runOptimizer, dogleg.c:1633-1818 entry points) on the host; all
// vector/matrix arithmetic is delegated to the HIP backend through dlg_backend.h.  Comparison senses, the lambda
// schedule, the un-applied terminal step and the cached-retry behaviour follow SURVEY.md 8a.  What is not in
// dogleg.c lives beside this file: driver_internal.h lists where.
//
// Host memory handed to user callbacks (x, J, Jt arrays) is pinned
// (hipHostMalloc) so the per-evaluation upload is a straight DMA.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include "driver_internal.h"

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

} // namespace

dogleg_parameters2_t g_params = k_defaults;

size_t dense_factor_size(const dogleg_solverContext_t* ctx)
{
  const size_t N = (size_t)ctx->Nstate;
  return (ctx->solve_type == DOGLEG_DENSE || ctx->parameters->JtJ_packed) ? N*(N+1)/2 : N*N;
}

namespace {

// ---- operating points ------------------------------------------------------
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

// dogleg.c:1479-1562, with the callback-visible arrays pinned.  The point is d->pts[s] from its first byte, its
// Gauss-Newton array hangs where free_point looks for it, and pinned_alloc books every pinned buffer as it is made:
// whatever this returns, free_point(d, s) frees all of it.
bool alloc_point(Driver* d, int s)
{
  dogleg_operatingPoint_t* pt = (dogleg_operatingPoint_t*)calloc(1, sizeof(*pt));
  if(!pt) return false;
  d->pts[s] = pt;
  const size_t N = (size_t)d->pub.Nstate, M = (size_t)d->pub.Nmeasurements;
  const dogleg_solve_type_t type = d->pub.solve_type;
  double* gn = (double*)calloc(N, sizeof(double));
  if(type == DOGLEG_SPARSE)
  {
    cholmod_dense* g = &d->gn_dense[s];
    memset(g, 0, sizeof(*g));
    g->nrow = N; g->ncol = 1; g->nzmax = N; g->d = N; g->x = gn;
    g->xtype = CHOLMOD_REAL; g->dtype = CHOLMOD_DOUBLE;
    pt->updateGN_cholmoddense = g;
  }
  else pt->updateGN_dense = gn;
  pt->p            = (double*)pinned_alloc(d, s, sizeof(double)*N);
  pt->Jt_x         = (double*)pinned_alloc(d, s, sizeof(double)*N);
  pt->updateCauchy = (double*)calloc(N, sizeof(double));
  pt->step_to_here = (double*)calloc(N, sizeof(double));
  if(!pt->p || !pt->Jt_x || !pt->updateCauchy || !pt->step_to_here || !gn) return false;
  if(type != DOGLEG_DENSE_PRODUCTS)
  { pt->x = (double*)pinned_alloc(d, s, sizeof(double)*M); if(!pt->x) return false; }
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
      if(!A->p || !A->i || !A->x) return false;
    }
    A->stype = 0; A->itype = CHOLMOD_INT; A->xtype = CHOLMOD_REAL; A->dtype = CHOLMOD_DOUBLE;
    A->sorted = 1; A->packed = 1;
    pt->Jt = A;
  }
  else if(type == DOGLEG_DENSE)
  {
    if(!d->f_device) { pt->J_dense = (double*)pinned_alloc(d, s, sizeof(double)*M*N); if(!pt->J_dense) return false; }
  }
  else
  {
    pt->JtJ = (double*)pinned_alloc(d, s, sizeof(double)*dense_factor_size(&d->pub));
    if(!pt->JtJ) return false;
  }
  return true;
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

// ---- the pattern of a sparse solve -------------------------------------------
// the backend was set up for another pattern of this shape
bool replace_pattern(Driver* d, const int* cp, const int* ri)
{
  return be_ok(dlg_sparse_drop_pattern(d->be), "dropping the previous solve's pattern") &&
         be_ok(dlg_sparse_set_pattern(d->be, cp, ri), "sparse symbolic analysis");
}
// the first evaluation of a sparse solve: the symbolic phase -- unless the backend was taken over from an
// earlier solve and is set up for this very pattern
bool set_pattern(Driver* d, const int* cp, const int* ri)
{
  if(!d->be_reused) return be_ok(dlg_sparse_set_pattern(d->be, cp, ri), "sparse symbolic analysis");
  return dlg_sparse_pattern_matches(d->be, cp, ri) || replace_pattern(d, cp, ri);
}

// Device callback, a backend taken over from the previous solve: whether its pattern is the caller's is 64 MB of comparison
// on config #4 (1 ms of a 5 ms solve).  It runs on a thread of its own beside the first evaluation, which is made with the
// backend's schedules -- if the patterns turn out to differ, that evaluation is thrown away: the callback's x and J stay
// where they are, the pattern is analysed and bind_and_evaluate runs again.  (Same shape, so every index the stale
// schedules hold is inside the arrays.)  Not on a rank of several: there the first evaluation gathers the rank's rows or
// binds a row slice and keeps the step's tail in line, which the second call would have to repeat exactly.
bool start_pattern_check(Driver* d)
{
  // (a bounded solve masks J behind the first evaluation: that evaluation must be THE evaluation, the comparison comes first)
  if(d->sharded || !d->be_reused || d->check_pattern || d->bounds || getenv("DOGLEG_AMD_NO_PATTERN_OVERLAP") != nullptr) return false;
  dlg_backend_t* be = d->be; const int* cp = d->dev_cp; const int* ri = d->dev_ri;
  // (a thread that cannot be started throws: then the comparison is made in line, as without the overlap)
  try { d->pat_check = new std::future<int>(std::async(std::launch::async, [be, cp, ri] { return dlg_sparse_pattern_matches(be, cp, ri); })); }
  catch(...) { d->pat_check = nullptr; }
  return d->pat_check != nullptr;
}
bool finish_pattern_check(Driver* d)
{
  Tick tk(d, TM_PATTERN);
  const int same = d->pat_check->get();
  delete d->pat_check; d->pat_check = nullptr;
  return same != 0;
}
bool device_pattern(Driver* d)
{
  if(d->pub.solve_type != DOGLEG_SPARSE || d->pattern_set) return true;
  Tick tk(d, TM_PATTERN);
  if(!start_pattern_check(d) && !set_pattern(d, d->dev_cp, d->dev_ri)) return false;
  d->pattern_set = true;
  return true;
}
// host callback: the pattern is what the first evaluation wrote into Jt->p / Jt->i
bool host_pattern(Driver* d, const int* cp, const int* ri)
{
  const size_t np = sizeof(int)*((size_t)d->pub.Nmeasurements + 1), ni = sizeof(int)*(size_t)d->nnz;
  if(!d->pattern_set)
  {
    Tick tk(d, TM_PATTERN);
    if(!set_pattern(d, cp, ri)) return false;
    d->pattern_set = true;
    if(d->check_pattern)
    {
      d->pat_p = (int*)malloc(np);
      d->pat_i = (int*)malloc(ni);
      memcpy(d->pat_p, cp, np);
      memcpy(d->pat_i, ri, ni);
    }
  }
  else if(d->check_pattern && (memcmp(d->pat_p, cp, np) || memcmp(d->pat_i, ri, ni)))
  { MSG("the sparsity pattern of Jt changed between evaluations; it must stay fixed (reference dogleg.c:648-649)"); return false; }
  return true;
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

// ---- one evaluation (dogleg.c:1004-1083): feed_* runs the model and hands x / J to the backend, evaluate_fed is
// dogleg.c:1024-1071 on the device ---------------------------------------------------------------------------------
int evaluate_fed(Driver* d, int s, double* norm2x, double* absmax)
{
  const dogleg_solve_type_t type = d->pub.solve_type;
  // once steps need the Gauss-Newton step an accepted point is factorised next: its JtJ is assembled
  // beside Jt*x (an unused assembly -- a rejected point -- is simply dropped; no number changes)
  // (a bounded solve: never -- an assembly at evaluation time would be one of the unmasked J)
  if(type == DOGLEG_SPARSE) dlg_backend_set_speculation(d->be, d->expect_gn && !d->bounds);
  // the model lives on the device: nothing on the host waits for p_new, and the expected improvement of a step is needed as
  // rho's denominator behind the evaluation of its trial point (dogleg.c:1410-1427; the `< 0` stop of 1403-1408 is made
  // there too, run_optimizer) -- its pass over J, if it needs one, runs beside this evaluation
  // (a bounded solve clips the step behind it and forms the value again: nothing is deferred)
  if(d->f_device && type != DOGLEG_DENSE_PRODUCTS && !d->sharded && !d->bounds) dlg_backend_set_defer_tail(d->be, 1);
  Tick te(d, TM_EVAL);
  return dlg_point_eval(d->be, s, norm2x, absmax);
}

// dogleg.c:1016-1022 with the model on the device: the callback writes x and the Jacobian values straight into the
// slot's HBM buffers, ordered on the backend's stream
struct DevicePoint { const double* p; double *x, *J; };
DevicePoint device_point(Driver* d, int s)
{
  return { (const double*)dlg_point_device_ptr(d->be, s, DLG_VEC_P), (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_X_OWN),
           (double*)dlg_point_device_ptr(d->be, s, DLG_VEC_J_OWN) };
}
// (a solve with a loss: the prelude -- weights, F, x and J times sqrt(w) -- goes onto the stream directly behind the callback's
// kernels, in front of whatever reads x and J of slot s; robust_prelude.hip)
void device_callback(Driver* d, int s, const double* p, double* x, double* J)
{
  Tick tk(d, TM_CALLBACK);
  (*d->f_device)(p, x, J, dlg_backend_get_stream(d->be), d->pub.cookie);
  if(d->robust) robust_enqueue(d, s, x, J);
}
// the backend takes the slot's own buffers as they are (dense on a rank: its rows, a contiguous slice of them)
bool bind_and_evaluate(Driver* d, int s, const DevicePoint& v, double* norm2x, double* absmax, int* rc_eval)
{
  const size_t r0 = d->sharded ? (size_t)d->row0 : 0;
  { Tick tu(d, TM_UPLOAD); if(!be_ok(dlg_point_bind_device(d->be, s, v.x + r0, v.J + r0*(size_t)d->pub.Nstate), "bind")) return false; }
  *rc_eval = evaluate_fed(d, s, norm2x, absmax);
  return true;
}
// sparse on a rank: the callback evaluates ALL rows (its contract does not know about ranks) into buffers of the full
// size, the rank's rows are gathered on the device
bool feed_device_rank_rows(Driver* d, int s, const DevicePoint& v)
{
  if(!d->x_full_dev)
  {
    d->x_full_dev = (double*)dlg_mem_alloc(sizeof(double)*(size_t)d->pub.Nmeasurements);
    d->J_full_dev = (double*)dlg_mem_alloc(sizeof(double)*(size_t)d->nnz);
    if(!d->x_full_dev || !d->J_full_dev) { MSG("out of device memory"); return false; }
  }
  device_callback(d, s, v.p, d->x_full_dev, d->J_full_dev);
  Tick tu(d, TM_UPLOAD);
  return be_ok(dlg_point_gather_device(d->be, s, d->x_full_dev, d->J_full_dev, d->dev_cp), "gather of the rank's rows");
}
bool eval_device(Driver* d, int s, double* norm2x, double* absmax, int* rc_eval)
{
  if(!device_pattern(d) || !rank_rows(d, d->dev_cp)) return false;
  const DevicePoint v = device_point(d, s);
  if(d->sharded && d->pub.solve_type == DOGLEG_SPARSE)
  {
    if(!feed_device_rank_rows(d, s, v)) return false;
    *rc_eval = evaluate_fed(d, s, norm2x, absmax);
    return true;
  }
  // (the callback of this point may have run already -- between_fn, from inside the step that made the point; a step
  // that was made again behind it moved the point: then it runs again)
  const bool early_cb = d->early_slot == s && !dlg_backend_between_redone(d->be);
  d->early_slot = -1;
  if(!early_cb) device_callback(d, s, v.p, v.x, v.J);
  if(!bind_and_evaluate(d, s, v, norm2x, absmax, rc_eval)) return false;
  if(d->pat_check && !finish_pattern_check(d))
  {
    // another pattern of the same shape: what was just evaluated is void
    { Tick tk(d, TM_PATTERN); if(!replace_pattern(d, d->dev_cp, d->dev_ri)) return false; }
    return bind_and_evaluate(d, s, v, norm2x, absmax, rc_eval);
  }
  return true;
}

bool feed_sparse(dogleg_operatingPoint_t* pt, Driver* d, int s)
{
  dogleg_solverContext_t* ctx = &d->pub;
  { Tick tk(d, TM_CALLBACK); (*ctx->f)(pt->p, pt->x, pt->Jt, ctx->cookie); }
  const int* cp = (const int*)pt->Jt->p; const int* ri = (const int*)pt->Jt->i;
  if(!host_pattern(d, cp, ri) || !rank_rows(d, cp)) return false;
  const double *x = pt->x, *Jv = (const double*)pt->Jt->x;
  if(d->sharded)
  {
    // one rank of several: the callback evaluated all rows (its contract does not know about ranks); the
    // rank's rows -- those the subtree partition gave it, in that order -- go to the device
    size_t q = 0;
    for(int i = 0; i < d->part_nrows; i++)
    {
      const int r = d->part_rows[i];
      d->x_loc[i] = pt->x[r];
      const size_t n = (size_t)(cp[r+1] - cp[r]);
      memcpy(d->J_loc + q, Jv + cp[r], sizeof(double)*n);
      q += n;
    }
    x = d->x_loc; Jv = d->J_loc;
  }
  Tick tu(d, TM_UPLOAD);
  return be_ok(dlg_point_upload(d->be, s, x, Jv), "upload");
}
bool feed_dense(dogleg_operatingPoint_t* pt, Driver* d, int s)
{
  dogleg_solverContext_t* ctx = &d->pub;
  { Tick tk(d, TM_CALLBACK); (*ctx->f_dense)(pt->p, pt->x, pt->J_dense, ctx->cookie); }
  // (a rank of several: its contiguous rows of what the callback wrote)
  const size_t r0 = d->sharded ? (size_t)d->row0 : 0;
  Tick tu(d, TM_UPLOAD);
  return be_ok(dlg_point_upload(d->be, s, pt->x + r0, pt->J_dense + r0*(size_t)ctx->Nstate), "upload");
}
bool feed_products(dogleg_operatingPoint_t* pt, Driver* d, int s)
{
  dogleg_solverContext_t* ctx = &d->pub;
  { Tick tk(d, TM_CALLBACK); (*ctx->f_dense_products)(pt->p, &pt->norm2_x, pt->Jt_x, pt->JtJ, ctx->cookie); }
  Tick tu(d, TM_UPLOAD);
  return be_ok(dlg_point_upload_products(d->be, s, pt->norm2_x, pt->Jt_x, pt->JtJ), "upload");
}

// dogleg.c:1004-1083
bool eval_point(bool* converged, dogleg_operatingPoint_t* pt, Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  const int s = slot_of(d, pt);
  const bool products = ctx->solve_type == DOGLEG_DENSE_PRODUCTS;
  pt->norm2_x = -1.;
  memset(pt->dummy_bits, 0, sizeof(pt->dummy_bits));
  d->ncallbacks++;
  double norm2x = 0, absmax = 0;
  int rc_eval;
  if(d->f_device) { if(!eval_device(d, s, &norm2x, &absmax, &rc_eval)) return false; }
  else
  {
    if(!(ctx->solve_type == DOGLEG_SPARSE ? feed_sparse(pt, d, s) : products ? feed_products(pt, d, s) : feed_dense(pt, d, s))) return false;
    rc_eval = evaluate_fed(d, s, &norm2x, &absmax);
  }
  if(!be_ok(rc_eval, products ? "gradient norm" : "Jt*x")) return false;
  pt->have_Jtx = true;
  if(products) pt->have_JtJ = true;                 // (norm2_x is the callback's)
  else { pt->norm2_x = norm2x; pt->have_x = pt->have_J = true; }
  // (a loss: the backend summed the squares of the weighted x; the gain ratio, the records and the return value take F)
  if(d->robust && !robust_F(d, s, &pt->norm2_x)) return false;
  // (bounds: the held set of this invocation of the callback, g_F for Jt x, zeros in the held columns of J; the test below is on |g_F|_inf)
  // (a gradient that is not finite stops the solve as it stops the plain one: the unmasked value stands)
  if(d->bounds)
  {
    double absmax_F = 0;
    if(!bounds_hold_mask(d, s, &absmax_F)) return false;
    if(std::isfinite(absmax)) absmax = absmax_F;
  }
  // dogleg.c:1073-1082: converged unless some |Jt_x[i]| exceeds the threshold
  *converged = !(absmax > ctx->parameters->Jt_x_threshold);
  if(*converged) VERBOSE(d, "gradient below threshold everywhere: done");
  return true;
}

// ---- what a step needs of the point it leaves ---------------------------------
bool need_Jtx(const dogleg_operatingPoint_t* pt, const char* what)
{
  if(pt->have_Jtx) return true;
  MSG("%s needs Jt_x, which is missing", what);
  return false;
}
bool need_J(const dogleg_operatingPoint_t* pt, const dogleg_solverContext_t* ctx)
{
  if(ctx->solve_type == DOGLEG_DENSE_PRODUCTS ? pt->have_JtJ : pt->have_J) return true;
  MSG("factorization needs J (or JtJ), which is missing");
  return false;
}

// dogleg.c:529-617
bool compute_cauchy(dogleg_operatingPoint_t* pt, Driver* d)
{
  if(!pt->have_updateCauchy)
  {
    if(!need_Jtx(pt, "Cauchy step")) return false;
    double n2 = 0;
    if(!be_ok(dlg_cauchy(d->be, slot_of(d, pt), &n2), "Cauchy step")) return false;
    pt->norm2_updateCauchy = n2;
    pt->have_updateCauchy = true;
    VERBOSE(d, "cauchy step length %.6g", sqrt(n2));
  }
  d->cur.norm2_cauchy = pt->norm2_updateCauchy;
  return true;
}

// The backend holds the factor of JtJ + lambda I at pt.  ctx->factorization of a sparse solve (dogleg.h:185-190; the
// reference gets it from cholmod_analyze, dogleg.c:650-654): an opaque, zero-filled cholmod_factor of which only the
// public fields n and minor are maintained (minor == n <=> the last factorisation succeeded, dogleg.c:667).
// The factor itself lives on the device; dogleg_amd_backend(ctx) + dlg_solve_with_factor use it.
bool factor_held(dogleg_operatingPoint_t* pt, Driver* d, double lambda_before)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(ctx->lambda != lambda_before) VERBOSE(d, "singular JtJ: adding %g I from now on", ctx->lambda);
  if(ctx->solve_type == DOGLEG_SPARSE)
  {
    if(!d->factor_handle) d->factor_handle = (cholmod_factor*)calloc(1, sizeof(cholmod_factor));
    if(!d->factor_handle) { MSG("out of memory"); return false; }
    d->factor_handle->n = d->factor_handle->minor = (size_t)ctx->Nstate;
    ctx->factorization = d->factor_handle;
  }
  pt->have_factorization = true;
  return true;
}

bool factorize(dogleg_operatingPoint_t* pt, Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(pt->have_factorization) return true;                      // dogleg.c:637
  if(!need_J(pt, ctx)) return false;
  while(true)
  {
    int ok = 0;
    if(!be_ok(dlg_factorize(d->be, slot_of(d, pt), ctx->lambda, &ok), "factorization")) return false;
    if(ok) break;
    ctx->lambda = (ctx->lambda == 0.0) ? LAMBDA_INITIAL : ctx->lambda*10.0;   // dogleg.c:671-672, 812-813
    if(!std::isfinite(ctx->lambda)) { MSG("lambda overflowed while regularising a singular JtJ"); return false; }
    VERBOSE(d, "singular JtJ: adding %g I from now on", ctx->lambda);          // (one line per attempt: the loop is here)
  }
  return factor_held(pt, d, ctx->lambda);
}

// dogleg.c:822-908
bool compute_gn(dogleg_operatingPoint_t* pt, Driver* d)
{
  if(!pt->have_updateGN)
  {
    if(!need_Jtx(pt, "GN step")) return false;
    double n2 = 0;
    if(!pt->have_factorization)
    {
      // factorisation (with the lambda loop, dogleg.c:656-677 / 806-815) and solve in one backend op:
      // one host synchronisation per attempt
      dogleg_solverContext_t* ctx = &d->pub;
      if(!need_J(pt, ctx)) return false;
      const double lambda_before = ctx->lambda;
      if(!be_ok(dlg_gauss_newton(d->be, slot_of(d, pt), &ctx->lambda, &n2), "factorization + GN solve")) return false;
      if(!factor_held(pt, d, lambda_before)) return false;
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
  const DevicePoint v = device_point(d, s);
  device_callback(d, s, v.p, v.x, v.J);
  d->early_slot = s;
  if(d->pub.solve_type == DOGLEG_SPARSE)
  {
    int done = 0;
    dlg_backend_set_speculation(d->be, d->expect_gn);
    (void)dlg_point_eval_early(d->be, s, v.x, v.J, &done);
  }
}
bool between_ok(const Driver* d)
{
  return d->f_device && !d->sharded && !d->no_between && !d->bounds && !d->pat_check &&
         (d->pub.solve_type == DOGLEG_DENSE || (d->pub.solve_type == DOGLEG_SPARSE && d->pattern_set));
}

// dogleg.c:1186-1211: the Cauchy step, and the Gauss-Newton step only if the Cauchy step ends inside the trust region
bool choose_step(int* kind, dogleg_operatingPoint_t* from, double trustregion, Driver* d)
{
  if(!compute_cauchy(from, d)) return false;
  if(from->norm2_updateCauchy >= trustregion*trustregion) { *kind = DLG_KIND_CAUCHY_TO_EDGE; return true; }
  if(!compute_gn(from, d)) return false;
  *kind = from->norm2_updateGN <= trustregion*trustregion ? DLG_KIND_GAUSSNEWTON : DLG_KIND_INTERPOLATED;
  return true;
}
// what a step of this kind says about the point it leaves, in the trial record, and to the next evaluation and step
void record_kind(int kind, dogleg_operatingPoint_t* from, Driver* d)
{
  d->cur.step_type = kind == DLG_KIND_CAUCHY_TO_EDGE ? DLG_STEP_CAUCHY : kind == DLG_KIND_GAUSSNEWTON ? DLG_STEP_GAUSSNEWTON : DLG_STEP_INTERPOLATED;
  from->didStepToEdgeOfTrustRegion = kind != DLG_KIND_GAUSSNEWTON;
  d->expect_gn = kind != DLG_KIND_CAUCHY_TO_EDGE;
}
// the expected improvement of the step just taken, where the backend was told to bring it later
// (dlg_backend_set_defer_tail) and it is still on its way
bool fetch_deferred_improvement(double* expectedImprovement, Driver* d)
{
  if(!d->tail_out) return true;
  d->tail_out = false;
  if(!be_ok(dlg_step_tail(d->be, expectedImprovement), "expected improvement")) return false;
  d->cur.expected_improvement = *expectedImprovement;
  return true;
}

// Steps 5 and 6 of the bounded solve (dogleg.h, above dogleg_amd_optimize_dense_batch_bounded) behind the step dlg_step made:
// clip it into the box and, if something was clamped, form the expected improvement again with the pass over J (the value from
// the solved system holds for combinations of the Cauchy and the Gauss-Newton step only); a clipped step the model does not
// like, or one below update_threshold, gives way to the Cauchy step cut at the first bound, which is recorded as a Cauchy step.
bool bounded_step(double* expectedImprovement, double* n2, double* k, double* amax, dogleg_operatingPoint_t* to, dogleg_operatingPoint_t* from,
                  double trustregion, Driver* d)
{
  const int sf = slot_of(d, from), st = slot_of(d, to);
  bounds_note_step(d, sf);
  double clamped = 0, smax = 0, s2 = 0;
  if(!bounds_clip(d, sf, st, &clamped, &smax, &s2)) return false;
  if(!(clamped > 0.0)) return true;                 // (nothing differs from the plain solve)
  VERBOSE(d, "%g components of the step clamped at their bounds", clamped);
  if(!be_ok(dlg_expected_improvement(d->be, sf, st, expectedImprovement), "expected improvement of the clipped step")) return false;
  if(*expectedImprovement <= 0.0 || smax <= d->pub.parameters->update_threshold)
  {
    const double t0 = fmin(1.0, trustregion/sqrt(from->norm2_updateCauchy));
    if(!bounds_fallback(d, sf, st, t0, &smax, &s2)) return false;
    if(!be_ok(dlg_expected_improvement(d->be, sf, st, expectedImprovement), "expected improvement of the fallback step")) return false;
    if(!(*expectedImprovement > 0.0) || !std::isfinite(*expectedImprovement))
    { MSG("the Cauchy step cut at the first bound has expected improvement %g", *expectedImprovement); return false; }
    VERBOSE(d, "fallback: the Cauchy step cut at the first bound");
    d->cur.step_type = DLG_STEP_CAUCHY; *k = NAN;
    from->didStepToEdgeOfTrustRegion = from->norm2_updateCauchy >= trustregion*trustregion;
  }
  *n2 = s2; *amax = smax;
  return be_ok(dlg_point_download(d->be, st, DLG_VEC_P, to->p, (size_t)d->pub.Nstate), "download of the clipped p");
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
  // inside the trust region (choose_step).  Once a step has needed both, the whole of
  // takeStepFrom for a fresh point -- both steps, the choice between them (same comparisons, made
  // on the device), the step, its expected improvement, p_new -- is ONE backend op behind one host
  // synchronisation; the values are the same, and a Gauss-Newton step the reference would not have
  // computed is discarded by the backend: neither cached nor reported, and lambda keeps its value.
  // Otherwise the step, its expected improvement and p_new are one backend op behind the steps it is made of.
  int kind = -1;
  double n2 = 0, k = NAN, amax = 0, o[7];
  // (a bounded solve: the fused step acts on the unclipped p_new and takes its expected improvement from the solved system -- never)
  const bool fused = !d->bounds && d->expect_gn && !from->have_updateCauchy && !from->have_updateGN && !from->have_factorization;
  if(fused) { if(!need_Jtx(from, "Cauchy step") || !need_J(from, ctx)) return false; }
  else
  {
    if(!choose_step(&kind, from, trustregion, d)) return false;
    record_kind(kind, from, d);
  }
  const double lambda_before = ctx->lambda;
  BetweenArgs ba{d, st};
  if(between_ok(d)) dlg_backend_set_between(d->be, driver_between, &ba);
  if(!be_ok(fused ? dlg_take_step(d->be, sf, st, trustregion, &ctx->lambda, o, to->p)
                  : dlg_step(d->be, sf, st, kind, trustregion, &n2, &k, &amax, expectedImprovement, to->p), "step")) return false;
  d->tail_out = dlg_step_tail_pending(d->be) != 0;          // (dlg_backend_set_defer_tail: run_optimizer fetches it behind the evaluation)
  if(fused)
  {
    kind = (int)o[2]; n2 = o[3]; k = o[4]; amax = o[5]; *expectedImprovement = o[6];
    // (on the Cauchy branch the backend dropped its speculative factor and GN step and left
    // lambda alone: dogleg.c:1192-1211 never gets to compute_updateGN)
    if(kind != DLG_KIND_CAUCHY_TO_EDGE && !factor_held(from, d, lambda_before)) return false;
    from->norm2_updateCauchy = o[0]; from->have_updateCauchy = true;
    d->cur.norm2_cauchy = o[0];
    VERBOSE(d, "cauchy step length %.6g", sqrt(o[0]));
    if(kind != DLG_KIND_CAUCHY_TO_EDGE)
    {
      from->norm2_updateGN = o[1]; from->have_updateGN = true;
      d->cur.norm2_gn = o[1]; VERBOSE(d, "gn step length %.6g", sqrt(o[1]));
    }
    record_kind(kind, from, d);
  }
  if(d->bounds && !bounded_step(expectedImprovement, &n2, &k, &amax, to, from, trustregion, d)) return false;
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
    // (no evaluation follows: the record of the terminal step still carries the computed value)
    if(!fetch_deferred_improvement(expectedImprovement, d)) return false;
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
        { Tick tt(d, TM_STEP); if(!fetch_deferred_improvement(&expectedImprovement, d)) return -1; }
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

// frees whatever of a Driver there is: one whose set-up stopped anywhere (no backend yet, no or half a point), one
// whose solve failed, one handed back by dogleg_freeContext
void destroy(Driver* d)
{
  if(!d) return;
  if(d->pat_check) { (void)d->pat_check->get(); delete d->pat_check; d->pat_check = nullptr; }      // (it reads the backend's pattern)
  free_point(d, 0); free_point(d, 1);
  robust_destroy(d);
  bounds_destroy(d);
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

// ---- one solve (dogleg.c:1633-1753) ---------------------------------------------
// DOGLEG_AMD_TIMING=1: wall time of the phases of a solve on stderr (where an end-to-end call spends its time)
struct Laps
{
  bool on; std::chrono::steady_clock::time_point last;
  void operator()(const char* what)
  {
    if(!on) return;
    const auto now = std::chrono::steady_clock::now();
    MSG("timing: %-34s %8.2f ms", what, std::chrono::duration<double, std::milli>(now - last).count());
    last = now;
  }
};

struct Callbacks
{
  dogleg_callback_t* f; dogleg_callback_dense_t* f_dense; dogleg_callback_dense_products_t* f_products;
  dogleg_callback_device_t* f_device; const int *dev_cp, *dev_ri;
};

// which of the solve types the caller's callback selects, and whether NJnnz goes with it
bool classify_callbacks(Driver* d, const Callbacks& cb)
{
  dogleg_solverContext_t* ctx = &d->pub;
  const unsigned int NJnnz = d->nnz, Nmeas = (unsigned int)ctx->Nmeasurements;
  if(cb.f_device)
  {
    // ctx->f stays NULL: the device callback has another signature and lives in the driver
    d->f_device = cb.f_device; d->dev_cp = cb.dev_cp; d->dev_ri = cb.dev_ri;
    ctx->solve_type = NJnnz > 0 ? DOGLEG_SPARSE : DOGLEG_DENSE;
    if(NJnnz == 0) return true;
    if(!cb.dev_cp || !cb.dev_ri) { MSG("a sparse device solve needs the pattern of Jt"); return false; }
    if(cb.dev_cp[0] != 0 || cb.dev_cp[Nmeas] != (int)NJnnz)
    { MSG("the pattern has %d entries, NJnnz says %u", cb.dev_cp[Nmeas], NJnnz); return false; }
    return true;
  }
  if(cb.f)
  {
    ctx->solve_type = DOGLEG_SPARSE; ctx->f = cb.f;
    if(NJnnz == 0) { MSG("sparse solves need NJnnz > 0"); return false; }
    return true;
  }
  if(!cb.f_dense && !cb.f_products) { MSG("exactly one of the callbacks must be given"); return false; }
  if(cb.f_dense) { ctx->solve_type = DOGLEG_DENSE; ctx->f_dense = cb.f_dense; }
  else           { ctx->solve_type = DOGLEG_DENSE_PRODUCTS; ctx->f_dense_products = cb.f_products; }
  if(NJnnz > 0) { MSG("dense solves need NJnnz == 0"); return false; }
  return true;
}

// the idle backend of the previous solve if it is of this shape (never for a rank of several), else a new one
bool obtain_backend(Driver* d, const Comm& cm, Laps& lap)
{
  const dogleg_solverContext_t* ctx = &d->pub;
  const int type = (int)ctx->solve_type, N = ctx->Nstate, M = ctx->Nmeasurements, nnz = (int)d->nnz;
  d->be_flags = (ctx->parameters->JtJ_packed ? DLG_FLAG_JTJ_PACKED : 0) | (ctx->parameters->JtJ_upper ? DLG_FLAG_JTJ_UPPER : 0);
  if(cache_on() && !cm.set) d->be = take_parked(type, N, M, nnz, d->be_flags, cm.device);
  if(d->be) { d->be_reused = true; lap("backend taken over from the previous solve"); return true; }
  if(dlg_backend_create(&d->be, type, N, M, nnz, d->be_flags, cm.device) != DLG_OK)
  { MSG("cannot create the GPU backend: %s", dlg_last_error()); return false; }
  lap("backend create (device buffers)");
  return true;
}

// dogleg.c:1694-1729: the two operating points and the host mirror of a dense factor; p0 goes to the device
bool allocate_points(Driver* d, const double* p)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(ctx->solve_type != DOGLEG_SPARSE)
  {
    ctx->factorization_dense = (double*)calloc(dense_factor_size(ctx), sizeof(double));          // dogleg.c:1707-1725
    if(!ctx->factorization_dense) { MSG("out of memory"); return false; }
  }
  const bool ok0 = alloc_point(d, 0), ok1 = alloc_point(d, 1);
  if(!ok0 || !ok1) { MSG("out of (pinned) host memory"); return false; }
  ctx->beforeStep = d->pts[0];
  ctx->afterStep  = d->pts[1];
  return true;
}

bool set_up(Driver* d, const Callbacks& cb, const double* p, Laps& lap)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(!classify_callbacks(d, cb)) return false;
  if(ctx->parameters->debug_vnlog) vnlog_legend();
  d->timing = lap.on;
  lap.last = std::chrono::steady_clock::now();
  Comm cm;
  if(!solve_communicator(&cm) || !obtain_backend(d, cm, lap) || !attach_communicator(d, cm)) return false;
  if(d->sharded) lap("communicator");
  if(d->robust && !robust_set_up(d)) return false;
  if(d->bounds && !bounds_set_up(d)) return false;
  if(!allocate_points(d, p)) return false;
  lap("operating points (pinned host)");
  memcpy(ctx->beforeStep->p, p, sizeof(double)*(size_t)ctx->Nstate);
  if(d->bounds) bounds_clamp_start(d, ctx->beforeStep->p);
  return be_ok(dlg_point_set_p(d->be, 0, ctx->beforeStep->p), "upload of p");
}

bool run(Driver* d, double* p, double* weights, Laps& lap)
{
  dogleg_solverContext_t* ctx = &d->pub;
  trace_begin(ctx->Nstate);
  const auto t_run = std::chrono::steady_clock::now();
  const int numsteps = run_optimizer(d);
  if(d->timing) timing_report(d, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_run).count());
  lap("run_optimizer (incl. symbolic phase)");
  trace_end(d);
  if(numsteps < 0) { MSG("the solve failed"); d->failed = true; return false; }
  // (the held set first: a download that fails leaves the weights alone too)
  if(d->bounds && !bounds_finish(d, slot_of(d, ctx->beforeStep))) { d->failed = true; return false; }
  if(d->robust && !robust_weights(d, slot_of(d, ctx->beforeStep), weights)) { d->failed = true; return false; }
  memcpy(p, ctx->beforeStep->p, sizeof(double)*(size_t)ctx->Nstate);        // dogleg.c:1745
  VERBOSE(d, "success: %d iterations", numsteps);
  return true;
}

// a context that outlives the call: its arrays are its own, the host mirrors of its point are up to date
bool hand_back(Driver* d)
{
  dogleg_solverContext_t* ctx = &d->pub;
  if(d->f_device && ctx->solve_type == DOGLEG_SPARSE && !own_pattern_copies(d)) { MSG("out of memory"); return false; }
  sync_point_to_host(d, ctx->beforeStep);
  if(ctx->solve_type != DOGLEG_SPARSE && ctx->beforeStep->have_factorization)
    dlg_factor_download_dense(d->be, ctx->factorization_dense, dense_factor_size(ctx));
  return true;
}

// dogleg.c:1633-1753
double optimize(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz, const Callbacks& cb, void* cookie,
                const dogleg_parameters2_t* parameters, dogleg_solverContext_t** returnContext,
                const dogleg_amd_batch_loss_t* loss = nullptr, double* weights = nullptr,
                const dogleg_amd_batch_bounds_t* bounds = nullptr)
{
  Driver* d = (Driver*)calloc(1, sizeof(Driver));
  if(!d) { MSG("out of memory"); return -1.0; }
  if(loss && !(d->robust = robust_create(loss))) { MSG("out of memory"); free(d); return -1.0; }
  if(bounds && !(d->bounds = bounds_create(bounds))) { MSG("out of memory"); robust_destroy(d); free(d); return -1.0; }
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

  Laps lap{getenv("DOGLEG_AMD_TIMING") != nullptr, {}};
  const bool ok = set_up(d, cb, p, lap) && run(d, p, weights, lap) && (!returnContext || hand_back(d));
  const double norm2_x = ok ? ctx->beforeStep->norm2_x : -1.0;
  if(ok && returnContext) *returnContext = ctx;
  else destroy(d);                                     // the one exit of every failure, and of a solve whose context nobody wants
  if(ok) lap("teardown");
  return norm2_x;
}

} // namespace

// ============================================================ public API ====
extern "C" {

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
  return optimize(p, Nstate, Nmeas, NJnnz, Callbacks{f, nullptr, nullptr, nullptr, nullptr, nullptr}, cookie, parameters, returnContext);
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
  return optimize(p, Nstate, Nmeas, 0, Callbacks{nullptr, f, nullptr, nullptr, nullptr, nullptr}, cookie, parameters, returnContext);
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
  return optimize(p, Nstate, Nmeas, NJnnz, Callbacks{nullptr, nullptr, nullptr, f, Jt_colptr, Jt_rowidx}, cookie, parameters, returnContext);
}
// dogleg.h, "robust loss functions in dogleg_optimize_device2": refused here, before any device work, is what needs no device
double dogleg_amd_optimize_device2_robust(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                                          const int* Jt_colptr, const int* Jt_rowidx,
                                          dogleg_callback_device_t* f, void* cookie,
                                          const dogleg_amd_batch_loss_t* loss, double* weights,
                                          const dogleg_parameters2_t* parameters,
                                          dogleg_solverContext_t** returnContext)
{
  if(!f) { MSG("dogleg_amd_optimize_device2_robust needs a device callback"); return -1.0; }
  if(!p || Nstate == 0) { MSG("dogleg_amd_optimize_device2_robust: a NULL p or no variables"); return -1.0; }
  if(!robust_loss_ok(loss, Nmeas, NJnnz, Jt_colptr) || !one_rank_only("dogleg_amd_optimize_device2_robust")) return -1.0;
  return optimize(p, Nstate, Nmeas, NJnnz, Callbacks{nullptr, nullptr, nullptr, f, Jt_colptr, Jt_rowidx}, cookie, parameters, returnContext,
                  loss, weights);
}
// dogleg.h, "box bounds in dogleg_optimize_device2": refused here, before any device work, is what needs no device
double dogleg_amd_optimize_device2_bounded(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                                           const int* Jt_colptr, const int* Jt_rowidx,
                                           dogleg_callback_device_t* f, void* cookie,
                                           const dogleg_amd_batch_loss_t* loss, double* weights,
                                           const dogleg_amd_batch_bounds_t* bounds,
                                           const dogleg_parameters2_t* parameters,
                                           dogleg_solverContext_t** returnContext)
{
  const char* who = "dogleg_amd_optimize_device2_bounded";
  if(!f) { MSG("%s needs a device callback", who); return -1.0; }
  if(!bounds_args_ok(bounds, loss, weights, p, Nstate)) return -1.0;
  if(loss && !robust_loss_ok(loss, Nmeas, NJnnz, Jt_colptr)) return -1.0;
  if(!one_rank_only(who)) return -1.0;
  return optimize(p, Nstate, Nmeas, NJnnz, Callbacks{nullptr, nullptr, nullptr, f, Jt_colptr, Jt_rowidx}, cookie, parameters, returnContext,
                  loss, weights, bounds);
}
double dogleg_optimize_dense_products(double* p, unsigned int Nstate,
                                      dogleg_callback_dense_products_t* f, void* cookie,
                                      const dogleg_parameters2_t* parameters,
                                      dogleg_solverContext_t** returnContext)
{
  return optimize(p, Nstate, 0, 0, Callbacks{nullptr, nullptr, f, nullptr, nullptr, nullptr}, cookie, parameters, returnContext);
}

// dogleg.h:304-310: make sure the factor of JtJ at `point` is held
bool dogleg_computeJtJfactorization(dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx)
{
  Driver* d = D(ctx);
  if(!factorize(point, d)) return false;
  return ctx->solve_type == DOGLEG_SPARSE ||
         dlg_factor_download_dense(d->be, ctx->factorization_dense, dense_factor_size(ctx)) == DLG_OK;
}

void dogleg_freeContext(dogleg_solverContext_t** ctx)
{
  if(!ctx || !*ctx) return;
  destroy(D(*ctx));
  *ctx = nullptr;
}

} // extern "C"
