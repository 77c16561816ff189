// api_extensions.cpp -- the entry points of dogleg.h that never enter the trust-region loop: they check their
// arguments and forward to the backend (outliers, covariance: the factor held for a context's point) or to a solver of
// their own (dense_batch.hip, gradcheck.hip).  No HIP call.
#include <cmath>
#include <cstdlib>
#include <vector>
#include "driver_internal.h"
#include "dense_batch.h"
#include "gradcheck.h"
#include "gradcheck_plan.h"
#include "../../include/dogleg_batch_models.h"

namespace {

// ---- outliers (dogleg.h; reference dogleg.c:2294-3149).  The leverage blocks come from the device (dlg_backend.h:
// dlg_feature_leverage); what is left here is the host logic around them.
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

// ---- covariance: what the reference's users get from cholmod_solve on ctx->factorization with unit right-hand sides
bool cov_ready(dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx, const char* who)
{
  if(!point || !ctx) { MSG("%s(): no point or context", who); return false; }
  const Driver* d = D(ctx);
  if(d->sharded && d->nranks > 1) { MSG("%s() works on one rank only (this context has %d)", who, d->nranks); return false; }
  return dogleg_computeJtJfactorization(point, ctx);
}

// ---- a batch of small dense problems: the shape every batch entry point takes.  prm: the products form, which has no Nmeas and
// takes the layout of JtJ from the parameters (dogleg.c:597-601 refuses packed lower too); nullptr: the J form
bool batch_shape_ok(const char* who, unsigned int B, unsigned int Nstate, unsigned int Nmeas, const char* larger,
                    const dogleg_parameters2_t* prm = nullptr)
{
  if(B == 0 || Nstate == 0 || (!prm && Nmeas == 0))
  {
    if(prm) MSG("%s: B = %u, Nstate = %u: neither may be 0", who, B, Nstate);
    else    MSG("%s: B = %u, Nstate = %u, Nmeas = %u: none may be 0", who, B, Nstate, Nmeas);
    return false;
  }
  if(Nstate > DOGLEG_AMD_BATCH_MAX_NSTATE)
  {
    MSG("%s: Nstate = %u, the batch kernels take at most %d variables (larger problems: %s)", who, Nstate,
        DOGLEG_AMD_BATCH_MAX_NSTATE, larger);
    return false;
  }
  if(B > 0x7fffffffu/4 || (!prm && Nmeas > 0x7fffffffu/(Nstate + 1)))
  {
    if(prm) MSG("%s: B = %u problems: beyond the index range of the batch kernels", who, B);
    else    MSG("%s: B = %u problems of %u x %u: beyond the index range of the batch kernels", who, B, Nmeas, Nstate);
    return false;
  }
  if(prm && prm->JtJ_packed && !prm->JtJ_upper)
  { MSG("%s: JtJ_packed without JtJ_upper (a packed lower triangle) is not supported: use the packed upper or the unpacked layout", who); return false; }
  return true;
}
// the shape of a request record a of either form (fJ or fP given); prm: defaulted.  larger_J: the J form's hint
template <class Req> bool request_shape_ok(const char* who, const Req& a, const dogleg_parameters2_t* prm, const char* larger_J)
{
  return batch_shape_ok(who, a.B, a.N, a.M, a.fP ? "a loop over dogleg_optimize_dense_products" : larger_J, a.fP ? prm : nullptr);
}

// the loss of the robust batch solve
bool batch_loss_ok(const char* who, const dogleg_amd_batch_loss_t* loss, unsigned int Nmeas)
{
  if(!loss) { MSG("%s: loss must be given (least squares: dogleg_amd_optimize_dense_batch, or DOGLEG_AMD_LOSS_TRIVIAL)", who); return false; }
  if(loss->kind < DOGLEG_AMD_LOSS_TRIVIAL || loss->kind > DOGLEG_AMD_LOSS_CAUCHY)
  { MSG("%s: loss->kind = %d is none of DOGLEG_AMD_LOSS_{TRIVIAL, HUBER, SOFT_L1, CAUCHY}", who, loss->kind); return false; }
  if(loss->kind != DOGLEG_AMD_LOSS_TRIVIAL && !(std::isfinite(loss->scale) && loss->scale > 0.0))
  { MSG("%s: loss->scale = %g must be finite and > 0", who, loss->scale); return false; }
  if(loss->featureSize > DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE)
  {
    MSG("%s: loss->featureSize = %d: sizes 1 to %d are supported", who, loss->featureSize, DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE);
    return false;
  }
  const unsigned int fs = loss->featureSize <= 1 ? 1u : (unsigned int)loss->featureSize;
  if(Nmeas % fs) { MSG("%s: Nmeas = %u is not a multiple of loss->featureSize = %u", who, Nmeas, fs); return false; }
  return true;
}
// features per problem under a (checked) loss; 0 without one
size_t loss_features(const dogleg_amd_batch_loss_t* loss, unsigned int Nmeas)
{
  return loss ? Nmeas/(loss->featureSize <= 1 ? 1u : (unsigned int)loss->featureSize) : 0;
}

// the bounds of the bounded batch solve: the struct must be given (its pointers may be NULL), weights belong to a loss, and the
// products form has no rows for either
bool batch_bounds_ok(const char* who, bool products, const dogleg_amd_batch_bounds_t* bounds, const dogleg_amd_batch_loss_t* loss,
                     const double* weights)
{
  if(products && (loss || weights))
  { MSG("%s: the products form has no rows: it takes neither a loss nor weights", who); return false; }
  if(!bounds) { MSG("%s: bounds must be given (no bounds at all: lower = upper = NULL inside it, or the entry point without _bounded)", who); return false; }
  if(weights && !loss) { MSG("%s: weights are those of a loss, and loss is NULL", who); return false; }
  return true;
}

// the fit of the ..._fit uncertainty and query calls, as it lies in a request record (all three NULL: nothing to check).  The
// products form has no rows, so it takes held only; with weights given, loss says only how many rows share one, and kind and
// scale are not read.  Nobservations: of a query call (the first rows must be whole features), < 0 otherwise
bool batch_fit_ok(const char* who, bool products, const dogleg_amd_batch_loss_t* loss, const double* weights, unsigned int Nmeas,
                  int Nobservations)
{
  if(products && (loss || weights))
  { MSG("%s: the products form has no rows to weight: fit->loss and fit->weights must be NULL there (fit->held is taken)", who); return false; }
  if(weights && !loss) { MSG("%s: fit->weights without fit->loss, which says how many rows share a weight", who); return false; }
  if(!loss) return true;
  if(weights)
  {
    // (featureSize alone: batch_loss_ok's two last checks)
    const dogleg_amd_batch_loss_t shape = {DOGLEG_AMD_LOSS_TRIVIAL, 1.0, loss->featureSize};
    if(!batch_loss_ok(who, &shape, Nmeas)) return false;
  }
  else if(!batch_loss_ok(who, loss, Nmeas)) return false;
  const int fs = loss->featureSize <= 1 ? 1 : loss->featureSize;
  if(Nobservations >= 0 && Nobservations % fs)
  { MSG("%s: Nobservations = %d is not a multiple of fit->loss->featureSize = %d", who, Nobservations, fs); return false; }
  return true;
}
// a fit into the last three members of a request record (dense_batch.h); fit == NULL: none
template <class Req> Req with_fit(Req a, const dogleg_amd_batch_fit_t* fit)
{
  if(fit) { a.loss = fit->loss; a.weights = fit->weights; a.held = fit->held; }
  return a;
}
// a (checked) model into a request record of the uncertainty or query kind: its shape, the likelihood and, of a fit, held alone
template <class Req> Req with_model(Req a, const dogleg_amd_batch_model_t* model, int likelihood, const unsigned char* held)
{
  a.N = (unsigned int)dogleg_batch_model_nstate(model->kind); a.M = model->Nmeas;
  a.held = held; a.model = model; a.likelihood = likelihood;
  return a;
}

// the record of a built-in model (dogleg.h: dogleg_amd_batch_model_t), from its members alone: no pointer's target is looked at
bool batch_model_ok(const char* who, const dogleg_amd_batch_model_t* model, int likelihood = DOGLEG_AMD_LIKELIHOOD_GAUSS)
{
  if(likelihood != DOGLEG_AMD_LIKELIHOOD_GAUSS && likelihood != DOGLEG_AMD_LIKELIHOOD_POISSON)
  {
    MSG("%s: likelihood = %d is neither DOGLEG_AMD_LIKELIHOOD_GAUSS nor DOGLEG_AMD_LIKELIHOOD_POISSON", who, likelihood);
    return false;
  }
  if(!model) { MSG("%s: model must be given", who); return false; }
  if(likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON && model->scale)
  {
    MSG("%s: model->scale must be NULL with DOGLEG_AMD_LIKELIHOOD_POISSON: counts carry their own variance", who);
    return false;
  }
  if(dogleg_batch_model_nstate(model->kind) < 0)
  {
    MSG("%s: model->kind = %d is none of DOGLEG_AMD_MODEL_{EXPDECAY, GAUSS1D, GAUSS2D, GAUSS2D_ELLIPTIC}", who, model->kind);
    return false;
  }
  if(!model->y) { MSG("%s: model->y must be given", who); return false; }
  if(model->Nmeas == 0) { MSG("%s: model->Nmeas = 0", who); return false; }
  const bool two_d = model->kind == DOGLEG_AMD_MODEL_GAUSS2D || model->kind == DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC;
  if(two_d && (unsigned long long)model->width*model->height != model->Nmeas)
  {
    MSG("%s: a window of model->width x model->height = %u x %u pixels, and model->Nmeas = %u", who, model->width, model->height,
        model->Nmeas);
    return false;
  }
  if(two_d && model->t) { MSG("%s: model->t must be NULL for the 2D kinds: the abscissae are the pixels' centres", who); return false; }
  if(!two_d && (model->width || model->height))
  { MSG("%s: model->width = %u, model->height = %u: both are 0 for the 1D kinds", who, model->width, model->height); return false; }
  return true;
}

// a (checked) camera record into a request record of the uncertainty or query kind: its model, whose y is NULL, and the record
template <class Req> Req with_camera(Req a, const dogleg_amd_batch_camera_t* camera, int likelihood, const unsigned char* held)
{
  a = with_model(a, &camera->model, likelihood, held);
  a.camera = camera;
  return a;
}
// bytes of one reading of a camera record; 0 for an unknown dtype
size_t camera_element(int dtype)
{
  return dtype == DOGLEG_AMD_DATA_F64 ? 8 : dtype == DOGLEG_AMD_DATA_F32 ? 4 : dtype == DOGLEG_AMD_DATA_U16 ? 2 : 0;
}
// the camera record (dogleg.h: dogleg_amd_batch_camera_t), from its members alone: no pointer's target is looked at.  Its model is
// checked as the fused solve checks a model record, with raw in the place of y
bool batch_camera_ok(const char* who, const dogleg_amd_batch_camera_t* camera, int likelihood)
{
  if(!camera) { MSG("%s: camera must be given", who); return false; }
  if(camera->model.y) { MSG("%s: camera->model.y must be NULL: the data of a camera record are camera->raw", who); return false; }
  if(!camera->raw) { MSG("%s: camera->raw must be given", who); return false; }
  dogleg_amd_batch_model_t m = camera->model;
  m.y = (const double*)camera->raw;
  if(!batch_model_ok(who, &m, likelihood)) return false;
  const size_t el = camera_element(camera->dtype);
  if(!el) { MSG("%s: camera->dtype = %d is none of DOGLEG_AMD_DATA_{F64, F32, U16}", who, camera->dtype); return false; }
  if((size_t)camera->raw % el) { MSG("%s: camera->raw = %p is not aligned to its element of %zu bytes", who, camera->raw, el); return false; }
  const bool any = camera->offset || camera->gain_inv || camera->origin || camera->sensor_width || camera->sensor_height;
  const bool all = camera->offset && camera->gain_inv && camera->origin && camera->sensor_width && camera->sensor_height;
  if((any || camera->readvar) && !all)
  {
    MSG("%s: calibration is given in part: camera->offset, gain_inv, origin, sensor_width and sensor_height go together (readvar only "
        "with them), or all of them are NULL / 0", who);
    return false;
  }
  if(!all) return true;
  const bool two_d = m.kind == DOGLEG_AMD_MODEL_GAUSS2D || m.kind == DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC;
  if(!two_d) { MSG("%s: calibration maps go with the 2D kinds only: model.kind = %d has no window on the sensor", who, m.kind); return false; }
  if(camera->sensor_width < m.width || camera->sensor_height < m.height)
  {
    MSG("%s: a sensor of %u x %u pixels is smaller than the window of %u x %u", who, camera->sensor_width, camera->sensor_height, m.width,
        m.height);
    return false;
  }
  if((unsigned long long)camera->sensor_width*camera->sensor_height > 2147483647ull)
  { MSG("%s: a sensor of %u x %u pixels: more than 2^31 - 1 are not supported", who, camera->sensor_width, camera->sensor_height); return false; }
  return true;
}

// a *_dev argument of the device-resident batch entry points: memory a kernel of the current device may touch over `bytes`
bool device_span_ok(const char* who, const char* name, const void* ptr, size_t bytes)
{
  if(dlg_batch_device_span_ok(ptr, bytes)) return true;
  MSG("%s: %s = %p is not device-accessible memory of the current device that covers the %zu bytes this call touches there "
      "(device, managed or registered host memory; host arrays go to the entry point without _device)", who, name, ptr, bytes);
  return false;
}
// an optional one
bool device_span_ok_or_null(const char* who, const char* name, const void* ptr, size_t bytes)
{
  return !ptr || device_span_ok(who, name, ptr, bytes);
}
// the arrays of a (checked) model record of B problems, which lie in device memory on either route; no model: nothing to check.
// camera: the (checked) record the model lies in, or NULL: its raw stands for y, and its maps and origins are checked too
bool model_spans_ok(const char* who, const dogleg_amd_batch_model_t* model, size_t B, const dogleg_amd_batch_camera_t* camera = nullptr)
{
  if(!model) return true;
  const size_t BM = B*model->Nmeas;
  if(camera)
  {
    const size_t px = sizeof(float)*(size_t)camera->sensor_width*camera->sensor_height;
    if(!(device_span_ok(who, "camera->raw", camera->raw, camera_element(camera->dtype)*BM) &&
         device_span_ok_or_null(who, "camera->offset", camera->offset, px) &&
         device_span_ok_or_null(who, "camera->gain_inv", camera->gain_inv, px) &&
         device_span_ok_or_null(who, "camera->readvar", camera->readvar, px) &&
         device_span_ok_or_null(who, "camera->origin", camera->origin, sizeof(int)*2*B))) return false;
  }
  else if(!device_span_ok(who, "model->y", model->y, sizeof(double)*BM)) return false;
  return device_span_ok_or_null(who, "model->t", model->t, sizeof(double)*(model->t_per_problem ? BM : (size_t)model->Nmeas)) &&
         device_span_ok_or_null(who, "model->scale", model->scale, sizeof(double)*BM);
}

// ---- the three kinds of batch request (dense_batch.h), each behind one function that makes every check of its entry points in
// one order: the required pointers, the shape, what the kind adds, one rank only; then, and only on the device route, the spans
// of the caller's arrays.  Nothing before the spans looks at a pointer's target.  who: the entry point
enum SolveKind { SOLVE_PLAIN, SOLVE_ROBUST, SOLVE_BOUNDED };
int batch_solve_entry(const char* who, SolveKind kind, DlgBatchSolve a)
{
  const char* dev = a.device ? "_dev" : "";
  if(!a.p || !(a.fJ || a.fP || a.model) || !a.results) { MSG("%s: p%s, the callback and results%s must be given", who, dev, dev); return -1; }
  // (every solve by a J callback comes through here: the plain, robust and bounded ones and their _device twins)
  if(a.fJ == dogleg_amd_batch_model_fisher_callback)
  {
    MSG("%s: dogleg_amd_batch_model_fisher_callback is no callback of a solve: its J is not the derivative of its x, and a solve through "
        "it would minimise Pearson's chi^2 with a wrong Jacobian.  The Poisson fit is dogleg_amd_optimize_dense_batch_model_mle; this "
        "callback serves the uncertainty, query and _fit calls", who);
    return -1;
  }
  if(a.fJ == dogleg_amd_batch_camera_fisher_callback)
  {
    MSG("%s: dogleg_amd_batch_camera_fisher_callback is no callback of a solve: its J is not the derivative of its x, and a solve through "
        "it would minimise Pearson's chi^2 with a wrong Jacobian.  The Poisson fit is dogleg_amd_optimize_dense_batch_camera; this "
        "callback serves the uncertainty, query and _fit calls", who);
    return -1;
  }
  if(!a.prm) a.prm = &g_params;
  a.unpacked = a.fP && !a.prm->JtJ_packed;
  if(!request_shape_ok(who, a, a.prm, "a loop over dogleg_optimize_dense2")) return -1;
  if((kind == SOLVE_ROBUST || a.loss) && !batch_loss_ok(who, a.loss, a.M)) return -1;
  if(kind == SOLVE_BOUNDED && !batch_bounds_ok(who, a.fP != nullptr, a.bounds, a.loss, a.weights)) return -1;
  if(!one_rank_only(who)) return -1;
  const size_t B = a.B, BN = B*a.N;
  const dogleg_amd_batch_bounds_t none = {nullptr, nullptr, nullptr}, &bounds = a.bounds ? *a.bounds : none;
  if(a.device &&
     !(device_span_ok(who, "p_dev", a.p, sizeof(double)*BN) &&
       device_span_ok(who, "results_dev", a.results, sizeof(dogleg_amd_batch_result_t)*B) &&
       device_span_ok_or_null(who, "lambda_dev", a.lambda, sizeof(double)*B) &&
       device_span_ok_or_null(who, "active_dev", a.active, B) &&
       device_span_ok_or_null(who, "weights_dev", a.weights, sizeof(double)*B*loss_features(a.loss, a.M)) &&
       device_span_ok_or_null(who, "bounds->lower", bounds.lower, sizeof(double)*BN) &&
       device_span_ok_or_null(who, "bounds->upper", bounds.upper, sizeof(double)*BN) &&
       device_span_ok_or_null(who, "bounds->held", bounds.held, BN))) return -1;
  if(!model_spans_ok(who, a.model, B, a.camera)) return -1;
  return dlg_dense_batch_solve(a);
}
// featureSize: as the caller gave it; a.fs is set here
int batch_unc_entry(const char* who, DlgBatchUnc a, const dogleg_parameters2_t* parameters, int featureSize)
{
  const char* dev = a.device ? "_dev" : "";
  if(!a.p || !(a.fJ || a.fP || a.model) || !a.status) { MSG("%s: p%s, the callback and status%s must be given", who, dev, dev); return -1; }
  const dogleg_parameters2_t* prm = parameters ? parameters : &g_params;
  a.unpacked = a.fP && !prm->JtJ_packed;
  if(!request_shape_ok(who, a, prm, "a loop over dogleg_optimize_dense2")) return -1;
  if(featureSize > 2) { MSG("%s: featureSize = %d: only 1 and 2 are supported", who, featureSize); return -1; }
  a.fs = featureSize <= 1 ? 1 : 2;
  const unsigned int NF = a.M/(unsigned int)a.fs;
  if(!a.covariance && !a.variances && !a.factors)
  {
    if(a.fP) MSG("%s: neither covariance%s nor variances%s is asked for", who, dev, dev);
    else     MSG("%s: none of covariance%s, variances%s, factors%s is asked for", who, dev, dev, dev);
    return -1;
  }
  if(a.factors && !a.scale)
  {
    if(a.device) MSG("%s: factors_dev needs scale_dev", who);
    else         MSG("%s: factors need scale", who);
    return -1;
  }
  if(a.factors && NF == 0) { MSG("%s: Nmeas = %u holds no feature of size %d", who, a.M, a.fs); return -1; }
  // a scale[b] <= 0 is to be computed, which needs Nmeas > Nstate + 1: the host route looks for one, the device route cannot
  if(a.factors && a.M <= a.N + 1)
  {
    if(a.device)
    {
      MSG("%s: factors_dev with Nmeas <= Nstate + 1 (%u, %u): a scale_dev[b] <= 0 could not be computed, and whether there is one "
          "cannot be seen without a copy", who, a.M, a.N);
      return -1;
    }
    for(unsigned int b = 0; b < a.B; b++)
      if(!(a.scale[b] > 0.0))
      {
        MSG("%s: scale[%u] <= 0 is to be computed, which needs Nmeas > Nstate + 1 (%u, %u)", who, b, a.M, a.N);
        return -1;
      }
  }
  if(!batch_fit_ok(who, a.fP != nullptr, a.loss, a.weights, a.M, -1)) return -1;
  if(!one_rank_only(who)) return -1;
  const size_t B = a.B, BN = B*a.N;
  if(a.device &&
     !(device_span_ok(who, "p_dev", a.p, sizeof(double)*BN) && device_span_ok(who, "status_dev", a.status, sizeof(int)*B) &&
       device_span_ok_or_null(who, "lambda_dev", a.lambda, sizeof(double)*B) &&
       device_span_ok_or_null(who, "covariance_dev", a.covariance, sizeof(double)*BN*a.N) &&
       device_span_ok_or_null(who, "variances_dev", a.variances, sizeof(double)*BN) &&
       (!a.factors || (device_span_ok(who, "factors_dev", a.factors, sizeof(double)*B*NF) &&
                       device_span_ok(who, "scale_dev", a.scale, sizeof(double)*B))) &&
       device_span_ok_or_null(who, "active_dev", a.active, B) &&
       device_span_ok_or_null(who, "fit->weights", a.weights, sizeof(double)*B*loss_features(a.loss, a.M)) &&
       device_span_ok_or_null(who, a.model ? "held_dev" : "fit->held", a.held, BN))) return -1;
  if(!model_spans_ok(who, a.model, B, a.camera)) return -1;
  return dlg_dense_batch_uncertainty(a);
}
// Nq queries of Qrows rows per problem, Nobservations of the J form's Nmeas
int batch_query_entry(const char* who, DlgBatchQuery a, const dogleg_parameters2_t* parameters)
{
  const char* dev = a.device ? "_dev" : "";
  if(!a.p || !(a.fJ || a.fP || a.model) || !a.Jq || !a.out || !a.status)
  { MSG("%s: p%s, the callback, Jq%s, out%s and status%s must be given", who, dev, dev, dev, dev); return -1; }
  const dogleg_parameters2_t* prm = parameters ? parameters : &g_params;
  a.unpacked = a.fP && !prm->JtJ_packed;
  if(!request_shape_ok(who, a, prm, "a loop over dogleg_optimize_dense2 and dogleg_amd_query_covariance")) return -1;
  if(a.Nq == 0 || a.Qrows == 0) { MSG("%s: Nq = %u, Qrows = %u: neither may be 0", who, a.Nq, a.Qrows); return -1; }
  if(a.Qrows > DOGLEG_AMD_BATCH_QUERY_MAX_ROWS)
  {
    MSG("%s: Qrows = %u, a query has at most %d rows (wider queries: dogleg_amd_dense_batch_uncertainty's covariance)", who, a.Qrows,
        DOGLEG_AMD_BATCH_QUERY_MAX_ROWS);
    return -1;
  }
  if((double)a.B*(double)a.Nq*(double)a.Qrows > (double)(0x7fffffffu/DOGLEG_AMD_BATCH_MAX_NSTATE))
  { MSG("%s: B = %u problems of %u queries of %u rows: beyond the index range of the batch kernels", who, a.B, a.Nq, a.Qrows); return -1; }
  if(a.Nobservations >= 0 && (unsigned int)a.Nobservations > a.M)
  { MSG("%s: Nobservations = %d exceeds Nmeas = %u (< 0 selects the plain form)", who, a.Nobservations, a.M); return -1; }
  if(!batch_fit_ok(who, a.fP != nullptr, a.loss, a.weights, a.M, a.fP ? -1 : a.Nobservations)) return -1;
  if(!one_rank_only(who)) return -1;
  const size_t B = a.B, rows = B*a.Nq*a.Qrows;
  if(a.device &&
     !(device_span_ok(who, "p_dev", a.p, sizeof(double)*B*a.N) && device_span_ok(who, "status_dev", a.status, sizeof(int)*B) &&
       device_span_ok_or_null(who, "lambda_dev", a.lambda, sizeof(double)*B) &&
       device_span_ok(who, "Jq_dev", a.Jq, sizeof(double)*rows*a.N) && device_span_ok(who, "out_dev", a.out, sizeof(double)*rows*a.Qrows) &&
       device_span_ok_or_null(who, "active_dev", a.active, B) &&
       device_span_ok_or_null(who, "fit->weights", a.weights, sizeof(double)*B*loss_features(a.loss, a.M)) &&
       device_span_ok_or_null(who, a.model ? "held_dev" : "fit->held", a.held, B*a.N))) return -1;
  if(!model_spans_ok(who, a.model, B, a.camera)) return -1;
  return dlg_dense_batch_query(a);
}

// ---- the Jacobian of a device callback against central differences
constexpr double GRADTEST_DELTA = 1e-6;             // dogleg.c:352
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

bool dlg_batch_camera_ok(const char* who, const dogleg_amd_batch_camera_t* camera, int likelihood)
{
  return batch_camera_ok(who, camera, likelihood);
}


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
// dlg_covariance_blocks)
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

// ---- extension (not in the reference): batches of small dense problems, the dog-leg loop on the device (dense_batch.hip).  Every
// entry point fills the request record of its kind (dense_batch.h: p, B, N, M, fJ, fP, cookie, unpacked, then the kind's own
// fields, active, stream, device) and hands it to the kind's checks above
int dogleg_amd_optimize_dense_batch(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                    dogleg_callback_device_batch_t* f, void* cookie,
                                    const dogleg_parameters2_t* parameters, dogleg_amd_batch_result_t* results)
{
  return batch_solve_entry(__func__, SOLVE_PLAIN, DlgBatchSolve{p, B, Nstate, Nmeas, f, nullptr, cookie, false, parameters, results});
}
// ---- the fused solve of a built-in model (dogleg.h: dogleg_amd_batch_model_t): the third form of the solve record, no callback.
// The record is checked first: Nstate and Nmeas come from it
int dogleg_amd_optimize_dense_batch_model(double* p, unsigned int B, const dogleg_amd_batch_model_t* model,
                                          const dogleg_parameters2_t* parameters, const dogleg_amd_batch_bounds_t* bounds,
                                          dogleg_amd_batch_result_t* results)
{
  if(!batch_model_ok(__func__, model)) return -1;
  DlgBatchSolve a{p, B, (unsigned int)dogleg_batch_model_nstate(model->kind), model->Nmeas, nullptr, nullptr, nullptr, false,
                  parameters, results};
  a.bounds = bounds; a.model = model;
  return batch_solve_entry(__func__, bounds ? SOLVE_BOUNDED : SOLVE_PLAIN, a);
}
int dogleg_amd_optimize_dense_batch_model_device(double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                 const dogleg_parameters2_t* parameters, const dogleg_amd_batch_bounds_t* bounds,
                                                 dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                 const unsigned char* active_dev, void* hip_stream)
{
  if(!batch_model_ok(__func__, model)) return -1;
  DlgBatchSolve a{p_dev, B, (unsigned int)dogleg_batch_model_nstate(model->kind), model->Nmeas, nullptr, nullptr, nullptr, false,
                  parameters, results_dev, lambda_dev, active_dev, hip_stream};
  a.bounds = bounds; a.device = true; a.model = model;
  return batch_solve_entry(__func__, bounds ? SOLVE_BOUNDED : SOLVE_PLAIN, a);
}
// ---- the same with a likelihood: GAUSS is the record of the two above; POISSON travels in it beside the model
int dogleg_amd_optimize_dense_batch_model_mle(double* p, unsigned int B, const dogleg_amd_batch_model_t* model, int likelihood,
                                              const dogleg_parameters2_t* parameters, const dogleg_amd_batch_bounds_t* bounds,
                                              dogleg_amd_batch_result_t* results)
{
  if(!batch_model_ok(__func__, model, likelihood)) return -1;
  DlgBatchSolve a{p, B, (unsigned int)dogleg_batch_model_nstate(model->kind), model->Nmeas, nullptr, nullptr, nullptr, false,
                  parameters, results};
  a.bounds = bounds; a.model = model; a.likelihood = likelihood; a.mle = true;
  return batch_solve_entry(__func__, bounds ? SOLVE_BOUNDED : SOLVE_PLAIN, a);
}
int dogleg_amd_optimize_dense_batch_model_mle_device(double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                     int likelihood, const dogleg_parameters2_t* parameters,
                                                     const dogleg_amd_batch_bounds_t* bounds,
                                                     dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                     const unsigned char* active_dev, void* hip_stream)
{
  if(!batch_model_ok(__func__, model, likelihood)) return -1;
  DlgBatchSolve a{p_dev, B, (unsigned int)dogleg_batch_model_nstate(model->kind), model->Nmeas, nullptr, nullptr, nullptr, false,
                  parameters, results_dev, lambda_dev, active_dev, hip_stream};
  a.bounds = bounds; a.device = true; a.model = model; a.likelihood = likelihood; a.mle = true;
  return batch_solve_entry(__func__, bounds ? SOLVE_BOUNDED : SOLVE_PLAIN, a);
}
// ---- the fused uncertainty and query calls of a built-in model: the records of the J form's calls with the model as their third
// form and held as their fit; the record is checked first, as in the fused solve
int dogleg_amd_dense_batch_model_uncertainty(const double* p, unsigned int B, const dogleg_amd_batch_model_t* model, int likelihood,
                                             double* lambda, double* covariance, double* variances, double* factors,
                                             double* scale, int featureSize, int* status, const unsigned char* held)
{
  if(!batch_model_ok(__func__, model, likelihood)) return -1;
  return batch_unc_entry(__func__, with_model(DlgBatchUnc{p, B, 0, 0, nullptr, nullptr, nullptr, false, lambda, covariance, variances,
                                                         factors, scale, 0, status}, model, likelihood, held), nullptr, featureSize);
}
int dogleg_amd_dense_batch_model_uncertainty_device(const double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                    int likelihood, double* lambda_dev, double* covariance_dev,
                                                    double* variances_dev, double* factors_dev, double* scale_dev, int featureSize,
                                                    int* status_dev, const unsigned char* held_dev,
                                                    const unsigned char* active_dev, void* hip_stream)
{
  if(!batch_model_ok(__func__, model, likelihood)) return -1;
  return batch_unc_entry(__func__, with_model(DlgBatchUnc{p_dev, B, 0, 0, nullptr, nullptr, nullptr, false, lambda_dev, covariance_dev,
                                                         variances_dev, factors_dev, scale_dev, 0, status_dev, active_dev, hip_stream,
                                                         true}, model, likelihood, held_dev), nullptr, featureSize);
}
int dogleg_amd_dense_batch_model_query_covariance(const double* p, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                  int likelihood, double* lambda, const double* Jq, unsigned int Nq,
                                                  unsigned int Qrows, int Nobservations, double* out, int* status,
                                                  const unsigned char* held)
{
  if(!batch_model_ok(__func__, model, likelihood)) return -1;
  return batch_query_entry(__func__, with_model(DlgBatchQuery{p, B, 0, 0, nullptr, nullptr, nullptr, false, lambda, Jq, Nq, Qrows,
                                                               Nobservations, out, status}, model, likelihood, held), nullptr);
}
int dogleg_amd_dense_batch_model_query_covariance_device(const double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                         int likelihood, double* lambda_dev, const double* Jq_dev, unsigned int Nq,
                                                         unsigned int Qrows, int Nobservations, double* out_dev, int* status_dev,
                                                         const unsigned char* held_dev, const unsigned char* active_dev,
                                                         void* hip_stream)
{
  if(!batch_model_ok(__func__, model, likelihood)) return -1;
  return batch_query_entry(__func__, with_model(DlgBatchQuery{p_dev, B, 0, 0, nullptr, nullptr, nullptr, false, lambda_dev, Jq_dev, Nq,
                                                               Qrows, Nobservations, out_dev, status_dev, active_dev, hip_stream,
                                                               true}, model, likelihood, held_dev), nullptr);
}
// ---- the same calls on a camera record: the model forms with camera->raw, and the calibration maps, as the source of the data
int dogleg_amd_optimize_dense_batch_camera(double* p, unsigned int B, const dogleg_amd_batch_camera_t* camera, int likelihood,
                                           const dogleg_parameters2_t* parameters, const dogleg_amd_batch_bounds_t* bounds,
                                           dogleg_amd_batch_result_t* results)
{
  if(!batch_camera_ok(__func__, camera, likelihood)) return -1;
  DlgBatchSolve a{p, B, (unsigned int)dogleg_batch_model_nstate(camera->model.kind), camera->model.Nmeas, nullptr, nullptr, nullptr, false,
                  parameters, results};
  a.bounds = bounds; a.model = &camera->model; a.likelihood = likelihood; a.mle = true; a.camera = camera;
  return batch_solve_entry(__func__, bounds ? SOLVE_BOUNDED : SOLVE_PLAIN, a);
}
int dogleg_amd_optimize_dense_batch_camera_device(double* p_dev, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                                  int likelihood, const dogleg_parameters2_t* parameters,
                                                  const dogleg_amd_batch_bounds_t* bounds, dogleg_amd_batch_result_t* results_dev,
                                                  double* lambda_dev, const unsigned char* active_dev, void* hip_stream)
{
  if(!batch_camera_ok(__func__, camera, likelihood)) return -1;
  DlgBatchSolve a{p_dev, B, (unsigned int)dogleg_batch_model_nstate(camera->model.kind), camera->model.Nmeas, nullptr, nullptr, nullptr,
                  false, parameters, results_dev, lambda_dev, active_dev, hip_stream};
  a.bounds = bounds; a.device = true; a.model = &camera->model; a.likelihood = likelihood; a.mle = true; a.camera = camera;
  return batch_solve_entry(__func__, bounds ? SOLVE_BOUNDED : SOLVE_PLAIN, a);
}
int dogleg_amd_dense_batch_camera_uncertainty(const double* p, unsigned int B, const dogleg_amd_batch_camera_t* camera, int likelihood,
                                              double* lambda, double* covariance, double* variances, double* factors, double* scale,
                                              int featureSize, int* status, const unsigned char* held)
{
  if(!batch_camera_ok(__func__, camera, likelihood)) return -1;
  return batch_unc_entry(__func__, with_camera(DlgBatchUnc{p, B, 0, 0, nullptr, nullptr, nullptr, false, lambda, covariance, variances,
                                                          factors, scale, 0, status}, camera, likelihood, held), nullptr, featureSize);
}
int dogleg_amd_dense_batch_camera_uncertainty_device(const double* p_dev, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                                     int likelihood, double* lambda_dev, double* covariance_dev,
                                                     double* variances_dev, double* factors_dev, double* scale_dev, int featureSize,
                                                     int* status_dev, const unsigned char* held_dev,
                                                     const unsigned char* active_dev, void* hip_stream)
{
  if(!batch_camera_ok(__func__, camera, likelihood)) return -1;
  return batch_unc_entry(__func__, with_camera(DlgBatchUnc{p_dev, B, 0, 0, nullptr, nullptr, nullptr, false, lambda_dev, covariance_dev,
                                                          variances_dev, factors_dev, scale_dev, 0, status_dev, active_dev, hip_stream,
                                                          true}, camera, likelihood, held_dev), nullptr, featureSize);
}
int dogleg_amd_dense_batch_camera_query_covariance(const double* p, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                                   int likelihood, double* lambda, const double* Jq, unsigned int Nq,
                                                   unsigned int Qrows, int Nobservations, double* out, int* status,
                                                   const unsigned char* held)
{
  if(!batch_camera_ok(__func__, camera, likelihood)) return -1;
  return batch_query_entry(__func__, with_camera(DlgBatchQuery{p, B, 0, 0, nullptr, nullptr, nullptr, false, lambda, Jq, Nq, Qrows,
                                                                Nobservations, out, status}, camera, likelihood, held), nullptr);
}
int dogleg_amd_dense_batch_camera_query_covariance_device(const double* p_dev, unsigned int B,
                                                          const dogleg_amd_batch_camera_t* camera, int likelihood,
                                                          double* lambda_dev, const double* Jq_dev, unsigned int Nq,
                                                          unsigned int Qrows, int Nobservations, double* out_dev, int* status_dev,
                                                          const unsigned char* held_dev, const unsigned char* active_dev,
                                                          void* hip_stream)
{
  if(!batch_camera_ok(__func__, camera, likelihood)) return -1;
  return batch_query_entry(__func__, with_camera(DlgBatchQuery{p_dev, B, 0, 0, nullptr, nullptr, nullptr, false, lambda_dev, Jq_dev, Nq,
                                                                Qrows, Nobservations, out_dev, status_dev, active_dev, hip_stream,
                                                                true}, camera, likelihood, held_dev), nullptr);
}
int dogleg_amd_batch_last_stats(double* out, int n) { return out ? dlg_dense_batch_last_stats(out, n) : 0; }
int dogleg_amd_dense_batch_uncertainty(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                       dogleg_callback_device_batch_t* f, void* cookie,
                                       double* lambda, double* covariance, double* variances, double* factors,
                                       double* scale, int featureSize, int* status)
{
  return batch_unc_entry(__func__, DlgBatchUnc{p, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda, covariance, variances,
                                               factors, scale, 0, status}, nullptr, featureSize);
}
int dogleg_amd_batch_uncertainty_last_stats(double* out, int n) { return out ? dlg_dense_batch_uncertainty_last_stats(out, n) : 0; }

// ---- the products form of the two: the callback hands back norm2(x), Jt x and JtJ, so there is no Nmeas
int dogleg_amd_optimize_dense_products_batch(double* p, unsigned int B, unsigned int Nstate,
                                             dogleg_callback_device_batch_products_t* f, void* cookie,
                                             const dogleg_parameters2_t* parameters, dogleg_amd_batch_result_t* results)
{
  return batch_solve_entry(__func__, SOLVE_PLAIN, DlgBatchSolve{p, B, Nstate, 0, nullptr, f, cookie, false, parameters, results});
}
int dogleg_amd_dense_products_batch_uncertainty(const double* p, unsigned int B, unsigned int Nstate,
                                                dogleg_callback_device_batch_products_t* f, void* cookie,
                                                const dogleg_parameters2_t* parameters,
                                                double* lambda, double* covariance, double* variances, int* status)
{
  return batch_unc_entry(__func__, DlgBatchUnc{p, B, Nstate, 0, nullptr, f, cookie, false, lambda, covariance, variances, nullptr,
                                               nullptr, 0, status}, parameters, 1);
}

// ---- the device-resident twins of the four
int dogleg_amd_optimize_dense_batch_device(double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           const dogleg_parameters2_t* parameters,
                                           dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                           const unsigned char* active_dev, void* hip_stream)
{
  return batch_solve_entry(__func__, SOLVE_PLAIN, DlgBatchSolve{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, parameters,
                                                                results_dev, lambda_dev, active_dev, hip_stream, nullptr, nullptr,
                                                                nullptr, true});
}
// ---- the robust form of the solve and its device twin
int dogleg_amd_optimize_dense_batch_robust(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                           dogleg_amd_batch_result_t* results, double* weights)
{
  return batch_solve_entry(__func__, SOLVE_ROBUST, DlgBatchSolve{p, B, Nstate, Nmeas, f, nullptr, cookie, false, parameters, results,
                                                                 nullptr, nullptr, nullptr, loss, weights});
}
int dogleg_amd_optimize_dense_batch_robust_device(double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                  dogleg_callback_device_batch_t* f, void* cookie,
                                                  const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                                  dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                  double* weights_dev, const unsigned char* active_dev, void* hip_stream)
{
  return batch_solve_entry(__func__, SOLVE_ROBUST, DlgBatchSolve{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, parameters,
                                                                 results_dev, lambda_dev, active_dev, hip_stream, loss, weights_dev,
                                                                 nullptr, true});
}
// ---- the bounded form and its device twin (loss may be NULL)
int dogleg_amd_optimize_dense_batch_bounded(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                            dogleg_callback_device_batch_t* f, void* cookie,
                                            const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                            const dogleg_amd_batch_bounds_t* bounds, dogleg_amd_batch_result_t* results,
                                            double* weights)
{
  return batch_solve_entry(__func__, SOLVE_BOUNDED, DlgBatchSolve{p, B, Nstate, Nmeas, f, nullptr, cookie, false, parameters, results,
                                                                  nullptr, nullptr, nullptr, loss, weights, bounds});
}
int dogleg_amd_optimize_dense_batch_bounded_device(double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                   dogleg_callback_device_batch_t* f, void* cookie,
                                                   const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                                   const dogleg_amd_batch_bounds_t* bounds,
                                                   dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                   double* weights_dev, const unsigned char* active_dev, void* hip_stream)
{
  return batch_solve_entry(__func__, SOLVE_BOUNDED, DlgBatchSolve{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, parameters,
                                                                  results_dev, lambda_dev, active_dev, hip_stream, loss, weights_dev,
                                                                  bounds, true});
}
// ---- the bounded products form and its device twin (no loss, no weights: the form has no rows)
int dogleg_amd_optimize_dense_products_batch_bounded(double* p, unsigned int B, unsigned int Nstate,
                                                     dogleg_callback_device_batch_products_t* f, void* cookie,
                                                     const dogleg_parameters2_t* parameters,
                                                     const dogleg_amd_batch_bounds_t* bounds, dogleg_amd_batch_result_t* results)
{
  return batch_solve_entry(__func__, SOLVE_BOUNDED, DlgBatchSolve{p, B, Nstate, 0, nullptr, f, cookie, false, parameters, results,
                                                                  nullptr, nullptr, nullptr, nullptr, nullptr, bounds});
}
int dogleg_amd_optimize_dense_products_batch_bounded_device(double* p_dev, unsigned int B, unsigned int Nstate,
                                                            dogleg_callback_device_batch_products_t* f, void* cookie,
                                                            const dogleg_parameters2_t* parameters,
                                                            const dogleg_amd_batch_bounds_t* bounds,
                                                            dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                            const unsigned char* active_dev, void* hip_stream)
{
  return batch_solve_entry(__func__, SOLVE_BOUNDED, DlgBatchSolve{p_dev, B, Nstate, 0, nullptr, f, cookie, false, parameters,
                                                                  results_dev, lambda_dev, active_dev, hip_stream, nullptr, nullptr,
                                                                  bounds, true});
}
int dogleg_amd_optimize_dense_products_batch_device(double* p_dev, unsigned int B, unsigned int Nstate,
                                                    dogleg_callback_device_batch_products_t* f, void* cookie,
                                                    const dogleg_parameters2_t* parameters,
                                                    dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                    const unsigned char* active_dev, void* hip_stream)
{
  return batch_solve_entry(__func__, SOLVE_PLAIN, DlgBatchSolve{p_dev, B, Nstate, 0, nullptr, f, cookie, false, parameters,
                                                                results_dev, lambda_dev, active_dev, hip_stream, nullptr, nullptr,
                                                                nullptr, true});
}
int dogleg_amd_dense_batch_uncertainty_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                              dogleg_callback_device_batch_t* f, void* cookie,
                                              double* lambda_dev, double* covariance_dev, double* variances_dev,
                                              double* factors_dev, double* scale_dev, int featureSize, int* status_dev,
                                              const unsigned char* active_dev, void* hip_stream)
{
  return batch_unc_entry(__func__, DlgBatchUnc{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda_dev, covariance_dev,
                                               variances_dev, factors_dev, scale_dev, 0, status_dev, active_dev, hip_stream, true},
                         nullptr, featureSize);
}
int dogleg_amd_dense_products_batch_uncertainty_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                       dogleg_callback_device_batch_products_t* f, void* cookie,
                                                       const dogleg_parameters2_t* parameters,
                                                       double* lambda_dev, double* covariance_dev, double* variances_dev,
                                                       int* status_dev, const unsigned char* active_dev, void* hip_stream)
{
  return batch_unc_entry(__func__, DlgBatchUnc{p_dev, B, Nstate, 0, nullptr, f, cookie, false, lambda_dev, covariance_dev,
                                               variances_dev, nullptr, nullptr, 0, status_dev, active_dev, hip_stream, true},
                         parameters, 1);
}

// ---- Jq Sigma_b Jq' of per-problem query Jacobians: the four entry points beside the four uncertainty calls
int dogleg_amd_dense_batch_query_covariance(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                            dogleg_callback_device_batch_t* f, void* cookie, double* lambda,
                                            const double* Jq, unsigned int Nq, unsigned int Qrows, int Nobservations,
                                            double* out, int* status)
{
  return batch_query_entry(__func__, DlgBatchQuery{p, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda, Jq, Nq, Qrows,
                                                   Nobservations, out, status}, nullptr);
}
int dogleg_amd_dense_products_batch_query_covariance(const double* p, unsigned int B, unsigned int Nstate,
                                                     dogleg_callback_device_batch_products_t* f, void* cookie,
                                                     const dogleg_parameters2_t* parameters, double* lambda,
                                                     const double* Jq, unsigned int Nq, unsigned int Qrows,
                                                     double* out, int* status)
{
  return batch_query_entry(__func__, DlgBatchQuery{p, B, Nstate, 0, nullptr, f, cookie, false, lambda, Jq, Nq, Qrows, -1, out, status},
                           parameters);
}
int dogleg_amd_dense_batch_query_covariance_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                   dogleg_callback_device_batch_t* f, void* cookie, double* lambda_dev,
                                                   const double* Jq_dev, unsigned int Nq, unsigned int Qrows, int Nobservations,
                                                   double* out_dev, int* status_dev,
                                                   const unsigned char* active_dev, void* hip_stream)
{
  return batch_query_entry(__func__, DlgBatchQuery{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda_dev, Jq_dev, Nq, Qrows,
                                                   Nobservations, out_dev, status_dev, active_dev, hip_stream, true}, nullptr);
}
int dogleg_amd_dense_products_batch_query_covariance_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                            dogleg_callback_device_batch_products_t* f, void* cookie,
                                                            const dogleg_parameters2_t* parameters, double* lambda_dev,
                                                            const double* Jq_dev, unsigned int Nq, unsigned int Qrows,
                                                            double* out_dev, int* status_dev,
                                                            const unsigned char* active_dev, void* hip_stream)
{
  return batch_query_entry(__func__, DlgBatchQuery{p_dev, B, Nstate, 0, nullptr, f, cookie, false, lambda_dev, Jq_dev, Nq, Qrows, -1,
                                                   out_dev, status_dev, active_dev, hip_stream, true}, parameters);
}

// ---- the eight uncertainty and query calls at the optimum of a robust or bounded fit: the records of the eight above with the
// fit in their last three members
int dogleg_amd_dense_batch_uncertainty_fit(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           double* lambda, double* covariance, double* variances, double* factors,
                                           double* scale, int featureSize, int* status, const dogleg_amd_batch_fit_t* fit)
{
  return batch_unc_entry(__func__, with_fit(DlgBatchUnc{p, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda, covariance, variances,
                                                        factors, scale, 0, status}, fit), nullptr, featureSize);
}
int dogleg_amd_dense_products_batch_uncertainty_fit(const double* p, unsigned int B, unsigned int Nstate,
                                                    dogleg_callback_device_batch_products_t* f, void* cookie,
                                                    const dogleg_parameters2_t* parameters,
                                                    double* lambda, double* covariance, double* variances, int* status,
                                                    const dogleg_amd_batch_fit_t* fit)
{
  return batch_unc_entry(__func__, with_fit(DlgBatchUnc{p, B, Nstate, 0, nullptr, f, cookie, false, lambda, covariance, variances,
                                                        nullptr, nullptr, 0, status}, fit), parameters, 1);
}
int dogleg_amd_dense_batch_uncertainty_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                  dogleg_callback_device_batch_t* f, void* cookie,
                                                  double* lambda_dev, double* covariance_dev, double* variances_dev,
                                                  double* factors_dev, double* scale_dev, int featureSize, int* status_dev,
                                                  const unsigned char* active_dev, void* hip_stream,
                                                  const dogleg_amd_batch_fit_t* fit)
{
  return batch_unc_entry(__func__, with_fit(DlgBatchUnc{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda_dev,
                                                        covariance_dev, variances_dev, factors_dev, scale_dev, 0, status_dev,
                                                        active_dev, hip_stream, true}, fit), nullptr, featureSize);
}
int dogleg_amd_dense_products_batch_uncertainty_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                           dogleg_callback_device_batch_products_t* f, void* cookie,
                                                           const dogleg_parameters2_t* parameters,
                                                           double* lambda_dev, double* covariance_dev, double* variances_dev,
                                                           int* status_dev, const unsigned char* active_dev, void* hip_stream,
                                                           const dogleg_amd_batch_fit_t* fit)
{
  return batch_unc_entry(__func__, with_fit(DlgBatchUnc{p_dev, B, Nstate, 0, nullptr, f, cookie, false, lambda_dev, covariance_dev,
                                                        variances_dev, nullptr, nullptr, 0, status_dev, active_dev, hip_stream,
                                                        true}, fit), parameters, 1);
}
int dogleg_amd_dense_batch_query_covariance_fit(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                dogleg_callback_device_batch_t* f, void* cookie, double* lambda,
                                                const double* Jq, unsigned int Nq, unsigned int Qrows, int Nobservations,
                                                double* out, int* status, const dogleg_amd_batch_fit_t* fit)
{
  return batch_query_entry(__func__, with_fit(DlgBatchQuery{p, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda, Jq, Nq, Qrows,
                                                            Nobservations, out, status}, fit), nullptr);
}
int dogleg_amd_dense_products_batch_query_covariance_fit(const double* p, unsigned int B, unsigned int Nstate,
                                                         dogleg_callback_device_batch_products_t* f, void* cookie,
                                                         const dogleg_parameters2_t* parameters, double* lambda,
                                                         const double* Jq, unsigned int Nq, unsigned int Qrows,
                                                         double* out, int* status, const dogleg_amd_batch_fit_t* fit)
{
  return batch_query_entry(__func__, with_fit(DlgBatchQuery{p, B, Nstate, 0, nullptr, f, cookie, false, lambda, Jq, Nq, Qrows, -1,
                                                            out, status}, fit), parameters);
}
int dogleg_amd_dense_batch_query_covariance_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                       dogleg_callback_device_batch_t* f, void* cookie, double* lambda_dev,
                                                       const double* Jq_dev, unsigned int Nq, unsigned int Qrows,
                                                       int Nobservations, double* out_dev, int* status_dev,
                                                       const unsigned char* active_dev, void* hip_stream,
                                                       const dogleg_amd_batch_fit_t* fit)
{
  return batch_query_entry(__func__, with_fit(DlgBatchQuery{p_dev, B, Nstate, Nmeas, f, nullptr, cookie, false, lambda_dev, Jq_dev,
                                                            Nq, Qrows, Nobservations, out_dev, status_dev, active_dev, hip_stream,
                                                            true}, fit), nullptr);
}
int dogleg_amd_dense_products_batch_query_covariance_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                                dogleg_callback_device_batch_products_t* f, void* cookie,
                                                                const dogleg_parameters2_t* parameters, double* lambda_dev,
                                                                const double* Jq_dev, unsigned int Nq, unsigned int Qrows,
                                                                double* out_dev, int* status_dev,
                                                                const unsigned char* active_dev, void* hip_stream,
                                                                const dogleg_amd_batch_fit_t* fit)
{
  return batch_query_entry(__func__, with_fit(DlgBatchQuery{p_dev, B, Nstate, 0, nullptr, f, cookie, false, lambda_dev, Jq_dev, Nq,
                                                            Qrows, -1, out_dev, status_dev, active_dev, hip_stream, true}, fit),
                           parameters);
}

// ---- extension (not in the reference): the Jacobian of a device callback against central differences (gradcheck.hip)
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
  if(!batch_shape_ok(who, B, Nstate, Nmeas, "dogleg_amd_check_jacobian_device")) return -1;
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

// ---- extension (not in the reference): the device backend behind a returned context, for
// dlg_solve_with_factor / dlg_point_download on the resident factor and vectors
dlg_backend_t* dogleg_amd_backend(dogleg_solverContext_t* ctx) { return ctx ? D(ctx)->be : nullptr; }
int dogleg_amd_point_slot(dogleg_solverContext_t* ctx, const dogleg_operatingPoint_t* point)
{ return (ctx && point) ? slot_of(D(ctx), point) : -1; }

} // extern "C"
