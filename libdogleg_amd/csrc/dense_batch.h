// dense_batch.h -- the batch solver of dense_batch.hip as the driver sees it (not installed).
#pragma once
#include <cstddef>
#include "../../include/dogleg.h"

// One request record per kind of call, checked by the caller (api_extensions.cpp); each call returns 0 / -1 with a message on
// stderr.  What the records share: one of fJ / fP is given; the products form (fP) has M = 0 and its layout of JtJ is `unpacked`
// (packed means packed upper: the caller refused packed lower).  device: every array of the caller lies in device memory (the
// dogleg_amd_*_batch_device entry points), active: [B] bytes or NULL, stream: a hipStream_t or NULL (the cache's own); otherwise
// host arrays, active and stream NULL.
#pragma GCC visibility push(hidden)
// dogleg_amd_optimize_dense[_products]_batch[_robust|_bounded][_device]
struct DlgBatchSolve
{
  double* p; unsigned int B, N, M;
  dogleg_callback_device_batch_t* fJ; dogleg_callback_device_batch_products_t* fP; void* cookie; bool unpacked;
  const dogleg_parameters2_t* prm;
  dogleg_amd_batch_result_t* results; double* lambda;          // lambda: the device route only, or NULL
  const unsigned char* active; void* stream;
  // the robust form (J form only; kind, scale and a featureSize <= 4 that divides M checked by the caller; weights: [B][M /
  // featureSize] or NULL), or both NULL
  const dogleg_amd_batch_loss_t* loss; double* weights;
  const dogleg_amd_batch_bounds_t* bounds;                     // the bounded form (either form; lower / upper / held may be NULL), or NULL
  bool device;
  // the model form (dogleg_amd_optimize_dense_batch_model[_device]): a third form beside fJ / fP, both NULL then; N and M are
  // those of the (checked) record, whose arrays lie in device memory on either route; no loss.  NULL otherwise
  const dogleg_amd_batch_model_t* model;
  // the likelihood of a model form (DOGLEG_AMD_LIKELIHOOD_*, checked; GAUSS: least squares, the model form as it was) and whether
  // the call came in by dogleg_amd_optimize_dense_batch_model_mle[_device] (its name in the messages)
  int likelihood; bool mle;
  // a model form whose data are those of a camera record (dogleg_amd_optimize_dense_batch_camera[_device]): the (checked) record,
  // model = &camera->model, whose y is NULL.  NULL otherwise.  The same in the two records below
  const dogleg_amd_batch_camera_t* camera;
};
int  dlg_dense_batch_solve(const DlgBatchSolve& a);
// the fit of the ..._fit entry points (dogleg_amd_batch_fit_t, checked by the caller), the last three members of the two records
// below: loss (a featureSize <= 4 that divides M; kind and scale checked where weights is NULL), weights [B][M / featureSize],
// held [B][N]; all NULL: the call without _fit.  Host or device arrays as the record's other arrays
// The model form of the two (dogleg_amd_dense_batch_model_uncertainty, _query_covariance and their _device twins), a third form
// beside fJ / fP, both NULL then: model, the (checked) record whose arrays lie in device memory on either route, N and M those of
// the record, and its likelihood (DOGLEG_AMD_LIKELIHOOD_*, checked).  No callback runs and no x / J buffer exists; of the fit only
// held is taken.  model NULL otherwise
// dogleg_amd_dense[_products]_batch_uncertainty[_fit][_device]; fs is 1 or 2 here
struct DlgBatchUnc
{
  const double* p; unsigned int B, N, M;
  dogleg_callback_device_batch_t* fJ; dogleg_callback_device_batch_products_t* fP; void* cookie; bool unpacked;
  double *lambda, *covariance, *variances, *factors, *scale; int fs; int* status;
  const unsigned char* active; void* stream;
  bool device;
  const dogleg_amd_batch_loss_t* loss; const double* weights; const unsigned char* held;
  const dogleg_amd_batch_model_t* model; int likelihood;
  const dogleg_amd_batch_camera_t* camera;
};
int  dlg_dense_batch_uncertainty(const DlgBatchUnc& a);
// dogleg_amd_dense[_products]_batch_query_covariance[_fit][_device]; the products form has no Nobservations (< 0: the plain form)
struct DlgBatchQuery
{
  const double* p; unsigned int B, N, M;
  dogleg_callback_device_batch_t* fJ; dogleg_callback_device_batch_products_t* fP; void* cookie; bool unpacked;
  double* lambda; const double* Jq; unsigned int Nq, Qrows; int Nobservations; double* out; int* status;
  const unsigned char* active; void* stream;
  bool device;
  const dogleg_amd_batch_loss_t* loss; const double* weights; const unsigned char* held;
  const dogleg_amd_batch_model_t* model; int likelihood;
  const dogleg_amd_batch_camera_t* camera;
};
int  dlg_dense_batch_query(const DlgBatchQuery& a);
#pragma GCC visibility pop
// whether a kernel of the current device may touch [ptr, ptr + bytes): device memory of this device whose allocation covers
// the span, managed memory or registered / page-locked host memory.  Exported: the one place both pointer checks are made,
// so that they can be tested without a launch on a bad pointer
extern "C" int dlg_batch_device_span_ok(const void* ptr, size_t bytes);
// whether a camera record (dogleg.h: dogleg_amd_batch_camera_t) is one the camera calls take with this likelihood, from its members
// alone; a message under `who` where it is not.  The one statement of these rules (api_extensions.cpp), for the entry points and
// for the two camera callbacks (batch_models.hip)
bool dlg_batch_camera_ok(const char* who, const dogleg_amd_batch_camera_t* camera, int likelihood);
// the last uncertainty or query call
int  dlg_dense_batch_uncertainty_last_stats(double* out, int n);
// the device buffers, the stream, the page-locked counter and staging kept between calls (dogleg_amd_release_cache)
void dlg_dense_batch_release();
int  dlg_dense_batch_last_stats(double* out, int n);
