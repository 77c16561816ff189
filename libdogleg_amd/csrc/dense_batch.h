// dense_batch.h -- the batch solver of dense_batch.hip as the driver sees it (not installed).
#pragma once
#include <cstddef>
#include "../../include/dogleg.h"

// arguments checked by the caller (api_extensions.cpp: dogleg_amd_optimize_dense_batch); 0 / -1 with a message on stderr
int  dlg_dense_batch_run(double* p, unsigned int B, unsigned int N, unsigned int M,
                         dogleg_callback_device_batch_t* f, void* cookie,
                         const dogleg_parameters2_t* prm, dogleg_amd_batch_result_t* results);
// dogleg_amd_optimize_dense_batch_robust: the same with a loss (checked by the caller: kind, scale, featureSize <= 4 that
// divides M); weights: [B][M / featureSize] or NULL
int  dlg_dense_batch_robust_run(double* p, unsigned int B, unsigned int N, unsigned int M,
                                dogleg_callback_device_batch_t* f, void* cookie, const dogleg_parameters2_t* prm,
                                const dogleg_amd_batch_loss_t* loss, dogleg_amd_batch_result_t* results, double* weights);
// dogleg_amd_optimize_dense_batch_bounded: the same with box bounds (bounds given; lower / upper / held may be NULL) and,
// where loss is given, the loss (checked as above; weights NULL without it)
int  dlg_dense_batch_bounded_run(double* p, unsigned int B, unsigned int N, unsigned int M,
                                 dogleg_callback_device_batch_t* f, void* cookie, const dogleg_parameters2_t* prm,
                                 const dogleg_amd_batch_loss_t* loss, const dogleg_amd_batch_bounds_t* bounds,
                                 dogleg_amd_batch_result_t* results, double* weights);
// dogleg_amd_dense_batch_uncertainty behind the driver's checks (fs is 1 or 2 here); 0 / -1 with a message on stderr
int  dlg_dense_batch_uncertainty_run(const double* p, unsigned int B, unsigned int N, unsigned int M,
                                     dogleg_callback_device_batch_t* f, void* cookie, double* lambda, double* covariance,
                                     double* variances, double* factors, double* scale, int fs, int* status);
// the products form of the two (dogleg_amd_optimize_dense_products_batch, dogleg_amd_dense_products_batch_uncertainty): the
// layout of JtJ is prm->JtJ_packed (packed means packed upper here: the caller refused packed lower) / `unpacked`
int  dlg_dense_products_batch_run(double* p, unsigned int B, unsigned int N, dogleg_callback_device_batch_products_t* f,
                                  void* cookie, const dogleg_parameters2_t* prm, dogleg_amd_batch_result_t* results);
int  dlg_dense_products_batch_uncertainty_run(const double* p, unsigned int B, unsigned int N,
                                              dogleg_callback_device_batch_products_t* f, void* cookie, bool unpacked,
                                              double* lambda, double* covariance, double* variances, int* status);
// ---- the device-resident twins (dogleg_amd_*_batch_device): every array in device memory, active: [B] bytes or NULL,
// stream: a hipStream_t or NULL (the cache's own).  Arguments and pointers checked by the caller.  One of fJ / fP is given;
// Nmeas is 0 in the products form, whose layout of JtJ is `unpacked`
struct DlgBatchDeviceSolve
{
  double* p; unsigned int B, N, M;
  dogleg_callback_device_batch_t* fJ; dogleg_callback_device_batch_products_t* fP; void* cookie; bool unpacked;
  const dogleg_parameters2_t* prm;
  dogleg_amd_batch_result_t* results; double* lambda; const unsigned char* active; void* stream;
  const dogleg_amd_batch_loss_t* loss; double* weights;        // the robust form (J form only), or both NULL
  const dogleg_amd_batch_bounds_t* bounds;                     // the bounded form (J form only; its three pointers: device), or NULL
};
int  dlg_dense_batch_device_run(const DlgBatchDeviceSolve& a);
struct DlgBatchDeviceUnc
{
  const double* p; unsigned int B, N, M;
  dogleg_callback_device_batch_t* fJ; dogleg_callback_device_batch_products_t* fP; void* cookie; bool unpacked;
  double *lambda, *covariance, *variances, *factors, *scale; int fs; int* status;
  const unsigned char* active; void* stream;
};
int  dlg_dense_batch_uncertainty_device_run(const DlgBatchDeviceUnc& a);
// dogleg_amd_dense_batch_query_covariance and its three twins behind the driver's checks.  One of fJ / fP is given; the
// products form has M = 0 and no Nobservations (< 0: the plain form).  _run: host pointers (active and stream unused);
// _device_run: every array in device memory
struct DlgBatchQuery
{
  const double* p; unsigned int B, N, M;
  dogleg_callback_device_batch_t* fJ; dogleg_callback_device_batch_products_t* fP; void* cookie; bool unpacked;
  double* lambda; const double* Jq; unsigned int Nq, Qrows; int Nobservations; double* out; int* status;
  const unsigned char* active; void* stream;
};
int  dlg_dense_batch_query_run(const DlgBatchQuery& a);
int  dlg_dense_batch_query_device_run(const DlgBatchQuery& a);
// whether a kernel of the current device may touch [ptr, ptr + bytes): device memory of this device whose allocation covers
// the span, managed memory or registered / page-locked host memory.  Exported: the one place both pointer checks are made,
// so that they can be tested without a launch on a bad pointer
extern "C" int dlg_batch_device_span_ok(const void* ptr, size_t bytes);
// the last call of either form
int  dlg_dense_batch_uncertainty_last_stats(double* out, int n);
// the device buffers, the stream, the page-locked counter and staging kept between calls (dogleg_amd_release_cache)
void dlg_dense_batch_release();
int  dlg_dense_batch_last_stats(double* out, int n);
