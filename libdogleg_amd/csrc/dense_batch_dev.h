// dense_batch_dev.h -- what the host code of the batch solver (dense_batch.hip) and its kernels (dense_batch_kernels.hip)
// share: the kernels' argument structs, the indices of the per-problem state and the launchers (internal, not installed).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/dogleg.h"

// per-problem state: sc [B][SC_COUNT] doubles, st [B][ST_COUNT] ints
enum { SC_N2X, SC_TR, SC_LAMBDA, SC_N2C, SC_N2GN, SC_EI, SC_COUNT = 8 };
enum { ST_FLAGS, ST_ITER, ST_EVAL, ST_STATUS, ST_COUNT = 4 };

// what a products callback wrote: norm2(x) [B], Jt x [B][N], JtJ [B][S]; unpacked: S = N^2 row-major, of which the
// entries [i][j], j >= i, are read; otherwise S = NP, row-major packed upper = the kernels' packed lower column-major.
// All nullptr in the J form: that is how the launchers tell the forms apart
struct ProductsDev
{
  const double* n2x; const double* xtJ; const double* JtJ;
  int unpacked;
};

// the loss of a robust solve: c = a^2, fs rows a feature
struct LossDev { int kind, fs; double a, c; };

// a built-in model (dogleg.h: dogleg_amd_batch_model_t) as the fused sweep reads it: y [B][M]; t nullptr (t_i = i), [M] or, with
// t_each, [B][M]; scale [B][M] or nullptr.  y == nullptr: no model, and that is how the launcher tells this form from the others.
// likelihood: DOGLEG_AMD_LIKELIHOOD_* (it lies where the three ints left a hole in front of the pointers, so that every other
// member of BatchDev stays where it was); read by the launcher only: POISSON is a form of its own
struct ModelDev
{
  int kind, width, t_each, likelihood;
  const double *y, *t, *scale;
};

// the data source of a camera record (dogleg.h: dogleg_amd_batch_camera_t) beside the ModelDev of its model, whose y is nullptr
// then: raw [B][M] readings of dtype (DOGLEG_AMD_DATA_*).  cal != 0: offset, gain_inv, readvar (or nullptr: 0) maps of sw floats a
// row, origin [B][2] ints, and the largest origin at which the window lies on the sensor: xmax = sw - width, ymax = sh - height,
// both >= 0.  raw == nullptr: no camera.  A record of its own behind ModelDev (BatchDev) and behind the points (ModelEvalDev), so
// that every member the other forms read lies where it did.  A camera record of doubles without calibration is no camera here: its
// raw is the model's y
struct CameraDev
{
  const void* raw; const float *offset, *gain_inv, *readvar; const int* origin;
  int dtype, sw, xmax, ymax, cal;
};

struct BatchDev
{
  int B, N, M, NP;
  const double* x; const double* J;
  double *p_before, *p_trial, *g, *cauchy, *gn, *JtJ, *sc;
  int* st; unsigned char* live; int* counter;
  int max_iterations;
  double trustregion0, dec_factor, dec_thr, inc_factor, inc_thr, jtx_thr, upd_thr, tr_thr;
  ProductsDev P;               // FORM_PRODUCTS (x, J, M unused there)
  LossDev L; int NF; double* wts;      // the robust form: NF = M / L.fs features, rho' at the point stepped from [B][NF]
  int robust;                  // (host side: which kernel is launched)
  // the bounded form (behind everything above: the other kernels read their arguments where they did): lo, hi [B][N] or nullptr
  // (no bound on that side), held [B][N] out or nullptr
  const double *lo, *hi; unsigned char* held;
  int bounded;                 // (host side: which kernel is launched)
  ModelDev Mdl;                // FORM_MODEL (x, J, P unused there), behind everything above
  CameraDev Cam;               // the camera forms, behind everything above
};

struct UncDev
{
  int B, N, M, NP, fs, NF;
  const double* x; const double* J;
  double *lam, *scale, *cov, *var, *fac;     // cov, var, fac (and scale with fac): nullptr where not asked for
  int* status;
  ProductsDev P;               // FORM_PRODUCTS (x, J, M, fs, NF unused there; fac and scale nullptr: they need J)
  const unsigned char* active; // [B] or nullptr (all): 0: problem b is skipped, only its status is written
};
// the fit of the ..._fit forms of the uncertainty and query calls (dogleg.h: dogleg_amd_batch_fit_t), a kernel argument of its own
// behind UncDev / QueryDev, so that the kernels without a fit read their arguments where they did.  L.fs rows a weight feature;
// wts [B][M / L.fs] or nullptr: w_f = rho'(s_f) from L at the callback's x (L.kind TRIVIAL: 1); held [B][N] or nullptr
struct FitDev
{
  LossDev L; const double* wts; const unsigned char* held;
  int fit;                     // (host side: which kernel is launched)
};

// the built-in model of the fused uncertainty and query calls (dogleg_amd_dense_batch_model_uncertainty, _query_covariance): the
// record and the points p [B][N] the rows are formed at, a kernel argument of its own behind FitDev, so that UncDev, QueryDev and
// FitDev lie where they did.  Mdl.y == nullptr: no model (the J and the products form, which do not read this argument); that is
// how the launchers tell the forms apart
struct ModelEvalDev
{
  ModelDev Mdl; const double* p;
  CameraDev Cam;
};

struct QueryDev
{
  UncDev U;                    // B, N, M, NP, x, J, P, lam, status, active; cov, var, fac, scale: nullptr
  const double* Jq;            // [B][Nq][Q][N]
  double* out;                 // [B][Nq][Q][Q]
  int Nq, Q, nobs;             // nobs < 0: the plain form
};

// 0 free, 1 held at lower, 2 held at upper: the held set at a point with the g of that point (held_mask, per element)
__host__ __device__ inline unsigned char held_code(double p, double g, double lo, double hi)
{
  return p == lo && g > 0.0 ? 1 : p == hi && g < 0.0 ? 2 : 0;
}

// ---- the launchers (dense_batch_kernels.hip): one launch each on st, the instantiation chosen from what the record says (the
// size class of N, the form, robust, bounded, fit).  The caller asks hipGetLastError
#pragma GCC visibility push(hidden)
void launch_batch_round(hipStream_t st, const BatchDev& A);
void launch_batch_uncertainty(hipStream_t st, const UncDev& A, const FitDev& F, const ModelEvalDev& E);
void launch_batch_query(hipStream_t st, const QueryDev& A, const FitDev& F, const ModelEvalDev& E);
// active: [B] or nullptr (all): the initial live bytes
void launch_batch_init(hipStream_t st, const BatchDev& A, const unsigned char* active);
void launch_batch_clamp(hipStream_t st, const BatchDev& A);
// the end of a device-resident solve, into the caller's device arrays (lambda, weights: or nullptr)
void launch_batch_finish(hipStream_t st, const BatchDev& A, double* p, dogleg_amd_batch_result_t* results, double* lambda,
                         double* weights);
#pragma GCC visibility pop
