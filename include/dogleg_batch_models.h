/* dogleg_batch_models.h -- the built-in fit models of the batch solver (dogleg_amd_batch_model_t in dogleg.h): one row of the
 * residual x and of its Jacobian J, from the parameters, one datum and one abscissa.  One function for the host and the device;
 * the adapter callback (dogleg_amd_batch_model_callback) and the fused sweep of dogleg_amd_optimize_dense_batch_model both go
 * through it, which is why the two routes give the same bits: the order of the operations is fixed below and nothing here may be
 * contracted into a fused multiply-add or reassociated, whatever the flags of the translation unit.  clang (hipcc: host and
 * device) is told so by the pragma; with another compiler use -ffp-contract=off.
 *
 *   x_i = s_i (f_i(p) - y_i),   J_ij = s_i d f_i / d p_j,   s_i = 1 without a scale
 *
 *   EXPDECAY          N = 3   p = A, k, c                   f_i = A exp(-k t_i) + c
 *   GAUSS1D           N = 4   p = A, mu, sigma, c           f_i = A exp(-(t_i - mu)^2 / (2 sigma^2)) + c
 *   GAUSS2D           N = 5   p = A, x0, y0, sigma, c       row i is pixel (ix, iy) = (i mod width, i div width), centres on the
 *                                                           integers: f_i = A exp(-((ix - x0)^2 + (iy - y0)^2) / (2 sigma^2)) + c
 *   GAUSS2D_ELLIPTIC  N = 6   p = A, x0, y0, sx, sy, c      f_i = A exp(-(ix - x0)^2 / (2 sx^2) - (iy - y0)^2 / (2 sy^2)) + c
 *
 * The Gaussians divide once, 1 / sigma, and work on z = (t - mu) / sigma: a sigma of exactly 0 gives a non-finite row. */
#ifndef DOGLEG_BATCH_MODELS_H
#define DOGLEG_BATCH_MODELS_H

#if defined(__HIPCC__)
#define DOGLEG_BATCH_MODEL_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#include <math.h>
#define DOGLEG_BATCH_MODEL_FN static inline
#endif

#define DOGLEG_BATCH_MODEL_EXPDECAY         0     /* = DOGLEG_AMD_MODEL_EXPDECAY */
#define DOGLEG_BATCH_MODEL_GAUSS1D          1     /* = DOGLEG_AMD_MODEL_GAUSS1D */
#define DOGLEG_BATCH_MODEL_GAUSS2D          2     /* = DOGLEG_AMD_MODEL_GAUSS2D */
#define DOGLEG_BATCH_MODEL_GAUSS2D_ELLIPTIC 3     /* = DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC */
#define DOGLEG_BATCH_MODEL_MAX_NSTATE       6

/* the number of parameters of a kind, -1 for an unknown one */
DOGLEG_BATCH_MODEL_FN int dogleg_batch_model_nstate(int kind)
{
  return kind == DOGLEG_BATCH_MODEL_EXPDECAY ? 3 : kind == DOGLEG_BATCH_MODEL_GAUSS1D ? 4 :
         kind == DOGLEG_BATCH_MODEL_GAUSS2D ? 5 : kind == DOGLEG_BATCH_MODEL_GAUSS2D_ELLIPTIC ? 6 : -1;
}

/* row i of a problem: p the N parameters, t the abscissa t_i (the 1D kinds; not read by the 2D kinds), width that of the window
 * (the 2D kinds; not read by the 1D kinds), y the datum y_i, s the scale s_i (1 without one).  *x gets x_i, J[0 .. N-1] row i of
 * J; J has room for DOGLEG_BATCH_MODEL_MAX_NSTATE doubles whatever the kind, and those behind N - 1 are written as 0 (the six
 * stores are unconditional, so that on the device the row stays in registers).  An unknown kind writes nothing.  Every kind
 * evaluates one exponential, e = exp(u): what leads to u comes first, then what every kind shares (x_i and the derivative with
 * respect to A), then the other derivatives. */
DOGLEG_BATCH_MODEL_FN void dogleg_batch_model_row(int kind, const double* p, int i, int width, double t, double y, double s,
                                                  double* x, double* J)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  /* A, c: amplitude and offset; z0, z1: (abscissa - centre) / width per axis (EXPDECAY: z0 = t); q0, q1: their squares */
  double A, c, u, inv0 = 0.0, inv1 = 0.0, z0 = 0.0, z1 = 0.0, q0 = 0.0, q1 = 0.0;
  switch(kind)
  {
  case DOGLEG_BATCH_MODEL_EXPDECAY:
  {
    const double kt = p[1] * t;
    A = p[0]; c = p[2];
    z0 = t;
    u = -kt;
    break;
  }
  case DOGLEG_BATCH_MODEL_GAUSS1D:
  {
    const double d = t - p[1];
    A = p[0]; c = p[3];
    inv0 = 1.0 / p[2];
    z0 = d * inv0;
    q0 = z0 * z0;
    u = -0.5 * q0;
    break;
  }
  case DOGLEG_BATCH_MODEL_GAUSS2D:
  {
    const int iy = i / width, ix = i - iy * width;
    const double dx = (double)ix - p[1];
    const double dy = (double)iy - p[2];
    A = p[0]; c = p[4];
    inv0 = 1.0 / p[3];
    z0 = dx * inv0;
    z1 = dy * inv0;
    q0 = z0 * z0;
    q1 = z1 * z1;
    const double q = q0 + q1;
    u = -0.5 * q;
    break;
  }
  case DOGLEG_BATCH_MODEL_GAUSS2D_ELLIPTIC:
  {
    const int iy = i / width, ix = i - iy * width;
    const double dx = (double)ix - p[1];
    const double dy = (double)iy - p[2];
    A = p[0]; c = p[5];
    inv0 = 1.0 / p[3];
    inv1 = 1.0 / p[4];
    z0 = dx * inv0;
    z1 = dy * inv1;
    q0 = z0 * z0;
    q1 = z1 * z1;
    const double q = q0 + q1;
    u = -0.5 * q;
    break;
  }
  default:
    return;
  }
  const double e  = exp(u);
  const double Ae = A * e;
  const double f  = Ae + c;
  const double r  = f - y;
  double j1, j2, j3 = 0.0, j4 = 0.0, j5 = 0.0;
  switch(kind)
  {
  case DOGLEG_BATCH_MODEL_EXPDECAY:
  {
    /* d/dk = -A t e */
    const double At = A * z0;
    const double dk = At * e;
    j1 = s * (-dk);
    j2 = s;
    break;
  }
  case DOGLEG_BATCH_MODEL_GAUSS1D:
  {
    /* d/dmu = A e z / sigma, d/dsigma = A e z^2 / sigma */
    const double Aei = Ae * inv0;
    const double dmu = Aei * z0;
    const double ds  = Aei * q0;
    j1 = s * dmu;
    j2 = s * ds;
    j3 = s;
    break;
  }
  case DOGLEG_BATCH_MODEL_GAUSS2D:
  {
    /* d/dx0 = A e zx / sigma, d/dy0 = A e zy / sigma, d/dsigma = A e (zx^2 + zy^2) / sigma */
    const double Aei = Ae * inv0;
    const double gx  = Aei * z0;
    const double gy  = Aei * z1;
    const double q   = q0 + q1;
    const double gs  = Aei * q;
    j1 = s * gx;
    j2 = s * gy;
    j3 = s * gs;
    j4 = s;
    break;
  }
  default:
  {
    /* GAUSS2D_ELLIPTIC: d/dx0 = A e zx / sx, d/dy0 = A e zy / sy, d/dsx = A e zx^2 / sx, d/dsy = A e zy^2 / sy */
    const double Aex = Ae * inv0;
    const double Aey = Ae * inv1;
    const double gx  = Aex * z0;
    const double gy  = Aey * z1;
    const double gsx = Aex * q0;
    const double gsy = Aey * q1;
    j1 = s * gx;
    j2 = s * gy;
    j3 = s * gsx;
    j4 = s * gsy;
    j5 = s;
    break;
  }
  }
  *x = s * r;
  J[0] = s * e;
  J[1] = j1; J[2] = j2; J[3] = j3; J[4] = j4; J[5] = j5;
}

/* row i of a problem under the Poisson likelihood (dogleg.h: DOGLEG_AMD_LIKELIHOOD_POISSON): y a count >= 0, no scale.
 *
 *   q_i = 1 / sqrt(f_i),   *x = (f_i - y_i) q_i,   J[j] = (d f_i / d p_j) q_i,
 *   *d  = 2 ((f_i - y_i) - y_i log(f_i / y_i)),    2 f_i where y_i == 0.0           (the row's share of the deviance)
 *
 * so that J'x = sum (r / f) grad f is half the gradient of the deviance and J'J = sum grad f grad f' / f the Fisher information.
 * f_i and its gradient come from dogleg_batch_model_row with y = 0 and s = 1, with the bits they have there; then, in this order
 * and uncontracted: r = f - y, sqrt(f), q = 1 / sqrt(f), the products with q, f / y, one log, y log, r - y log, times 2.  The
 * test is y == 0.0 and not y > 0: a NaN datum reaches the logarithm, a negative one makes it NaN.
 * Returns whether the row is feasible, f_i > 0.  An infeasible row (a NaN f included) gets *x = *d = NaN and a J of NaN: what is
 * done with it is the caller's rule (the fused sweep stages zeros and makes the cost +infinity, the Fisher callback writes the
 * NaN).  An unknown kind writes nothing and returns 0. */
DOGLEG_BATCH_MODEL_FN int dogleg_batch_model_row_poisson(int kind, const double* p, int i, int width, double t, double y,
                                                         double* x, double* J, double* d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double f = 0.0;
  if(dogleg_batch_model_nstate(kind) < 0) return 0;
  dogleg_batch_model_row(kind, p, i, width, t, 0.0, 1.0, &f, J);
  const int feasible = f > 0.0;
  const double r  = f - y;
  const double sf = sqrt(f);
  const double q  = feasible ? 1.0 / sf : NAN;
  const double xq = r * q;
  J[0] = J[0] * q; J[1] = J[1] * q; J[2] = J[2] * q; J[3] = J[3] * q; J[4] = J[4] * q; J[5] = J[5] * q;
  double dev;
  if(y == 0.0) dev = f;
  else
  {
    const double fy = f / y;
    const double lg = log(fy);
    const double yl = y * lg;
    dev = r - yl;
  }
  *x = xq;
  *d = feasible ? 2.0 * dev : NAN;
  return feasible;
}

/* one datum of a camera record (dogleg.h: dogleg_amd_batch_camera_t) from a raw reading already converted to double (the
 * conversions of float and of a 16-bit integer are exact) and the three calibration values of its sensor pixel:
 *
 *   *y = (raw - (double)offset) * (double)gain_inv   photoelectrons,   *v = (double)readvar   photoelectrons^2
 *
 * one subtraction and one product, uncontracted.  Without calibration pass offset = 0, gain_inv = 1, readvar = 0: *y has the bits of
 * raw then (a -0.0 becomes +0.0 under the subtraction, which no later comparison tells apart). */
DOGLEG_BATCH_MODEL_FN void dogleg_batch_camera_datum(double raw, float offset, float gain_inv, float readvar, double* y, double* v)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double o = (double)offset;
  const double g = (double)gain_inv;
  const double e = raw - o;
  *y = e * g;
  *v = (double)readvar;
}

/* row i of a problem under the Poisson likelihood with read noise (the sCMOS estimator of Huang et al. 2013: the variance v of the
 * Gaussian read noise, in photoelectrons^2, added to the datum and to the model, so that y + v is again nearly Poisson with the
 * expectation f + v).  With f' = f_i + v and y' = max(y_i + v, 0):
 *
 *   q_i = 1 / sqrt(f'),   *x = (f' - y') q_i,   J[j] = (d f_i / d p_j) q_i,
 *   *d  = 2 ((f' - y') - y' log(f' / y')),      2 f' where y' == 0.0
 *
 * f_i and its gradient come from dogleg_batch_model_row with y = 0 and s = 1; then, in this order and uncontracted: f' = f + v,
 * y' = y + v, the clamp y' = y' < 0.0 ? 0.0 : y' (a comparison, not fmax: a NaN datum stays NaN and fails the problem as it does
 * without read noise; a reading below the offset by more than v counts as no photon), the test f' > 0, r = f' - y', sqrt(f'),
 * q = 1 / sqrt(f'), the products with q, f' / y', one log, y' log, r - y' log, times 2.
 * Returns whether the row is feasible, f' > 0; an infeasible row gets *x = *d = NaN and a J of NaN, as in
 * dogleg_batch_model_row_poisson.  With v == 0 and a y that is >= 0 or NaN every output has the bits of that function: f + 0 and
 * y + 0 change no bit that is read later (-0.0 becomes +0.0, equal in every comparison and under f - y; an f of -0.0 is infeasible
 * either way).  An unknown kind writes nothing and returns 0. */
DOGLEG_BATCH_MODEL_FN int dogleg_batch_model_row_poisson_v(int kind, const double* p, int i, int width, double t, double y, double v,
                                                           double* x, double* J, double* d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double f = 0.0;
  if(dogleg_batch_model_nstate(kind) < 0) return 0;
  dogleg_batch_model_row(kind, p, i, width, t, 0.0, 1.0, &f, J);
  const double fv = f + v;
  const double ys = y + v;
  const double yv = ys < 0.0 ? 0.0 : ys;
  const int feasible = fv > 0.0;
  const double r  = fv - yv;
  const double sf = sqrt(fv);
  const double q  = feasible ? 1.0 / sf : NAN;
  const double xq = r * q;
  J[0] = J[0] * q; J[1] = J[1] * q; J[2] = J[2] * q; J[3] = J[3] * q; J[4] = J[4] * q; J[5] = J[5] * q;
  double dev;
  if(yv == 0.0) dev = fv;
  else
  {
    const double fy = fv / yv;
    const double lg = log(fy);
    const double yl = yv * lg;
    dev = r - yl;
  }
  *x = xq;
  *d = feasible ? 2.0 * dev : NAN;
  return feasible;
}
#endif
