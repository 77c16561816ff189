/* dogleg_numeric_step.h -- the step rule of the numeric Jacobians of a batch (dogleg_amd_batch_numeric_* in dogleg.h): where a
 * variable is evaluated for its difference quotient, and what the quotient divides by.  One function for the host and the
 * device; the library's kernels, the naive reference of problems/device_batch_values.hip and the exported
 * dogleg_amd_numeric_step all go through it, and tests/batch_numeric_oracle.py restates it in numpy bit for bit.  That holds
 * only while every operation below is rounded on its own: nothing here may be contracted into a fused multiply-add or
 * reassociated.  clang (hipcc: host and device) is told so by the pragma; with another compiler use -ffp-contract=off.
 *
 *   h = delta_rel |p| + delta_abs
 *   forward: tp = p + h; where tp > hi: tp = max(p - h, lo).            d = tp - p,  J = (x(tp) - x(p)) / d
 *   central: tp = min(p + h, hi), tm = max(p - h, lo).                  d = tp - tm, J = (x(tp) - x(tm)) / d
 * so no point outside [lo, hi] is evaluated while p itself lies inside, a central difference is one-sided by itself on a
 * bound, and d == 0 (lo == hi) stands for a column of exact zeros.  max(a, lo) is a < lo ? lo : a and min(a, hi) is
 * a > hi ? hi : a: a NaN p gives NaN points and a NaN divisor.  lo = -inf, hi = +inf: no bounds. */
#ifndef DOGLEG_NUMERIC_STEP_H
#define DOGLEG_NUMERIC_STEP_H

#if defined(__HIPCC__)
#define DOGLEG_NUMERIC_STEP_FN __host__ __device__ static inline
#else
#define DOGLEG_NUMERIC_STEP_FN static inline
#endif

#define DOGLEG_NUMERIC_STEP_FORWARD 0     /* = DOGLEG_AMD_NUMERIC_FORWARD */
#define DOGLEG_NUMERIC_STEP_CENTRAL 1     /* = DOGLEG_AMD_NUMERIC_CENTRAL */
/* the defaults of delta_rel and delta_abs: 2^-26 ~ sqrt(eps) forward, 2^-17 ~ cbrt(eps) central */
#define DOGLEG_NUMERIC_DELTA_FORWARD 1.490116119384765625e-08
#define DOGLEG_NUMERIC_DELTA_CENTRAL 7.62939453125e-06

/* *tp: the plus point, *tm: the minus point (forward: p itself), *d: the divisor */
DOGLEG_NUMERIC_STEP_FN void dogleg_numeric_step(int scheme, double p, double lo, double hi, double delta_rel, double delta_abs,
                                                double* tp, double* tm, double* d)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double ap  = __builtin_fabs(p);
  const double rel = delta_rel * ap;
  const double h   = rel + delta_abs;
  const double up  = p + h;
  const double dn  = p - h;
  if(scheme == DOGLEG_NUMERIC_STEP_CENTRAL)
  {
    const double a = up > hi ? hi : up;
    const double b = dn < lo ? lo : dn;
    *tp = a; *tm = b; *d = a - b;
  }
  else
  {
    double a = up;
    if(up > hi) a = dn < lo ? lo : dn;
    *tp = a; *tm = p; *d = a - p;
  }
}
#endif
