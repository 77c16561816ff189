/* The parts of include/dogleg.h that the built-in batch models add: the record's layout, the kinds' values and the prototypes.
 * Compiled as C by tests/test_dense_batch_model_cpu.py from dogleg.h alone; the calls it makes are refused. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

typedef int (*model_fn)(double*, unsigned int, const dogleg_amd_batch_model_t*, const dogleg_parameters2_t*,
                        const dogleg_amd_batch_bounds_t*, dogleg_amd_batch_result_t*);
typedef int (*model_device_fn)(double*, unsigned int, const dogleg_amd_batch_model_t*, const dogleg_parameters2_t*,
                               const dogleg_amd_batch_bounds_t*, dogleg_amd_batch_result_t*, double*, const unsigned char*, void*);

_Static_assert(DOGLEG_AMD_MODEL_EXPDECAY == 0 && DOGLEG_AMD_MODEL_GAUSS1D == 1 && DOGLEG_AMD_MODEL_GAUSS2D == 2 &&
               DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC == 3, "the kinds");
_Static_assert(offsetof(dogleg_amd_batch_model_t, kind) == 0 && offsetof(dogleg_amd_batch_model_t, Nmeas) == 4 &&
               offsetof(dogleg_amd_batch_model_t, width) == 8 && offsetof(dogleg_amd_batch_model_t, height) == 12 &&
               offsetof(dogleg_amd_batch_model_t, y) == 16 && offsetof(dogleg_amd_batch_model_t, t) == 24 &&
               offsetof(dogleg_amd_batch_model_t, scale) == 32 && offsetof(dogleg_amd_batch_model_t, t_per_problem) == 40 &&
               sizeof(dogleg_amd_batch_model_t) == 48, "the record");

int main(void)
{
  model_fn a = &dogleg_amd_optimize_dense_batch_model;
  model_device_fn b = &dogleg_amd_optimize_dense_batch_model_device;
  dogleg_callback_device_batch_t* cb = &dogleg_amd_batch_model_callback;
  unsigned long long (*count)(void) = &dogleg_amd_batch_model_callback_invocations;
  const double y[4] = {1.0, 2.0, 3.0, 4.0};
  dogleg_amd_batch_model_t m = { DOGLEG_AMD_MODEL_GAUSS2D, 4, 2, 3, y, NULL, NULL, 0 };
  dogleg_amd_batch_result_t r;
  double p[5] = {1.0, 2.0, 3.0, 4.0, 5.0}, lam[1] = {-3.0};
  /* a NULL model on both entry points, then a window that is not Nmeas: -1, p and lambda as they were */
  printf("%d %d %d %g %g %g\n", a(p, 1, NULL, NULL, NULL, &r), b(p, 1, NULL, NULL, NULL, &r, lam, NULL, NULL),
         a(p, 1, &m, NULL, NULL, &r), p[0], p[4], lam[0]);
  printf("%d %d %d %d %d %llu\n", dogleg_amd_batch_model_nstate(DOGLEG_AMD_MODEL_EXPDECAY),
         dogleg_amd_batch_model_nstate(DOGLEG_AMD_MODEL_GAUSS1D), dogleg_amd_batch_model_nstate(DOGLEG_AMD_MODEL_GAUSS2D),
         dogleg_amd_batch_model_nstate(DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC), dogleg_amd_batch_model_nstate(4), count());
  return (a && b && cb) ? 0 : 1;
}
