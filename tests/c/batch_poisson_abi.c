/* The parts of include/dogleg.h that the Poisson fit of the built-in models adds: the likelihoods' values and the prototypes.
 * Compiled as C by tests/test_dense_batch_poisson_cpu.py from dogleg.h alone; the calls it makes are refused. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

typedef int (*mle_fn)(double*, unsigned int, const dogleg_amd_batch_model_t*, int, const dogleg_parameters2_t*,
                      const dogleg_amd_batch_bounds_t*, dogleg_amd_batch_result_t*);
typedef int (*mle_device_fn)(double*, unsigned int, const dogleg_amd_batch_model_t*, int, const dogleg_parameters2_t*,
                             const dogleg_amd_batch_bounds_t*, dogleg_amd_batch_result_t*, double*, const unsigned char*, void*);

_Static_assert(DOGLEG_AMD_LIKELIHOOD_GAUSS == 0 && DOGLEG_AMD_LIKELIHOOD_POISSON == 1, "the likelihoods");
_Static_assert(sizeof(dogleg_amd_batch_model_t) == 48, "the record did not grow");

int main(void)
{
  mle_fn a = &dogleg_amd_optimize_dense_batch_model_mle;
  mle_device_fn b = &dogleg_amd_optimize_dense_batch_model_mle_device;
  dogleg_callback_device_batch_t* cb = &dogleg_amd_batch_model_fisher_callback;
  const double y[4] = {1.0, 2.0, 3.0, 4.0};
  dogleg_amd_batch_model_t m = { DOGLEG_AMD_MODEL_EXPDECAY, 4, 0, 0, y, NULL, y, 0 };
  dogleg_amd_batch_result_t r;
  double p[3] = {1.0, 2.0, 3.0}, lam[1] = {-3.0};
  /* an unknown likelihood on both entry points, then a scale with POISSON: -1, p and lambda as they were */
  printf("%d %d %d %g %g %g\n", a(p, 1, &m, 2, NULL, NULL, &r), b(p, 1, &m, -1, NULL, NULL, &r, lam, NULL, NULL),
         a(p, 1, &m, DOGLEG_AMD_LIKELIHOOD_POISSON, NULL, NULL, &r), p[0], p[2], lam[0]);
  return (a && b && cb) ? 0 : 1;
}
