/* The parts of include/dogleg.h that the robust batch solve adds: the loss struct, the four kinds, the limit of the feature
 * size and the two prototypes.  Compiled as C by tests/test_dense_batch_robust_cpu.py; the one call it makes is refused. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

_Static_assert(DOGLEG_AMD_LOSS_TRIVIAL == 0 && DOGLEG_AMD_LOSS_HUBER == 1 && DOGLEG_AMD_LOSS_SOFT_L1 == 2 &&
               DOGLEG_AMD_LOSS_CAUCHY == 3, "the kinds of loss");
_Static_assert(DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE == 4, "DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE");

typedef int (*robust_fn)(double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                         const dogleg_parameters2_t*, const dogleg_amd_batch_loss_t*, dogleg_amd_batch_result_t*, double*);
typedef int (*robust_device_fn)(double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                                const dogleg_parameters2_t*, const dogleg_amd_batch_loss_t*, dogleg_amd_batch_result_t*, double*,
                                double*, const unsigned char*, void*);

static void cb(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
               void* hip_stream, void* cookie)
{ (void)p_dev; (void)x_dev; (void)J_dev; (void)live_dev; (void)B; (void)hip_stream; (void)cookie; }

int main(void)
{
  robust_fn a = &dogleg_amd_optimize_dense_batch_robust;
  robust_device_fn b = &dogleg_amd_optimize_dense_batch_robust_device;
  dogleg_amd_batch_loss_t loss = { DOGLEG_AMD_LOSS_CAUCHY, 0.5, 2 };
  dogleg_amd_batch_result_t r;
  double p[2] = {1.0, 2.0}, w[2] = {-3.0, -3.0};
  printf("%zu %zu %zu %zu\n", sizeof(dogleg_amd_batch_loss_t), offsetof(dogleg_amd_batch_loss_t, kind),
         offsetof(dogleg_amd_batch_loss_t, scale), offsetof(dogleg_amd_batch_loss_t, featureSize));
  /* Nmeas = 3 is no multiple of featureSize = 2: -1, p and the weights as they were */
  printf("%d %g %g %g %g\n", a(p, 1, 2, 3, &cb, NULL, NULL, &loss, &r, w), p[0], p[1], w[0], w[1]);
  return (a && b) ? 0 : 1;
}
