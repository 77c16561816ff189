/* The parts of include/dogleg.h that the device-resident batch entry points make ABI: the layout of
 * dogleg_amd_batch_result_t (a kernel writes it as an array of structs), the two status codes of a problem that is not
 * run, and the four prototypes.  Compiled as C by tests/test_dense_batch_device_cpu.py; it only links, it calls nothing. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

_Static_assert(sizeof(dogleg_amd_batch_result_t) == 40, "dogleg_amd_batch_result_t is 40 bytes");
_Static_assert(offsetof(dogleg_amd_batch_result_t, norm2_x) == 0, "norm2_x");
_Static_assert(offsetof(dogleg_amd_batch_result_t, trustregion) == 8, "trustregion");
_Static_assert(offsetof(dogleg_amd_batch_result_t, lambda) == 16, "lambda");
_Static_assert(offsetof(dogleg_amd_batch_result_t, iterations) == 24, "iterations");
_Static_assert(offsetof(dogleg_amd_batch_result_t, evaluations) == 28, "evaluations");
_Static_assert(offsetof(dogleg_amd_batch_result_t, status) == 32, "status");
_Static_assert(DOGLEG_AMD_BATCH_NOT_RUN == 0, "DOGLEG_AMD_BATCH_NOT_RUN");
_Static_assert(DOGLEG_AMD_BATCH_UNC_SKIPPED == 2, "DOGLEG_AMD_BATCH_UNC_SKIPPED");

typedef int (*solve_fn)(double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                        const dogleg_parameters2_t*, dogleg_amd_batch_result_t*, double*, const unsigned char*, void*);
typedef int (*solve_products_fn)(double*, unsigned int, unsigned int, dogleg_callback_device_batch_products_t*, void*,
                                 const dogleg_parameters2_t*, dogleg_amd_batch_result_t*, double*, const unsigned char*, void*);
typedef int (*unc_fn)(const double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                      double*, double*, double*, double*, double*, int, int*, const unsigned char*, void*);
typedef int (*unc_products_fn)(const double*, unsigned int, unsigned int, dogleg_callback_device_batch_products_t*, void*,
                               const dogleg_parameters2_t*, double*, double*, double*, int*, const unsigned char*, void*);

int main(void)
{
  solve_fn a = &dogleg_amd_optimize_dense_batch_device;
  solve_products_fn b = &dogleg_amd_optimize_dense_products_batch_device;
  unc_fn c = &dogleg_amd_dense_batch_uncertainty_device;
  unc_products_fn d = &dogleg_amd_dense_products_batch_uncertainty_device;
  printf("%zu %d %d\n", sizeof(dogleg_amd_batch_result_t), DOGLEG_AMD_BATCH_NOT_RUN, DOGLEG_AMD_BATCH_UNC_SKIPPED);
  return (a && b && c && d) ? 0 : 1;
}
