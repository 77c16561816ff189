/* The parts of include/dogleg.h that the bounded products batch solve adds: the two prototypes, on the bounds struct of the J form.
 * Compiled as C by tests/test_dense_products_batch_bounds_cpu.py; the three calls it makes are refused. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

typedef int (*bounded_fn)(double*, unsigned int, unsigned int, dogleg_callback_device_batch_products_t*, void*,
                          const dogleg_parameters2_t*, const dogleg_amd_batch_bounds_t*, dogleg_amd_batch_result_t*);
typedef int (*bounded_device_fn)(double*, unsigned int, unsigned int, dogleg_callback_device_batch_products_t*, void*,
                                 const dogleg_parameters2_t*, const dogleg_amd_batch_bounds_t*, dogleg_amd_batch_result_t*,
                                 double*, const unsigned char*, void*);

static void cb(const double* p_dev, double* norm2x_dev, double* xtJ_dev, double* JtJ_dev, const unsigned char* live_dev,
               unsigned int B, void* hip_stream, void* cookie)
{ (void)p_dev; (void)norm2x_dev; (void)xtJ_dev; (void)JtJ_dev; (void)live_dev; (void)B; (void)hip_stream; (void)cookie; }

int main(void)
{
  bounded_fn a = &dogleg_amd_optimize_dense_products_batch_bounded;
  bounded_device_fn b = &dogleg_amd_optimize_dense_products_batch_bounded_device;
  const double lower[2] = {0.0, 0.0}, upper[2] = {3.0, 3.0};
  unsigned char held[2] = {9, 9};
  dogleg_amd_batch_bounds_t bounds = { lower, upper, held };
  dogleg_amd_batch_result_t r;
  double p[2] = {1.0, 2.0}, lam[1] = {-3.0};
  /* a NULL bounds on both entry points, then no variables: -1, p, held and lambda as they were */
  printf("%d %d %d %g %g %d %d %g\n", a(p, 1, 2, &cb, NULL, NULL, NULL, &r),
         b(p, 1, 2, &cb, NULL, NULL, NULL, &r, lam, NULL, NULL), a(p, 1, 0, &cb, NULL, NULL, &bounds, &r), p[0], p[1], held[0],
         held[1], lam[0]);
  return (a && b) ? 0 : 1;
}
