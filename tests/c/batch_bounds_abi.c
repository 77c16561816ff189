/* The parts of include/dogleg.h that the bounded batch solve adds: the bounds struct (three pointers) and the two prototypes.
 * Compiled as C by tests/test_dense_batch_bounds_cpu.py; the two calls it makes are refused. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

typedef int (*bounded_fn)(double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                          const dogleg_parameters2_t*, const dogleg_amd_batch_loss_t*, const dogleg_amd_batch_bounds_t*,
                          dogleg_amd_batch_result_t*, double*);
typedef int (*bounded_device_fn)(double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                                 const dogleg_parameters2_t*, const dogleg_amd_batch_loss_t*, const dogleg_amd_batch_bounds_t*,
                                 dogleg_amd_batch_result_t*, double*, double*, const unsigned char*, void*);

static void cb(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
               void* hip_stream, void* cookie)
{ (void)p_dev; (void)x_dev; (void)J_dev; (void)live_dev; (void)B; (void)hip_stream; (void)cookie; }

int main(void)
{
  bounded_fn a = &dogleg_amd_optimize_dense_batch_bounded;
  bounded_device_fn b = &dogleg_amd_optimize_dense_batch_bounded_device;
  const double lower[2] = {0.0, 0.0}, upper[2] = {3.0, 3.0};
  unsigned char held[2] = {9, 9};
  dogleg_amd_batch_bounds_t bounds = { lower, upper, held };
  /* the members are pointers of these types */
  const double** pl = &bounds.lower; const double** pu = &bounds.upper; unsigned char** ph = &bounds.held;
  dogleg_amd_batch_result_t r;
  double p[2] = {1.0, 2.0}, w[3] = {-3.0, -3.0, -3.0};
  printf("%zu %zu %zu %zu %zu\n", sizeof(dogleg_amd_batch_bounds_t), offsetof(dogleg_amd_batch_bounds_t, lower),
         offsetof(dogleg_amd_batch_bounds_t, upper), offsetof(dogleg_amd_batch_bounds_t, held), sizeof(void*));
  /* a NULL bounds, then weights without a loss: -1, p, held and the weights as they were */
  printf("%d %d %g %g %d %d %g\n", a(p, 1, 2, 3, &cb, NULL, NULL, NULL, NULL, &r, NULL),
         a(p, 1, 2, 3, &cb, NULL, NULL, NULL, &bounds, &r, w), p[0], p[1], held[0], held[1], w[0]);
  return (a && b && *pl == lower && *pu == upper && *ph == held) ? 0 : 1;
}
