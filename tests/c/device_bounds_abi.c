/* device_bounds_abi.c -- dogleg_amd_optimize_device2_bounded as a C user compiles against it (tests/test_device_bounds_cpu.py):
 * takes the address of the entry point under its prototype and calls it with arguments it refuses on the host (no GPU needed);
 * prints the return values and whether p, weights and held kept their bits. */
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "dogleg.h"

typedef double (*bounded_fn)(double*, unsigned int, unsigned int, unsigned int, const int*, const int*, dogleg_callback_device_t*,
                             void*, const dogleg_amd_batch_loss_t*, double*, const dogleg_amd_batch_bounds_t*,
                             const dogleg_parameters2_t*, dogleg_solverContext_t**);
typedef int (*stats_fn)(double*, int);

static void never_called(const double* p, double* x, double* J, void* stream, void* cookie)
{
  (void)p; (void)x; (void)J; (void)stream; (void)cookie;
  printf("the callback was invoked\n");
}
int main(void)
{
  bounded_fn f = &dogleg_amd_optimize_device2_bounded;
  stats_fn g = &dogleg_amd_bounded_last_stats;
  double p[3] = {1.5, -2.5, 3.5}, w[2] = {-7.0, -7.0}, st[8];
  unsigned char held[3] = {9, 9, 9};
  const double p0[3] = {1.5, -2.5, 3.5}, w0[2] = {-7.0, -7.0};
  const unsigned char held0[3] = {9, 9, 9};
  const double lo[3] = {0.0, -3.0, 0.0}, hi[3] = {2.0, -1.0, 4.0}, crossed[3] = {0.0, 0.0, 0.0}, nan_lo[3] = {0.0, NAN, 0.0};
  const dogleg_amd_batch_bounds_t good = {lo, hi, held}, bad_order = {lo, crossed, held}, bad_nan = {nan_lo, hi, held};
  const double r0 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, NULL, NULL, NULL, NULL, NULL);          /* NULL bounds */
  const double r1 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, NULL, w, &good, NULL, NULL);            /* weights without a loss */
  const double r2 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, NULL, NULL, &bad_order, NULL, NULL);    /* lower > upper */
  const double r3 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, NULL, NULL, &bad_nan, NULL, NULL);      /* a NaN bound */
  printf("%g %g %g %g %d %d\n", r0, r1, r2, r3,
         memcmp(p, p0, sizeof(p)) == 0 && memcmp(w, w0, sizeof(w)) == 0 && memcmp(held, held0, sizeof(held)) == 0, g(st, 8));
  return 0;
}
