/* The parts of include/dogleg.h that the fused uncertainty and query calls of the built-in models add: the four prototypes.
 * Compiled as C by tests/test_dense_batch_model_uncertainty_cpu.py from dogleg.h alone; the calls it makes are refused. */
#include <stddef.h>
#include <stdio.h>
#include "dogleg.h"

typedef int (*unc_fn)(const double*, unsigned int, const dogleg_amd_batch_model_t*, int, double*, double*, double*, double*, double*,
                      int, int*, const unsigned char*);
typedef int (*unc_device_fn)(const double*, unsigned int, const dogleg_amd_batch_model_t*, int, double*, double*, double*, double*,
                             double*, int, int*, const unsigned char*, const unsigned char*, void*);
typedef int (*query_fn)(const double*, unsigned int, const dogleg_amd_batch_model_t*, int, double*, const double*, unsigned int,
                        unsigned int, int, double*, int*, const unsigned char*);
typedef int (*query_device_fn)(const double*, unsigned int, const dogleg_amd_batch_model_t*, int, double*, const double*,
                               unsigned int, unsigned int, int, double*, int*, const unsigned char*, const unsigned char*, void*);

_Static_assert(sizeof(dogleg_amd_batch_model_t) == 48, "the record did not grow");

int main(void)
{
  unc_fn a = &dogleg_amd_dense_batch_model_uncertainty;
  unc_device_fn b = &dogleg_amd_dense_batch_model_uncertainty_device;
  query_fn c = &dogleg_amd_dense_batch_model_query_covariance;
  query_device_fn d = &dogleg_amd_dense_batch_model_query_covariance_device;
  double p[3] = {1.0, 2.0, 3.0}, lam[1] = {-3.0}, cov[9] = {-5.0}, Jq[3] = {1.0, 0.0, 0.0}, out[1] = {-4.0};
  int status[1] = {7};
  /* a NULL model on the four entry points: -1, the outputs as they were */
  const int ra = a(p, 1, NULL, DOGLEG_AMD_LIKELIHOOD_GAUSS, lam, cov, NULL, NULL, NULL, 1, status, NULL);
  const int rb = b(p, 1, NULL, DOGLEG_AMD_LIKELIHOOD_POISSON, lam, cov, NULL, NULL, NULL, 1, status, NULL, NULL, NULL);
  const int rc = c(p, 1, NULL, DOGLEG_AMD_LIKELIHOOD_GAUSS, lam, Jq, 1, 1, -1, out, status, NULL);
  const int rd = d(p, 1, NULL, DOGLEG_AMD_LIKELIHOOD_POISSON, lam, Jq, 1, 1, -1, out, status, NULL, NULL, NULL);
  printf("%d %d %d %d %g %g %g %d\n", ra, rb, rc, rd, lam[0], cov[0], out[0], status[0]);
  return (a && b && c && d) ? 0 : 1;
}
