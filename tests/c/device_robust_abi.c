/* device_robust_abi.c -- dogleg_amd_optimize_device2_robust as a C user compiles against it (tests/test_device_robust_cpu.py), and
 * what tests/test_device_robust_gpu.py reads of a returned context through the public structs of dogleg.h.
 *   as a program (-DDEVICE_ROBUST_ABI_MAIN): takes the address of the entry point under its prototype and calls it with
 *     arguments it refuses on the host (no GPU needed): prints the return values and whether p and weights kept their bits;
 *   as a shared library: accessors of dogleg_solverContext_t / dogleg_operatingPoint_t for ctypes. */
#include <stdio.h>
#include <string.h>
#include "dogleg.h"

typedef double (*robust_fn)(double*, unsigned int, unsigned int, unsigned int, const int*, const int*, dogleg_callback_device_t*,
                            void*, const dogleg_amd_batch_loss_t*, double*, const dogleg_parameters2_t*, dogleg_solverContext_t**);

double                   robust_ctx_lambda(const dogleg_solverContext_t* ctx)   { return ctx->lambda; }
dogleg_operatingPoint_t* robust_ctx_before(const dogleg_solverContext_t* ctx)   { return ctx->beforeStep; }
double                   robust_point_norm2x(const dogleg_operatingPoint_t* pt) { return pt->norm2_x; }
const double*            robust_point_x(const dogleg_operatingPoint_t* pt)      { return pt->x; }
const double*            robust_point_p(const dogleg_operatingPoint_t* pt)      { return pt->p; }

#ifdef DEVICE_ROBUST_ABI_MAIN
static void never_called(const double* p, double* x, double* J, void* stream, void* cookie)
{
  (void)p; (void)x; (void)J; (void)stream; (void)cookie;
  printf("the callback was invoked\n");
}
int main(void)
{
  robust_fn f = &dogleg_amd_optimize_device2_robust;
  double p[3] = {1.5, -2.5, 3.5}, w[2] = {-7.0, -7.0};
  const double p0[3] = {1.5, -2.5, 3.5}, w0[2] = {-7.0, -7.0};
  const dogleg_amd_batch_loss_t bad_kind = {17, 1.0, 2}, bad_fs = {DOGLEG_AMD_LOSS_CAUCHY, 1.0, 3};
  const double r0 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, NULL, w, NULL, NULL);
  const double r1 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, &bad_kind, w, NULL, NULL);
  const double r2 = f(p, 3, 4, 0, NULL, NULL, &never_called, NULL, &bad_fs, w, NULL, NULL);
  printf("%g %g %g %d\n", r0, r1, r2, memcmp(p, p0, sizeof(p)) == 0 && memcmp(w, w0, sizeof(w)) == 0);
  return 0;
}
#endif
