/* dogleg_batch_model_row_poisson of include/dogleg_batch_models.h compiled for the host as C: the rows of one problem, for
 * tests/test_dense_batch_poisson_cpu.py (a shared object, loaded with ctypes).  t: [M] or NULL; J: [M][N]; d: [M]; feasible: [M]. */
#include <stddef.h>
#include "dogleg_batch_models.h"

void model_rows_poisson(int kind, const double* p, int M, int width, const double* t, const double* y, double* x, double* J,
                        double* d, int* feasible)
{
  const int N = dogleg_batch_model_nstate(kind);
  for(int i = 0; i < M; i++)
  {
    double row[DOGLEG_BATCH_MODEL_MAX_NSTATE];
    feasible[i] = dogleg_batch_model_row_poisson(kind, p, i, width, t ? t[i] : (double)i, y[i], &x[i], row, &d[i]);
    for(int j = 0; j < N; j++) J[(size_t)i*N + j] = row[j];
  }
}
