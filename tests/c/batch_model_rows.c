/* include/dogleg_batch_models.h compiled for the host as C: the rows of one problem, for tests/test_dense_batch_model_cpu.py
 * (a shared object, loaded with ctypes).  t, scale: [M] or NULL; J: [M][N]. */
#include <stddef.h>
#include "dogleg_batch_models.h"

int model_nstate(int kind) { return dogleg_batch_model_nstate(kind); }

void model_rows(int kind, const double* p, int M, int width, const double* t, const double* y, const double* scale, double* x,
                double* J)
{
  const int N = dogleg_batch_model_nstate(kind);
  for(int i = 0; i < M; i++)
  {
    double row[DOGLEG_BATCH_MODEL_MAX_NSTATE];
    dogleg_batch_model_row(kind, p, i, width, t ? t[i] : (double)i, y[i], scale ? scale[i] : 1.0, &x[i], row);
    for(int j = 0; j < N; j++) J[(size_t)i*N + j] = row[j];
  }
}
