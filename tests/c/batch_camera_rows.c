/* dogleg_batch_camera_datum and dogleg_batch_model_row_poisson_v of include/dogleg_batch_models.h compiled for the host as C, and
 * the layout of dogleg_amd_batch_camera_t, for tests/test_dense_batch_camera_cpu.py (a shared object, loaded with ctypes).
 * t: [M] or NULL; J: [M][N]; d: [M]; feasible: [M]. */
#include <stddef.h>
#include "dogleg.h"
#include "dogleg_batch_models.h"

/* dtype: DOGLEG_AMD_DATA_*; raw: [n] readings of it; the maps: [n] floats */
void camera_data(int dtype, const void* raw, int n, const float* offset, const float* gain_inv, const float* readvar, double* y,
                 double* v)
{
  for(int i = 0; i < n; i++)
  {
    const double r = dtype == DOGLEG_AMD_DATA_U16 ? (double)((const unsigned short*)raw)[i] :
                     dtype == DOGLEG_AMD_DATA_F32 ? (double)((const float*)raw)[i] : ((const double*)raw)[i];
    dogleg_batch_camera_datum(r, offset[i], gain_inv[i], readvar[i], &y[i], &v[i]);
  }
}

/* with_v == 0: dogleg_batch_model_row_poisson on y (v is not read) */
void camera_rows_poisson(int with_v, int kind, const double* p, int M, int width, const double* t, const double* y, const double* v,
                         double* x, double* J, double* d, int* feasible)
{
  const int N = dogleg_batch_model_nstate(kind);
  for(int i = 0; i < M; i++)
  {
    double row[DOGLEG_BATCH_MODEL_MAX_NSTATE];
    const double ti = t ? t[i] : (double)i;
    feasible[i] = with_v ? dogleg_batch_model_row_poisson_v(kind, p, i, width, ti, y[i], v[i], &x[i], row, &d[i])
                         : dogleg_batch_model_row_poisson(kind, p, i, width, ti, y[i], &x[i], row, &d[i]);
    for(int j = 0; j < N; j++) J[(size_t)i*N + j] = row[j];
  }
}

/* sizeof and the offsets of the members, in the order of the declaration; returns how many were written */
int camera_layout(size_t* out)
{
  int k = 0;
  out[k++] = sizeof(dogleg_amd_batch_camera_t);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, model);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, dtype);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, raw);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, sensor_width);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, sensor_height);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, offset);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, gain_inv);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, readvar);
  out[k++] = offsetof(dogleg_amd_batch_camera_t, origin);
  out[k++] = sizeof(dogleg_amd_batch_model_t);
  return k;
}
