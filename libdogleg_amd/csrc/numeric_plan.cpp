// numeric_plan.cpp -- the host-only planner of the single-problem numeric Jacobians (numeric_plan.h).  Plain C++, no HIP.
#include "numeric_plan.h"
#include "gradcheck_plan.h"
#include <climits>
#include <cstdio>

int numeric_plan(NumericPlan& P, unsigned N, unsigned M, unsigned nnz, const int* colptr, const int* rowidx, int scheme,
                 bool want_entries, char* err, size_t errlen)
{
  P = NumericPlan();
  if(N == 0 || M == 0) { snprintf(err, errlen, "Nstate and Nmeas must not be 0"); return -1; }
  if(N > (unsigned)INT_MAX - 1 || M > (unsigned)INT_MAX - 1 || nnz > (unsigned)INT_MAX)
  { snprintf(err, errlen, "Nstate = %u, Nmeas = %u or NJnnz = %u is beyond the index range", N, M, nnz); return -1; }
  if(scheme != 0 && scheme != 1)
  { snprintf(err, errlen, "unknown scheme (DOGLEG_AMD_NUMERIC_FORWARD or DOGLEG_AMD_NUMERIC_CENTRAL)"); return -1; }
  P.N = (int)N; P.M = (int)M; P.nnz = (int)nnz; P.dense = nnz == 0;
  if(P.dense) { P.C = P.N; P.longest_row = P.N; }
  else
  {
    if(gradcheck_check_pattern(P.N, P.M, (long)nnz, colptr, rowidx, err, errlen)) return -1;
    P.colour.assign((size_t)N, 0);
    P.C = gradcheck_colour(P.N, P.M, colptr, rowidx, P.colour.data());
    for(int r = 0; r < P.M; r++)
      if(colptr[r + 1] - colptr[r] > P.longest_row) P.longest_row = colptr[r + 1] - colptr[r];
  }
  const double K = (scheme == 1 ? 2.0 : 1.0)*(double)P.C + 1.0;
  const double index_bytes = P.dense ? 0.0 : 4.0*((double)N + 2.0*(double)nnz + (double)M + 1.0);
  P.device_bytes = 8.0*(K*((double)N + (double)M) + (double)N) + index_bytes;
  if(K > (double)INT_MAX || P.device_bytes > NUMERIC_MAX_BYTES)
  {
    snprintf(err, errlen, "C = %d colours make K = %.0f copies of %u + %u doubles, %.3g bytes of device memory: too large (the "
             "longest row holds %d variables, and a row of R variables forces R colours)", P.C, K, N, M, P.device_bytes,
             P.longest_row);
    return -1;
  }
  P.K = (int)K;
  if(want_entries && !P.dense)
  {
    P.entry_colour.resize((size_t)nnz);
    for(size_t t = 0; t < (size_t)nnz; t++) P.entry_colour[t] = P.colour[rowidx[t]];
  }
  return 0;
}
