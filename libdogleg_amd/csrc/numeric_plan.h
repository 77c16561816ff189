// numeric_plan.h -- host-only planner of the numeric Jacobians of a values-only single-problem model (numeric_device.hip,
// dogleg.h: dogleg_amd_numeric_*): the colouring the adapter perturbs by, the number of copies it evaluates, what its
// Jacobian kernel reads per entry and the device memory its handle owns.  Plain C++, no HIP.
//
// The colouring is gradcheck_colour's (gradcheck_plan.h), called as it is: the adapter and the Jacobian check agree on the
// groups.  A dense problem (nnz == 0) materialises neither a pattern nor a colouring: every variable is its own colour.
#ifndef DLG_NUMERIC_PLAN_H
#define DLG_NUMERIC_PLAN_H
#include <cstddef>
#include <vector>

struct NumericPlan
{
  int N = 0, M = 0, nnz = 0;
  bool dense = false;
  int C = 0;                       // colours: N for a dense problem
  int K = 0;                       // copies: C + 1 (forward), 2 C + 1 (central)
  int longest_row = 0;             // most variables in one measurement row (dense: N); C >= longest_row
  double device_bytes = 0.0;       // what the handle allocates: copies, divisors and index arrays (without copied bounds)
  std::vector<int> colour;         // [N]; empty for a dense problem
  std::vector<int> entry_colour;   // [nnz]: colour[rowidx[t]], what the Jacobian kernel reads beside rowidx; only if asked for
};

// scheme: 0 forward, 1 central (DOGLEG_AMD_NUMERIC_*).  nnz == 0: dense, colptr / rowidx are not read.  want_entries: fill
// entry_colour.  0, or -1 with a message in err: zero sizes, sizes beyond the index range, a pattern gradcheck_check_pattern
// refuses or that disagrees with nnz, an unknown scheme, copies that do not fit (the message names C, K, the bytes and the
// longest row).
int numeric_plan(NumericPlan& P, unsigned N, unsigned M, unsigned nnz, const int* colptr, const int* rowidx, int scheme,
                 bool want_entries, char* err, size_t errlen);

// the bytes beyond which a plan is refused: no device holds them
constexpr double NUMERIC_MAX_BYTES = 1.0e15;
#endif
