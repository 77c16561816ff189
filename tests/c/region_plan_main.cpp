// region_plan_main.cpp -- the factorisation's host-only planner as a stand-alone program, so that it can be built
// with -fsanitize=address,undefined (tests/test_library_cpu.py).  Links the sparse_symbolic*.cpp files and sparse_region.cpp
// only: no HIP, no GPU.
//   region_plan_main PATTERN NCU
// PATTERN: int32 words N, M, colptr[M+1], rowidx[colptr[M]] (the pattern of Jt, CSC).  The knobs come from the
// environment, as in the library.  Prints the schedule's and the level parameters' hashes (hex).
#include "sparse_region.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  if(argc != 3) { fprintf(stderr, "usage: %s PATTERN NCU\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  int nm[2];
  if(!f || fread(nm, sizeof(int), 2, f) != 2 || nm[0] <= 0 || nm[1] <= 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int N = nm[0], M = nm[1];
  std::vector<int> colptr((size_t)M + 1);
  if(fread(colptr.data(), sizeof(int), colptr.size(), f) != colptr.size() || colptr[M] < 0) { fprintf(stderr, "short pattern file\n"); return 2; }
  std::vector<int> rowidx((size_t)colptr[M]);
  if(fread(rowidx.data(), sizeof(int), rowidx.size(), f) != rowidx.size()) { fprintf(stderr, "short pattern file\n"); return 2; }
  fclose(f);

  char err[512];
  SymHost H;
  if(sym_analyze(H, N, M, colptr.data(), rowidx.data(), 0, M, err, sizeof(err))) { fprintf(stderr, "symbolic analysis: %s\n", err); return 1; }
  const RegionKnobs K = region_knobs_env(atoi(argv[2]));
  FacLevels L;
  if(fac_level_params(H, L, err, sizeof(err))) { fprintf(stderr, "%s\n", err); return 1; }
  const RegionPlan R = region_plan(H, L, 1, H.nlevels - 1, K);
  if(region_check(H, R, nullptr, err, sizeof(err))) { fprintf(stderr, "%s\n", err); return 1; }
  printf("%016llx %016llx\n", (unsigned long long)region_plan_hash(R), (unsigned long long)fac_levels_hash(L));
  return 0;
}
