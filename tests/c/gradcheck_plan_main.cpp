// gradcheck_plan_main.cpp -- the host-only planner of the Jacobian check as a stand-alone program, so that it can be
// built with -fsanitize=address,undefined (tests/test_jacobian_check_cpu.py).  Links gradcheck_plan.cpp only: no HIP,
// no GPU.
//   gradcheck_plan_main PATTERN
// PATTERN: int32 words N, M, colptr[M+1], rowidx[colptr[M]] (the pattern of Jt, CSC).  Checks the pattern, plans it
// coloured and one variable at a time, checks both plans, and prints "ncolours" and then the colour of every variable.
#include "gradcheck_plan.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
  if(argc != 2) { fprintf(stderr, "usage: %s PATTERN\n", argv[0]); return 2; }
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
  if(gradcheck_check_pattern(N, M, colptr[M], colptr.data(), rowidx.data(), err, sizeof(err))) { fprintf(stderr, "%s\n", err); return 1; }
  std::vector<int> colour((size_t)N, -1);
  const int nc = gradcheck_colour(N, M, colptr.data(), rowidx.data(), colour.data());
  for(int one = 0; one < 2; one++)
  {
    GradcheckPlan P;
    if(gradcheck_plan(P, N, M, colptr.data(), rowidx.data(), one != 0, err, sizeof(err))) { fprintf(stderr, "%s\n", err); return 1; }
    if(gradcheck_plan_check(P, colptr.data(), rowidx.data(), err, sizeof(err))) { fprintf(stderr, "%s\n", err); return 1; }
    if(P.ncolours != (one ? N : nc) || (!one && P.colour != colour)) { fprintf(stderr, "plan and colouring disagree\n"); return 1; }
  }
  printf("%d\n", nc);
  for(int v = 0; v < N; v++) printf("%d%c", colour[v], v + 1 < N ? ' ' : '\n');
  return 0;
}
