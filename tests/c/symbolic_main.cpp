// symbolic_main.cpp -- the symbolic phase as a stand-alone program, so that it can be built with a sanitizer
// (tests/test_library_cpu.py: address + undefined behaviour, and thread for its four-thread section).  Links the
// sparse_symbolic*.cpp files only: no HIP, no GPU.
//   symbolic_main PATTERN [rows ROW0 ROW1 | part RANK NRANKS]
// PATTERN: int32 words N, M, colptr[M+1], rowidx[colptr[M]] (the pattern of Jt, CSC).  rows: a row shard; part: the
// subtree partition as rank RANK of NRANKS sees it.  The knobs come from the environment, as in the library.  Prints
// sym_hash of the analysis (hex).
#include "sparse_symbolic.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv)
{
  if(argc != 2 && !(argc == 5 && (!strcmp(argv[2], "rows") || !strcmp(argv[2], "part"))))
  { fprintf(stderr, "usage: %s PATTERN [rows ROW0 ROW1 | part RANK NRANKS]\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  int nm[2];
  if(!f || fread(nm, sizeof(int), 2, f) != 2 || nm[0] <= 0 || nm[1] <= 0) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const int N = nm[0], M = nm[1];
  std::vector<int> colptr((size_t)M + 1);
  if(fread(colptr.data(), sizeof(int), colptr.size(), f) != colptr.size() || colptr[M] < 0) { fprintf(stderr, "short pattern file\n"); return 2; }
  std::vector<int> rowidx((size_t)colptr[M]);
  if(fread(rowidx.data(), sizeof(int), rowidx.size(), f) != rowidx.size()) { fprintf(stderr, "short pattern file\n"); return 2; }
  fclose(f);

  const bool part = argc == 5 && !strcmp(argv[2], "part");
  const int a = argc == 5 ? atoi(argv[3]) : 0, b = argc == 5 ? atoi(argv[4]) : M;
  char err[512];
  SymHost H;
  if(part ? sym_analyze(H, N, M, colptr.data(), rowidx.data(), 0, M, err, sizeof(err), a, b)
          : sym_analyze(H, N, M, colptr.data(), rowidx.data(), a, b, err, sizeof(err)))
  { fprintf(stderr, "symbolic analysis: %s\n", err); return 1; }
  printf("%016llx\n", (unsigned long long)sym_hash(H));
  return 0;
}
