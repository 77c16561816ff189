// gradcheck_plan.h -- host-only planner of the Jacobian check (gradcheck.hip): which variables are perturbed together,
// and what each group's compare launch reads.  Plain C++, no HIP (tests/c/gradcheck_plan_main.cpp builds it alone).
//
// Variables that share no measurement row can be perturbed in one evaluation (Curtis, Powell, Reid): a row then moves
// through at most one of them and the central difference of that row belongs to that variable.  A colouring of the
// variables in which no row holds two of one colour gives the groups.
#ifndef DLG_GRADCHECK_PLAN_H
#define DLG_GRADCHECK_PLAN_H
#include <cstddef>
#include <vector>

// The pattern of Jt (CSC, N rows x M columns) as the entry points receive it: colptr[0] == 0, colptr ascending,
// row indices in 0 .. N-1 and strictly ascending within a column.  nnz < 0: not compared with colptr[M].
// 0, or -1 with a message in err.
int gradcheck_check_pattern(int N, int M, long nnz, const int* colptr, const int* rowidx, char* err, size_t errlen);

// First-fit colouring in natural variable order: variable v takes the smallest colour that no variable u < v sharing a
// row with it holds; a variable in no row gets colour 0.  Cost: sum over the rows of |row|^2.  Returns the number of
// colours (0 for N == 0).  The pattern must have passed gradcheck_check_pattern.
int gradcheck_colour(int N, int M, const int* colptr, const int* rowidx, int* colour);

struct GradcheckPlan
{
  int N = 0, M = 0, nnz = 0, ncolours = 0;
  std::vector<int> colour;         // [N]
  // the entries of Jt sorted by (colour, variable, row); colour c holds ent_ptr[c] .. ent_ptr[c+1] - 1
  std::vector<int> ent_ptr;        // [ncolours + 1]
  std::vector<int> ent_t, ent_r, ent_v;     // [nnz]: index into Jt's values, measurement row, variable
  // the rows that hold no entry of colour c, ascending: out_ptr[c] .. out_ptr[c+1] - 1
  std::vector<int> out_ptr;        // [ncolours + 1]
  std::vector<int> out_r;
  int max_entries = 0;             // the longest entry list of a colour
};
// one_at_a_time: every variable is its own group (colour[v] = v), else first-fit.  0, or -1 with a message in err
// (the row lists of all colours together exceed the index range).
int gradcheck_plan(GradcheckPlan& P, int N, int M, const int* colptr, const int* rowidx, bool one_at_a_time,
                   char* err, size_t errlen);
// the invariants the device code relies on: every entry of Jt in exactly one list, at the colour of its variable,
// the lists sorted, every (row, colour) pair either in an entry list or in the row list.  0, or -1 with a message.
int gradcheck_plan_check(const GradcheckPlan& P, const int* colptr, const int* rowidx, char* err, size_t errlen);
#endif
