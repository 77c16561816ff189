// gradcheck_plan.cpp -- the host-only planner of the Jacobian check: pattern checks, first-fit colouring, and the
// per-colour entry and row lists (gradcheck_plan.h).  Plain C++, no HIP.
#include "gradcheck_plan.h"
#include <climits>
#include <cstdio>

int gradcheck_check_pattern(int N, int M, long nnz, const int* colptr, const int* rowidx, char* err, size_t errlen)
{
  if(N <= 0 || M <= 0 || !colptr) { snprintf(err, errlen, "the pattern needs Nstate > 0, Nmeas > 0 and Jt_colptr"); return -1; }
  if(colptr[0] != 0) { snprintf(err, errlen, "Jt_colptr[0] = %d, not 0", colptr[0]); return -1; }
  for(int r = 0; r < M; r++)
    if(colptr[r + 1] < colptr[r]) { snprintf(err, errlen, "Jt_colptr decreases at column %d", r); return -1; }
  if(nnz >= 0 && (long)colptr[M] != nnz)
  { snprintf(err, errlen, "Jt_colptr[Nmeas] = %d disagrees with NJnnz = %ld", colptr[M], nnz); return -1; }
  if(colptr[M] > 0 && !rowidx) { snprintf(err, errlen, "Jt_rowidx is NULL"); return -1; }
  for(int r = 0; r < M; r++)
    for(int t = colptr[r]; t < colptr[r + 1]; t++)
    {
      if(rowidx[t] < 0 || rowidx[t] >= N)
      { snprintf(err, errlen, "Jt_rowidx[%d] = %d is outside 0 .. %d (column %d)", t, rowidx[t], N - 1, r); return -1; }
      if(t > colptr[r] && rowidx[t] <= rowidx[t - 1])
      { snprintf(err, errlen, "the row indices of column %d are not ascending (%d after %d)", r, rowidx[t], rowidx[t - 1]); return -1; }
    }
  return 0;
}

namespace {
// the transpose of the pattern: the rows of variable v are vrow[vptr[v] .. vptr[v+1] - 1], ascending, and vt holds the
// index of that entry in Jt's arrays
void transpose(int N, int M, const int* colptr, const int* rowidx, std::vector<int>& vptr, std::vector<int>& vrow,
               std::vector<int>& vt)
{
  const int nnz = colptr[M];
  vptr.assign((size_t)N + 1, 0);
  for(int t = 0; t < nnz; t++) vptr[(size_t)rowidx[t] + 1]++;
  for(int v = 0; v < N; v++) vptr[(size_t)v + 1] += vptr[v];
  vrow.resize((size_t)nnz); vt.resize((size_t)nnz);
  std::vector<int> next(vptr.begin(), vptr.end() - 1);
  for(int r = 0; r < M; r++)
    for(int t = colptr[r]; t < colptr[r + 1]; t++)
    {
      const int k = next[rowidx[t]]++;
      vrow[k] = r; vt[k] = t;
    }
}

int first_fit(int N, const int* colptr, const int* rowidx, const std::vector<int>& vptr, const std::vector<int>& vrow,
              int* colour)
{
  // taken[c] == v: colour c is held by a neighbour of v.  A variable has at most v coloured neighbours: N + 1 slots do
  std::vector<int> taken((size_t)N + 1, -1);
  int ncolours = 0;
  for(int v = 0; v < N; v++)
  {
    for(int k = vptr[v]; k < vptr[(size_t)v + 1]; k++)
    {
      const int r = vrow[k];
      // (row indices ascend: the variables before v come first)
      for(int t = colptr[r]; t < colptr[r + 1] && rowidx[t] < v; t++) taken[colour[rowidx[t]]] = v;
    }
    int c = 0;
    while(taken[c] == v) c++;
    colour[v] = c;
    if(c + 1 > ncolours) ncolours = c + 1;
  }
  return ncolours;
}
} // namespace

int gradcheck_colour(int N, int M, const int* colptr, const int* rowidx, int* colour)
{
  if(N <= 0) return 0;
  std::vector<int> vptr, vrow, vt;
  transpose(N, M, colptr, rowidx, vptr, vrow, vt);
  return first_fit(N, colptr, rowidx, vptr, vrow, colour);
}

int gradcheck_plan(GradcheckPlan& P, int N, int M, const int* colptr, const int* rowidx, bool one_at_a_time,
                   char* err, size_t errlen)
{
  P = GradcheckPlan();
  P.N = N; P.M = M; P.nnz = colptr[M];
  std::vector<int> vptr, vrow, vt;
  transpose(N, M, colptr, rowidx, vptr, vrow, vt);
  P.colour.assign((size_t)N, 0);
  if(one_at_a_time) { for(int v = 0; v < N; v++) P.colour[v] = v; P.ncolours = N; }
  else P.ncolours = first_fit(N, colptr, rowidx, vptr, vrow, P.colour.data());
  const int C = P.ncolours;

  // entries by (colour, variable, row): a stable counting sort of the variables by colour, each with its rows
  P.ent_ptr.assign((size_t)C + 1, 0);
  for(int v = 0; v < N; v++) P.ent_ptr[(size_t)P.colour[v] + 1] += vptr[(size_t)v + 1] - vptr[v];
  for(int c = 0; c < C; c++) P.ent_ptr[(size_t)c + 1] += P.ent_ptr[c];
  P.ent_t.resize((size_t)P.nnz); P.ent_r.resize((size_t)P.nnz); P.ent_v.resize((size_t)P.nnz);
  {
    std::vector<int> next(P.ent_ptr.begin(), P.ent_ptr.end() - 1);
    for(int v = 0; v < N; v++)
      for(int k = vptr[v]; k < vptr[(size_t)v + 1]; k++)
      {
        const int e = next[P.colour[v]]++;
        P.ent_t[e] = vt[k]; P.ent_r[e] = vrow[k]; P.ent_v[e] = v;
      }
  }
  for(int c = 0; c < C; c++)
    if(P.ent_ptr[(size_t)c + 1] - P.ent_ptr[c] > P.max_entries) P.max_entries = P.ent_ptr[(size_t)c + 1] - P.ent_ptr[c];

  // rows without an entry of colour c.  A row holds at most one entry of a colour, so the count is M minus the
  // colour's entries.
  long long total = 0;
  for(int c = 0; c < C; c++) total += (long long)M - (P.ent_ptr[(size_t)c + 1] - P.ent_ptr[c]);
  if(total > (long long)INT_MAX)
  {
    snprintf(err, errlen, "%d groups over %d rows: the lists of untouched rows hold %lld entries, beyond the index range",
             C, M, total);
    return -1;
  }
  P.out_ptr.assign((size_t)C + 1, 0);
  P.out_r.reserve((size_t)total);
  std::vector<int> mark((size_t)M, -1);
  for(int c = 0; c < C; c++)
  {
    for(int e = P.ent_ptr[c]; e < P.ent_ptr[(size_t)c + 1]; e++) mark[P.ent_r[e]] = c;
    for(int r = 0; r < M; r++) if(mark[r] != c) P.out_r.push_back(r);
    P.out_ptr[(size_t)c + 1] = (int)P.out_r.size();
  }
  return 0;
}

int gradcheck_plan_check(const GradcheckPlan& P, const int* colptr, const int* rowidx, char* err, size_t errlen)
{
  const int C = P.ncolours, N = P.N, M = P.M, nnz = P.nnz;
  if((int)P.colour.size() != N || (int)P.ent_ptr.size() != C + 1 || (int)P.out_ptr.size() != C + 1 ||
     (int)P.ent_t.size() != nnz || (int)P.ent_r.size() != nnz || (int)P.ent_v.size() != nnz ||
     P.ent_ptr[0] != 0 || P.ent_ptr[C] != nnz || P.out_ptr[0] != 0 || P.out_ptr[C] != (int)P.out_r.size())
  { snprintf(err, errlen, "gradcheck plan: array sizes"); return -1; }
  std::vector<char> seen((size_t)nnz, 0);
  std::vector<int> mark((size_t)M, -1);
  for(int c = 0; c < C; c++)
  {
    for(int e = P.ent_ptr[c]; e < P.ent_ptr[(size_t)c + 1]; e++)
    {
      const int t = P.ent_t[e], r = P.ent_r[e], v = P.ent_v[e];
      if(t < 0 || t >= nnz || r < 0 || r >= M || v < 0 || v >= N || seen[t] || rowidx[t] != v || t < colptr[r] ||
         t >= colptr[r + 1] || P.colour[v] != c)
      { snprintf(err, errlen, "gradcheck plan: entry %d of colour %d is wrong", e, c); return -1; }
      seen[t] = 1;
      if(mark[r] == c) { snprintf(err, errlen, "gradcheck plan: row %d holds two variables of colour %d", r, c); return -1; }
      mark[r] = c;
      if(e > P.ent_ptr[c] && (P.ent_v[e - 1] > v || (P.ent_v[e - 1] == v && P.ent_r[e - 1] >= r)))
      { snprintf(err, errlen, "gradcheck plan: the entries of colour %d are not sorted at %d", c, e); return -1; }
    }
    for(int k = P.out_ptr[c]; k < P.out_ptr[(size_t)c + 1]; k++)
    {
      const int r = P.out_r[k];
      if(r < 0 || r >= M || mark[r] == c || (k > P.out_ptr[c] && P.out_r[k - 1] >= r))
      { snprintf(err, errlen, "gradcheck plan: row list of colour %d is wrong at %d", c, k); return -1; }
    }
    if((P.ent_ptr[(size_t)c + 1] - P.ent_ptr[c]) + (P.out_ptr[(size_t)c + 1] - P.out_ptr[c]) != M)
    { snprintf(err, errlen, "gradcheck plan: colour %d does not cover every row once", c); return -1; }
  }
  for(int t = 0; t < nnz; t++) if(!seen[t]) { snprintf(err, errlen, "gradcheck plan: entry %d of Jt is in no list", t); return -1; }
  return 0;
}
