/* selinv_harness.c -- test helper (compiled by tests/test_selected_inverse_gpu.py with gcc): drives
 * dogleg_amd_covariance_entries of include/dogleg.h as a C user would.  A small synthetic bundle adjustment is solved with
 * returnContext; then the call asks for every entry (i, j), i >= j, whose variables share a measurement row, on
 * ctx->beforeStep (its factor is held) and on ctx->afterStep (it is not: the call factorises there first).  Prints
 * "key v0 v1 ..." lines (doubles in %a) for the Python side to check against numpy from J at the same point. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <dogleg.h>

typedef struct synth_s synth_t;
synth_t* synth_ba_create(int Nc, int Np, int Nobs, int g, uint64_t seed, double eps, double noise,
                         double p0_spread, double scale_decades, int n_zero_cols);
int  synth_nstate(const synth_t* S);
int  synth_nmeas (const synth_t* S);
int  synth_nnz   (const synth_t* S);
void synth_p0    (const synth_t* S, double* out);
void synth_cb_sparse(const double* p, double* x, cholmod_sparse* Jt, void* cookie);

enum { NC = 4, NP = 20, G = 6 };

static void dump(const char* key, const double* v, long n)
{
  printf("%s", key);
  for(long i = 0; i < n; i++) printf(" %a", v[i]);
  printf("\n");
}

static void run(const char* tag, dogleg_operatingPoint_t* pt, dogleg_solverContext_t* ctx, int M, int nnz,
                long n, const int* row, const int* col)
{
  double* out = calloc((size_t)n, sizeof(double));
  const int rc = dogleg_amd_covariance_entries(out, n, row, col, pt, ctx);
  char key[64];
  printf("%s_rc %d\n", tag, rc);
  printf("%s_lambda %a\n", tag, ctx->lambda);
  snprintf(key, sizeof(key), "%s_vals", tag); dump(key, out, n);
  printf("%s_Jp", tag); for(int i = 0; i <= M; i++) printf(" %d", ((int*)pt->Jt->p)[i]); printf("\n");
  printf("%s_Ji", tag); for(int i = 0; i < nnz; i++) printf(" %d", ((int*)pt->Jt->i)[i]); printf("\n");
  snprintf(key, sizeof(key), "%s_Jx", tag); dump(key, (double*)pt->Jt->x, nnz);
  free(out);
}

int main(void)
{
  synth_t* S = synth_ba_create(NC, NP, 400, G, 2, 0.4, 0.01, 0.8, 0.0, 0);
  const int N = synth_nstate(S), M = synth_nmeas(S), nnz = synth_nnz(S);
  double* p = malloc(sizeof(double)*N);
  synth_p0(S, p);
  dogleg_parameters2_t prm;
  dogleg_getDefaultParameters(&prm);
  prm.max_iterations = 50;
  dogleg_solverContext_t* ctx = NULL;
  if(dogleg_optimize2(p, N, M, nnz, &synth_cb_sparse, S, &prm, &ctx) < 0 || !ctx) { printf("FAILED solve\n"); return 1; }
  printf("dims %d %d %d\n", N, M, nnz);
  /* every pair of variables that share a measurement row, once (i >= j) */
  char* seen = calloc((size_t)N*N, 1);
  int* row = malloc(sizeof(int)*(size_t)N*N);
  int* col = malloc(sizeof(int)*(size_t)N*N);
  long n = 0;
  const int* Jp = (const int*)ctx->beforeStep->Jt->p;
  const int* Ji = (const int*)ctx->beforeStep->Jt->i;
  for(int r = 0; r < M; r++)
    for(int a = Jp[r]; a < Jp[r+1]; a++)
      for(int b = Jp[r]; b < Jp[r+1]; b++)
      {
        const int i = Ji[a], j = Ji[b];
        if(i < j || seen[(size_t)i*N + j]) continue;
        seen[(size_t)i*N + j] = 1; row[n] = i; col[n] = j; n++;
      }
  printf("ent");
  for(long e = 0; e < n; e++) printf(" %d %d", row[e], col[e]);
  printf("\n");
  run("before", ctx->beforeStep, ctx, M, nnz, n, row, col);
  run("fresh", ctx->afterStep, ctx, M, nnz, n, row, col);
  /* refusals: a variable outside the state; NULL entry arrays */
  double tmp[4];
  const int br[2] = {0, N}, bc[2] = {0, 0};
  const int rc_out = dogleg_amd_covariance_entries(tmp, 2, br, bc, ctx->beforeStep, ctx);
  const int rc_null = dogleg_amd_covariance_entries(tmp, 1, NULL, NULL, ctx->beforeStep, ctx);
  printf("refuse %d %d\n", rc_out, rc_null);
  dogleg_freeContext(&ctx);
  free(seen); free(row); free(col); free(p);
  printf("alive 1\n");
  return 0;
}
