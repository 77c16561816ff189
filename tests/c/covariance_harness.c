/* covariance_harness.c -- test helper (compiled by tests/test_covariance_gpu.py with gcc): drives the covariance entry
 * points of include/dogleg.h as a C user would.  A small synthetic bundle adjustment is solved with returnContext; then
 * dogleg_amd_covariance_blocks and dogleg_amd_marginal_variances run on ctx->beforeStep (its factor is held) and on
 * ctx->afterStep (it is not: the call factorises there first).  Prints "key v0 v1 ..." lines (doubles in %a) for the
 * Python side to check against numpy from J at the same point. */
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

static void dump(const char* key, const double* v, int n)
{
  printf("%s", key);
  for(int i = 0; i < n; i++) printf(" %a", v[i]);
  printf("\n");
}

static void run(const char* tag, dogleg_operatingPoint_t* pt, dogleg_solverContext_t* ctx, int N, int M, int nnz,
                int nreq, const int* r0, const int* nr, const int* c0, const int* nc, int nout)
{
  double* out = calloc((size_t)nout, sizeof(double));
  double* var = calloc((size_t)N, sizeof(double));
  const int rc_b = dogleg_amd_covariance_blocks(out, nreq, r0, nr, c0, nc, pt, ctx);
  const int rc_v = dogleg_amd_marginal_variances(var, pt, ctx);
  char key[64];
  printf("%s_rc %d %d\n", tag, rc_b, rc_v);
  printf("%s_lambda %a\n", tag, ctx->lambda);
  snprintf(key, sizeof(key), "%s_blocks", tag); dump(key, out, nout);
  snprintf(key, sizeof(key), "%s_var", tag); dump(key, var, N);
  printf("%s_Jp", tag); for(int i = 0; i <= M; i++) printf(" %d", ((int*)pt->Jt->p)[i]); printf("\n");
  printf("%s_Ji", tag); for(int i = 0; i < nnz; i++) printf(" %d", ((int*)pt->Jt->i)[i]); printf("\n");
  snprintf(key, sizeof(key), "%s_Jx", tag); dump(key, (double*)pt->Jt->x, nnz);
  free(out); free(var);
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
  /* requests: the global block, every camera and point block, camera x point and global x camera blocks */
  int r0[64], nr[64], c0[64], nc[64], n = 0, nout = 0;
  const int cam0 = G, pt0 = G + 6*NC;
  r0[n] = 0; nr[n] = G; c0[n] = 0; nc[n] = G; n++;
  for(int c = 0; c < NC; c++) { r0[n] = cam0 + 6*c; nr[n] = 6; c0[n] = r0[n]; nc[n] = 6; n++; }
  for(int q = 0; q < NP; q += 3) { r0[n] = pt0 + 3*q; nr[n] = 3; c0[n] = r0[n]; nc[n] = 3; n++; }
  for(int c = 0; c < NC; c++) { r0[n] = cam0 + 6*c; nr[n] = 6; c0[n] = pt0 + 3*(5*c + 1); nc[n] = 3; n++; }
  for(int c = 0; c < NC; c++) { r0[n] = pt0 + 3*((7*c + 2) % NP); nr[n] = 3; c0[n] = cam0 + 6*c; nc[n] = 6; n++; }
  for(int c = 0; c < NC; c++) { r0[n] = 0; nr[n] = G; c0[n] = cam0 + 6*c; nc[n] = 6; n++; }
  printf("req");
  for(int q = 0; q < n; q++) { printf(" %d %d %d %d", r0[q], nr[q], c0[q], nc[q]); nout += nr[q]*nc[q]; }
  printf("\n");
  run("before", ctx->beforeStep, ctx, N, M, nnz, n, r0, nr, c0, nc, nout);
  run("fresh", ctx->afterStep, ctx, N, M, nnz, n, r0, nr, c0, nc, nout);
  /* refusals: 17 distinct variables; NULL request arrays */
  double tmp[256];
  const int wr0 = 0, wnr = 9, wc0 = 40, wnc = 8;
  const int rc_wide = dogleg_amd_covariance_blocks(tmp, 1, &wr0, &wnr, &wc0, &wnc, ctx->beforeStep, ctx);
  const int rc_null = dogleg_amd_covariance_blocks(tmp, 1, NULL, NULL, NULL, NULL, ctx->beforeStep, ctx);
  printf("refuse %d %d\n", rc_wide, rc_null);
  dogleg_freeContext(&ctx);
  printf("alive 1\n");
  return 0;
}
