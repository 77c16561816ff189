/* batch_uncertainty_harness.c -- test helper (compiled by tests/test_dense_batch_uncertainty_gpu.py with gcc): the
 * single-problem route to what dogleg_amd_dense_batch_uncertainty gives for a whole batch.  DenseProblem(M, N, seed, eps,
 * noise, p0_spread) of problems.c is run through dogleg_optimize_dense2 FROM the given point with a returnContext; the
 * parameters make that solve stop where it starts (every step counts as a small step, which is not applied), so
 * ctx->beforeStep is the given point.  Then dogleg_amd_marginal_variances and dogleg_getOutliernessFactors on it.
 * Prints "key v0 v1 ..." lines (doubles in %a).
 *
 * usage: batch_uncertainty_harness M N SEED EPS NOISE P0_SPREAD FS P[0] ... P[N-1]       (the doubles in %a or decimal) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <dogleg.h>

typedef struct synth_s synth_t;
synth_t* synth_dense_create(int M, int N, uint64_t seed, double eps, double noise, double p0_spread);
void synth_free(synth_t* S);
void synth_cb_dense(const double* p, double* x, double* J, void* cookie);

static void dump(const char* key, const double* v, int n)
{
  printf("%s", key);
  for(int i = 0; i < n; i++) printf(" %a", v[i]);
  printf("\n");
}

int main(int argc, char** argv)
{
  if(argc < 8) return 2;
  const int M = atoi(argv[1]), N = atoi(argv[2]), fs = atoi(argv[7]);
  if(argc != 8 + N) return 2;
  synth_t* S = synth_dense_create(M, N, (uint64_t)strtoull(argv[3], NULL, 10), atof(argv[4]), atof(argv[5]), atof(argv[6]));
  double* p = malloc(sizeof(double)*N);
  for(int i = 0; i < N; i++) p[i] = strtod(argv[8 + i], NULL);
  dogleg_parameters2_t prm;
  dogleg_getDefaultParameters(&prm);
  prm.max_iterations = 1;
  prm.update_threshold = 1e300;
  dogleg_solverContext_t* ctx = NULL;
  if(dogleg_optimize_dense2(p, N, M, &synth_cb_dense, S, &prm, &ctx) < 0 || !ctx) { printf("FAILED solve\n"); return 1; }
  dogleg_operatingPoint_t* pt = ctx->beforeStep;
  dump("p", pt->p, N);
  double* var = calloc((size_t)N, sizeof(double));
  printf("rc_var %d\n", dogleg_amd_marginal_variances(var, pt, ctx));
  dump("var", var, N);
  const int nf = M/(fs < 1 ? 1 : fs);
  double* f = calloc((size_t)nf, sizeof(double));
  double scale = -1.0;
  printf("ok %d\n", (int)dogleg_getOutliernessFactors(f, &scale, fs, nf, 0, pt, ctx));
  printf("scale %a\n", scale);
  dump("factors", f, nf);
  printf("lambda %a\n", ctx->lambda);
  dogleg_freeContext(&ctx);
  synth_free(S);
  printf("alive 1\n");
  return 0;
}
