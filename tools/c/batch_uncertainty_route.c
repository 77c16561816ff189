/* batch_uncertainty_route.c -- helper of tools/batch_uncertainty_bench.py (compiled there with gcc into a shared object):
 * the route to per-problem covariance and outlierness factors that exists without dogleg_amd_dense_batch_uncertainty.
 * Per problem: dogleg_optimize_dense2 from p[b] with a returnContext (host callback of problems.c; max_iterations 1 and an
 * update_threshold of 1e300 make the solve stop where it starts, so ctx->beforeStep is p[b]: one evaluation, one step computed),
 * dogleg_amd_covariance_blocks for the full Sigma (Nstate <= 16: one diagonal block), dogleg_getOutliernessFactors. */
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include <dogleg.h>

typedef struct synth_s synth_t;
synth_t* synth_dense_create(int M, int N, uint64_t seed, double eps, double noise, double p0_spread);
void synth_free(synth_t* S);
void synth_cb_dense(const double* p, double* x, double* J, void* cookie);

typedef struct { int M, N, B; synth_t** S; } route_t;

route_t* route_create(int M, int N, int B, uint64_t seed0, double eps, double noise, double p0_spread)
{
  route_t* R = calloc(1, sizeof(route_t));
  R->M = M; R->N = N; R->B = B;
  R->S = calloc((size_t)B, sizeof(synth_t*));
  for(int b = 0; b < B; b++) R->S[b] = synth_dense_create(M, N, seed0 + (uint64_t)b, eps, noise, p0_spread);
  return R;
}
void route_free(route_t* R)
{
  for(int b = 0; b < R->B; b++) synth_free(R->S[b]);
  free(R->S); free(R);
}
/* p: [B][N]; cov: [B][N][N]; factors: [B][M / fs]; returns the number of problems that went through */
int route_run(route_t* R, const double* p, int fs, double* cov, double* factors)
{
  const int N = R->N, M = R->M, nf = M/(fs < 1 ? 1 : fs), zero = 0;
  double* q = malloc(sizeof(double)*(size_t)N);
  dogleg_parameters2_t prm;
  dogleg_getDefaultParameters(&prm);
  prm.max_iterations = 1;
  prm.update_threshold = 1e300;
  int done = 0;
  for(int b = 0; b < R->B; b++)
  {
    memcpy(q, p + (size_t)b*N, sizeof(double)*(size_t)N);
    dogleg_solverContext_t* ctx = NULL;
    if(dogleg_optimize_dense2(q, N, M, &synth_cb_dense, R->S[b], &prm, &ctx) < 0 || !ctx) continue;
    double scale = -1.0;
    const int rc = dogleg_amd_covariance_blocks(cov + (size_t)b*N*N, 1, &zero, &N, &zero, &N, ctx->beforeStep, ctx);
    const bool ok = dogleg_getOutliernessFactors(factors + (size_t)b*nf, &scale, fs, nf, 0, ctx->beforeStep, ctx);
    if(rc == 0 && ok) done++;
    dogleg_freeContext(&ctx);
  }
  free(q);
  return done;
}
