/* query_harness.c -- test helper (compiled by tests/test_query_covariance_gpu.py with gcc): drives
 * dogleg_amd_query_covariance as a C user would.  A small synthetic bundle adjustment is solved with returnContext; then a
 * batch of pixel-style queries (rows over the globals, one camera and one point) runs through the public call on
 * ctx->beforeStep and through dlg_query_covariance on the backend of the context, and the observation form through the
 * public call.  Prints "key v0 v1 ..." lines (doubles in %a). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <dogleg.h>
#include <dlg_backend.h>

typedef struct synth_s synth_t;
synth_t* synth_ba_create(int Nc, int Np, int Nobs, int g, uint64_t seed, double eps, double noise,
                         double p0_spread, double scale_decades, int n_zero_cols);
int  synth_nstate(const synth_t* S);
int  synth_nmeas (const synth_t* S);
int  synth_nnz   (const synth_t* S);
void synth_p0    (const synth_t* S, double* out);
void synth_cb_sparse(const double* p, double* x, cholmod_sparse* Jt, void* cookie);

enum { NC = 4, NP = 20, G = 6, NQ = 12 };

static void dump(const char* key, const double* v, int n)
{
  printf("%s", key);
  for(int i = 0; i < n; i++) printf(" %a", v[i]);
  printf("\n");
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
  /* query k: 1 + k % 3 rows over the globals, camera k % NC and point (5 k + 1) % NP */
  int qrow[NQ + 1], rowptr[3*NQ + 1], var[3*NQ*15];
  double val[3*NQ*15];
  int nrow = 0, ne = 0, nout = 0;
  qrow[0] = 0; rowptr[0] = 0;
  for(int k = 0; k < NQ; k++)
  {
    const int fs = 1 + k % 3, cam = G + 6*(k % NC), pt = G + 6*NC + 3*((5*k + 1) % NP);
    for(int r = 0; r < fs; r++)
    {
      for(int j = 0; j < 15; j++)
      {
        var[ne] = j < G ? j : j < G + 6 ? cam + j - G : pt + j - G - 6;
        val[ne] = 0.25*(double)((7*k + 3*r + j) % 11) - 1.0;
        ne++;
      }
      rowptr[++nrow] = ne;
    }
    qrow[k + 1] = nrow;
    nout += fs*fs;
  }
  double* pub = calloc((size_t)nout, sizeof(double));
  double* bck = calloc((size_t)nout, sizeof(double));
  double* obs = calloc((size_t)nout, sizeof(double));
  const int rc_pub = dogleg_amd_query_covariance(pub, NQ, qrow, rowptr, var, val, -1, ctx->beforeStep, ctx);
  const int rc_be = dlg_query_covariance(dogleg_amd_backend(ctx), dogleg_amd_point_slot(ctx, ctx->beforeStep), NQ, qrow,
                                         rowptr, var, val, -1, bck);
  const int rc_obs = dogleg_amd_query_covariance(obs, NQ, qrow, rowptr, var, val, M, ctx->beforeStep, ctx);
  printf("rc %d %d %d\n", rc_pub, rc_be, rc_obs);
  dump("public", pub, nout);
  dump("backend", bck, nout);
  dump("public_obs", obs, nout);
  free(pub); free(bck); free(obs);
  dogleg_freeContext(&ctx);
  printf("alive 1\n");
  return 0;
}
