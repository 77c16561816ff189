/* outlier_harness.c -- test helper (compiled by tests/test_outliers_gpu.py with gcc): drives the outlier API of
 * include/dogleg.h as a C user would.  A small synthetic bundle adjustment (two measurements per observation) with
 * three corrupted measurements is solved with returnContext; the outlier entry points then run on ctx->beforeStep.
 * Prints "key v0 v1 ..." lines (doubles in %a) for the Python side to check against numpy.
 *
 * usage: outlier_harness factors FS NOUT SCALE
 *        outlier_harness mark FS CHOSEN PREMARKED NEGATIVE     (CHOSEN / PREMARKED: comma-separated features or "-";
 *                                                               NEGATIVE: the feature whose confidence is < 0, -1: none,
 *                                                               -2: the initial confidence is < 0)
 *        outlier_harness report FS
 *        outlier_harness trace FEATURE ISTATE NSTATE
 *        outlier_harness refuse */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <dogleg.h>

typedef struct synth_s synth_t;
synth_t* synth_ba_create(int Nc, int Np, int Nobs, int g, uint64_t seed, double eps, double noise,
                         double p0_spread, double scale_decades, int n_zero_cols);
void synth_free(synth_t* S);
int  synth_nstate(const synth_t* S);
int  synth_nmeas (const synth_t* S);
int  synth_nnz   (const synth_t* S);
void synth_p0    (const synth_t* S, double* out);
void synth_cb_sparse(const double* p, double* x, cholmod_sparse* Jt, void* cookie);

static const int k_corrupt[3] = {7, 40, 81};
static void cb_corrupted(const double* p, double* x, cholmod_sparse* Jt, void* cookie)
{
  synth_cb_sparse(p, x, Jt, cookie);
  if(x) for(int k = 0; k < 3; k++) x[k_corrupt[k]] += 3.0;
}

static void dump(const char* key, const double* v, int n)
{
  printf("%s", key);
  for(int i = 0; i < n; i++) printf(" %a", v[i]);
  printf("\n");
}

/* getConfidence: counts its calls; CHOSEN features lose 1 % of the confidence, the others half of it */
static int g_calls = 0, g_negative = -1, g_nf = 0;
static char g_chosen[4096];
static double confidence(int i)
{
  g_calls++;
  if(i == -1) return g_negative == -2 ? -1.0 : 100.0;
  if(i == g_negative) return -1.0;
  return (i >= 0 && i < g_nf && g_chosen[i]) ? 99.0 : 50.0;
}
static void parse_list(const char* s, char* flags, int n)
{
  memset(flags, 0, (size_t)n);
  if(!strcmp(s, "-")) return;
  for(const char* q = s; *q;)
  {
    const int k = atoi(q);
    if(k >= 0 && k < n) flags[k] = 1;
    const char* c = strchr(q, ',');
    if(!c) break;
    q = c + 1;
  }
}

/* DENSE_PRODUCTS: x = p - 1 (Nstate = Nmeas = 3) */
static void cb_products(const double* p, double* norm2x, double* xtJ, double* JtJ, void* cookie)
{
  (void)cookie;
  double n2 = 0;
  for(int i = 0; i < 3; i++) { const double xi = p[i] - 1.0; n2 += xi*xi; xtJ[i] = xi; }
  *norm2x = n2;
  memset(JtJ, 0, sizeof(double)*9);
  for(int i = 0; i < 3; i++) JtJ[i*3 + i] = 1.0;
}

int main(int argc, char** argv)
{
  if(argc < 2) return 2;
  const char* mode = argv[1];
  synth_t* S = synth_ba_create(4, 20, 400, 6, 2, 0.4, 0.01, 0.8, 0.0, 0);
  const int N = synth_nstate(S), M = synth_nmeas(S), nnz = synth_nnz(S);
  double* p = malloc(sizeof(double)*N);
  synth_p0(S, p);
  dogleg_parameters2_t prm;
  dogleg_getDefaultParameters(&prm);
  prm.max_iterations = 50;
  dogleg_solverContext_t* ctx = NULL;
  if(dogleg_optimize2(p, N, M, nnz, &cb_corrupted, S, &prm, &ctx) < 0 || !ctx) { printf("FAILED solve\n"); return 1; }
  dogleg_operatingPoint_t* pt = ctx->beforeStep;
  printf("dims %d %d %d\n", N, M, nnz);
  printf("norm2_x %a\n", pt->norm2_x);
  dump("x", pt->x, M);
  printf("Jt_p"); for(int i = 0; i <= M; i++) printf(" %d", ((int*)pt->Jt->p)[i]); printf("\n");
  printf("Jt_i"); for(int i = 0; i < nnz; i++) printf(" %d", ((int*)pt->Jt->i)[i]); printf("\n");
  dump("Jt_x_vals", (double*)pt->Jt->x, nnz);

  if(!strcmp(mode, "factors") && argc >= 5)
  {
    const int fs = atoi(argv[2]), nout = atoi(argv[3]);
    double scale = atof(argv[4]);
    const int nf = M/(fs < 1 ? 1 : fs);
    double* f = calloc((size_t)nf, sizeof(double));
    const bool ok = dogleg_getOutliernessFactors(f, &scale, fs, nf, nout, pt, ctx);
    printf("ok %d\n", (int)ok);
    printf("scale %a\n", scale);
    dump("factors", f, nf);
    /* a second call gives the same bits */
    double* f2 = calloc((size_t)nf, sizeof(double));
    double scale2 = scale;
    dogleg_getOutliernessFactors(f2, &scale2, fs, nf, nout, pt, ctx);
    printf("repeat_same %d\n", memcmp(f, f2, sizeof(double)*(size_t)nf) == 0);
    free(f); free(f2);
  }
  else if(!strcmp(mode, "mark") && argc >= 6)
  {
    const int fs = atoi(argv[2]), nf = M/fs;
    g_nf = nf;
    parse_list(argv[3], g_chosen, nf);
    struct dogleg_outliers_t* marked = calloc((size_t)nf, sizeof(*marked));
    char pre[4096];
    parse_list(argv[4], pre, nf);
    int npre = 0;
    for(int i = 0; i < nf; i++) if(pre[i]) { marked[i].marked = 1; npre++; }
    g_negative = atoi(argv[5]);
    /* the factors markOutliers sees: scale recomputed with the features marked so far */
    double* f = calloc((size_t)nf, sizeof(double));
    double s0 = -1.0;
    dogleg_getOutliernessFactors(f, &s0, fs, nf, npre, pt, ctx);
    dump("factors", f, nf);
    int nout = npre;
    double scale = -1.0;
    const bool any = dogleg_markOutliers(marked, &scale, &nout, &confidence, fs, nf, pt, ctx);
    printf("ret %d\n", (int)any);
    printf("noutliers %d\n", nout);
    printf("calls %d\n", g_calls);
    printf("marked");
    for(int i = 0; i < nf; i++) if(marked[i].marked) printf(" %d", i);
    printf("\n");
    free(f); free(marked);
  }
  else if(!strcmp(mode, "report") && argc >= 3)
  {
    const int fs = atoi(argv[2]), nf = M/fs;
    g_nf = nf;
    memset(g_chosen, 0, sizeof(g_chosen));
    double scale = -1.0;
    fflush(stdout);
    dogleg_reportOutliers(&confidence, &scale, fs, nf, 0, pt, ctx);
    fflush(stderr);
    printf("calls %d\n", g_calls);
  }
  else if(!strcmp(mode, "trace") && argc >= 5)
  {
    const int feat = atoi(argv[2]), i0 = atoi(argv[3]), ns = atoi(argv[4]);
    /* the query: the two rows of an existing feature, restricted to the states i0 .. i0 + ns - 1 */
    double* Jq = calloc((size_t)2*ns, sizeof(double));
    const int* jp = (const int*)pt->Jt->p; const int* ji = (const int*)pt->Jt->i; const double* jx = (const double*)pt->Jt->x;
    for(int c = 0; c < 2; c++)
      for(int q = jp[2*feat + c]; q < jp[2*feat + c + 1]; q++)
        if(ji[q] >= i0 && ji[q] < i0 + ns) Jq[(size_t)c*ns + ji[q] - i0] = jx[q];
    dump("Jq", Jq, 2*ns);
    printf("trace %a\n", dogleg_getOutliernessTrace_newFeature_sparse(Jq, i0, ns, 2, 0, pt, ctx));
    printf("trace_nout3 %a\n", dogleg_getOutliernessTrace_newFeature_sparse(Jq, i0, ns, 2, 3, pt, ctx));
    printf("trace_fs3 %a\n", dogleg_getOutliernessTrace_newFeature_sparse(Jq, i0, ns, 3, 0, pt, ctx));
    pt->have_J = 0;
    printf("trace_noJ %a\n", dogleg_getOutliernessTrace_newFeature_sparse(Jq, i0, ns, 2, 0, pt, ctx));
    pt->have_J = 1;
    free(Jq);
  }
  else if(!strcmp(mode, "refuse"))
  {
    double f[64], scale = -1.0;
    printf("fs3 %d\n", (int)dogleg_getOutliernessFactors(f, &scale, 3, 10, 0, pt, ctx));
    printf("too_many %d\n", (int)dogleg_getOutliernessFactors(f, &scale, 2, M, 0, pt, ctx));
    double q[3] = {3.0, -2.0, 5.0};
    dogleg_solverContext_t* c2 = NULL;
    if(dogleg_optimize_dense_products(q, 3, &cb_products, NULL, &prm, &c2) < 0 || !c2) { printf("FAILED products solve\n"); return 1; }
    scale = -1.0;
    printf("products %d\n", (int)dogleg_getOutliernessFactors(f, &scale, 1, 3, 0, c2->beforeStep, c2));
    dogleg_freeContext(&c2);
  }
  else { printf("bad mode\n"); return 2; }
  printf("lambda %a\n", ctx->lambda);
  dogleg_freeContext(&ctx);
  printf("alive 1\n");
  free(p);
  synth_free(S);
  return 0;
}
