/* dogleg.h -- public API of the MI355X-native dog-leg solver.
 *
 * Drop-in for libdogleg's dogleg.h (reference: /root/reference/dogleg.h):
 * identical function names, argument order, callback contracts, struct and
 * field names, so a program written against libdogleg re-links against
 * libdogleg_amd.so unchanged.  The trust-region control flow runs on the
 * host; every per-iteration linear-algebra op (Jt*x, |J v|^2, JtJ assembly,
 * Cholesky factor + solve, dog-leg interpolation) runs in HIP kernels on
 * gfx950 through the C-ABI declared in dlg_backend.h.
 *
 * What is NOT provided (out of the hot-path scope):
 * the experimental outlier / confidence API.
 *
 * Binary layout note: like the reference (dogleg.h:166-210) the context embeds
 * a cholmod_common by value as its first member, so the *binary* layout
 * depends on the CHOLMOD headers in use; source compatibility is the goal.
 */
#ifndef DOGLEG_AMD_DOGLEG_H
#define DOGLEG_AMD_DOGLEG_H

#include <stddef.h>
#include <stdbool.h>
#include "dogleg_cholmod_compat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- user callbacks (reference dogleg.h:11-45) --------------------------- */

/* sparse: fill x[Nmeas] and Jt (CSC, Nstate rows x Nmeas cols; column r holds
 * d x[r] / d p, row indices ascending).  Jt->p/i/x are int/int/double arrays
 * owned by the library. */
typedef void (dogleg_callback_t)(const double* p, double* x,
                                 cholmod_sparse* Jt, void* cookie);

/* dense: fill x[Nmeas] and J[Nmeas][Nstate] (row-major) */
typedef void (dogleg_callback_dense_t)(const double* p, double* x,
                                       double* J, void* cookie);

/* dense products: the callback reduces over the measurements itself and
 * returns norm2(x), Jt*x and JtJ (full N*N, or one packed triangle) */
typedef void (dogleg_callback_dense_products_t)(const double* p,
                                                double* norm2x, double* xtJ,
                                                double* JtJ, void* cookie);

/* ---- one operating point (reference dogleg.h:48-105) ---------------------- */
typedef struct
{
  double* p;                       /* always valid */
  double* x;
  double  norm2_x;
  union
  {
    cholmod_sparse* Jt;            /* DOGLEG_SPARSE         */
    double*         J_dense;       /* DOGLEG_DENSE, [Nmeas][Nstate] */
    double*         JtJ;           /* DOGLEG_DENSE_PRODUCTS */
  };
  double* Jt_x;

  /* cached steps: a rejected trial is retried from these */
  double* updateCauchy;
  union
  {
    cholmod_dense* updateGN_cholmoddense;
    double*        updateGN_dense;
  };
  double norm2_updateCauchy, norm2_updateGN;

  union
  {
    int dummy_bits[3];
    struct
    {
      bool have_updateCauchy          : 1;
      bool have_updateGN              : 1;
      bool have_factorization         : 1;
      bool have_x                     : 1;
      bool have_J                     : 1;
      bool have_Jtx                   : 1;
      bool have_JtJ                   : 1;
      bool have_step_to_here          : 1;
      bool didStepToEdgeOfTrustRegion : 1;
    };
  };

  double* step_to_here;
  double  norm2_step_to_here;
} dogleg_operatingPoint_t;

/* ---- parameters (reference dogleg.h:107-153) ----------------------------- */
#define DOGLEG_DEBUG_VNLOG_BIT 30
#define DOGLEG_DEBUG_VNLOG     (1 << DOGLEG_DEBUG_VNLOG_BIT)

typedef struct
{
  int max_iterations;
  union
  {
    int dogleg_debug;              /* legacy view of the bits below */
    struct
    {
      bool debug       : 1;
      bool JtJ_packed  : 1;        /* dense-products: LAPACK packed triangle */
      bool JtJ_upper   : 1;        /* ... row-major upper if set             */
      int  dummy       : DOGLEG_DEBUG_VNLOG_BIT - 3;
      bool debug_vnlog : 1;        /* lands on bit DOGLEG_DEBUG_VNLOG_BIT    */
    };
  };

  double trustregion0;

  double trustregion_decrease_factor;
  double trustregion_decrease_threshold;
  double trustregion_increase_factor;
  double trustregion_increase_threshold;

  /* termination thresholds */
  double Jt_x_threshold;
  double update_threshold;
  double trustregion_threshold;
} dogleg_parameters2_t;

#ifndef __cplusplus
_Static_assert(offsetof(dogleg_parameters2_t, trustregion0) == 2 * sizeof(int),
               "dogleg_parameters2_t layout differs from libdogleg");
#else
static_assert(offsetof(dogleg_parameters2_t, trustregion0) == 2 * sizeof(int),
              "dogleg_parameters2_t layout differs from libdogleg");
#endif

typedef enum
{
  DOGLEG_DENSE          = 0,
  DOGLEG_SPARSE         = 1,
  DOGLEG_DENSE_PRODUCTS = 2
} dogleg_solve_type_t;

/* ---- solver context (reference dogleg.h:166-210) -------------------------- */
typedef struct
{
  cholmod_common common;

  union
  {
    dogleg_callback_t*                f;
    dogleg_callback_dense_t*          f_dense;
    dogleg_callback_dense_products_t* f_dense_products;
  };
  void* cookie;

  dogleg_operatingPoint_t* beforeStep;  /* current point between steps      */
  dogleg_operatingPoint_t* afterStep;   /* scratch point while trying a step */

  union
  {
    cholmod_factor* factorization;       /* sparse: handle to the GPU factor  */
    double*         factorization_dense; /* dense: packed factor, host mirror */
  };

  double lambda;                         /* sticky diagonal damping           */

  dogleg_solve_type_t solve_type;
  int Nstate, Nmeasurements;

  const dogleg_parameters2_t* parameters;
} dogleg_solverContext_t;

/* ---- parameter handling (reference dogleg.h:214-257, dogleg.c:117-181) ---- */
void dogleg_getDefaultParameters(dogleg_parameters2_t* parameters);
void dogleg_setMaxIterations(int n);
void dogleg_setTrustregionUpdateParameters(double downFactor, double downThreshold,
                                           double upFactor,   double upThreshold);
void dogleg_setDebug(int debug);
void dogleg_setInitialTrustregion(double t);
void dogleg_setThresholds(double Jt_x, double update, double trustregion);

/* ---- solves (reference dogleg.h:278-302, dogleg.c:1633-1818) --------------
 * p: in = initial estimate, out = optimum.  Return norm2(x) at the optimum, or
 * a negative number on error.  parameters == NULL selects the process-global
 * set edited by the dogleg_set*() functions.  A non-NULL returnContext
 * receives the solver state; release it with dogleg_freeContext(). */
double dogleg_optimize(double* p, unsigned int Nstate,
                       unsigned int Nmeas, unsigned int NJnnz,
                       dogleg_callback_t* f, void* cookie,
                       dogleg_solverContext_t** returnContext);
double dogleg_optimize2(double* p, unsigned int Nstate,
                        unsigned int Nmeas, unsigned int NJnnz,
                        dogleg_callback_t* f, void* cookie,
                        const dogleg_parameters2_t* parameters,
                        dogleg_solverContext_t** returnContext);
double dogleg_optimize_dense(double* p, unsigned int Nstate, unsigned int Nmeas,
                             dogleg_callback_dense_t* f, void* cookie,
                             dogleg_solverContext_t** returnContext);
double dogleg_optimize_dense2(double* p, unsigned int Nstate, unsigned int Nmeas,
                              dogleg_callback_dense_t* f, void* cookie,
                              const dogleg_parameters2_t* parameters,
                              dogleg_solverContext_t** returnContext);
double dogleg_optimize_dense_products(double* p, unsigned int Nstate,
                                      dogleg_callback_dense_products_t* f, void* cookie,
                                      const dogleg_parameters2_t* parameters,
                                      dogleg_solverContext_t** returnContext);

/* make sure ctx holds the Cholesky factor of JtJ at `point`
 * (reference dogleg.h:304-310, dogleg.c:634-820) */
bool dogleg_computeJtJfactorization(dogleg_operatingPoint_t* point,
                                    dogleg_solverContext_t* ctx);

void dogleg_freeContext(dogleg_solverContext_t** ctx);

/* ---- extensions of this implementation (nothing below exists in the reference) -------------
 *
 * Device-side evaluation.  The reference evaluates the user's model on the host at
 * every trial point (computeCallbackOperatingPoint, dogleg.c:1016-1022); here that means the
 * Jacobian values cross PCIe once per evaluation, which is the end-to-end bottleneck once the
 * kernels are fast.  A model that already lives on the GPU supplies a device callback instead:
 *   p_dev     in : Nstate doubles, device memory
 *   x_dev     out: Nmeas doubles, device memory (library-owned)
 *   J_dev     out: sparse: the NJnnz values of Jt in the order of the pattern (column r of Jt =
 *                  gradient of measurement r); dense: J[Nmeas][Nstate] row-major.  Device memory.
 *   hip_stream   : the hipStream_t (as void*) the callback must enqueue its kernels on; the
 *                  library orders its own work behind it on the same stream and the callback
 *                  must not synchronise.
 * dogleg_optimize_device2: the sparsity pattern of Jt is constant over a solve (as the reference
 * assumes, dogleg.c:648-649), so it is given once, on the host (Jt_colptr[Nmeas+1],
 * Jt_rowidx[NJnnz], row indices ascending within a column).  NJnnz == 0 and NULL pattern
 * pointers select the dense path.  Everything else -- p in/out on the host, return value, the
 * iterate sequence, returnContext -- is as dogleg_optimize2 / dogleg_optimize_dense2, except that
 * the Jacobian values of a returned context stay on the device (point->Jt->x / J_dense == NULL;
 * dlg_point_download(dogleg_amd_backend(ctx), slot, DLG_VEC_J, ...) fetches them). */
typedef void (dogleg_callback_device_t)(const double* p_dev, double* x_dev, double* J_dev,
                                        void* hip_stream, void* cookie);
double dogleg_optimize_device2(double* p, unsigned int Nstate,
                               unsigned int Nmeas, unsigned int NJnnz,
                               const int* Jt_colptr, const int* Jt_rowidx,
                               dogleg_callback_device_t* f, void* cookie,
                               const dogleg_parameters2_t* parameters,
                               dogleg_solverContext_t** returnContext);

/* Multi-GPU (the reference is single-threaded CPU code; its row sums dogleg.c:253-260, 269-278, 712-714 are
 * what is split).  One process per GPU; EVERY rank calls dogleg_optimize* / dogleg_optimize_device2 with the
 * same arguments and the same callback.  The callback keeps its contract -- it evaluates ALL measurement
 * rows at the p it is given (every rank sees the same p: the sums over the ranks leave identical bits
 * everywhere) --; the library takes from it the rows of its rank (sparse: those the subtree partition of
 * the elimination tree assigns, include/dlg_backend.h; dense: a contiguous slice), assembles / factors /
 * solves its share and sums Jt*x, the top of the tree (dense: JtJ), the solution and two scalars per step
 * over the ranks.  p, the return value, the iterate sequence and a returned context are the same on every
 * rank (the vectors of a returned context are complete; dogleg_amd_rank tells a rank which one it is).
 * dense-products solves have no rows to split: every rank does all of it (replicas).
 *
 * How a solve finds its communicator, in this order:
 *   dogleg_amd_set_communicator   per calling thread, before the solve: rank, ranks, the GPU (device index,
 *       -1: the current one) and the 128-byte RCCL id rank 0 made with dogleg_amd_rccl_unique_id and handed
 *       to the others by any means (MPI_Bcast, a file ...).  The sums are ncclAllReduce calls on the
 *       solve's own stream.
 *   dogleg_amd_set_allreduce      ... with the caller's sum-all-reduce over `count` doubles at a device
 *       address instead of RCCL (MPI, or the in-process sum the single-GPU tests use); host-synchronous.
 *   the environment               DOGLEG_AMD_WORLD_SIZE > 1, DOGLEG_AMD_RANK, DOGLEG_AMD_LOCAL_RANK (the GPU,
 *       default: the rank), DOGLEG_AMD_RCCL_ID_FILE (a path all ranks see: rank 0 writes the id there,
 *       the others wait for it; DOGLEG_AMD_RUN_ID names the launch, see dogleg_amd_id_file_publish): a program that was only re-linked against this library, started once
 *       per GPU by a launcher, needs no source change.  The communicator is made once per process.
 * All return 0 on success, -1 on bad arguments. */
typedef int (*dogleg_amd_allreduce_t)(void* buf_dev, size_t count, void* cookie);
int  dogleg_amd_set_communicator(int rank, int nranks, int device, const void* rccl_unique_id128);
int  dogleg_amd_set_allreduce(int rank, int nranks, int device, dogleg_amd_allreduce_t fn, void* cookie);
void dogleg_amd_clear_communicator(void);
int  dogleg_amd_rccl_unique_id(void* out128);
int  dogleg_amd_rank(const dogleg_solverContext_t* ctx, int* nranks);
/* The id file of the environment contract, for launchers that hand the id round themselves: rank 0 publishes
 * the 128-byte id (tmp + rename: never seen half-written), the others wait for a complete file that carries
 * the same run id (any string that names the launch; the environment contract uses DOGLEG_AMD_RUN_ID, else
 * TORCHELASTIC_RUN_ID, else ""), so that a file an earlier launch left at the path is not taken for this
 * launch's.  Under one run id the path must be fresh for each launch.  Host only, no GPU call.  0 / -1. */
int  dogleg_amd_id_file_publish(const char* path, const void* id128, const char* run_id);
int  dogleg_amd_id_file_wait(const char* path, void* id128_out, const char* run_id, int timeout_ms);

/* Between solves the library keeps one idle backend (device buffers, the uploaded sparsity pattern and its
 * schedules) and the page-locked host buffers of the operating points: a program that solves many problems
 * of one shape -- the same scene, new measurements -- pays allocations, uploads and the symbolic analysis
 * once (the reference redoes all of it per solve, dogleg.c:1479-1562, 1633-1753: its solves take seconds).
 * dogleg_amd_release_cache gives everything back; DOGLEG_AMD_NO_BACKEND_CACHE=1 never keeps anything. */
void dogleg_amd_release_cache(void);
/* measurement: where the calling thread's last solve spent its wall time, if DOGLEG_AMD_TIMING=1 was set for it (the same
 * numbers it printed on stderr): ms7 / calls7 = {pattern, model callback, inputs to the backend, dlg_point_eval,
 * dlg_take_step + dlg_step, trace records, run_optimizer as a whole}.  Returns the number of entries (7). */
int  dogleg_amd_last_solve_timing(double* ms7, int* calls7);

/* the device backend (include/dlg_backend.h) behind a returned context, and the backend slot of
 * one of its operating points: what dlg_solve_with_factor / dlg_solve_multi /
 * dlg_pseudoinverse_chunk / dlg_point_download need to work with the factor and the vectors that
 * stay on the device after a solve (the reference hands out a cholmod_factor / LAPACK factor
 * for the same purpose, dogleg.h:185-194) */
struct dlg_backend;
struct dlg_backend* dogleg_amd_backend(dogleg_solverContext_t* ctx);
int dogleg_amd_point_slot(dogleg_solverContext_t* ctx, const dogleg_operatingPoint_t* point);

/* gradient check of a callback (reference dogleg.h:312-322): prints, for variable `var`, the
 * reported d x[i] / d p[var] next to a central difference, one line per measurement, as a
 * vnlog-style table on stdout.  Host only. */
void dogleg_testGradient(unsigned int var, const double* p0,
                         unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                         dogleg_callback_t* f, void* cookie);
void dogleg_testGradient_dense(unsigned int var, const double* p0,
                               unsigned int Nstate, unsigned int Nmeas,
                               dogleg_callback_dense_t* f, void* cookie);
void dogleg_testGradient_dense_products(unsigned int var, const double* p0,
                                        unsigned int Nstate, unsigned int Nmeas,
                                        dogleg_callback_dense_products_t* f, void* cookie);

/* ---- outliers (reference dogleg.h:331-392; experimental there, and the prototypes are kept as they are).  Every entry
 * point needs x and J of `point`, factorises JtJ + lambda I there (dogleg_computeJtJfactorization) if that is not held,
 * and reads the leverage blocks A_f = J_f (JtJ + lambda I)^-1 J_f^T of the features from the device (dlg_backend.h:
 * dlg_feature_leverage).  A feature is featureSize consecutive measurements starting at i*featureSize; featureSize <= 1
 * means 1, sizes above 2 are refused.  Not available with DENSE_PRODUCTS (no Jacobian).
 *
 * Outlierness factors: one per feature, scaled by *scale, which is computed when *scale <= 0 (and written back):
 * Nn = Nmeasurements - NoutlierFeatures*featureSize, scale = Nn / (4 (Nstate+1) |x|^2 / (Nn - Nstate - 1)).
 * Size 1: x^2 / (1 - a) * scale/8; size 2: x^T (B + B^2) x * scale/8 with B = (A_f - I)^-1; DBL_MAX where the
 * denominator (1 - a, det(A_f - I)) is below 1e-8 in magnitude. */
bool dogleg_getOutliernessFactors(double* factors, double* scale, int featureSize, int Nfeatures,
                                  int NoutlierFeatures, dogleg_operatingPoint_t* point,
                                  dogleg_solverContext_t* ctx);

/* one flag per feature */
struct dogleg_outliers_t
{
  unsigned char marked : 1;
};
/* Marks new outliers: a feature not yet marked whose factor is >= 1 is marked when leaving it out costs less than 5 % of
 * the confidence, 1 - getConfidence(i)/getConfidence(-1) < 0.05.  *Noutliers: the marked features before (it is the
 * NoutlierFeatures of the factors) and after the call.  Returns whether any feature was newly marked; false also when
 * the factors or getConfidence(-1) fail (*Noutliers unchanged) or a getConfidence(i) is negative (the count so far). */
bool dogleg_markOutliers(struct dogleg_outliers_t* markedOutliers, double* scale, int* Noutliers,
                         double (getConfidence)(int i_feature_exclude), int featureSize, int Nfeatures,
                         dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx);

/* debug report on stderr: a header, then per feature its factor and the relative drop of the confidence without it
 * (getConfidence is called Nfeatures + 1 times) */
void dogleg_reportOutliers(double (getConfidence)(int i_feature_exclude), double* scale, int featureSize,
                           int Nfeatures, int Noutliers, dogleg_operatingPoint_t* point,
                           dogleg_solverContext_t* ctx);

/* the outlierness of a query feature that is not part of J (featureSize 2 only): Jq is 2 x NstateActive, row-major, on
 * the states istateActive ..; A = Jq (JtJ + lambda I)^-1 Jq^T; returns scale (2 - tr (I + A)^-1), the scale recomputed
 * with NoutlierFeatures, or -1.0 on failure */
double dogleg_getOutliernessTrace_newFeature_sparse(const double* JqueryFeature, int istateActive,
                                                    int NstateActive, int featureSize, int NoutlierFeatures,
                                                    dogleg_operatingPoint_t* point,
                                                    dogleg_solverContext_t* ctx);

/* ---- extension (not in the reference): parameter uncertainty from the factor held on the device.  Blocks of
 * Sigma = (JtJ + lambda I)^-1 at `point`, lambda = ctx->lambda (the lambda of that factorisation), UNSCALED: multiply by
 * sigma^2, for example |x|^2 / (Nmeasurements - Nstate), for the covariance of the parameters.  This replaces
 * cholmod_solve on ctx->factorization with unit right-hand sides.  Request q is Sigma[r0[q] : r0[q]+nr[q],
 * c0[q] : c0[q]+nc[q]], written row-major into out, the blocks of all requests one after another; its two ranges hold at
 * most 16 distinct variables together (a diagonal block up to 16 wide, a cross block nr + nc <= 16), see
 * dlg_backend.h: dlg_covariance_blocks.  Wider blocks: dlg_solve_multi with unit columns.
 * Factorises at `point` if that factor is not held (dogleg_computeJtJfactorization).  All three solve types; one rank
 * only.  0 on success, -1 on failure (with a message). */
int dogleg_amd_covariance_blocks(double* out, int nreq, const int* r0, const int* nr, const int* c0, const int* nc,
                                 dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx);
/* diag(Sigma), Nstate values */
int dogleg_amd_marginal_variances(double* var, dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx);
/* Sigma at n single entries (row[e], col[e]), either order, written to out in entry order: entries of the structure of
 * the factor, which holds every entry (i, j) whose variables share a measurement row (every block of JtJ: in bundle
 * adjustment the camera, point and global blocks and every observed camera x point block) and the fill of the
 * factorisation.  An entry off it is refused.  All of them come from one sweep over the factor (the selected inverse),
 * see dlg_backend.h: dlg_covariance_entries.  Factorises at `point` if that factor is not held; all three solve types;
 * one rank only.  0 on success, -1 on failure (with a message). */
int dogleg_amd_covariance_entries(double* out, long n, const int* row, const int* col,
                                  dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx);
/* the covariance of derived quantities: for query k (rows qrow[k] .. qrow[k+1] - 1 of the CSR rowptr / var / val, 1 to 16
 * rows over the Nstate variables), the fs x fs block Jq Sigma Jq^T, written in full, row-major, the queries' blocks one
 * after another.  Nobservations < 0: that plain form; 0 <= Nobservations <= Nmeasurements: the observation (sandwich)
 * form Jq Sigma J_obs^T J_obs Sigma Jq^T, J_obs the first Nobservations measurement rows (for measurement vectors that
 * carry regularisation or prior terms behind the observations; not with DENSE_PRODUCTS).  See dlg_backend.h:
 * dlg_query_covariance.  Wider queries: dlg_solve_multi on the columns of Jq^T.  Factorises at `point` if that factor is
 * not held; one rank only.  0 on success, -1 on failure (with a message). */
int dogleg_amd_query_covariance(double* out, int nq, const int* qrow, const int* rowptr, const int* var,
                                const double* val, int Nobservations,
                                dogleg_operatingPoint_t* point, dogleg_solverContext_t* ctx);

/* ---- extension (not in the reference): many small dense problems at once, the whole dog-leg loop on the device.
 * B independent problems of one shape (Nstate, Nmeas) advance together in rounds; every problem has its own trust
 * region, lambda and stopping test, and problem b does exactly what dogleg_optimize_dense2 does on that problem alone
 * with the same parameters: the same trial points, accept / reject decisions, trust-region updates, lambda schedule
 * (0 -> 1e-10 -> x10, only when a factorisation the reference would attempt fails) and the same ways to stop.  A round
 * is one call of the batch callback for the live problems' trial points and a constant number of launches of the
 * library, whatever B is; the host reads one counter of live problems per round.
 *
 * The batch callback evaluates the LIVE problems.  All pointers are device memory.
 *   p_dev    in : [B][Nstate]
 *   x_dev    out: [B][Nmeas]
 *   J_dev    out: [B][Nmeas][Nstate], row-major per problem (the dense callback's layout)
 *   live_dev in : [B] bytes; 0: problem b needs no evaluation in this call, whatever is written for it is ignored
 *                 (a callback may evaluate it anyway)
 *   hip_stream  : enqueue here, do not synchronise (as dogleg_callback_device_t)
 *
 * Limits (refused with a message and -1): B, Nstate or Nmeas 0, a NULL p / f / results, Nstate above
 * DOGLEG_AMD_BATCH_MAX_NSTATE = 64, the width of a wavefront: one lane holds one variable (larger problems: a loop over
 * dogleg_optimize_dense2), a set communicator (one rank only),
 * device memory: B * Nmeas * (Nstate + 1) doubles for x and J of the trial points, plus B * (Nstate * (Nstate + 11) / 2 + 8)
 * doubles of state (a call that does not fit fails with a message that names the size).  The debug / debug_vnlog bits of the parameters are ignored.  There is no returnContext: the
 * covariance and the outlierness factors of every problem come from dogleg_amd_dense_batch_uncertainty below; for the factor
 * itself, or for marking outliers, run the problem through dogleg_optimize_dense2 from the returned p[b]. */
typedef void (dogleg_callback_device_batch_t)(const double* p_dev, double* x_dev, double* J_dev,
                                              const unsigned char* live_dev, unsigned int B,
                                              void* hip_stream, void* cookie);
#define DOGLEG_AMD_BATCH_MAX_NSTATE     64
#define DOGLEG_AMD_BATCH_JTX            1   /* |Jt x|_inf <= Jt_x_threshold at the start or at an accepted point   */
#define DOGLEG_AMD_BATCH_SMALL_STEP     2   /* max |step| <= update_threshold: that step is not applied             */
#define DOGLEG_AMD_BATCH_TRUSTREGION    3   /* trustregion < trustregion_threshold after a rejected trial           */
#define DOGLEG_AMD_BATCH_MAX_ITERATIONS 4   /* max_iterations accepted steps                                        */
#define DOGLEG_AMD_BATCH_FAILED         5   /* non-finite x or J, lambda overflow, an undefined (NaN) gain ratio    */
#define DOGLEG_AMD_BATCH_NOT_RUN        0   /* the device-resident entry points: active_dev[b] was 0                */
/* The layout of this struct is part of the ABI: the device-resident entry points write it from a kernel as an array of
 * structs.  40 bytes; the doubles at offsets 0, 8 and 16, the ints at offsets 24, 28 and 32 (4 bytes of padding at the
 * end, never written). */
typedef struct
{
  double norm2_x;        /* at the returned p[b]; negative: this problem failed                     */
  double trustregion;    /* when it stopped                                                         */
  double lambda;         /* its sticky damping when it stopped                                      */
  int    iterations;     /* accepted steps                                                          */
  int    evaluations;    /* times the callback's result for this problem was used                   */
  int    status;         /* DOGLEG_AMD_BATCH_{JTX, SMALL_STEP, TRUSTREGION, MAX_ITERATIONS, FAILED, NOT_RUN} */
} dogleg_amd_batch_result_t;
/* p: [B][Nstate] on the host, in = initial estimates, out = optima.  0, or -1 on bad arguments / no device /
 * allocation failure (message on stderr, p untouched).  A problem that fails is reported in its result (its p[b]
 * stays as it was on input) and does not stop the others.  parameters == NULL: the process-global set. */
int dogleg_amd_optimize_dense_batch(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                    dogleg_callback_device_batch_t* f, void* cookie,
                                    const dogleg_parameters2_t* parameters,
                                    dogleg_amd_batch_result_t* results);
/* measurement: the calling thread's last batch call: out[0] = rounds, and, if DOGLEG_AMD_BATCH_TIMING=1 was set for
 * it (three events a round on the stream), out[1] = ms in the callback's kernels, out[2] = ms in the library's.
 * Returns the number of entries written (at most n, at most 3). */
int dogleg_amd_batch_last_stats(double* out, int n);

/* Per-problem uncertainty of a batch: at the points p[b] (normally what the batch solve returned), Sigma_b = (JtJ + lambda I)^-1
 * with J of problem b at p[b], its diagonal, and the outlierness factors of the problem's features, for all B problems in
 * one call: the batch callback is invoked exactly ONCE, at p, with every live byte 1, and one launch of the library
 * follows it, whatever B is.
 *   lambda      [B] in/out, or NULL (start at 0, not reported): problem b is factorised at lambda[b] -- pass results[b].lambda
 *               of the solve --; where a pivot is <= 0 the solve's schedule applies (0 -> 1e-10 -> x10) until the
 *               factorisation succeeds or lambda is no longer finite.  The lambda that was used is written back.  A negative
 *               or NaN lambda[b] fails that problem alone (FAILED; it is written back as it came).
 *   covariance  [B][Nstate][Nstate] full, row-major, UNSCALED as dogleg_amd_covariance_blocks (multiply by sigma^2), or NULL
 *   variances   [B][Nstate], the diagonals (the same bits as the diagonal of covariance), or NULL
 *   factors     [B][Nmeas / featureSize], or NULL: the contract written above dogleg_getOutliernessFactors with the leverage
 *               block A_f = J_f Sigma_b J_f^T; features are consecutive measurements from 0 (a trailing odd measurement is
 *               not covered at size 2); DBL_MAX where |1 - a| or |det(A_f - I)| is below 1e-8
 *   scale       [B] in/out, required with factors: a scale[b] <= 0 is computed with NoutlierFeatures = 0,
 *               Nmeas / (4 (Nstate+1) |x|^2 / (Nmeas - Nstate - 1)), and written back
 *   featureSize <= 1 means 1, sizes above 2 are refused
 *   status      [B], required: DOGLEG_AMD_BATCH_UNC_OK or _FAILED.  A FAILED problem gets NaN in every requested output (and
 *               in a scale that was to be computed from a non-finite x); it does not disturb the others and the call still
 *               returns 0.
 * Problem b's output bits do not depend on B, on its position or on its neighbours.
 * Refused with a message and -1 before any device work, outputs untouched: a NULL p / f / status, B, Nstate or Nmeas 0,
 * Nstate above DOGLEG_AMD_BATCH_MAX_NSTATE, featureSize above 2, factors without scale, a scale[b] <= 0 while
 * Nmeas <= Nstate + 1, all three outputs NULL, a set communicator, device memory that does not fit (the message names the
 * size): B * Nmeas * (Nstate + 1) doubles for x and J plus the inputs and the requested outputs.
 * Memory the library keeps after the call (dogleg_amd_release_cache gives it back): the device buffers, and one page-locked
 * host buffer as large as the inputs and the requested outputs together, 8 B (2 Nstate + 3 + Nstate^2 + Nmeas / featureSize)
 * bytes with everything asked for -- about 370 MB for B = 131 072 problems of 96 x 16.
 * Not covered on a batch: NoutlierFeatures / marking outliers, and covariance blocks across several problems. */
#define DOGLEG_AMD_BATCH_UNC_OK      0
#define DOGLEG_AMD_BATCH_UNC_FAILED  1   /* non-finite x or J at p[b], or lambda overflowed before a factorisation succeeded */
                                         /* (also: a negative or NaN lambda[b] on input) */
#define DOGLEG_AMD_BATCH_UNC_SKIPPED 2   /* the device-resident entry points: active_dev[b] was 0, nothing else written */
int dogleg_amd_dense_batch_uncertainty(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                       dogleg_callback_device_batch_t* f, void* cookie,
                                       double* lambda, double* covariance, double* variances, double* factors,
                                       double* scale, int featureSize, int* status);
/* measurement: the calling thread's last uncertainty call: out[0] = kernel launches of the library, out[1] = stream
 * synchronisations, out[2] = copies and fills on the stream (none of the three depends on B), and, if
 * DOGLEG_AMD_BATCH_TIMING=1 was set for it, out[3] = ms in the callback's kernels, out[4] = ms in the library's.
 * Returns the number of entries written (at most n, at most 5). */
int dogleg_amd_batch_uncertainty_last_stats(double* out, int n);

/* ---- the products form of a batch (the batch twin of dogleg_optimize_dense_products): the callback reduces over its
 * measurements itself and hands back, for every LIVE problem, norm2(x), Jt x and JtJ.  Nmeas is not an argument: every
 * problem may have its own number of measurements, the library never sees them, and nothing of size Nmeas is stored.
 * B independent problems of Nstate variables advance together in rounds; every problem has its own trust region, lambda
 * and stopping test, and problem b does exactly what dogleg_optimize_dense_products does on that problem alone with the
 * same parameters: the same trial points, accept / reject decisions, trust-region updates, lambda schedule (0 -> 1e-10 ->
 * x10, only when a factorisation the reference would attempt fails) and the same ways to stop.  A round is one call of
 * the callback, one launch of the library and one 4-byte read-back, whatever B is.  The result struct, the status codes
 * and the meanings of evaluations and iterations are those of dogleg_amd_optimize_dense_batch; dogleg_amd_batch_last_stats
 * reports the calling thread's last batch solve of either form.
 *
 * All pointers are device memory; live_dev and hip_stream as in dogleg_callback_device_batch_t.
 *   p_dev      in : [B][Nstate]
 *   norm2x_dev out: [B]
 *   xtJ_dev    out: [B][Nstate], Jt x
 *   JtJ_dev    out: [B][S], the layout chosen by parameters->JtJ_packed / JtJ_upper as in the reference:
 *     unpacked            S = Nstate^2, row-major.  ONLY the entries [i][j] with j >= i are read (the triangle the
 *                         reference's dpotrf 'L' reads through its column-major view); the others are never read and
 *                         need not be written.
 *     packed and upper    S = Nstate (Nstate + 1) / 2, row-major upper triangle: row 0 (Nstate entries), row 1 from its
 *                         diagonal (Nstate - 1 entries), ...
 *     packed, not upper   refused with a message and -1, as the reference refuses it.
 * DOGLEG_AMD_BATCH_FAILED also covers a non-finite norm2x, a non-finite entry of xtJ and a non-finite entry of JtJ among
 * those that are read (every one of them is checked, off the diagonal too).
 *
 * Refused with a message and -1, p untouched, no device work: a NULL p / f / results, B or Nstate 0, Nstate above
 * DOGLEG_AMD_BATCH_MAX_NSTATE, the packed lower layout, a set communicator (one rank only), device memory that does not
 * fit (the message names the size): B * (1 + Nstate + S) doubles of callback output plus B * (Nstate * (Nstate + 11) / 2 + 8)
 * doubles of state.  parameters == NULL: the process-global set (unpacked).
 * What the products form does not give: outlierness factors (they need J; the reference's outlier API refuses
 * DENSE_PRODUCTS for the same reason). */
typedef void (dogleg_callback_device_batch_products_t)(const double* p_dev, double* norm2x_dev, double* xtJ_dev,
                                                       double* JtJ_dev, const unsigned char* live_dev, unsigned int B,
                                                       void* hip_stream, void* cookie);
int dogleg_amd_optimize_dense_products_batch(double* p, unsigned int B, unsigned int Nstate,
                                             dogleg_callback_device_batch_products_t* f, void* cookie,
                                             const dogleg_parameters2_t* parameters,
                                             dogleg_amd_batch_result_t* results);
/* Sigma_b = (JtJ + lambda I)^-1 and its diagonal with the JtJ the products callback returns at p[b]: the contract of
 * dogleg_amd_dense_batch_uncertainty for lambda, covariance, variances and status (one callback with every live byte 1,
 * then one launch; the same lambda schedule; a negative or NaN lambda[b], or anything non-finite among what is read of
 * problem b's norm2x, xtJ and JtJ, fails that problem alone and gives it NaN outputs; a problem's bits do not depend on B
 * or on its neighbours).  Of parameters only JtJ_packed / JtJ_upper are read (NULL: the global set).  There are no
 * outlierness factors and no scale: they need J.  Refused with a message and -1 before any device work, outputs
 * untouched: a NULL p / f / status, B or Nstate 0, Nstate above DOGLEG_AMD_BATCH_MAX_NSTATE, the packed lower layout, both
 * outputs NULL, a set communicator, device memory that does not fit.  dogleg_amd_batch_uncertainty_last_stats covers it. */
int dogleg_amd_dense_products_batch_uncertainty(const double* p, unsigned int B, unsigned int Nstate,
                                                dogleg_callback_device_batch_products_t* f, void* cookie,
                                                const dogleg_parameters2_t* parameters,
                                                double* lambda, double* covariance, double* variances, int* status);

/* ---- device-resident batches: the four entry points above with every array in DEVICE memory, so that a batch whose start
 * points come from a kernel and whose optima feed another kernel never passes through the host.  The callback types, the
 * parameters, the size classes, the limits, the status codes, the layouts of all arrays and the bits of every result are
 * those of the host-pointer twin.
 *
 * Common to the four:
 *   *_dev       device-accessible memory of the current device: device, managed or registered / page-locked host memory.
 *               Refused before any device work: a pointer of any other kind (pageable host memory among them), a device
 *               allocation of another device, a device allocation that does not cover the bytes the call touches from
 *               that pointer.
 *   hip_stream  a hipStream_t, or NULL.  Non-NULL: every copy, the callback and every launch go onto that stream, behind
 *               whatever was enqueued there before (the kernel that wrote p_dev, say), and the callback receives that
 *               stream.  NULL: the library's own non-blocking stream, as the host-pointer entry points; the caller must have
 *               finished writing the inputs.
 *   The call blocks the host until its work is complete (the solve reads its 4-byte counter of live problems every round,
 *   the uncertainty call synchronises once at its end).  Nothing else is copied between host and device and no page-locked
 *   staging buffer is allocated.
 *   active_dev  [B] bytes or NULL (all active).  active_dev[b] == 0: problem b is NOT RUN.  The callback sees the mask
 *               through live_dev: the solve's live bytes start as the mask, the uncertainty call's live bytes are the mask.
 *               An active problem's bits do not depend on the mask.  With no active problem the call returns 0, invokes
 *               the callback at most once and writes nothing but the records of problems that are not run.
 *
 * The solve:
 *   p_dev       [B][Nstate] in/out.  A problem that FAILED or is not run keeps its input bits.
 *   results_dev [B] dogleg_amd_batch_result_t, an array of structs (the layout written above the typedef); only the six
 *               fields are written.  Not run: {norm2_x -1, trustregion 0, lambda 0, iterations 0, evaluations 0,
 *               status DOGLEG_AMD_BATCH_NOT_RUN}.
 *   lambda_dev  [B] or NULL: results_dev[b].lambda as a contiguous array (0 where not run), the lambda_dev argument of the
 *               uncertainty call below.
 * dogleg_amd_batch_last_stats covers these solves.  Refused with a message and -1: what the host-pointer twin refuses, and
 * the pointers described above. */
int dogleg_amd_optimize_dense_batch_device(double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           const dogleg_parameters2_t* parameters,
                                           dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                           const unsigned char* active_dev, void* hip_stream);
int dogleg_amd_optimize_dense_products_batch_device(double* p_dev, unsigned int B, unsigned int Nstate,
                                                    dogleg_callback_device_batch_products_t* f, void* cookie,
                                                    const dogleg_parameters2_t* parameters,
                                                    dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                    const unsigned char* active_dev, void* hip_stream);
/* The uncertainty calls: the arguments of dogleg_amd_dense_batch_uncertainty / dogleg_amd_dense_products_batch_uncertainty,
 * read and written where they lie.  A problem that is not run gets status_dev[b] = DOGLEG_AMD_BATCH_UNC_SKIPPED and nothing
 * else: none of its outputs, its lambda_dev[b] or its scale_dev[b] is written.  One invocation of the callback and one
 * launch, whatever B is; dogleg_amd_batch_uncertainty_last_stats reports launches 1, synchronisations 1 and at most 2 fills
 * (the live bytes without a mask, the lambda scratch for a NULL lambda_dev).  Refused with a message and -1: what the
 * host-pointer twin refuses, the pointers described above, and factors_dev together with Nmeas <= Nstate + 1 (whether every
 * scale_dev[b] is given cannot be seen without a copy). */
int dogleg_amd_dense_batch_uncertainty_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                              dogleg_callback_device_batch_t* f, void* cookie,
                                              double* lambda_dev, double* covariance_dev, double* variances_dev,
                                              double* factors_dev, double* scale_dev, int featureSize, int* status_dev,
                                              const unsigned char* active_dev, void* hip_stream);
int dogleg_amd_dense_products_batch_uncertainty_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                       dogleg_callback_device_batch_products_t* f, void* cookie,
                                                       const dogleg_parameters2_t* parameters,
                                                       double* lambda_dev, double* covariance_dev, double* variances_dev,
                                                       int* status_dev, const unsigned char* active_dev, void* hip_stream);

/* ---- robust loss functions in the batch solve: every problem minimises F = sum_f rho(s_f), s_f = |x_f|^2, over its features
 * (featureSize consecutive measurements from 0) in place of norm2(x), so that gross outliers lose their pull inside the solve.
 * With w_f = rho'(s_f) at the point the sweep is made at, the dog-leg loop of dogleg_amd_optimize_dense_batch runs with
 *   F = sum_f rho(s_f)        in place of norm2(x): the gain ratio (F_before - F_trial) / expected improvement, results[b].norm2_x
 *   g = sum_f w_f J_f^T x_f   in place of Jt x:     the Cauchy step, the Jt_x_threshold test, the expected improvement
 *   H = sum_f w_f J_f^T J_f   in place of JtJ:      the factorisation with lambda, |J g|^2, |J s|^2, the expected improvement
 * and nothing else changed.  This is the first-order treatment (IRLS; Triggs' correction without its curvature term), what
 * Ceres' corrector does for every loss with rho'' <= 0; all losses here have rho'' <= 0, so H stays positive semidefinite.
 * A callback cannot supply this alone: rows scaled by sqrt(rho') give g and H, but the gain ratio must compare sum rho.
 *   kind, with scale a > 0 and c = a^2:          rho(s)                        rho'(s)
 *     DOGLEG_AMD_LOSS_TRIVIAL                    s                             1                (scale is ignored)
 *     DOGLEG_AMD_LOSS_HUBER                      s <= c: s, else 2 a sqrt(s) - c       s <= c: 1, else a / sqrt(s)
 *     DOGLEG_AMD_LOSS_SOFT_L1                    2 c (sqrt(1 + s/c) - 1)       1 / sqrt(1 + s/c)
 *     DOGLEG_AMD_LOSS_CAUCHY                     c log1p(s/c)                  1 / (1 + s/c)
 *   featureSize <= 1 means 1; sizes 1 to DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE = 4; Nmeas must be a multiple of it.
 * The contract is that of dogleg_amd_optimize_dense_batch (and of its _device twin): the callback type and the live bytes, one
 * callback, one launch and one 4-byte read-back per round, the status codes, the meaning of iterations and evaluations,
 * dogleg_amd_batch_last_stats, and for the twin the pointer checks, the stream rule and the mask.
 *   results[b].norm2_x  is F at the returned p[b] (NOT norm2(x)); negative: the problem failed.
 *   weights     [B][Nmeas / featureSize] or NULL: rho'(s_f) at the returned p[b], in (0, 1]: what a caller thresholds to name
 *               the outliers.  A FAILED problem gets NaN weights (and keeps its input p[b]); the weights of a problem that is not
 *               run (active_dev[b] == 0) are not written.
 * With DOGLEG_AMD_LOSS_TRIVIAL and featureSize 1 every result has the bits dogleg_amd_optimize_dense_batch gives (at other
 * feature sizes the rows are summed in tiles of another height: norm2_x may differ in its last bits), and every weight is 1.
 * Refused with a message and -1 before any device work, outputs untouched: what the plain twin refuses, a NULL loss, an unknown
 * kind, a scale that is not finite and > 0 (unless TRIVIAL), featureSize above 4, Nmeas not a multiple of featureSize, a set
 * communicator; the device twin also refuses weights_dev as it refuses the other pointers.  Device memory: the plain solve's,
 * plus B * Nmeas / featureSize doubles.
 * Not provided: the products form with a loss (it has no per-feature x); per-problem scales (normalise x in the callback);
 * losses that are not concave in s (Tukey's biweight): H would need the curvature term.  The uncertainty and the query
 * covariances of the reweighted problem at the returned p: dogleg_amd_dense_batch_uncertainty_fit / _query_covariance_fit below,
 * with this loss and these weights in their fit record. */
#define DOGLEG_AMD_LOSS_TRIVIAL 0
#define DOGLEG_AMD_LOSS_HUBER   1
#define DOGLEG_AMD_LOSS_SOFT_L1 2
#define DOGLEG_AMD_LOSS_CAUCHY  3
#define DOGLEG_AMD_BATCH_LOSS_MAX_FEATURESIZE 4
typedef struct
{
  int    kind;           /* DOGLEG_AMD_LOSS_*                                              */
  double scale;          /* a: residual norms |x_f| below it are treated as least squares  */
  int    featureSize;    /* measurements per feature, 1 .. 4 (<= 1: 1)                     */
} dogleg_amd_batch_loss_t;
int dogleg_amd_optimize_dense_batch_robust(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                           dogleg_amd_batch_result_t* results, double* weights);
int dogleg_amd_optimize_dense_batch_robust_device(double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                  dogleg_callback_device_batch_t* f, void* cookie,
                                                  const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                                  dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                  double* weights_dev, const unsigned char* active_dev, void* hip_stream);

/* ---- robust loss functions in dogleg_optimize_device2: the sparse (NJnnz > 0) and the dense (NJnnz == 0) device solve
 * minimise F = sum_f rho(s_f) in place of norm2(x), with the losses, the struct and the first-order treatment written above:
 * F replaces norm2(x) in the gain ratio and in the return value, g = sum_f w_f J_f^T x_f replaces Jt x and H = sum_f w_f J_f^T J_f
 * replaces JtJ everywhere else, w_f = rho'(s_f); features are featureSize consecutive measurement rows counted from row 0.
 * Every argument but loss and weights, the callback's contract, the trust-region loop, the lambda schedule and the ways to stop
 * are those of dogleg_optimize_device2.
 *
 * How: directly behind every invocation of the callback, on the same stream, the library computes s_f from the rows of x (summed
 * in row order), writes w_f, sums rho(s_f) in a fixed order (no floating-point atomics: F has the same bits on every run) and
 * multiplies row r of x and of J, in place, by sqrt(w_{r / featureSize}).  Everything behind that -- Jt x, the assembly of JtJ,
 * the factorisation, both steps, the expected improvement -- is the plain solve's code on the weighted rows; only the gain
 * ratio, the trace / vnlog records and the return value take F (one 8-byte copy an evaluation) where they took norm2(x).  The
 * sparse pass finds the row of an entry from THIS call's Jt_colptr, of which the solve keeps a device copy of its own.
 *   loss        kind DOGLEG_AMD_LOSS_*, scale a > 0 (ignored by TRIVIAL), featureSize 1 .. 4 (<= 1 means 1).
 *   weights     host, [Nmeas / featureSize], or NULL: rho'(s_f) at the returned p, in (0, 1].
 * Returns F at the returned p.  A solve that fails returns -1.0 and leaves p and weights untouched.
 * With DOGLEG_AMD_LOSS_TRIVIAL every weight is exactly 1, x and J keep their bits and the iterates are those of
 * dogleg_optimize_device2; F is summed in another order than norm2(x), so its last bits may differ.
 *
 * A returned context holds the WEIGHTED point:
 *   beforeStep->norm2_x is F (NOT norm2 of the x it holds);
 *   beforeStep->x and the device-resident J (dlg_point_download, DLG_VEC_J) are the callback's rows times sqrt(w_f);
 *   Jt_x is g, and the factor held is that of H + lambda I.
 * dogleg_getOutliernessFactors, dogleg_amd_covariance_blocks, dogleg_amd_marginal_variances, dogleg_amd_covariance_entries and
 * dogleg_amd_query_covariance, called on that context, are therefore those of the reweighted problem (JtWJ + lambda I)^-1.
 *
 * Refused with a message and -1.0 before any device work, p and weights untouched: everything dogleg_optimize_device2 refuses, a
 * Jt_colptr that decreases somewhere, a NULL loss, an unknown kind, a scale that is not finite and > 0 (unless TRIVIAL),
 * featureSize above 4, Nmeas not a multiple of featureSize, and more than one rank, whether by dogleg_amd_set_communicator,
 * dogleg_amd_set_allreduce or the environment contract.
 * Device memory beyond the plain solve's: 2 Nmeas / featureSize doubles of weights, Nmeas + 1 ints of pattern (sparse), and
 * about Nmeas / (256 featureSize) doubles of partial sums.
 * Not provided: robust solves on several GPUs; a loss for the host-callback entry points (dogleg_optimize2 / _dense2) and for
 * the products form (it has no per-feature x); per-feature scales (normalise x in the callback); losses that are not concave
 * in s; Triggs' curvature term. */
double dogleg_amd_optimize_device2_robust(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                                          const int* Jt_colptr, const int* Jt_rowidx,
                                          dogleg_callback_device_t* f, void* cookie,
                                          const dogleg_amd_batch_loss_t* loss,
                                          double* weights,      /* host, [Nmeas / featureSize], or NULL */
                                          const dogleg_parameters2_t* parameters,
                                          dogleg_solverContext_t** returnContext);
/* measurement: the calling thread's last robust device solve: out[0] = evaluations the prelude ran behind, out[1] = kernel
 * launches of the prelude per evaluation, and, if DOGLEG_AMD_TIMING=1 was set for the solve (two events an evaluation on the
 * stream), out[2] = ms in the prelude's kernels over the solve.  Returns the number of entries written (at most n, at most 3). */
int dogleg_amd_robust_last_stats(double* out, int n);

/* ---- box bounds in the batch solve: every problem minimises norm2(x) (or, with a loss, F) subject to lower[b] <= p[b] <=
 * upper[b], by an active-set dog-leg loop: variables on a bound whose gradient pushes outwards are held, the two steps are
 * those of the free variables, the step chosen is clipped into the box, and a clipped step that the model does not like
 * gives way to a Cauchy step cut at the first bound.  A callback cannot supply this alone (a reparameterisation changes the
 * problem and its covariance and fails at the bound itself): the held set changes the Gauss-Newton system and the stopping
 * test, the clipped step changes the expected improvement the gain ratio divides by.  The reference has no bounds.
 * One problem, in the plain form's terms (with a loss read H, g, F for JtJ, Jt x, norm2(x), as in the robust form above):
 *   1. Start.  p_i = min(max(p_i, lower_i), upper_i) before the first evaluation.  A problem with a NaN bound or with
 *      lower_i > upper_i for any i is DOGLEG_AMD_BATCH_FAILED alone: evaluations 0, p[b] keeps its input bits, its held row is 0.
 *   2. Held set, at the point stepped from (feasible by construction): i is held at lower if p_i == lower_i && g_i > 0, at
 *      upper if p_i == upper_i && g_i < 0.  Equality is exact: the clamp of step 5 lands on the bound's bits.  The set is a
 *      function of that point, its g and the bounds only: a rejected trial forms it again, nothing is stored for it.
 *   3. Free gradient g_F: g with its held entries 0.  The Jt_x_threshold test is on |g_F|_inf (every variable held: 0, so the
 *      problem stops with DOGLEG_AMD_BATCH_JTX before any division).  The Cauchy step is k g_F, k = -|g_F|^2 / (g_F' JtJ g_F).
 *   4. Gauss-Newton step on the free set: in the copy of JtJ that is factorised, after lambda is added, every held row and
 *      column gets zero off-diagonals and a diagonal of 1; the right-hand side is g_F, so the step is exactly 0 where held.
 *      The factorisation, the lambda schedule and the choice among Cauchy-to-the-edge, Gauss-Newton and the interpolated
 *      step are the plain solve's, on these two steps.
 *   5. Clip.  trial_i = min(max(p_i + s_i, lower_i), upper_i); s'_i = s_i where nothing was clamped, bound_i - p_i where it
 *      was.  With no component clamped nothing differs from the plain solve.  Expected improvement: -2 g's' - s'' JtJ s'.
 *   6. Fallback, if some component was clamped and the expected improvement is <= 0 or max|s'| <= update_threshold:
 *      d = t0 Cauchy with t0 = min(1, trustregion / |Cauchy|); alpha = min(1, min_i (far_i - p_i) / d_i) over the i with d_i != 0,
 *      far_i = upper_i if d_i > 0, lower_i otherwise; the step is alpha d, clamped as in 5 (rounding only), with its own expected
 *      improvement.  In the fallback the component that sets alpha ends on its bound's bits whichever way p + alpha d rounds:
 *      trial_i = far_i, s'_i = far_i - p_i for every i with d_i != 0 whose own ratio equals alpha (one ulp short of the bound the
 *      variable would be neither held nor free to move, and the next fallback would be cut at alpha ~ 1e-16).
 *      The step counts as one to the edge of the trust region iff |Cauchy| >= trustregion.  A free variable on a
 *      bound has -g pointing inwards, so alpha > 0, and JtJ is positive semidefinite, so the improvement is > 0 up to rounding:
 *      one that is <= 0 or not finite is DOGLEG_AMD_BATCH_FAILED.
 *   7. update_threshold tests the step that is applied; the trial point is `trial`; the gain ratio, the trust-region update,
 *      acceptance and what a rejected trial reuses are the plain solve's.
 *   8. held[b] is the held set at the returned p[b].
 * With bounds that clamp nothing (lower = upper = NULL, infinite entries, a box that is never met) every result has the bits of
 * dogleg_amd_optimize_dense_batch (with a loss: of _robust), and held is all 0.
 * The contract is that of dogleg_amd_optimize_dense_batch, _robust and their _device twins: the callback type and the live
 * bytes, one callback, one launch and one 4-byte read-back per round, the result struct and the status codes (none is new),
 * dogleg_amd_batch_last_stats, and for the twin the pointer checks (the three pointers inside *bounds, which itself is host
 * memory, included), the stream rule and the mask (held of a problem that is not run is not written).
 *   loss        NULL: least squares.  weights: as in the robust form; NULL unless a loss is given.
 * Refused with a message and -1 before any device work, outputs untouched: what the plain (with a loss: the robust) twin refuses,
 * a NULL bounds, weights without a loss; the device twin also refuses lower, upper and held as it refuses the other pointers.
 * Device memory: the plain or robust solve's; the host-pointer form adds B Nstate doubles for each of lower and upper that
 * is given (held is formed on the host from the returned point's p and g).
 * Not provided: general linear constraints.  The products form: dogleg_amd_optimize_dense_products_batch_bounded below.  The
 * uncertainty and the query covariances of the free variables at the returned p: dogleg_amd_dense_batch_uncertainty_fit / _query_covariance_fit below, with held (and, with a loss,
 * the loss and the weights) in their fit record. */
typedef struct
{
  const double*  lower;   /* [B][Nstate] or NULL: no lower bounds; -INFINITY entries allowed */
  const double*  upper;   /* [B][Nstate] or NULL: no upper bounds; +INFINITY entries allowed */
  unsigned char* held;    /* [B][Nstate] out or NULL: at the returned p[b]: 0 free, 1 held at lower, 2 held at upper */
} dogleg_amd_batch_bounds_t;
int dogleg_amd_optimize_dense_batch_bounded(double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                            dogleg_callback_device_batch_t* f, void* cookie,
                                            const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                            const dogleg_amd_batch_bounds_t* bounds, dogleg_amd_batch_result_t* results,
                                            double* weights);
int dogleg_amd_optimize_dense_batch_bounded_device(double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                   dogleg_callback_device_batch_t* f, void* cookie,
                                                   const dogleg_parameters2_t* parameters, const dogleg_amd_batch_loss_t* loss,
                                                   const dogleg_amd_batch_bounds_t* bounds,
                                                   dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                   double* weights_dev, const unsigned char* active_dev, void* hip_stream);

/* ---- box bounds in the products form of the batch solve: the bounded solve above for a callback that hands back norm2(x),
 * Jt x and JtJ per problem (dogleg_callback_device_batch_products_t), so for ragged batches -- every problem with its own number
 * of measurements -- and for problems whose x and J would not fit.  Steps 1 to 8 written above
 * dogleg_amd_optimize_dense_batch_bounded apply word for word; JtJ, Jt x and norm2(x) are what the callback returned.  Everything
 * the bounds add lies behind the load of the products, on the on-chip JtJ, g and the two cached steps, as it lies behind the sweep
 * in the J form.  There is no loss and there are no weights: the products form has no rows.
 * Step 6 here: the J form's JtJ is a sum of squares, so positive semidefinite, and the fallback's expected improvement is > 0 up
 * to rounding.  Here the callback answers for that: with a JtJ that is not positive semidefinite along the fallback step the
 * improvement may be <= 0, and one that is <= 0 or not finite stays DOGLEG_AMD_BATCH_FAILED for that problem alone.
 * held[b] is what dogleg_amd_dense_products_batch_uncertainty_fit / _query_covariance_fit take in their fit record, unchanged.
 * With bounds that clamp nothing (lower = upper = NULL, infinite entries, a box that is never met) every result has the bits of
 * dogleg_amd_optimize_dense_products_batch, and held is all 0.
 * Everything else is the contract of dogleg_amd_optimize_dense_products_batch and its _device twin: the three layouts of JtJ
 * (packed upper, unpacked with either triangle read as the parameters say; packed lower refused), the finiteness vote over
 * everything read, the live bytes, one callback, one launch and one 4-byte read-back per round, the result struct and the status
 * codes (none is new), dogleg_amd_batch_last_stats; and for the twin the pointer checks (lower, upper and held inside *bounds,
 * which itself is host memory, included), the stream rule and the mask (held of a problem that is not run is not written).
 * Refused with a message and -1 before any device work, outputs untouched: what the plain products twin refuses, and a NULL
 * bounds; the device twin also refuses lower, upper and held as it refuses the other pointers.
 * Device memory: the plain products solve's; the host-pointer form adds B Nstate doubles for each of lower and upper that is
 * given (held is formed on the host from the returned point's p and g).
 * Not provided: a loss (no rows); general linear constraints; bounds for the host-callback dogleg_optimize_dense_products. */
int dogleg_amd_optimize_dense_products_batch_bounded(double* p, unsigned int B, unsigned int Nstate,
                                                     dogleg_callback_device_batch_products_t* f, void* cookie,
                                                     const dogleg_parameters2_t* parameters,
                                                     const dogleg_amd_batch_bounds_t* bounds, dogleg_amd_batch_result_t* results);
int dogleg_amd_optimize_dense_products_batch_bounded_device(double* p_dev, unsigned int B, unsigned int Nstate,
                                                            dogleg_callback_device_batch_products_t* f, void* cookie,
                                                            const dogleg_parameters2_t* parameters,
                                                            const dogleg_amd_batch_bounds_t* bounds,
                                                            dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                            const unsigned char* active_dev, void* hip_stream);

/* ---- box bounds in dogleg_optimize_device2: the sparse (NJnnz > 0) and the dense (NJnnz == 0) device solve minimise norm2(x)
 * (with a loss: F, as dogleg_amd_optimize_device2_robust defines H, g and F) subject to lower <= p <= upper.  The algorithm is
 * steps 1 to 8 written above dogleg_amd_optimize_dense_batch_bounded, word for word, placed in the loop of
 * dogleg_optimize_device2: the start clamp on the host before p is uploaded; the held set and g_F at every evaluated point; the
 * Jt_x_threshold test on |g_F|_inf; the factor of H + lambda I with the held rows and columns made the identity's; the chosen
 * step clipped and its expected improvement formed again when something was clamped; the Cauchy fallback; update_threshold on
 * the step that is applied; held at the returned p.  What follows from there being one problem: a failing fallback (step 6)
 * fails the solve; a NaN bound or lower_i > upper_i is refused before any device work; the ways to stop, the trace and the vnlog
 * records are those of dogleg_optimize_device2, and a fallback step is recorded as a Cauchy step; in the fallback the component
 * that sets alpha ends on its bound's bits whichever way p + alpha d rounds (one ulp short of the bound the variable would be
 * neither held nor free to move, and the next fallback would be cut at alpha ~ 1e-16).
 *
 * How: directly behind every evaluation the library forms the held bytes of that invocation of the callback (per operating
 * point: a rejected trial steps again from the bytes of the point it returns to), writes g_F over Jt x and zeros over the held
 * columns of J, in place, and sums |g_F|_inf, |g_F|^2 and the number of held variables in a fixed order (no floating-point
 * atomics: the same bits on every run; one 24-byte read-back an evaluation).  Everything behind that -- the Cauchy step, the
 * assembly, the factorisation, the Gauss-Newton solve, the expected improvement of an unclipped step -- is the plain solve's
 * code on J_F and g_F; the assembled matrix gets a diagonal of exactly 1 in the held rows after lambda is added.  With a loss the
 * rows are scaled first, then evaluated, then held and masked; F is not affected by the mask.  The sparse mask finds the
 * variable of an entry from THIS call's Jt_rowidx, of which the solve keeps a device copy of its own.  A bounded solve does
 * without the fused step, the assembly at evaluation time and the work the plain solve puts between a step and its wait.
 *   loss        NULL: least squares.  weights: as in dogleg_amd_optimize_device2_robust; NULL unless a loss is given.
 *   bounds      the batch struct with B = 1: lower, upper and held are host arrays of Nstate; lower or upper may be NULL, entries
 *               may be -INFINITY / +INFINITY; held (out, or NULL): 0 free, 1 held at lower, 2 held at upper, at the returned p.
 * Returns norm2(x) (with a loss: F) at the returned p.  A solve that fails returns -1.0 and leaves p, weights and held untouched.
 * With bounds that clamp nothing the iterates are those of dogleg_optimize_device2 (with a loss: of _robust) to rounding: Jt x is
 * summed in another fixed order than the one-pass evaluation of the plain solve sums it; held is all 0.
 *
 * A returned context holds the MASKED point:
 *   Jt_x is g_F (exact zeros in the held entries);
 *   the device-resident J (dlg_point_download, DLG_VEC_J) has exact zeros in the held columns, every other entry keeps its bits
 *   (with a loss: the weighted rows');
 *   the factor held is that of the matrix of step 4: H + lambda I with the held rows and columns made the identity's.
 * dogleg_getOutliernessFactors, dogleg_amd_covariance_blocks, dogleg_amd_marginal_variances, dogleg_amd_covariance_entries and
 * dogleg_amd_query_covariance, called on that context, therefore give the free problem's values on the free variables, and in a
 * held row or column the identity's entries: 1.0 on the diagonal, 0 elsewhere.
 *
 * Refused with a message and -1.0 before any device work, p, weights and held untouched: everything dogleg_optimize_device2
 * refuses; with a loss everything dogleg_amd_optimize_device2_robust refuses; a NULL bounds; weights without a loss; a NaN bound
 * or lower_i > upper_i; more than one rank, whether by dogleg_amd_set_communicator, dogleg_amd_set_allreduce or the
 * environment contract.
 * Device memory beyond the plain (robust) solve's: 2 Nstate doubles of bounds, 2 Nstate bytes of held sets, NJnnz ints of pattern
 * (sparse) and about Nstate / 64 doubles of partial results.
 * Not provided: bounds on several GPUs; bounds for the host-callback entry points (dogleg_optimize2 / _dense2) and in the
 * products form; general linear constraints; a fused or overlapped bounded step. */
double dogleg_amd_optimize_device2_bounded(double* p, unsigned int Nstate, unsigned int Nmeas, unsigned int NJnnz,
                                           const int* Jt_colptr, const int* Jt_rowidx,
                                           dogleg_callback_device_t* f, void* cookie,
                                           const dogleg_amd_batch_loss_t* loss,     /* NULL: least squares */
                                           double* weights,                         /* as in _robust; NULL unless loss */
                                           const dogleg_amd_batch_bounds_t* bounds, /* the batch struct with B = 1 */
                                           const dogleg_parameters2_t* parameters,
                                           dogleg_solverContext_t** returnContext);
/* measurement: the calling thread's last bounded device solve: out[0] = evaluations, out[1] = steps with a clamped component,
 * out[2] = fallbacks (step 6), out[3] = steps taken with a held variable, and, if DOGLEG_AMD_TIMING=1 was set for the solve
 * (two events a launch group on the stream), out[4] = ms in the feature's own kernels over the solve and out[5] = the part of
 * that in the mask passes over J.  Returns the number of entries written (at most n, at most 6). */
int dogleg_amd_bounded_last_stats(double* out, int n);

/* ---- covariance of per-problem query Jacobians of a batch: Var(q) = Jq Sigma_b Jq^T with Sigma_b = (JtJ + lambda I)^-1 of
 * problem b at p[b], the batch twin of dogleg_amd_query_covariance.  Sigma_b is neither formed nor written: per problem the
 * answer is Nq blocks of Qrows x Qrows.  Four entry points, mirroring the four uncertainty entry points above: the same
 * callback types, size classes (Nstate <= DOGLEG_AMD_BATCH_MAX_NSTATE), lambda contract, status codes, stream rule, active
 * mask and pointer checks.
 *   Jq          [B][Nq][Qrows][Nstate], row-major: every problem has Nq >= 1 queries of Qrows rows, 1 <= Qrows <=
 *               DOGLEG_AMD_BATCH_QUERY_MAX_ROWS (the limit of dogleg_amd_query_covariance).  Callers with ragged queries pad
 *               with zero rows: a zero row of Jq gives a zero row and column of its block.
 *   Nobservations (J form only) < 0: Jq Sigma_b Jq^T.  0 <= Nobservations <= Nmeas: the observations-only form
 *               Jq Sigma_b J_obs^T J_obs Sigma_b Jq^T with J_obs the first Nobservations measurement rows of problem b, the
 *               contract of dogleg_amd_query_covariance (0: exact zeros).  Nobservations > Nmeas is refused.  The products
 *               form has no such argument: the form needs J.
 *   out         [B][Nq][Qrows][Qrows] full, row-major, UNSCALED as every covariance output of this library (multiply by
 *               sigma^2).  Every block is bitwise symmetric; in the plain form its diagonal is a sum of squares.
 *   lambda      [B] in/out or NULL, and status [B]: as in dogleg_amd_dense_batch_uncertainty.  A FAILED problem gets NaN in
 *               all of its out and does not disturb the others (the call still returns 0); a SKIPPED problem (active_dev[b]
 *               == 0) has nothing but its status written.
 * One call of the batch callback with every live byte 1 (or the mask), then ONE launch of the library whatever B and Nq
 * are, one synchronisation; dogleg_amd_batch_uncertainty_last_stats covers these calls (the device twins: at most 2 fills).
 * Problem b's output bits do not depend on B, on its position, on its neighbours or on the other queries.
 * The host-pointer forms upload p, lambda and Jq and download out, lambda and status through the page-locked staging buffer
 * of the uncertainty calls (8 B (Nstate + 2 + Nq Qrows (Nstate + Qrows)) bytes); the device forms copy nothing.
 * Refused with a message and -1 before any device work, out / status untouched: a NULL p / f / Jq / out / status, B, Nstate,
 * Nmeas, Nq or Qrows 0, Qrows above DOGLEG_AMD_BATCH_QUERY_MAX_ROWS, Nstate above DOGLEG_AMD_BATCH_MAX_NSTATE, Nobservations
 * above Nmeas, the packed lower layout (products form), a set communicator, device memory that does not fit (the message
 * names the size); the device twins also refuse the pointers described above "device-resident batches" (Jq_dev and out_dev
 * with their full spans).
 * Not covered: per-problem Nq / Qrows, queries of more than DOGLEG_AMD_BATCH_QUERY_MAX_ROWS rows, the observations-only form
 * in the products form. */
#define DOGLEG_AMD_BATCH_QUERY_MAX_ROWS 16
int dogleg_amd_dense_batch_query_covariance(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                            dogleg_callback_device_batch_t* f, void* cookie, double* lambda,
                                            const double* Jq, unsigned int Nq, unsigned int Qrows, int Nobservations,
                                            double* out, int* status);
int dogleg_amd_dense_products_batch_query_covariance(const double* p, unsigned int B, unsigned int Nstate,
                                                     dogleg_callback_device_batch_products_t* f, void* cookie,
                                                     const dogleg_parameters2_t* parameters, double* lambda,
                                                     const double* Jq, unsigned int Nq, unsigned int Qrows,
                                                     double* out, int* status);
int dogleg_amd_dense_batch_query_covariance_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                   dogleg_callback_device_batch_t* f, void* cookie, double* lambda_dev,
                                                   const double* Jq_dev, unsigned int Nq, unsigned int Qrows, int Nobservations,
                                                   double* out_dev, int* status_dev,
                                                   const unsigned char* active_dev, void* hip_stream);
int dogleg_amd_dense_products_batch_query_covariance_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                            dogleg_callback_device_batch_products_t* f, void* cookie,
                                                            const dogleg_parameters2_t* parameters, double* lambda_dev,
                                                            const double* Jq_dev, unsigned int Nq, unsigned int Qrows,
                                                            double* out_dev, int* status_dev,
                                                            const unsigned char* active_dev, void* hip_stream);

/* ---- uncertainty and query calls at the optimum of a robust or bounded fit: the eight calls above (uncertainty and query
 * covariance, J and products form, host and _device) with one more argument, a record that says how the fit was made.  Without
 * it the eight compute (JtJ + lambda I)^-1 of the unweighted, unconstrained problem, which at an optimum whose outliers were
 * down-weighted, or whose variables sit on a bound, is the covariance of another problem.  The weights are applied while a row
 * is staged and the held set is a mask on the matrix that is factorised: J is read as often as in the plain call and nothing
 * is written back into it.
 *   fit->loss     NULL: unweighted.  Otherwise its featureSize (1 .. 4, <= 1: 1; called lfs below) says how many consecutive rows
 *                 share a weight; kind and scale are read only if weights is NULL.  lfs is independent of the featureSize
 *                 argument of the outlierness factors, which stays 1 or 2.
 *   fit->weights  [B][Nmeas / lfs] or NULL.  Given (what the robust or bounded solve wrote): used as they come; 0 is allowed and
 *                 drops the feature; a weight that is negative or not finite makes that problem DOGLEG_AMD_BATCH_UNC_FAILED alone
 *                 (so a problem whose solve FAILED, with its NaN weights, fails here too).  NULL with a loss: w_f = rho'(s_f) is
 *                 computed from the callback's x at p[b], the bits the robust solve returns at that p.
 *   fit->held     [B][Nstate] or NULL: nonzero = variable held (what the bounded solve wrote).
 * For problem b, with row r in weight feature r / lfs:
 *   1. x~_r = sqrt(w_f) x_r and J~_r = sqrt(w_f) J_r, every product rounded once, as a callback that scales the rows would write
 *      them.  H = J~^T J~.
 *   2. After lambda is added, every held row and column of the matrix to be factorised gets zero off-diagonals and a diagonal of 1
 *      (step 4 of the bounded solve); the lambda schedule (0 -> 1e-10 -> x10) runs on that matrix.  With every variable held the
 *      factorisation succeeds at the lambda that came in.
 *   3. covariance: (H_FF + lambda I)^-1 on the free variables; every entry in a held row or column is exactly +0.0 (a variable on
 *      its bound is not estimated).  variances: that diagonal.
 *   4. factors: the leverage block is J~_f Sigma J~_f^T with x~_f; a computed scale is Nmeas / (4 (N_F + 1) |x~|^2 / (Nmeas - N_F - 1))
 *      with N_F the number of free variables and |x~|^2 the sum of the squares of the weighted x (NOT the robust cost).  The
 *      refusal of a scale to be computed while Nmeas <= Nstate + 1 is unchanged.
 *   5. query: Jq Sigma Jq^T; the observations-only form takes J_obs = the first Nobservations rows of J~, and with a loss
 *      Nobservations must be a multiple of lfs.
 *   6. the products form has no rows: it takes held only.
 * fit == NULL, or all three members NULL: the call without _fit, bit for bit.  With DOGLEG_AMD_LOSS_TRIVIAL of size 1 and no held
 * variable, and with weights that are all 1.0, Sigma, the variances and the query blocks have the bits of the call without _fit
 * too; at other lfs the rows of x are summed in tiles of another height, so a computed scale and the factors may differ in their
 * last bits, as they may from a callback that scales the rows.
 * Everything else is the contract of the call without _fit: one callback, one launch, one synchronisation
 * (dogleg_amd_batch_uncertainty_last_stats covers these calls), the active mask, the stream rule, the status codes, NaN in every
 * output of a FAILED problem, and problem b's bits independent of B, of its position and of its neighbours.
 * The host-pointer forms stage weights and held through the page-locked buffer of the uncertainty calls, 8 B Nmeas / lfs bytes
 * and B Nstate bytes more, and keep as many in device memory; the _device forms read them where they lie (fit itself is host
 * memory) and copy nothing.
 * Refused with a message and -1 before any device work, outputs untouched: what the call without _fit refuses; weights without
 * loss; an unknown kind, or a scale that is not finite and > 0 (unless TRIVIAL), while weights is NULL; featureSize above 4 or not
 * dividing Nmeas; with a loss, an Nobservations >= 0 that is not a multiple of lfs; a loss or weights in the products form; the
 * _device forms also refuse weights and held as they refuse their other pointers, over [B][Nmeas / lfs] doubles and [B][Nstate]
 * bytes.
 * Not provided: a loss in the products form (it has no rows); per-problem loss scales;
 * losses that are not concave in s; weights that differ between J and x; marking outliers on a batch. */
typedef struct
{
  const dogleg_amd_batch_loss_t* loss;     /* NULL: unweighted.  Gives featureSize (1..4) of the weights; kind / scale are read only if weights is NULL */
  const double*                  weights;  /* [B][Nmeas / loss->featureSize] in, or NULL: w_f = rho'(s_f) is computed from x at p[b] with *loss */
  const unsigned char*           held;     /* [B][Nstate] in, or NULL: nonzero = variable held (what the bounded solve wrote) */
} dogleg_amd_batch_fit_t;
int dogleg_amd_dense_batch_uncertainty_fit(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           double* lambda, double* covariance, double* variances, double* factors,
                                           double* scale, int featureSize, int* status, const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_products_batch_uncertainty_fit(const double* p, unsigned int B, unsigned int Nstate,
                                                    dogleg_callback_device_batch_products_t* f, void* cookie,
                                                    const dogleg_parameters2_t* parameters,
                                                    double* lambda, double* covariance, double* variances, int* status,
                                                    const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_batch_uncertainty_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                  dogleg_callback_device_batch_t* f, void* cookie,
                                                  double* lambda_dev, double* covariance_dev, double* variances_dev,
                                                  double* factors_dev, double* scale_dev, int featureSize, int* status_dev,
                                                  const unsigned char* active_dev, void* hip_stream,
                                                  const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_products_batch_uncertainty_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                           dogleg_callback_device_batch_products_t* f, void* cookie,
                                                           const dogleg_parameters2_t* parameters,
                                                           double* lambda_dev, double* covariance_dev, double* variances_dev,
                                                           int* status_dev, const unsigned char* active_dev, void* hip_stream,
                                                           const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_batch_query_covariance_fit(const double* p, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                dogleg_callback_device_batch_t* f, void* cookie, double* lambda,
                                                const double* Jq, unsigned int Nq, unsigned int Qrows, int Nobservations,
                                                double* out, int* status, const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_products_batch_query_covariance_fit(const double* p, unsigned int B, unsigned int Nstate,
                                                         dogleg_callback_device_batch_products_t* f, void* cookie,
                                                         const dogleg_parameters2_t* parameters, double* lambda,
                                                         const double* Jq, unsigned int Nq, unsigned int Qrows,
                                                         double* out, int* status, const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_batch_query_covariance_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate, unsigned int Nmeas,
                                                       dogleg_callback_device_batch_t* f, void* cookie, double* lambda_dev,
                                                       const double* Jq_dev, unsigned int Nq, unsigned int Qrows,
                                                       int Nobservations, double* out_dev, int* status_dev,
                                                       const unsigned char* active_dev, void* hip_stream,
                                                       const dogleg_amd_batch_fit_t* fit);
int dogleg_amd_dense_products_batch_query_covariance_fit_device(const double* p_dev, unsigned int B, unsigned int Nstate,
                                                                dogleg_callback_device_batch_products_t* f, void* cookie,
                                                                const dogleg_parameters2_t* parameters, double* lambda_dev,
                                                                const double* Jq_dev, unsigned int Nq, unsigned int Qrows,
                                                                double* out_dev, int* status_dev,
                                                                const unsigned char* active_dev, void* hip_stream,
                                                                const dogleg_amd_batch_fit_t* fit);

/* ---- extension (not in the reference): the Jacobian of a DEVICE callback checked against central differences, on the
 * device.  dogleg_testGradient* above take host callbacks, one variable a call.  Here the whole Jacobian is compared, and
 * on a sparse problem the variables that share no measurement row are perturbed together (Curtis, Powell, Reid): a
 * first-fit colouring of the variables over the pattern gives the groups, 15 of them on a problem with 15 entries a row
 * whatever Nstate is, and the check costs 2 * ncolours evaluations of the callback.
 *
 * The arithmetic is that of dogleg_testGradient (reference dogleg.c:352-522): for a group G, x0, J0 at
 * p0 - delta/2 sum_{v in G} e_v and x1, J1 at p0 + delta/2 sum_{v in G} e_v; for a declared entry (row r, variable v in G)
 * observed = (x1[r] - x0[r]) / delta, reported = (J0 + J1) / 2 at that entry, err = |reported - observed|, relative error
 * err / ((|reported| + |observed|) / 2), 0 / 0 = 0.  An entry is bad when err > atol + rtol (|reported| + |observed|) / 2
 * or when one of the four values is not finite.  delta <= 0 selects the reference's 1e-6; rtol and atol are the caller's
 * (negative or NaN: refused).
 *
 * A row with NO declared entry in G must not move: where x1[r] != x0[r] the pair (row, group) is counted in noutside and
 * reported in `bad` with var = -1 - (index of the group), reported = 0 and its observed.
 *
 * All per-group work is enqueued on one stream (a kernel that perturbs p, the callback twice, the compare kernels), with
 * one synchronisation and one download at the end.  Buffers live for the call only. */
typedef struct
{
  long long nchecked;     /* Jacobian entries compared                                                   */
  long long nbad;         /* err > atol + rtol (|rep| + |obs|) / 2, or a non-finite x / J involved        */
  long long nnonfinite;   /* of those: non-finite                                                        */
  long long noutside;     /* sparse: (row, colour) pairs with NO declared entry whose x moved (obs != 0) */
  double max_error, max_error_relative;   /* over the finite entries; 0 / 0 = 0 as in the reference       */
  int worst_var, worst_meas; double worst_reported, worst_observed;   /* an entry attaining max_error     */
  int ncolours, evaluations;              /* callback invocations = 2 ncolours                            */
} dogleg_amd_jacobian_report_t;
typedef struct { int problem, var, meas; double reported, observed; } dogleg_amd_jacobian_entry_t;
#define DOGLEG_AMD_JACOBIAN_ONE_AT_A_TIME 1   /* flags: every variable its own group on a sparse problem too */

/* the groups: colour[v] of the first-fit colouring in natural variable order (v takes the smallest colour that no
 * variable before it sharing a row with it holds; a variable in no row gets 0).  Host only.  Returns the number of
 * colours, or -1 (message) on a bad pattern: see dogleg_optimize_device2 for the pattern's contract. */
int dogleg_amd_jacobian_colouring(unsigned Nstate, unsigned Nmeas, const int* Jt_colptr, const int* Jt_rowidx,
                                  int* colour /* [Nstate] out */);
/* p0 on the host.  The pattern as dogleg_optimize_device2 takes it; NJnnz == 0 and NULL pattern pointers: dense, every
 * variable its own group.  var_error[Nstate] (or NULL): the largest finite err per variable.  bad[max_bad] (or NULL)
 * receives min(nbad + noutside, max_bad) records, sorted by (meas, var); which survive beyond max_bad is unspecified.
 * worst_var is -1 when no finite entry was compared.  Returns the number of records written to bad, or -1 (message;
 * outputs untouched when the arguments are refused: a NULL p0 / f / report, zero sizes, a pattern that disagrees with
 * NJnnz or whose row indices do not ascend within a column, a negative or NaN rtol / atol, a set communicator). */
int dogleg_amd_check_jacobian_device(const double* p0, unsigned Nstate, unsigned Nmeas, unsigned NJnnz,
                                     const int* Jt_colptr, const int* Jt_rowidx,
                                     dogleg_callback_device_t* f, void* cookie,
                                     double delta, double rtol, double atol, int flags,
                                     dogleg_amd_jacobian_report_t* report,
                                     double* var_error /* [Nstate] max err per variable, or NULL */,
                                     dogleg_amd_jacobian_entry_t* bad, int max_bad);
/* the same for a batch callback: column v of all B problems in one pair of evaluations (2 Nstate invocations whatever B
 * is, every live byte 1).  reports[b] is problem b's and does not depend on B or on its neighbours; bad records carry the
 * problem, sorted by (problem, meas, var); *nbad_total (or NULL) receives the number written.  0 / -1; refused as above,
 * and Nstate above DOGLEG_AMD_BATCH_MAX_NSTATE. */
int dogleg_amd_check_jacobian_device_batch(const double* p0 /* [B][Nstate] */, unsigned B, unsigned Nstate, unsigned Nmeas,
                                           dogleg_callback_device_batch_t* f, void* cookie,
                                           double delta, double rtol, double atol,
                                           dogleg_amd_jacobian_report_t* reports /* [B] */,
                                           dogleg_amd_jacobian_entry_t* bad, int max_bad, long long* nbad_total);
/* dogleg_testGradient for a device callback: the same table on stdout for variable `var` (two evaluations, one compare
 * launch, one download; the print on the host). */
void dogleg_amd_testGradient_device(unsigned var, const double* p0, unsigned Nstate, unsigned Nmeas, unsigned NJnnz,
                                    const int* Jt_colptr, const int* Jt_rowidx, dogleg_callback_device_t* f, void* cookie);
/* measurement: the calling thread's last check: out[0] = callback invocations, out[1] = kernel launches of the library,
 * out[2] = stream synchronisations, out[3] = copies on the stream; counted where they are issued; and, if
 * DOGLEG_AMD_CHECK_TIMING=1 was set for a dogleg_amd_check_jacobian_device call (three events a group on the stream),
 * out[4] = ms in the callback's kernels, out[5] = ms in the library's compare kernels.  Returns the number of entries
 * written (at most n, at most 6). */
int dogleg_amd_check_jacobian_last_stats(double* out, int n);  /* callback calls, library launches, syncs, copies */

/* ---- extension (not in the reference): numeric Jacobians for a batch whose model comes as VALUES ONLY.  An adapter, not a
 * solver: dogleg_amd_batch_numeric_callback is a dogleg_callback_device_batch_t that evaluates the caller's values-only model
 * at p and at perturbed copies of p and writes the difference quotients into the J it is handed, [B][Nmeas][Nstate].  Passed
 * as f with cookie = the handle it serves EVERY J-form batch entry point above -- the plain, robust and bounded solves, the
 * uncertainty, query and _fit calls, all their _device twins and dogleg_amd_check_jacobian_device_batch -- and none of them
 * knows.  Not covered: the products form, the sparse and the single-problem solvers.
 *
 * The values callback evaluates x at `copies` points per problem.  All pointers are device memory.
 *   p_dev    in : [copies][B][Nstate]
 *   x_dev    out: [copies][B][Nmeas]
 *   live_dev in : [B] bytes; problem b is evaluated in every copy or in none (what is written for a dead one is ignored)
 *   hip_stream  : enqueue here, do not synchronise
 *
 * The step rule (include/dogleg_numeric_step.h, one function for host and device; dogleg_amd_numeric_step below is that
 * function).  With p = p[b][j], lo / hi = lower / upper[b][j] (-inf / +inf without) and h = delta_rel |p| + delta_abs:
 *   forward: tp = p + h, and where tp > hi: tp = max(p - h, lo).  d = tp - p,  J[r][j] = (x(tp)[r] - x(p)[r]) / d
 *   central: tp = min(p + h, hi), tm = max(p - h, lo).            d = tp - tm, J[r][j] = (x(tp)[r] - x(tm)[r]) / d
 * (central: one-sided by itself when p lies on a bound).  d == 0, a variable with lo == hi, gives a column of exact zeros (its
 * gradient entry is then exactly 0, so the bounded solve reports held = 0 for it: it stays put because its box is a point).
 * delta_rel and delta_abs both <= 0: 2^-26 for both (forward), 2^-17 for both (central).  The quotient is one IEEE division.
 * With the bounds of dogleg_amd_optimize_dense_batch_bounded no point outside the box is ever evaluated: the solve keeps p
 * inside, and the rule keeps the perturbed points inside.  The copies: copy 0 is p, copy 1 + j the plus point of variable j,
 * and for central differences copy 1 + Nstate + j its minus point; x_dev handed back is copy 0's x.
 *
 * One invocation of the adapter is ONE launch that writes the copies, ONE call of f and ONE launch that forms J, whatever B
 * is, all on the stream it is handed and without a synchronisation.  Dead problems' x and J are not touched.  Non-finite
 * values propagate by the arithmetic alone, so a problem whose model fails fails alone.
 *
 * dogleg_amd_batch_numeric_create allocates, on the current device, the copies: K B (Nstate + Nmeas) + B Nstate doubles with
 * K = Nstate + 1 (forward) or 2 Nstate + 1 (central) -- about 2 GB for B = 131 072 problems of 96 x 16 with forward
 * differences -- plus 2 B Nstate doubles for host bounds, which it copies; bounds_on_device != 0: lower / upper are device
 * arrays that are read where they lie at every invocation (they are the caller's to keep alive, and are not checked).  NULL and
 * a message: B, Nstate or Nmeas 0, Nstate above DOGLEG_AMD_BATCH_MAX_NSTATE, a NULL f, an unknown scheme, a negative or NaN
 * delta, host bounds with lower[b][j] > upper[b][j] or a NaN, a size that does not fit (the message names it), no device.  The
 * arguments are checked before any device is touched.  A handle serves calls of its B or fewer problems of its shape, one at a
 * time.  The adapter can return nothing: invoked with a B above the handle's it writes NaN into x of every live problem -- each
 * then fails alone with FAILED --, calls nothing and prints one message. */
typedef void (dogleg_callback_device_batch_values_t)(const double* p_dev, double* x_dev, const unsigned char* live_dev,
                                                     unsigned int B, unsigned int copies, void* hip_stream, void* cookie);
#define DOGLEG_AMD_NUMERIC_FORWARD 0
#define DOGLEG_AMD_NUMERIC_CENTRAL 1
typedef struct
{
  int scheme;                     /* DOGLEG_AMD_NUMERIC_FORWARD or _CENTRAL                                     */
  double delta_rel, delta_abs;    /* both <= 0: the scheme's default                                            */
  const double* lower;            /* [B][Nstate] or NULL; entries may be -inf                                   */
  const double* upper;            /* [B][Nstate] or NULL; entries may be +inf                                   */
  int bounds_on_device;           /* lower / upper are device memory                                            */
} dogleg_amd_numeric_options_t;
struct dogleg_amd_batch_numeric;  /* opaque */
/* opt == NULL: forward differences, default deltas, no bounds */
struct dogleg_amd_batch_numeric* dogleg_amd_batch_numeric_create(unsigned B, unsigned Nstate, unsigned Nmeas,
                                                                 dogleg_callback_device_batch_values_t* f, void* cookie,
                                                                 const dogleg_amd_numeric_options_t* opt);
void dogleg_amd_batch_numeric_destroy(struct dogleg_amd_batch_numeric* h);
/* a dogleg_callback_device_batch_t: pass it as f, with cookie = h, to any J-form batch entry point */
void dogleg_amd_batch_numeric_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                       unsigned int B, void* hip_stream, void* cookie);
/* measurement, since the handle was made: out[0] = invocations of the adapter, out[1] = invocations of f, out[2] =
 * problem-copies requested of f (copies x B, summed), out[3] = kernel launches of the library, and, if DOGLEG_AMD_BATCH_TIMING=1
 * was set when an invocation ran (four events an invocation on its stream, read here: this call waits for the last of them),
 * out[4] = ms in f's kernels, out[5] = ms in the library's.  Returns the number of entries written (at most n, at most 6). */
int dogleg_amd_batch_numeric_stats(struct dogleg_amd_batch_numeric* h, double* out, int n);
/* tests and debugging: the device buffers of the handle as the last invocation left them: p_copies [K][B'][Nstate], x_copies
 * [K][B'][Nmeas], divisor [B'][Nstate] with B' the B of that invocation.  Returns K, or -1 on a NULL handle. */
int dogleg_amd_batch_numeric_buffers(struct dogleg_amd_batch_numeric* h, const double** p_copies_dev,
                                     const double** x_copies_dev, const double** divisor_dev);
/* the step rule on the host: the plus point, the minus point (forward: p) and the divisor of one variable, with the deltas as
 * given (no defaults are substituted here) */
void dogleg_amd_numeric_step(int scheme, double p, double lo, double hi, double delta_rel, double delta_abs,
                             double* tp, double* tm, double* d);

/* ---- extension (not in the reference): numeric Jacobians for ONE problem whose model comes as VALUES ONLY, sparse or dense.
 * An adapter, not a solver: dogleg_amd_numeric_callback is a dogleg_callback_device_t that evaluates the caller's values-only
 * model at p and at perturbed copies of p and writes x and the difference quotients into the buffers it is handed.  Passed as f
 * with cookie = the handle it serves dogleg_optimize_device2, dogleg_amd_optimize_device2_robust, _bounded,
 * dogleg_amd_check_jacobian_device, dogleg_amd_testGradient_device and the held-factor users of a returned context, and none
 * of them knows.  Not covered: the products form, the host-callback solvers, several GPUs.
 *
 * The pattern is the one dogleg_optimize_device2 takes: Jt in CSC, rows ascending within a column, and J_dev receives the values
 * of Jt in pattern order.  NJnnz == 0 (the pattern pointers are then not read) is the dense solve: J[Nmeas][Nstate] row-major.
 * Variables that share no measurement row are perturbed TOGETHER: the colouring is exactly dogleg_amd_jacobian_colouring's
 * (first fit, natural order, a variable in no row gets colour 0), so the adapter and the Jacobian check agree on the groups.
 * With C colours the model is evaluated at K = C + 1 (forward) or 2 C + 1 (central) points per invocation -- 16 or 31 on a
 * block-arrowhead pattern of 15 entries a row whatever Nstate is.  A dense problem has every variable as its own colour, C =
 * Nstate.  One row that holds R variables forces R colours; dogleg_amd_numeric_plan tells C, K and the memory without a device.
 *
 * The copies: copy 0 is p; copy 1 + c has every variable of colour c at its plus point; copy 1 + C + c (central) has them at
 * their minus points; x_dev handed back is copy 0's x.  For entry t of Jt in row r with variable v = Jt_rowidx[t] of colour c:
 *   J[t] = d[v] == 0 ? 0 : (x[1 + c][r] - xm[r]) / d[v],   xm = copy 1 + C + c (central) or copy 0 (forward)
 * one subtraction and one IEEE division.  The step rule, its defaults and the options are those of the batch adapter above
 * (dogleg_numeric_step, dogleg_amd_numeric_options_t), with lower / upper [Nstate] here, host arrays that are copied or, with
 * bounds_on_device, device arrays read where they lie.  With the bounds of dogleg_amd_optimize_device2_bounded in the options
 * no point outside the box is ever evaluated, and a variable with lower == upper has exact zeros in all its entries.
 *
 * One invocation is ONE launch that writes the copies and divisors, ONE call of f and ONE launch that forms x and J, whatever
 * Nstate, Nmeas and C are, on the stream it is handed, with no synchronisation, allocation or copy.  Non-finite values
 * propagate by the arithmetic alone.  The handle owns K (Nstate + Nmeas) + Nstate doubles and, for a sparse problem, Nstate +
 * Nmeas + 1 + 2 NJnnz ints (plus Nstate doubles per copied host bound), on the device that is current at creation.
 *
 * dogleg_amd_numeric_create returns NULL with a message, before any device is touched, for: Nstate or Nmeas 0, a NULL f, a
 * pattern that is not a valid Jt or disagrees with NJnnz, an unknown scheme, a negative or NaN delta, host bounds with lower[j] >
 * upper[j] or a NaN, a size that does not fit (the message names C, K, the bytes and the longest row); then for no device.  A
 * handle serves one call at a time. */
typedef void (dogleg_callback_device_values_t)(const double* p_dev /* [copies][Nstate] */,
                                               double* x_dev       /* [copies][Nmeas]  */,
                                               unsigned int copies, void* hip_stream, void* cookie);
struct dogleg_amd_numeric;  /* opaque */
/* host only, touches no device: the colouring (colour[Nstate], or NULL), the copies K (or NULL) and the device bytes the handle
 * would own without copied bounds (or NULL) for scheme DOGLEG_AMD_NUMERIC_FORWARD or _CENTRAL.  Returns C, or -1 with a message. */
int dogleg_amd_numeric_plan(unsigned Nstate, unsigned Nmeas, unsigned NJnnz, const int* Jt_colptr, const int* Jt_rowidx,
                            int scheme, int* colour, int* copies, double* device_bytes);
/* opt == NULL: forward differences, default deltas, no bounds */
struct dogleg_amd_numeric* dogleg_amd_numeric_create(unsigned Nstate, unsigned Nmeas, unsigned NJnnz,
                                                     const int* Jt_colptr, const int* Jt_rowidx,
                                                     dogleg_callback_device_values_t* f, void* cookie,
                                                     const dogleg_amd_numeric_options_t* opt);
void dogleg_amd_numeric_destroy(struct dogleg_amd_numeric* h);
/* a dogleg_callback_device_t: pass it as f, with cookie = h */
void dogleg_amd_numeric_callback(const double* p_dev, double* x_dev, double* J_dev, void* hip_stream, void* cookie);
/* measurement, since the handle was made: out[0] = invocations of the adapter, out[1] = invocations of f, out[2] = copies
 * requested of f (summed), out[3] = kernel launches of the library, and, if DOGLEG_AMD_NUMERIC_TIMING=1 was set when an invocation
 * ran (four events an invocation on its stream, read here: this call waits for the last of them), out[4] = ms in f's kernels,
 * out[5] = ms in the library's.  Returns the number of entries written (at most n, at most 6). */
int dogleg_amd_numeric_stats(struct dogleg_amd_numeric* h, double* out, int n);
/* tests and debugging: the device buffers of the handle as the last invocation left them: p_copies [K][Nstate], x_copies
 * [K][Nmeas], divisor [Nstate].  Returns K, or -1 on a NULL handle. */
int dogleg_amd_numeric_buffers(struct dogleg_amd_numeric* h, const double** p_copies_dev, const double** x_copies_dev,
                               const double** divisor_dev);

/* ---- built-in fit models of the batch solver: the textbook curves "one fit per pixel or track" users fit, so that a batch can be
 * fitted without writing device code.  The models, their parameters and the fixed order of their arithmetic: dogleg_batch_models.h
 * (x_i = s_i (f_i(p) - y_i), J its exact derivative; EXPDECAY N = 3, GAUSS1D N = 4, GAUSS2D N = 5, GAUSS2D_ELLIPTIC N = 6).
 *
 * The model record is host memory; its arrays are device-accessible memory of the current device in EVERY entry point below (the
 * host-pointer solve included) and are checked as the _device twins check their pointers, before any device work:
 *   kind        DOGLEG_AMD_MODEL_*
 *   Nmeas       rows per problem, > 0
 *   width, height   the 2D kinds: the pixel window, width * height == Nmeas (row i is pixel (i mod width, i div width)); the 1D
 *               kinds: both 0
 *   y           [B][Nmeas] the data, required
 *   t           the abscissae of the 1D kinds: NULL (t_i = i), [Nmeas] shared by all problems, or [B][Nmeas] with t_per_problem
 *               != 0.  Must be NULL for the 2D kinds
 *   scale       [B][Nmeas] s_i (for instance 1 / the standard deviation of y_i), or NULL: 1
 * A sigma of exactly 0, a NaN datum and the like give non-finite rows: that problem ends DOGLEG_AMD_BATCH_FAILED by the rule of
 * dogleg_amd_optimize_dense_batch, alone.
 *
 * 1. The model as an ordinary callback.  dogleg_amd_batch_model_callback is a dogleg_callback_device_batch_t whose cookie is a
 * const dogleg_amd_batch_model_t* (Nstate = dogleg_amd_batch_model_nstate(kind), Nmeas = its Nmeas): one launch on the stream
 * it is given, x and J of the live problems.  With it every batch entry point above takes a built-in model: the plain, robust and
 * bounded solves, the uncertainty, query and _fit calls, their _device twins and dogleg_amd_check_jacobian_device_batch.  The
 * record is not checked there: a record the fused solve would refuse makes the callback write nothing.
 * dogleg_amd_batch_model_callback_invocations: how often it has run in this process (measurement).
 *
 * 2. The fused solve.  dogleg_amd_optimize_dense_batch_model[_device] have the contract of dogleg_amd_optimize_dense_batch and
 * dogleg_amd_optimize_dense_batch_bounded (bounds != NULL) and of their _device twins in every respect but one: no callback is
 * invoked and no x / J buffer exists.  The lane that would stage row i of J forms it in registers, through the same function as the
 * callback above, and puts it into the on-chip tile; the sweep behind it is the J form's.  EVERY OUTPUT HAS THE BITS OF THE SAME
 * SOLVE THROUGH dogleg_amd_batch_model_callback (with bounds: of the bounded solve through it): p, the six result fields, lambda,
 * held.  Device memory: the state only, B (N (N + 11) / 2 + 8) doubles, plus the bounds in the host-pointer form.  A round is ONE
 * launch and one 4-byte read-back; dogleg_amd_batch_last_stats reports the rounds and 0 ms of callback.  evaluations counts the
 * evaluations of the model for that problem.
 * Refused with a message and -1 before any device work, outputs untouched: what the plain or bounded twin refuses, a NULL model or
 * a NULL y, an unknown kind, Nmeas 0, a 2D kind whose width * height != Nmeas, a 1D kind with a width or height, t given for a 2D
 * kind, a set communicator, and arrays of the record that are not device-accessible over their span.
 *
 * Not provided: a loss in the fused form (the adapter route has it: dogleg_amd_optimize_dense_batch_robust / _bounded with the
 * callback above); float or integer data in this record (item 5 takes them); rotated Gaussians; user-defined models in the fused
 * form (that is what a callback is).
 *
 * 3. Maximum-likelihood fits of count data.  dogleg_amd_optimize_dense_batch_model_mle[_device] are the fused solve above with a
 * likelihood.  DOGLEG_AMD_LIKELIHOOD_GAUSS: the fused solve above, bit for bit.  DOGLEG_AMD_LIKELIHOOD_POISSON: the data y_i >= 0
 * are counts and the model value f_i(p) their expectation, which must be > 0:
 *   cost   F(p) = sum_i d_i, the Poisson deviance (2 (-log L) up to a constant): d_i = 2 (r_i - y_i log(f_i / y_i)), r_i = f_i - y_i,
 *          and d_i = 2 f_i where y_i == 0.0
 *   rows   x~_i = r_i q_i, J~_ij = (d f_i / d p_j) q_i with q_i = 1 / sqrt(f_i): g = J~' x~ = sum (r_i / f_i) grad f_i = 1/2 grad F,
 *          H = J~' J~ = sum grad f_i grad f_i' / f_i, the Fisher information (Fisher scoring; sum (y_i / f_i^2) grad f grad f' is
 *          not taken: the zero counts drop out of it and H loses definiteness at low counts)
 *   loop   that of the fused solve, plain or bounded, unchanged: F takes the place of norm2(x) in the gain ratio and in
 *          results[b].norm2_x, g and H that of J'x and J'J everywhere else, as in the robust solve
 * A row with !(f_i > 0) makes a point infeasible: its cost is +infinity.  An infeasible TRIAL point is a rejected step by the
 * ordinary rule (rho = -infinity: the trust region shrinks and the loop steps again from the cached steps, down to
 * DOGLEG_AMD_BATCH_TRUSTREGION); an infeasible START point ends DOGLEG_AMD_BATCH_FAILED, alone.  A negative or NaN datum makes the
 * cost or the gradient NaN at the first evaluation: FAILED, alone.  The arithmetic of a row: dogleg_batch_model_row_poisson in
 * dogleg_batch_models.h.  In every other respect the contract is that of dogleg_amd_optimize_dense_batch_model[_device]: bounds or
 * none, held, the active mask, the stream rule, one launch and one 4-byte read-back a round, no x / J buffer.
 * Refused with a message and -1 before any device work, outputs untouched: what the fused solve above refuses, a likelihood that
 * is neither of the two, and model->scale != NULL with POISSON (counts carry their own variance).
 *
 * dogleg_amd_batch_model_fisher_callback is a dogleg_callback_device_batch_t whose cookie is the model record (scale NULL); it
 * writes x~ and J~ of the Poisson definition, NaN in an infeasible row, in one launch.  It is there for the uncertainty, query and
 * _fit calls: through it they return (H + lambda I)^-1, at the optimum of the Poisson solve the Cramer-Rao bound of the fit; pass
 * held of the bounded solve in the fit record.  ITS J~ IS NOT d x~ / d p (that has the term -(f + y) / (2 f^(3/2)) grad f instead
 * of grad f / sqrt(f)), so dogleg_amd_check_jacobian_device_batch reports it, rightly, and a solve through it would minimise
 * Pearson's chi^2 with a wrong Jacobian: EVERY BATCH SOLVE ENTRY POINT REFUSES THIS CALLBACK with a message and -1 (the plain,
 * robust and bounded solves and their _device twins).
 * Not provided: a loss in this form; other likelihoods; a gain or offset per datum in this record (item 5 has the sCMOS model; no
 * EMCCD excess-noise model); the products form.
 *
 * 4. The fused uncertainty and query calls.  dogleg_amd_dense_batch_model_uncertainty[_device] and
 * dogleg_amd_dense_batch_model_query_covariance[_device] are dogleg_amd_dense_batch_uncertainty_fit[_device] and
 * dogleg_amd_dense_batch_query_covariance_fit[_device] of a built-in model with no callback and no x / J buffer: the error bars of
 * a fused fit (with POISSON at its optimum: the Cramer-Rao bound) without the B Nmeas (Nstate + 1) doubles a callback would write.
 * Nstate = dogleg_amd_batch_model_nstate(model->kind), Nmeas = model->Nmeas.  held: [B][Nstate] bytes as the bounded fused solve
 * writes them (device memory in the _device twins), or NULL; it has the meaning of held in dogleg_amd_batch_fit_t.  There is no
 * loss and there are no weights, as in the fused solve.
 * EVERY OUTPUT HAS THE BITS OF THE CALL IT REPLACES: lambda, covariance, variances, factors, scale, status, out, the NaN of a problem
 * that failed and the untouched outputs of one that was skipped.  With DOGLEG_AMD_LIKELIHOOD_GAUSS that call is the _fit call (held
 * == NULL: the call without _fit) through dogleg_amd_batch_model_callback with the fit {NULL, NULL, held}; with
 * DOGLEG_AMD_LIKELIHOOD_POISSON the same call through dogleg_amd_batch_model_fisher_callback: the covariance is the inverse Fisher
 * information, a problem with a row of !(f_i > 0) is DOGLEG_AMD_BATCH_UNC_FAILED, alone, and a scale computed for it is NaN.  All
 * other semantics are those of the replaced calls: featureSize, scale[b] <= 0 meaning "compute it" (from the sum of the squares of
 * the rows, x~ with POISSON, and the free variables), the lambda loop on a failed pivot, Nobservations (the first rows of the
 * model), the limits on Qrows and Nq, the mask and the stream.  One launch; the rows are formed in the lanes in the first sweep
 * and, for the factors, again in the second.  Device memory of a call: the host-pointer forms keep the staged inputs and outputs
 * (p, held, lambda, scale, status, and covariance, variances, factors or Jq and out as asked for); the _device twins B doubles
 * where lambda_dev is NULL and nothing otherwise.  dogleg_amd_batch_uncertainty_last_stats covers them and reports 0 ms of callback.
 * Refused with a message and -1 before any device work, outputs untouched: what the replaced call refuses, what the fused solve
 * refuses of a model record, an unknown likelihood, model->scale with POISSON, a set communicator, and arrays of the record (and,
 * in the _device twins, of the call) that are not device-accessible over their span.
 * Not provided: a loss in the fused form; float or integer data in this record (item 5 takes them); the products form; queries of
 * more than DOGLEG_AMD_BATCH_QUERY_MAX_ROWS rows; other likelihoods.
 *
 * 5. Raw camera frames.  dogleg_amd_batch_camera_t is the model record with the data as the camera delivers them: readings of
 * uint16 ADU, float or double, and, for an sCMOS sensor, the per-pixel calibration maps.  Every call of items 1 to 4 has a camera
 * twin that forms the datum in the lane that forms the row, so that the only per-problem stream is the raw one (2 bytes a pixel
 * where the model record reads 8) and no kernel of the caller cuts windows out of the maps:
 *   model       the record above with y == NULL; all else as in the fused solve
 *   dtype, raw  DOGLEG_AMD_DATA_F64 / _F32 / _U16 and [B][Nmeas] readings of that type, aligned to the element
 *   calibration either none (every member below NULL / 0) or sensor_width, sensor_height, offset, gain_inv and origin together,
 *               the 2D kinds only.  offset (ADU), gain_inv (photoelectrons per ADU) and readvar (photoelectrons^2, or NULL: 0) are
 *               float maps [sensor_height][sensor_width]; origin [B][2] ints: the sensor column and row of pixel (0, 0) of problem
 *               b's window.  Row i is window pixel (ix, iy) = (i mod width, i div width), sensor pixel (ox + ix, oy + iy)
 *   datum       without calibration y = (double)raw, v = 0; with it y = ((double)raw - (double)offset) * (double)gain_inv,
 *               v = (double)readvar, uncontracted (dogleg_batch_camera_datum in dogleg_batch_models.h)
 * All arrays are device-accessible memory of the current device, as those of the model record.
 * DOGLEG_AMD_LIKELIHOOD_GAUSS reads y alone (readvar may be given and is not read; model.scale stays available, for instance
 * 1 / sqrt(variance)).  DOGLEG_AMD_LIKELIHOOD_POISSON without calibration is item 3 on y (a negative float datum fails its problem
 * as there); with calibration it is the sCMOS estimator of Huang et al. 2013, the Poisson fit of y + v against f + v, y + v clamped
 * at 0: dogleg_batch_model_row_poisson_v.  With readvar NULL or 0 and no negative y that is item 3 on y, bit for bit.
 * A window that leaves the sensor (ox < 0, oy < 0, ox + width > sensor_width or oy + height > sensor_height) reads nothing from
 * the maps; its data are NaN, so that problem ends DOGLEG_AMD_BATCH_FAILED (DOGLEG_AMD_BATCH_UNC_FAILED), alone.  The test is made
 * in the kernel, once a problem: origin is device memory.
 * dogleg_amd_optimize_dense_batch_camera[_device] have the contract of dogleg_amd_optimize_dense_batch_model_mle[_device],
 * dogleg_amd_dense_batch_camera_uncertainty[_device] and dogleg_amd_dense_batch_camera_query_covariance[_device] that of the
 * _model_ calls of item 4: bounds, held, the active mask, the stream rule, one launch and one 4-byte read-back a round, what the
 * host-pointer forms stage.  On data that are exactly representable EVERY OUTPUT HAS THE BITS OF THE _model_ CALL ON THE y ABOVE.
 * dogleg_amd_batch_camera_callback and dogleg_amd_batch_camera_fisher_callback are the adapter route: dogleg_callback_device_batch_t
 * whose cookie is the camera record, one launch each; the first writes x and J of the GAUSS definition, the second x~ and J~ of
 * the Poisson definition (with read noise under calibration).  EVERY BATCH SOLVE ENTRY POINT REFUSES THE SECOND as it refuses
 * dogleg_amd_batch_model_fisher_callback.
 * Refused with a message and -1 before any device work, outputs untouched: what the mirrored call refuses of camera->model, a NULL
 * camera, model.y != NULL, raw NULL or misaligned for its dtype, an unknown dtype, calibration given in part (readvar without the
 * rest included), calibration with a 1D kind, a sensor smaller than the window, model.scale with POISSON, and arrays that are not
 * device-accessible over their span (the maps: sensor_width sensor_height floats, origin: 2 B ints).
 * Not provided: calibration for the 1D kinds; uint8 / int32 data; EMCCD excess-noise models; a loss in the fused form; the
 * products form. */
#define DOGLEG_AMD_MODEL_EXPDECAY         0
#define DOGLEG_AMD_MODEL_GAUSS1D          1
#define DOGLEG_AMD_MODEL_GAUSS2D          2
#define DOGLEG_AMD_MODEL_GAUSS2D_ELLIPTIC 3
typedef struct
{
  int           kind;
  unsigned int  Nmeas;
  unsigned int  width, height;
  const double* y;
  const double* t;
  const double* scale;
  int           t_per_problem;
} dogleg_amd_batch_model_t;
int dogleg_amd_batch_model_nstate(int kind);
void dogleg_amd_batch_model_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                     unsigned int B, void* hip_stream, void* cookie);
unsigned long long dogleg_amd_batch_model_callback_invocations(void);
int dogleg_amd_optimize_dense_batch_model(double* p, unsigned int B, const dogleg_amd_batch_model_t* model,
                                          const dogleg_parameters2_t* parameters,
                                          const dogleg_amd_batch_bounds_t* bounds /* NULL: none */,
                                          dogleg_amd_batch_result_t* results);
int dogleg_amd_optimize_dense_batch_model_device(double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                 const dogleg_parameters2_t* parameters,
                                                 const dogleg_amd_batch_bounds_t* bounds,
                                                 dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                 const unsigned char* active_dev, void* hip_stream);
#define DOGLEG_AMD_LIKELIHOOD_GAUSS   0
#define DOGLEG_AMD_LIKELIHOOD_POISSON 1
int dogleg_amd_optimize_dense_batch_model_mle(double* p, unsigned int B, const dogleg_amd_batch_model_t* model, int likelihood,
                                              const dogleg_parameters2_t* parameters,
                                              const dogleg_amd_batch_bounds_t* bounds /* NULL: none */,
                                              dogleg_amd_batch_result_t* results);
int dogleg_amd_optimize_dense_batch_model_mle_device(double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                     int likelihood, const dogleg_parameters2_t* parameters,
                                                     const dogleg_amd_batch_bounds_t* bounds,
                                                     dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                     const unsigned char* active_dev, void* hip_stream);
void dogleg_amd_batch_model_fisher_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                            unsigned int B, void* hip_stream, void* cookie);
int dogleg_amd_dense_batch_model_uncertainty(const double* p, unsigned int B, const dogleg_amd_batch_model_t* model, int likelihood,
                                             double* lambda, double* covariance, double* variances, double* factors,
                                             double* scale, int featureSize, int* status, const unsigned char* held /* or NULL */);
int dogleg_amd_dense_batch_model_uncertainty_device(const double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                    int likelihood, double* lambda_dev, double* covariance_dev,
                                                    double* variances_dev, double* factors_dev, double* scale_dev, int featureSize,
                                                    int* status_dev, const unsigned char* held_dev,
                                                    const unsigned char* active_dev, void* hip_stream);
int dogleg_amd_dense_batch_model_query_covariance(const double* p, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                  int likelihood, double* lambda, const double* Jq, unsigned int Nq,
                                                  unsigned int Qrows, int Nobservations, double* out, int* status,
                                                  const unsigned char* held /* or NULL */);
int dogleg_amd_dense_batch_model_query_covariance_device(const double* p_dev, unsigned int B, const dogleg_amd_batch_model_t* model,
                                                         int likelihood, double* lambda_dev, const double* Jq_dev, unsigned int Nq,
                                                         unsigned int Qrows, int Nobservations, double* out_dev, int* status_dev,
                                                         const unsigned char* held_dev, const unsigned char* active_dev,
                                                         void* hip_stream);
#define DOGLEG_AMD_DATA_F64 0
#define DOGLEG_AMD_DATA_F32 1
#define DOGLEG_AMD_DATA_U16 2
typedef struct
{
  dogleg_amd_batch_model_t model;   /* model.y must be NULL; all else as in the fused solve */
  int           dtype;              /* DOGLEG_AMD_DATA_* */
  const void*   raw;                /* [B][Nmeas] readings of dtype, aligned to the element */
  /* calibration: none (all of the below NULL / 0) or offset, gain_inv and origin together; 2D kinds only */
  unsigned int  sensor_width, sensor_height;
  const float*  offset;             /* [sensor_height][sensor_width], ADU */
  const float*  gain_inv;           /* same shape, photoelectrons per ADU */
  const float*  readvar;            /* same shape, photoelectrons^2, or NULL: 0 */
  const int*    origin;             /* [B][2]: sensor column, row of pixel (0,0) of problem b's window */
} dogleg_amd_batch_camera_t;
void dogleg_amd_batch_camera_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                      unsigned int B, void* hip_stream, void* cookie);
void dogleg_amd_batch_camera_fisher_callback(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev,
                                             unsigned int B, void* hip_stream, void* cookie);
int dogleg_amd_optimize_dense_batch_camera(double* p, unsigned int B, const dogleg_amd_batch_camera_t* camera, int likelihood,
                                           const dogleg_parameters2_t* parameters,
                                           const dogleg_amd_batch_bounds_t* bounds /* NULL: none */,
                                           dogleg_amd_batch_result_t* results);
int dogleg_amd_optimize_dense_batch_camera_device(double* p_dev, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                                  int likelihood, const dogleg_parameters2_t* parameters,
                                                  const dogleg_amd_batch_bounds_t* bounds,
                                                  dogleg_amd_batch_result_t* results_dev, double* lambda_dev,
                                                  const unsigned char* active_dev, void* hip_stream);
int dogleg_amd_dense_batch_camera_uncertainty(const double* p, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                              int likelihood, double* lambda, double* covariance, double* variances,
                                              double* factors, double* scale, int featureSize, int* status,
                                              const unsigned char* held /* or NULL */);
int dogleg_amd_dense_batch_camera_uncertainty_device(const double* p_dev, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                                     int likelihood, double* lambda_dev, double* covariance_dev,
                                                     double* variances_dev, double* factors_dev, double* scale_dev, int featureSize,
                                                     int* status_dev, const unsigned char* held_dev,
                                                     const unsigned char* active_dev, void* hip_stream);
int dogleg_amd_dense_batch_camera_query_covariance(const double* p, unsigned int B, const dogleg_amd_batch_camera_t* camera,
                                                   int likelihood, double* lambda, const double* Jq, unsigned int Nq,
                                                   unsigned int Qrows, int Nobservations, double* out, int* status,
                                                   const unsigned char* held /* or NULL */);
int dogleg_amd_dense_batch_camera_query_covariance_device(const double* p_dev, unsigned int B,
                                                          const dogleg_amd_batch_camera_t* camera, int likelihood,
                                                          double* lambda_dev, const double* Jq_dev, unsigned int Nq,
                                                          unsigned int Qrows, int Nobservations, double* out_dev, int* status_dev,
                                                          const unsigned char* held_dev, const unsigned char* active_dev,
                                                          void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
