// dense_batch_kernels.hip -- the device code of the batch solver (host side: dense_batch.hip; arguments and launchers:
// dense_batch_dev.h).  dogleg_amd_optimize_dense_batch: B small dense problems of one shape, the whole dog-leg loop
// (dogleg.c:1016-1022, 529-998, 1172-1476) per problem on the device.
//
// A round: the caller's batch callback evaluates x, J at the live problems' trial points (its kernels, on our stream),
// then ONE launch of k_batch_round does for every live problem what eval_point + evaluate_step + take_step do, then
// the host reads one counter of live problems (a 4-byte copy into page-locked memory).  Launches and synchronisations
// per round: constant, whatever B is.
//
// One wavefront per problem, BatchCfg<NMAX>::WPB problems per workgroup (4 up to 32 variables, 2 in the class of 48,
// 1 in the class of 64: the LDS a wavefront needs grows with the packed triangle).  The wave sweeps the problem's J ONCE (coalesced loads
// of row tiles into LDS, the next tile's loads in flight while the current one is used): norm2(x), Jt x and the packed
// lower triangle of JtJ come out of that sweep, JtJ in registers (lane l holds entries l, l + 64, ...), then in LDS.
// Everything after it -- |J g|^2 = g' JtJ g, the packed Cholesky with the lambda loop, the two triangular solves, the
// choice of step, |J s|^2 = s' JtJ s -- is wave-level code on that on-chip copy.  What a rejected trial needs again of
// the point it started from (p, Jt x, the Cauchy and Gauss-Newton steps, JtJ: N (N + 11) / 2 doubles) lies in device
// memory per problem; the J of a point is never read a second time and only one x / J buffer per problem exists.
// Plain FMAs, no MFMA: DESIGN.md section 3, "Batches of small dense problems".
//
// dogleg_amd_dense_batch_uncertainty (k_batch_uncertainty, below the round kernel): covariance, variances and outlierness
// factors of every problem at given points, one callback and one launch, on the same sweep, Cholesky and cache.
//
// dogleg_amd_dense_batch_query_covariance (k_batch_query, below the uncertainty kernel): Jq Sigma_b Jq' of caller-supplied
// query Jacobians per problem, and the observations-only form, behind the same front half (factor_and_invert) in one launch;
// Sigma itself is neither formed nor written.
//
// The products form (dogleg_amd_optimize_dense_products_batch, dogleg_amd_dense_products_batch_uncertainty): the callback
// hands back norm2(x), Jt x and JtJ of every live problem, so there is no sweep.  A second front end (load_products) puts
// the same three things where sweep_point leaves them; from evaluate_step on both forms run the same functions.  The
// kernels are templates over the form: the J-form instantiations keep their arithmetic and their order of operations.
//
// The model form (dogleg_amd_optimize_dense_batch_model): a built-in closed-form model (include/dogleg_batch_models.h) instead of a
// callback.  A third front end (sweep_model) forms each row of x and J in the lane that would have staged it and puts it into the
// tile; x and J never lie in memory, and the results have the bits of the J form on what the adapter callback (batch_models.hip)
// would have written.  Only the class of 8 is instantiated: every model has at most 6 variables.
//
// The Poisson form (dogleg_amd_optimize_dense_batch_model_mle with DOGLEG_AMD_LIKELIHOOD_POISSON): the model form's sweep with the
// rows of dogleg_batch_model_row_poisson, x~ = (f - y) / sqrt(f) and J~ = grad f / sqrt(f), and the Poisson deviance summed where
// the model form sums x^2: the cost the gain ratio compares is apart from the rows that form g and H, as in the robust form.  A row
// with !(f > 0) is staged as zeros and makes the point's cost +infinity, which the finite test of this form accepts once the
// problem has started: rho is then -infinity, an ordinary rejected step.  Everything behind the sweep is the model form's text.
//
// The fused uncertainty and query calls of a built-in model (dogleg_amd_dense_batch_model_uncertainty, _query_covariance): the forms
// FORM_MODEL and FORM_POISSON of k_batch_uncertainty and k_batch_query.  Their sweeps -- the first, the second for the outlierness
// factors and the one for G -- form the rows in the lanes as the fused solve does; with POISSON the rows are those of
// dogleg_amd_batch_model_fisher_callback (ROWS_FISHER of sweep_model: NaN in an infeasible row, the squares of x~ summed).  Every
// output has the bits of the J form's call behind the respective callback; no x, no J in memory.
//
// The camera forms (dogleg_amd_optimize_dense_batch_camera, dogleg_amd_dense_batch_camera_uncertainty, _query_covariance): the model
// and the Poisson form with the data of a camera record (dogleg.h: dogleg_amd_batch_camera_t) -- readings of uint16, float or
// double, as they are (FORM_MODEL_RAW, FORM_POISSON_RAW) or calibrated by sensor-sized maps at the window's origin (FORM_MODEL_CAL,
// FORM_POISSON_CAL; FORM_POISSON_CALV with the read-noise variance v: the Poisson fit of y + v against f + v).  The lane that forms
// a row loads its own reading and gathers its pixel's map values (CamSrc, CamLane above sweep_model); everything behind the sweep
// is the model forms' text, and FORM_MODEL and FORM_POISSON themselves are compiled as they were.
//
// The device-resident twins (dogleg_amd_*_batch_device): the same rounds and the same launch of k_batch_uncertainty with every
// array of the caller in device memory.  The solve takes its initial p by a copy within the device and ends in k_batch_finish,
// which writes p, the result structs and lambda where the caller has them; the uncertainty kernel's per-output pointers point
// at the caller's arrays.  An active mask is the initial value of the solve's live bytes and a wave-uniform return at the head
// of k_batch_uncertainty.  k_batch_round is the same for both routes.
//
// The bounded form (dogleg_amd_optimize_dense_batch_bounded and its _device twin): box bounds per problem by an active-set loop,
// the eight steps above the prototype in dogleg.h.  BOUNDED is a template flag of batch_problem and k_batch_round beside ROBUST
// (either form: dogleg_amd_optimize_dense_products_batch_bounded is the FORM_PRODUCTS instantiation of the same text); everything
// it adds lies behind the sweep or the load of the products, on the on-chip JtJ, g and the two cached steps, and needs no LDS of
// its own.  k_batch_clamp (behind k_batch_init) clamps the start points; k_batch_finish, or solve_locked (dense_batch.hip) on the host, forms held.
//
// The fit forms (dogleg_amd_dense[_products]_batch_uncertainty_fit, _query_covariance_fit and their _device twins): the two
// kernels above at the optimum of a robust or bounded solve.  FIT is a template flag of factor_and_invert, unc_problem,
// query_problem and the two kernels: the rows of x and J are multiplied by sqrt(w) of their feature while they are staged
// (SWEEP_FIT of sweep_point; the second sweep and the sweep for G do the same), the held rows and columns of the matrix that is
// factorised are those of the identity, and the held diagonal entries of X = L^-1 are cleared, so that everything behind X has
// exact zeros there.  The held set is one 64-bit value a wave; no LDS is added.  The instantiations without FIT keep their text.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cfloat>
#include <type_traits>
#include "dense_batch_dev.h"
#include "../../include/dogleg_batch_models.h"

namespace {

constexpr int BATCH_TILE = 256;         // doubles of J staged per tile (and 64 of x behind them)
constexpr double LAMBDA_INITIAL = 1e-10;       // dogleg.c:138

enum { F_CAUCHY = 1, F_GN = 2, F_EDGE = 4, F_STARTED = 8 };

// (the camera forms: the model and the Poisson form with another source of the data, see the head of this file)
enum { FORM_J = 0, FORM_PRODUCTS = 1, FORM_MODEL = 2, FORM_POISSON = 3, FORM_MODEL_RAW = 4, FORM_POISSON_RAW = 5, FORM_MODEL_CAL = 6,
       FORM_POISSON_CAL = 7, FORM_POISSON_CALV = 8 };
// where the rows' data come from: the model record's y; a camera record's raw readings as they are; those calibrated by the offset
// and gain maps; and with the read-noise map beside them (the Poisson form alone reads it: least squares has no use for v)
enum { SRC_F64 = 0, SRC_RAW = 1, SRC_CAL = 2, SRC_CALV = 3 };
constexpr bool form_gauss(int F)   { return F == FORM_MODEL || F == FORM_MODEL_RAW || F == FORM_MODEL_CAL; }
constexpr bool form_poisson(int F) { return F == FORM_POISSON || F == FORM_POISSON_RAW || F == FORM_POISSON_CAL || F == FORM_POISSON_CALV; }
constexpr bool form_rows(int F)    { return form_gauss(F) || form_poisson(F); }      // rows formed in the lanes
constexpr int  form_src(int F)     { return F == FORM_MODEL_RAW || F == FORM_POISSON_RAW ? SRC_RAW :
                                            F == FORM_MODEL_CAL || F == FORM_POISSON_CAL ? SRC_CAL :
                                            F == FORM_POISSON_CALV ? SRC_CALV : SRC_F64; }
constexpr bool src_cal(int S)      { return S == SRC_CAL || S == SRC_CALV; }

template <int NMAX> struct BatchCfg
{
  static constexpr int NP = NMAX*(NMAX + 1)/2;
  static constexpr int NE = (NP + 63)/64;                       // entries of JtJ a lane accumulates
  static constexpr int SCR = NP > BATCH_TILE + 64 ? NP : BATCH_TILE + 64;     // the factor; during the sweep: the tile and its x
  static constexpr int LDSW = NP + SCR + NMAX;                  // doubles of LDS per wavefront
  // problems (wavefronts) per workgroup: 18 688 B at most up to <32>, 38 400 B at <48>, 33 792 B at <64>, so that four
  // workgroups of any class fit a CU's 160 KB
  static constexpr int WPB = NMAX <= 32 ? 4 : NMAX <= 48 ? 2 : 1;
};
// the same per form: the products form has no row tile, the second region holds the factor only (the model form stages the J
// form's tile)
template <int NMAX, int FORM> struct FormCfg
{
  static constexpr int SCR = FORM != FORM_PRODUCTS ? BatchCfg<NMAX>::SCR : BatchCfg<NMAX>::NP;
  static constexpr int LDSW = BatchCfg<NMAX>::NP + SCR + NMAX;
};

// LDS of ONE wavefront written by some lanes and read by others: the hardware keeps a wave's LDS operations in
// order, the compiler must not move them across this point
__device__ inline void wsync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// butterfly sums: every lane ends with the same bits (a + b == b + a at every level)
__device__ inline double wave_sum(double v)
{
  for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double wave_max(double v)
{
  for(int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline double wave_min(double v)
{
  for(int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
// the bounded form (dogleg.h: dogleg_amd_batch_bounds_t).  Bit i of the held set: variable i sits on a bound, bit for bit, and
// its gradient pushes outwards.  A function of the point stepped from, g and the bounds alone; every lane gets the whole mask
__device__ __forceinline__ unsigned long long held_mask(double p, double g, double lo, double hi, int lane, int N)
{
  return __ballot(lane < N && ((p == lo && g > 0.0) || (p == hi && g < 0.0)));
}
// this lane's entry of an array of bounds [B][N], or `none` where there is no array or no variable
__device__ __forceinline__ double bound_at(const double* bounds, size_t bN, int lane, int N, double none)
{
  return bounds && lane < N ? bounds[bN + lane] : none;
}
// p + s clamped into [lo, hi]; s becomes the step that was applied (untouched where nothing was clamped: then the sum is the
// plain solve's).  Returns the point; clamped: whether this lane's component was
__device__ __forceinline__ double clip_step(double p, double& s, double lo, double hi, bool& clamped)
{
  double t = p + s;
  clamped = false;
  if(t < lo) { t = lo; clamped = true; }
  if(t > hi) { t = hi; clamped = true; }
  if(clamped) s = t - p;
  return t;
}
// first entry of column c of the packed lower triangle (column-major; the same bytes as the reference's row-major
// packed upper, dogleg.c:788-790)
__device__ inline int col_off(int c, int N) { return c*N - c*(c - 1)/2; }
__device__ inline double sym_at(const double* A, int i, int j, int N)
{
  return i >= j ? A[col_off(j, N) + i - j] : A[col_off(i, N) + j - i];
}
// v' A v, lane i holds v[i] (0 beyond N); V: N doubles of LDS
__device__ inline double quad_form(const double* A, double* V, double v, int N, int lane)
{
  wsync();
  if(lane < N) V[lane] = v;
  wsync();
  double r = 0.0;
  if(lane < N)
    for(int j = 0; j < N; j++) r += sym_at(A, lane, j, N)*V[j];
  return wave_sum(r*v);
}
// DPPTRF 'L' on the packed triangle in LDS (right-looking, as the reference's LAPACK call dogleg.c:782): false where
// a pivot is <= 0
__device__ inline bool chol_packed(double* L, int N, int lane)
{
  for(int j = 0; j < N; j++)
  {
    const int jj = col_off(j, N), m = N - j - 1;
    const double ajj = L[jj];
    if(ajj <= 0.0) return false;
    const double d = sqrt(ajj), inv = 1.0/d;
    double ci = 0.0;
    if(lane < m) ci = L[jj + 1 + lane]*inv;
    wsync();
    if(lane == 0) L[jj] = d;
    if(lane < m) L[jj + 1 + lane] = ci;
    wsync();
    if(lane < m)
      for(int c = 0; c <= lane; c++)
        L[col_off(j + 1 + c, N) + lane - c] -= ci*L[jj + 1 + c];
    wsync();
  }
  return true;
}
// (L L') u = rhs, lane i holds rhs[i] and gets u[i]
__device__ inline double solve_packed(const double* L, double b, int N, int lane)
{
  for(int j = 0; j < N; j++)
  {
    const double bj = __shfl(b, j, 64)/L[col_off(j, N)];
    if(lane == j) b = bj;
    else if(lane > j && lane < N) b -= bj*L[col_off(j, N) + lane - j];
  }
  for(int j = N - 1; j >= 0; j--)
  {
    const double xj = __shfl(b, j, 64)/L[col_off(j, N)];
    if(lane == j) b = xj;
    else if(lane < j) b -= xj*L[col_off(lane, N) + j - lane];
  }
  return b;
}

// entry lane + 64 k of the packed triangle is (ei[k], ej[k]), ei >= ej; (0, 0) beyond NP
template <int NMAX>
__device__ __forceinline__ void packed_entries(int N, int NP, int lane, int* ei, int* ej)
{
#pragma unroll
  for(int k = 0; k < BatchCfg<NMAX>::NE; k++)
  {
    const int e = lane + 64*k;
    int c = 0;
    if(e < NP) { while(e >= col_off(c + 1, N)) c++; }
    ej[k] = c; ei[k] = e < NP ? c + e - col_off(c, N) : 0;
  }
}

// rho(s) and w = rho'(s) of the loss L (dogleg.h: dogleg_amd_batch_loss_t); a NaN s gives NaN in both
__device__ __forceinline__ void loss_eval(const LossDev& L, double s, double& rho, double& w)
{
  const double q = s/L.c;
  switch(L.kind)
  {
  case DOGLEG_AMD_LOSS_HUBER:
    if(s <= L.c) { rho = s; w = 1.0; }
    else { const double r = sqrt(s); rho = 2.0*L.a*r - L.c; w = L.a/r; }
    break;
  case DOGLEG_AMD_LOSS_SOFT_L1:
  {
    // 2 c (r - 1) = 2 s / (r + 1): no cancellation for s << c
    const double r = sqrt(1.0 + q);
    rho = 2.0*s/(r + 1.0); w = 1.0/r;
    break;
  }
  case DOGLEG_AMD_LOSS_CAUCHY:
    rho = L.c*log1p(q); w = 1.0/(1.0 + q);
    break;
  default:
    rho = s; w = 1.0;
  }
}
// s of a feature of fs rows from x in memory: the products rounded, summed in the rows' order, as the sweep sums them
__device__ __forceinline__ double feature_s(const double* xf, int fs)
{
#pragma clang fp contract(off)
  double s = xf[0]*xf[0];
  for(int k = 1; k < fs; k++) s += xf[k]*xf[k];
  return s;
}

// the sweep over one point's x and J (xb: M, Jb: M x N row-major): returns norm2(x), leaves the packed lower triangle of
// JtJ in SA and (Jt x)[lane] in gacc (eval_point, dogleg.c:1004-1083, and the rows' outer products dogleg.c:712-714).
// tile: BATCH_TILE + 64 doubles of LDS.  Shared by the round and the uncertainty kernel: one order of operations.
//
// ROBUST: the same sweep with the loss L (first order: the curvature term of rho'' is left out, as Ceres' corrector does
// for rho'' <= 0).  The tile height is a multiple of L.fs, so no feature straddles two tiles; the lane that holds x of row t
// gets s of its feature by shuffles, evaluates rho and rho' and stages sqrt(w) x; every staged element of J is multiplied
// by the sqrt(w) of its row (the element -> row map is the same for every tile).  The loop over the tile's rows is the plain
// one.  Returns F.
//
// SWEEP_FIT: the sweep of the weighted problem at a point that is given (the fit forms of the uncertainty and query calls): the
// tile height, the element -> row map and the staging are those of SWEEP_ROBUST; w of a row's feature comes from wb ([M / L.fs],
// loaded with the tile's x, so one tile ahead) or, with wb == nullptr, from the loss as above.  Every product sqrt(w) x and
// sqrt(w) J is rounded once, as a callback that scales the rows would write it.  Returns the sum of the squares of the WEIGHTED
// x, not F: with L TRIVIAL of size 1 and no wb, SWEEP_PLAIN's bits.  bad: a weight of wb that is negative or not finite.
enum { SWEEP_PLAIN = 0, SWEEP_ROBUST = 1, SWEEP_FIT = 2 };
template <int NMAX, int MODE = SWEEP_PLAIN>
__device__ __forceinline__ double sweep_point(const double* Jb, const double* xb, int N, int M, int NP, int lane,
                                              double* SA, double* tile, double& gacc_out, const LossDev& L = LossDev(),
                                              const double* wb = nullptr, bool* bad = nullptr)
{
  constexpr bool ROBUST = MODE == SWEEP_ROBUST, FIT = MODE == SWEEP_FIT;
  using C = BatchCfg<NMAX>;
  double* xt = tile + BATCH_TILE;
  int ei[C::NE], ej[C::NE];
  packed_entries<NMAX>(N, NP, lane, ei, ej);
  int T = min(64, BATCH_TILE/N);
  double acc[C::NE], gacc = 0.0, n2 = 0.0;
#pragma unroll
  for(int k = 0; k < C::NE; k++) acc[k] = 0.0;
  constexpr int NL = BATCH_TILE/64;
  double v[NL], xv;
  int rowof[NL], t0 = 0;       // ROBUST: the row of the tile element lane + 64 u; the first row of this lane's feature
  if constexpr(ROBUST || FIT)
  {
    T -= T % L.fs;
    t0 = lane - lane % L.fs;
#pragma unroll
    for(int u = 0; u < NL; u++) rowof[u] = min((lane + 64*u)/N, 63);     // (elements behind the tile's rows hold 0)
  }
  [[maybe_unused]] double wv = 1.0;             // FIT with wb: w of this lane's row (1 behind the tile's rows)
  [[maybe_unused]] bool wbad = false;
  {
    const int tc = min(T, M), cnt = tc*N;
#pragma unroll
    for(int u = 0; u < NL; u++) v[u] = lane + 64*u < cnt ? Jb[lane + 64*u] : 0.0;
    xv = lane < tc ? xb[lane] : 0.0;
    if constexpr(FIT) { if(wb && lane < tc) wv = wb[lane/L.fs]; }
  }
  for(int r0 = 0; r0 < M; r0 += T)
  {
    const int tc = min(T, M - r0);
    if constexpr(FIT)
    {
      double sw = 1.0;
      if(wb)
      {
        // (rows behind the tile's hold w = 1)
        wbad = wbad || !(wv >= 0.0) || !isfinite(wv);
        sw = sqrt(wv);
      }
      else if(L.kind != DOGLEG_AMD_LOSS_TRIVIAL)
      {
        // s of the feature as SWEEP_ROBUST forms it: the bits of feature_s, so w has the bits the robust solve returns
        const double x2 = xv*xv;
        double s = x2;
        if(L.fs > 1)
        {
          s = __shfl(x2, t0, 64);
          for(int k = 1; k < L.fs; k++) s += __shfl(x2, t0 + k, 64);
        }
        double rho, w;
        loss_eval(L, s, rho, w);
        if(lane < tc) sw = sqrt(w);
      }
      const double xs = sw*xv;
      wsync();
#pragma unroll
      for(int u = 0; u < NL; u++) tile[lane + 64*u] = v[u]*__shfl(sw, rowof[u], 64);
      xt[lane] = xs;
      wsync();
      n2 = __builtin_fma(xs, xs, n2);
    }
    else if constexpr(ROBUST)
    {
      // sqrt(w) of this lane's row (1 behind the tile's rows) and the feature's rho, once a feature
      double sw = 1.0;
      // (the plain sweep's arithmetic, where the compiler contracts n2 += xv*xv; here the product is shared with the other
      // branch and would not be contracted: hence spelled out, for the same bits)
      if(L.kind == DOGLEG_AMD_LOSS_TRIVIAL) n2 = __builtin_fma(xv, xv, n2);
      else
      {
        const double x2 = xv*xv;
        double s = x2;
        if(L.fs > 1)
        {
          // the rows of the feature in their order, in every one of its lanes: one s, one w a feature
          s = __shfl(x2, t0, 64);
          for(int k = 1; k < L.fs; k++) s += __shfl(x2, t0 + k, 64);
        }
        double rho, w;
        loss_eval(L, s, rho, w);
        if(lane < tc)
        {
          sw = sqrt(w);
          if(lane == t0) n2 += rho;
        }
      }
      wsync();
#pragma unroll
      for(int u = 0; u < NL; u++) tile[lane + 64*u] = v[u]*__shfl(sw, rowof[u], 64);
      xt[lane] = sw*xv;
      wsync();
    }
    else
    {
      wsync();
#pragma unroll
      for(int u = 0; u < NL; u++) tile[lane + 64*u] = v[u];
      xt[lane] = xv;
      wsync();
      n2 += xv*xv;
    }
    if(r0 + T < M)
    {
      const int r1 = r0 + T, tn = min(T, M - r1), cnt = tn*N;
      const double* Jn = Jb + (size_t)r1*N;
#pragma unroll
      for(int u = 0; u < NL; u++) v[u] = lane + 64*u < cnt ? Jn[lane + 64*u] : 0.0;
      xv = lane < tn ? xb[r1 + lane] : 0.0;
      if constexpr(FIT) { if(wb) wv = lane < tn ? wb[(r1 + lane)/L.fs] : 1.0; }
    }
    for(int t = 0; t < tc; t++)
    {
      const double* row = tile + t*N;
#pragma unroll
      for(int k = 0; k < C::NE; k++) acc[k] += row[ei[k]]*row[ej[k]];
      if(lane < N) gacc += row[lane]*xt[t];
    }
  }
  const double n2x = wave_sum(n2);
  wsync();
#pragma unroll
  for(int k = 0; k < C::NE; k++) if(lane + 64*k < NP) SA[lane + 64*k] = acc[k];
  wsync();
  gacc_out = gacc;
  if constexpr(FIT) { if(bad) *bad = __any(wbad); }
  return n2x;
}

// the front end of the products form: what the callback wrote for problem b goes where sweep_point leaves its results.
// Lane l copies the entries l, l + 64, ... of the packed triangle into SA (packed upper: the same bytes, coalesced;
// unpacked: entry (ei, ej), ei >= ej, is G[ej][ei], the triangle the reference's dpotrf 'L' reads through its
// column-major view, dogleg.c:802-806; the other triangle is never read).  finite: whether EVERYTHING read is finite --
// an off-diagonal NaN of JtJ does not show on the diagonal the way a NaN of J does.
template <int NMAX>
__device__ __forceinline__ double load_products(const ProductsDev& P, int b, int N, int NP, int lane, double* SA,
                                                double& g_out, bool& finite)
{
  using C = BatchCfg<NMAX>;
  bool fin = true;
  wsync();
  if(P.unpacked)
  {
    int ei[C::NE], ej[C::NE];
    packed_entries<NMAX>(N, NP, lane, ei, ej);
    const double* Gb = P.JtJ + (size_t)b*N*N;
#pragma unroll
    for(int k = 0; k < C::NE; k++)
      if(lane + 64*k < NP)
      {
        const double v = Gb[ej[k]*N + ei[k]];
        fin = fin && isfinite(v);
        SA[lane + 64*k] = v;
      }
  }
  else
  {
    const double* Gb = P.JtJ + (size_t)b*NP;
#pragma unroll
    for(int k = 0; k < C::NE; k++)
      if(lane + 64*k < NP)
      {
        const double v = Gb[lane + 64*k];
        fin = fin && isfinite(v);
        SA[lane + 64*k] = v;
      }
  }
  wsync();
  const double g = lane < N ? P.xtJ[(size_t)b*N + lane] : 0.0;
  const double n2x = P.n2x[b];
  finite = __all(fin && isfinite(g) && isfinite(n2x));
  g_out = g;
  return n2x;
}

// the data source of the camera forms (dense_batch_dev.h: CameraDev; dogleg.h: dogleg_amd_batch_camera_t).
// CamLane: what a lane holds of one row while its loads are in flight: the reading's bits as loaded (a uint16 zero-extended, a
// float's or a double's bits) and, with calibration, the two or three map values of its sensor pixel.  SRC_CALV: a read-noise map
// is given and read; it is an instantiation of its own because the test for a null map, kept live across the sweep, cost the
// bounded Poisson kernel the scalar registers it had left.
// CamSrc: made ONCE a problem -- the problem's readings and, with calibration, the window's origin and the index of its first sensor
// pixel, or -1 where the window does not lie on the sensor as a whole; such a window reads nothing (its origin apart) and every
// datum of it is NaN.  That test is all that keeps the gather inside the maps: ox >= 0, oy >= 0, ox <= xmax = sw - width and
// oy <= ymax = sh - height, both >= 0 (formed and checked on the host), so no sum overflows and (oy + iy) sw + ox + ix < sw sh for
// every pixel of the window.
// The type of the readings is a switch that is uniform over the launch, around one load and one conversion: a template parameter
// would triple the instantiations for one instruction each
template <int SRC> struct CamLane { unsigned long long bits; };
template <> struct CamLane<SRC_F64> {};
template <> struct CamLane<SRC_CAL> { unsigned long long bits; float off, gi; };
template <> struct CamLane<SRC_CALV> { unsigned long long bits; float off, gi, rv; };
template <int SRC> struct CamSrc
{
  const char* rb; int dtype;
  const float *off, *gi, *rv; int width, sw, first;
  // (b is the same in every lane of the wave, which the compiler cannot see: what follows from it is made scalar by hand)
  __device__ __forceinline__ CamSrc(const CameraDev& Cm, int b, int Ms, int w)
  {
    const int bu = __builtin_amdgcn_readfirstlane(b);
    dtype = Cm.dtype;
    rb = (const char*)Cm.raw + (size_t)b*Ms*(dtype == DOGLEG_AMD_DATA_U16 ? 2 : dtype == DOGLEG_AMD_DATA_F32 ? 4 : 8);
    off = gi = rv = nullptr; width = w; sw = 0; first = 0;
    if constexpr(src_cal(SRC))
    {
      const int ox = __builtin_amdgcn_readfirstlane(Cm.origin[2*(size_t)bu]), oy = __builtin_amdgcn_readfirstlane(Cm.origin[2*(size_t)bu + 1]);
      off = Cm.offset; gi = Cm.gain_inv; rv = Cm.readvar; sw = Cm.sw;
      // the first sensor pixel of the window (the host has checked that sw sh fits an int), -1: the window leaves the sensor
      first = ox >= 0 && oy >= 0 && ox <= Cm.xmax && oy <= Cm.ymax ? oy*Cm.sw + ox : -1;
    }
  }
  __device__ __forceinline__ bool inside() const { return first >= 0; }
  // the loads of row i
  __device__ __forceinline__ void load(int i, CamLane<SRC>& r) const
  {
    if constexpr(src_cal(SRC))
    {
      if(!inside()) return;
      const int iy = i/width, ix = i - iy*width;
      const int px = first + iy*sw + ix;
      r.off = off[px]; r.gi = gi[px];
      if constexpr(SRC == SRC_CALV) r.rv = rv[px];
    }
    if(dtype == DOGLEG_AMD_DATA_U16)      r.bits = ((const unsigned short*)rb)[i];
    else if(dtype == DOGLEG_AMD_DATA_F32) r.bits = ((const unsigned int*)rb)[i];
    else                                  r.bits = ((const unsigned long long*)rb)[i];
  }
  // y and v of what was loaded
  __device__ __forceinline__ void datum(const CamLane<SRC>& r, double& y, double& v) const
  {
    const double raw = dtype == DOGLEG_AMD_DATA_U16 ? (double)(unsigned int)r.bits :
                       dtype == DOGLEG_AMD_DATA_F32 ? (double)__uint_as_float((unsigned int)r.bits) : __longlong_as_double((long long)r.bits);
    if constexpr(src_cal(SRC))
    {
      float rvv = 0.0f;
      if constexpr(SRC == SRC_CALV) rvv = r.rv;
      if(inside()) dogleg_batch_camera_datum(raw, r.off, r.gi, rvv, &y, &v);
      else { y = __builtin_nan(""); v = 0.0; }
    }
    else { y = raw; v = 0.0; }
  }
};
template <> struct CamSrc<SRC_F64>
{
  __device__ __forceinline__ CamSrc(const CameraDev&, int, int, int) {}
};

// the front end of the model form (dogleg_amd_optimize_dense_batch_model): sweep_point<NMAX, SWEEP_PLAIN> over an x and a J that
// never lie in memory.  Lane t of the wave forms row r0 + t of the tile from p (pb: N doubles, the same in every lane), its datum,
// abscissa and scale through dogleg_batch_model_row -- the function the adapter callback writes x and J with, its contraction
// switched off -- and puts it where sweep_point would have staged it: tile[t N ..] and xt[t].  The tile height, the zeros behind
// the tile's rows, the sum for norm2(x) and the loop over the tile's rows are sweep_point's, so the results have its bits on what
// the adapter would have written.  The loads of the next tile's y, t and scale are in flight under the loop; only the lanes that
// hold a row evaluate the model.
// ROWS_POISSON: the rows and the cost of the Poisson form (the head of this file); no scale is read there.
// ROWS_FISHER: the rows of the Poisson form as dogleg_amd_batch_model_fisher_callback writes them, for the uncertainty and query
// kernels, which stand in for that callback and a J-form launch: an infeasible row is staged as the header function returns it (NaN,
// so the problem fails the finiteness test alone), and the sum is that of the squares of the staged x~, not the deviance.
// M rows are swept (the query kernel's G: the first Nobservations); the problem's data lie Ms apart
// ROWS_POISSON_V, ROWS_FISHER_V: the two with the read-noise variance of a calibrated camera record
// (dogleg_batch_model_row_poisson_v).
// SRC: where the data come from.  SRC_F64: Md.y, the text as it was.  SRC_RAW, SRC_CAL: a camera record (CamSrc above): the lane
// loads its own reading, 2, 4 or 8 bytes, and with calibration gathers its sensor pixel's three map values; what was loaded stays
// as it came (CamLane) while the loads are in flight under the row loop and becomes y and v at the head of the next tile
enum { ROWS_GAUSS = 0, ROWS_POISSON = 1, ROWS_FISHER = 2, ROWS_POISSON_V = 3, ROWS_FISHER_V = 4 };
constexpr int rows_solve(int F) { return form_poisson(F) ? (src_cal(form_src(F)) ? ROWS_POISSON_V : ROWS_POISSON) : ROWS_GAUSS; }
constexpr int rows_eval(int F)  { return form_poisson(F) ? (src_cal(form_src(F)) ? ROWS_FISHER_V : ROWS_FISHER) : ROWS_GAUSS; }
// a Poisson row of either kind
template <int MODE>
__device__ __forceinline__ int poisson_row(int kind, const double* p, int i, int width, double t, double y, double v, double* x,
                                           double* J, double* d)
{
  if constexpr(MODE == ROWS_POISSON_V || MODE == ROWS_FISHER_V) return dogleg_batch_model_row_poisson_v(kind, p, i, width, t, y, v, x, J, d);
  else return dogleg_batch_model_row_poisson(kind, p, i, width, t, y, x, J, d);
}
template <int NMAX, int MODE = ROWS_GAUSS, int SRC = SRC_F64>
__device__ __forceinline__ double sweep_model(const ModelDev& Md, const CameraDev& Cm, const double* pb, int b, int N, int M, int Ms,
                                              int NP, int lane, double* SA, double* tile, double& gacc_out)
{
  constexpr bool POISSON = MODE == ROWS_POISSON || MODE == ROWS_POISSON_V;
  using C = BatchCfg<NMAX>;
  constexpr int NM = DOGLEG_BATCH_MODEL_MAX_NSTATE;
  static_assert(NM <= NMAX, "every built-in model lies in the smallest size class");
  double* xt = tile + BATCH_TILE;
  int ei[C::NE], ej[C::NE];
  packed_entries<NMAX>(N, NP, lane, ei, ej);
  const int T = min(64, BATCH_TILE/N);
  double acc[C::NE], gacc = 0.0, n2 = 0.0;
#pragma unroll
  for(int k = 0; k < C::NE; k++) acc[k] = 0.0;
  double p[NM];
#pragma unroll
  for(int j = 0; j < NM; j++) p[j] = j < N ? pb[j] : 0.0;
  const double* yb = SRC == SRC_F64 ? Md.y + (size_t)b*Ms : nullptr;
  const double* tb = Md.t ? Md.t + (Md.t_each ? (size_t)b*Ms : (size_t)0) : nullptr;
  const double* sb = Md.scale ? Md.scale + (size_t)b*Ms : nullptr;
  double yv = 0.0, tv = 0.0, sv = 1.0;
  [[maybe_unused]] double vv = 0.0;      // the read-noise variance of the row (SRC_CAL)
  const CamSrc<SRC> cs(Cm, b, Ms, Md.width);
  CamLane<SRC> cl{};
  bool infeasible = false;     // POISSON: a row of this lane had !(f > 0)
  if(lane < min(T, M))
  {
    if constexpr(SRC == SRC_F64) yv = yb[lane]; else cs.load(lane, cl);
    tv = tb ? tb[lane] : (double)lane;
    if(sb) sv = sb[lane];
  }
  for(int r0 = 0; r0 < M; r0 += T)
  {
    const int tc = min(T, M - r0);
    double xv = 0.0, jr[NM];
#pragma unroll
    for(int j = 0; j < NM; j++) jr[j] = 0.0;
    double dv = 0.0;           // POISSON: the row's share of the deviance
    if constexpr(SRC != SRC_F64) cs.datum(cl, yv, vv);
    if constexpr(POISSON)
    {
      if(lane < tc && !poisson_row<MODE>(Md.kind, p, r0 + lane, Md.width, tv, yv, vv, &xv, jr, &dv))
      {
        infeasible = true;
        xv = 0.0; dv = 0.0;
#pragma unroll
        for(int j = 0; j < NM; j++) jr[j] = 0.0;
      }
    }
    else if constexpr(MODE == ROWS_FISHER || MODE == ROWS_FISHER_V)
    {
      if(lane < tc) (void)poisson_row<MODE>(Md.kind, p, r0 + lane, Md.width, tv, yv, vv, &xv, jr, &dv);
    }
    else if(lane < tc) dogleg_batch_model_row(Md.kind, p, r0 + lane, Md.width, tv, yv, sv, &xv, jr);
    wsync();
    if(lane < T)
    {
#pragma unroll
      for(int j = 0; j < NM; j++) if(j < N) tile[lane*N + j] = jr[j];
    }
    xt[lane] = xv;
    wsync();
    if constexpr(POISSON) n2 += dv; else n2 = __builtin_fma(xv, xv, n2);
    if(r0 + T < M)
    {
      const int r1 = r0 + T, tn = min(T, M - r1);
      if(lane < tn)
      {
        if constexpr(SRC == SRC_F64) yv = yb[r1 + lane]; else cs.load(r1 + lane, cl);
        tv = tb ? tb[r1 + lane] : (double)(r1 + lane);
        if(sb) sv = sb[r1 + lane];
      }
    }
    for(int t = 0; t < tc; t++)
    {
      const double* row = tile + t*N;
#pragma unroll
      for(int k = 0; k < C::NE; k++) acc[k] += row[ei[k]]*row[ej[k]];
      if(lane < N) gacc += row[lane]*xt[t];
    }
  }
  double n2x = wave_sum(n2);
  if constexpr(POISSON) { if(__any(infeasible)) n2x = INFINITY; }
  wsync();
#pragma unroll
  for(int k = 0; k < C::NE; k++) if(lane + 64*k < NP) SA[lane + 64*k] = acc[k];
  wsync();
  gacc_out = gacc;
  return n2x;
}

// one round of problem b; returns whether the problem is still live.
// BOUNDED (either form): box bounds by an active set, the eight steps above dogleg_amd_optimize_dense_batch_bounded in dogleg.h.
// Everything it adds lies behind the sweep (products form: behind load_products), on the on-chip JtJ, g and the two cached
// steps; the other instantiations keep their text.
template <int NMAX, int FORM, bool ROBUST, bool BOUNDED>
__device__ bool batch_problem(const BatchDev& A, int b, int lane, double* S)
{
  using C = BatchCfg<NMAX>;
  const int N = A.N, M = A.M, NP = A.NP;
  double* SA = S;                      // JtJ of the point the step is taken from
  double* SL = S + C::NP;              // its factor; during the sweep the row tile
  double* SV = SL + FormCfg<NMAX, FORM>::SCR;     // an N-vector
  const size_t bN = (size_t)b*N;

  double gacc, n2x;
  bool finite;
  if constexpr(FORM == FORM_J)
  {
    // ---- the sweep over the trial point's x and J: norm2(x), Jt x, JtJ (ROBUST: F, g, H in their places) ----
    n2x = sweep_point<NMAX, ROBUST>(A.J + (size_t)b*M*N, A.x + (size_t)b*M, N, M, NP, lane, SA, SL, gacc, A.L);
    // a non-finite x or J shows in norm2(x) or on the diagonal of JtJ
    const double dg = lane < N ? SA[col_off(lane, N)] : 0.0;
    finite = __all(isfinite(n2x) && isfinite(gacc) && isfinite(dg));
  }
  else if constexpr(form_gauss(FORM))
  {
    // ---- the same sweep over rows formed on the way into the tile: no x, no J in memory ----
    static_assert(!ROBUST, "the model form has no loss");
    n2x = sweep_model<NMAX, ROWS_GAUSS, form_src(FORM)>(A.Mdl, A.Cam, A.p_trial + bN, b, N, M, M, NP, lane, SA, SL, gacc);
    const double dg = lane < N ? SA[col_off(lane, N)] : 0.0;
    finite = __all(isfinite(n2x) && isfinite(gacc) && isfinite(dg));
  }
  else if constexpr(form_poisson(FORM))
  {
    // ---- the model form's sweep over the Poisson rows; n2x is the deviance, +infinity at an infeasible point: no start point,
    // but a trial point like any other that is worse than the point it was stepped from ----
    static_assert(!ROBUST, "the Poisson form has no loss");
    n2x = sweep_model<NMAX, rows_solve(FORM), form_src(FORM)>(A.Mdl, A.Cam, A.p_trial + bN, b, N, M, M, NP, lane, SA, SL, gacc);
    const double dg = lane < N ? SA[col_off(lane, N)] : 0.0;
    const bool started = (A.st[(size_t)ST_COUNT*b + ST_FLAGS] & F_STARTED) != 0;
    finite = __all((isfinite(n2x) || (started && n2x == INFINITY)) && isfinite(gacc) && isfinite(dg));
  }
  else
  {
    (void)M;
    n2x = load_products<NMAX>(A.P, b, N, NP, lane, SA, gacc, finite);
  }

  // ---- evaluate_step (dogleg.c:1303-1356) and the swap of the two points (1427-1470) ----
  int* st = A.st + (size_t)ST_COUNT*b; double* sc = A.sc + (size_t)SC_COUNT*b;
  int flags = st[ST_FLAGS], iters = st[ST_ITER], status = 0;
  const int evals = st[ST_EVAL] + 1;
  double n2x_b = sc[SC_N2X], tr = sc[SC_TR], lam = sc[SC_LAMBDA], n2c = sc[SC_N2C], n2gn = sc[SC_N2GN];
  double EI = sc[SC_EI];
  double p_r = 0.0, g_r = 0.0, ca_r = 0.0, gn_r = 0.0;
  // BOUNDED: the held set of the point stepped from; this lane's bounds (none beyond N) are read where they are used, not
  // kept in registers across the sweep and the factorisation
  unsigned long long hm = 0;
  bool take = false;           // the trial point becomes the point to step from
  if(!finite) status = DOGLEG_AMD_BATCH_FAILED;
  else if(!(flags & F_STARTED)) take = true;
  else
  {
    const double rho = (n2x_b - n2x)/EI;
    if(rho != rho) status = DOGLEG_AMD_BATCH_FAILED;         // (the reference never leaves its retry loop there)
    else
    {
      if(rho < A.dec_thr)
      {
        if(!(flags & F_EDGE)) tr = sqrt(n2gn);
        tr *= A.dec_factor;
      }
      else if(rho > A.inc_thr && (flags & F_EDGE)) tr *= A.inc_factor;
      if(rho > 0.0) { take = true; iters++; }
      else if(tr < A.tr_thr) status = DOGLEG_AMD_BATCH_TRUSTREGION;
      else
      {
        // rejected: again from the cached steps of the point before (no evaluation, no factorisation)
        if(lane < N)
        {
          p_r = A.p_before[bN + lane]; g_r = A.g[bN + lane];
          if(flags & F_CAUCHY) ca_r = A.cauchy[bN + lane];
          if(flags & F_GN) gn_r = A.gn[bN + lane];
        }
        const double* Gb = A.JtJ + (size_t)b*NP;
        wsync();
        for(int e = lane; e < NP; e += 64) SA[e] = Gb[e];
        wsync();
        // (the cached steps are those of this held set: it is recomputed, not stored)
        if constexpr(BOUNDED) hm = held_mask(p_r, g_r, bound_at(A.lo, bN, lane, N, -INFINITY), bound_at(A.hi, bN, lane, N, INFINITY), lane, N);
      }
    }
  }
  if(take)
  {
    flags = F_STARTED; n2x_b = n2x; g_r = gacc;
    if(lane < N)
    {
      p_r = A.p_trial[bN + lane];
      A.p_before[bN + lane] = p_r; A.g[bN + lane] = g_r;
    }
    double* Gb = A.JtJ + (size_t)b*NP;
    for(int e = lane; e < NP; e += 64) Gb[e] = SA[e];
    if constexpr(ROBUST)
    {
      // the weights of the point now stepped from: A.x still holds its x, so a rejected trial never needs them
      const double* xb = A.x + (size_t)b*M; double* wb = A.wts + (size_t)b*A.NF;
      for(int f = lane; f < A.NF; f += 64)
      {
        double rho, w;
        loss_eval(A.L, feature_s(xb + (size_t)f*A.L.fs, A.L.fs), rho, w);
        wb[f] = w;
      }
    }
    double gmax;
    if constexpr(BOUNDED)
    {
      // the stopping test is on the free gradient: 0 with every variable held
      hm = held_mask(p_r, g_r, bound_at(A.lo, bN, lane, N, -INFINITY), bound_at(A.hi, bN, lane, N, INFINITY), lane, N);
      gmax = wave_max((hm >> lane) & 1 ? 0.0 : fabs(g_r));
    }
    else gmax = wave_max(fabs(g_r));
    if(gmax <= A.jtx_thr) status = DOGLEG_AMD_BATCH_JTX;
    else if(iters >= A.max_iterations) status = DOGLEG_AMD_BATCH_MAX_ITERATIONS;
  }
  // the free gradient: g with its held entries 0 (the Cauchy step and the right-hand side of the Gauss-Newton step); the
  // expected improvement keeps g
  double gf_r = g_r;
  if constexpr(BOUNDED) { if((hm >> lane) & 1) gf_r = 0.0; }

  // ---- take_step (dogleg.c:1172-1297) ----
  if(status == 0)
  {
    const double tr2 = tr*tr;
    if(!(flags & F_CAUCHY))
    {
      const double g2 = wave_sum(gf_r*gf_r);
      const double Jg2 = quad_form(SA, SV, gf_r, N, lane);
      const double k = -g2/Jg2;
      n2c = k*k*g2; ca_r = k*gf_r;
      if(lane < N) A.cauchy[bN + lane] = ca_r;
      flags |= F_CAUCHY;
    }
    double s_r = 0.0;
    if(n2c >= tr2)
    {
      s_r = tr/sqrt(n2c)*ca_r;
      flags |= F_EDGE;
    }
    else
    {
      if(!(flags & F_GN))
      {
        // the factorisation is attempted only here, so lambda moves only here (dogleg.c:634-820)
        while(true)
        {
          wsync();
          for(int e = lane; e < NP; e += 64) SL[e] = SA[e];
          wsync();
          if(lam > 0.0 && lane < N) SL[col_off(lane, N)] += lam;
          wsync();
          if constexpr(BOUNDED)
          {
            // the system on the free set: a held row and column is that of the identity, so that gn is exactly 0 there
            if(hm)
            {
              int c = 0;
              for(int e = lane; e < NP; e += 64)
              {
                while(e >= col_off(c + 1, N)) c++;
                const int i = c + e - col_off(c, N);
                if(((hm >> c) | (hm >> i)) & 1) SL[e] = i == c ? 1.0 : 0.0;
              }
              wsync();
            }
          }
          if(chol_packed(SL, N, lane)) break;
          lam = lam == 0.0 ? LAMBDA_INITIAL : lam*10.0;
          if(!isfinite(lam)) { status = DOGLEG_AMD_BATCH_FAILED; break; }
        }
        if(status == 0)
        {
          gn_r = -solve_packed(SL, gf_r, N, lane);
          if(lane >= N) gn_r = 0.0;
          n2gn = wave_sum(gn_r*gn_r);
          if(lane < N) A.gn[bN + lane] = gn_r;
          flags |= F_GN;
        }
      }
      if(status == 0)
      {
        if(n2gn <= tr2) { s_r = gn_r; flags &= ~F_EDGE; }
        else
        {
          // dogleg.c:927-998
          const double d = ca_r - gn_r;
          const double l2 = wave_sum(d*d), neg_c = wave_sum(d*ca_r);
          double disc = neg_c*neg_c - l2*(n2c - tr2);
          if(disc < 0.0) disc = 0.0;
          const double k = (neg_c + sqrt(disc))/l2;
          s_r = ca_r + k*(gn_r - ca_r);
          flags |= F_EDGE;
        }
      }
    }
    // BOUNDED: the step clipped into the box.  With no component clamped the text below this block is the plain solve's
    bool clipped = false;
    if constexpr(BOUNDED)
    {
      if(status == 0)
      {
        const double lo_r = bound_at(A.lo, bN, lane, N, -INFINITY), hi_r = bound_at(A.hi, bN, lane, N, INFINITY);
        bool cl;
        double sc_r = s_r;
        double t_r = clip_step(p_r, sc_r, lo_r, hi_r, cl);
        clipped = __any(cl);
        if(clipped)
        {
          s_r = sc_r;
          double Js2 = quad_form(SA, SV, s_r, N, lane);
          EI = -2.0*wave_sum(g_r*s_r) - Js2;
          double smax = wave_max(fabs(s_r));
          if(EI <= 0.0 || smax <= A.upd_thr)
          {
            // the clipped step is no descent step of the model, or no step at all: the Cauchy step, cut at the trust region,
            // then at the first bound a free variable meets.  The component that set alpha (its own ratio equals alpha) ends ON
            // its bound: p + ((far - p) / d) d rounds onto the bound's bits, one ulp beyond it (which the clamp brings back) or
            // one ulp short of it, and one ulp short the variable is on no bound, is not held at the next point, and the next
            // fallback is cut at alpha ~ 1e-16: the solve would stop on update_threshold over a rounding.  So that component
            // takes the clamp's form whichever way the sum rounds (k_bounds_fallback, bounds_device.hip)
            const double d_r = fmin(1.0, tr/sqrt(n2c))*ca_r;
            const double far_r = d_r > 0.0 ? hi_r : lo_r;
            double a_r = 1.0;
            if(lane < N && d_r != 0.0) a_r = (far_r - p_r)/d_r;
            const double alpha = fmin(1.0, wave_min(a_r));
            s_r = alpha*d_r;
            if(lane < N && d_r != 0.0 && a_r == alpha) { t_r = far_r; s_r = far_r - p_r; }
            else t_r = clip_step(p_r, s_r, lo_r, hi_r, cl);
            Js2 = quad_form(SA, SV, s_r, N, lane);
            EI = -2.0*wave_sum(g_r*s_r) - Js2;
            smax = wave_max(fabs(s_r));
            if(n2c >= tr2) flags |= F_EDGE; else flags &= ~F_EDGE;
            if(!(EI > 0.0) || !isfinite(EI)) status = DOGLEG_AMD_BATCH_FAILED;
          }
          if(status == 0)
          {
            if(smax <= A.upd_thr) status = DOGLEG_AMD_BATCH_SMALL_STEP;
            else if(lane < N) A.p_trial[bN + lane] = t_r;
          }
        }
      }
    }
    if(!clipped && status == 0)
    {
      const double Js2 = quad_form(SA, SV, s_r, N, lane);
      EI = -2.0*wave_sum(g_r*s_r) - Js2;
      // the terminal small step is neither applied nor evaluated (dogleg.c:1289-1296, 1403-1408)
      if(wave_max(fabs(s_r)) <= A.upd_thr) status = DOGLEG_AMD_BATCH_SMALL_STEP;
      else if(lane < N) A.p_trial[bN + lane] = p_r + s_r;
    }
  }
  if(lane == 0)
  {
    sc[SC_N2X] = n2x_b; sc[SC_TR] = tr; sc[SC_LAMBDA] = lam; sc[SC_N2C] = n2c; sc[SC_N2GN] = n2gn; sc[SC_EI] = EI;
    st[ST_FLAGS] = flags; st[ST_ITER] = iters; st[ST_EVAL] = evals; st[ST_STATUS] = status;
    if(status != 0) A.live[b] = 0;
  }
  return status == 0;
}

// (the Poisson form asks for the model form's 4 waves a SIMD: left alone it takes 130 VGPRs, two more than 4 waves allow; held to
// 128 it takes 126 and no scratch.  1 is the default: the other instantiations are compiled as they were)
template <int NMAX, int FORM, bool ROBUST, bool BOUNDED>
__global__ void __launch_bounds__(64*BatchCfg<NMAX>::WPB) __attribute__((amdgpu_waves_per_eu(form_poisson(FORM) ? 4 : 1)))
k_batch_round(BatchDev A)
{
  constexpr int LDSW = FormCfg<NMAX, FORM>::LDSW, WPB = BatchCfg<NMAX>::WPB;
  __shared__ double lds[WPB*LDSW];
  __shared__ int s_live[WPB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x*WPB + w;
  bool still = false;
  if(b < A.B && A.live[b]) still = batch_problem<NMAX, FORM, ROBUST, BOUNDED>(A, b, lane, lds + w*LDSW);
  if(lane == 0) s_live[w] = still ? 1 : 0;
  __syncthreads();
  if(threadIdx.x == 0)
  {
    int n = 0;
    for(int k = 0; k < WPB; k++) n += s_live[k];
    if(n) atomicAdd(A.counter, n);
  }
}

// ---- dogleg_amd_dense_batch_uncertainty: Sigma_b = (JtJ + lambda I)^-1, its diagonal and the outlierness factors of every
// problem at the points p[b], ONE launch behind one call of the batch callback.  Per wave: the sweep of the round kernel
// (|x|^2, JtJ), the lambda loop on chol_packed, the factor inverted in place, Sigma = L^-T L^-1 into the LDS that held JtJ
// (it is not needed once the factorisation stands: Sigma costs no LDS of its own), then a second sweep over J in which
// one lane takes one feature.  No sum crosses lanes after the first sweep.
// x' (B + B^2) x scale / 8 with B = (A_f - I)^-1, dogleg.h above dogleg_getOutliernessFactors (the arithmetic of
// k_lev_finish, sparse_multi.hip)
__device__ inline double factor1(double a, double x0, double k)
{
  const double den = 1.0 - a;
  return fabs(den) < 1e-8 ? DBL_MAX : x0*x0/den*k;
}
__device__ inline double factor2(double a00, double a01, double a11, double x0, double x1, double k)
{
  const double m00 = a00 - 1.0, m01 = a01, m11 = a11 - 1.0;
  const double det = m00*m11 - m01*m01;
  if(fabs(det) < 1e-8) return DBL_MAX;
  const double j00 = m11, j01 = -m01, j11 = m00;           // adjugate of A_f - I
  const double xBx = (x0*x0*j00 + 2.0*x0*x1*j01 + x1*x1*j11)/det;
  const double v0 = x0*j00 + x1*j01, v1 = x0*j01 + x1*j11;
  return (xBx + (v0*v0 + v1*v1)/(det*det))*k;
}

// the factor of one feature of one (r) or two rows (ra, ra + NS) of J against Sigma, packed in SA: a = J_f Sigma J_f', the
// arithmetic and the order of operations of the second sweep of the classes up to 32 in unc_problem (which keeps its own
// text: through these functions its instantiations come out with other registers), for the classes above
__device__ inline double feature1(const double* SA, const double* r, int N, double x0, double kf)
{
  double a = 0.0;
  int idx = 0;
  for(int j = 0; j < N; j++)
  {
    const double rj = r[j], d = SA[idx++];
    double t0 = 0.0;
    for(int i = j + 1; i < N; i++) t0 += SA[idx++]*r[i];
    a += rj*(d*rj + 2.0*t0);
  }
  return factor1(a, x0, kf);
}
__device__ inline double feature2(const double* SA, const double* ra, int NS, int N, double x0, double x1, double kf)
{
  const double* rb = ra + NS;
  double a00 = 0.0, a01 = 0.0, a11 = 0.0;
  int idx = 0;
  for(int j = 0; j < N; j++)
  {
    const double aj = ra[j], bj = rb[j], d = SA[idx++];
    double t0 = 0.0, t1 = 0.0;
    for(int i = j + 1; i < N; i++) { const double s = SA[idx++]; t0 += s*ra[i]; t1 += s*rb[i]; }
    a00 += aj*(d*aj + 2.0*t0); a01 += aj*(d*bj + t1) + bj*t0; a11 += bj*(d*bj + 2.0*t1);
  }
  return factor2(a00, a01, a11, x0, x1, kf);
}

// the front half of a problem of the uncertainty and of the query kernel, one text for both: the sweep (or the products) into
// SA, the finiteness test, the lambda loop on chol_packed in SL and, where that stands, X = L^-1 in place.  Between the two,
// report(ok, lambda, norm2(x)) is the caller's: what it writes back of the factorisation and, for a problem that failed, the
// NaN of its outputs.  Returns whether the factorisation stands.
//
// FIT (dogleg.h: dogleg_amd_batch_fit_t): the sweep is that of the weighted rows (SWEEP_FIT; report gets the sum of their
// squares, NaN with a bad weight); hm gets the held set, bit i for variable i, the same in every lane; the held rows and columns of
// the matrix that is factorised are the identity's, as in the bounded solve, so the factor and X have unit vectors there; and the
// held diagonal entries of X are cleared: X' X, X q and X' z then have exact zeros in the held places and the inverse of the free
// block in the others.  hm stays 0 otherwise.
//
// FORM_MODEL, FORM_POISSON (dogleg_amd_dense_batch_model_uncertainty, _query_covariance; E: the model and the points): the sweep is
// sweep_model over rows formed in the lanes, which leaves in SA and gacc what sweep_point leaves on the rows of
// dogleg_amd_batch_model_callback (FORM_MODEL) or dogleg_amd_batch_model_fisher_callback (FORM_POISSON: ROWS_FISHER).  No loss and
// no weights, so FIT adds the held set only; a weight of exactly 1 would change no bit of a row
template <int NMAX, int FORM, bool FIT, class Report>
__device__ __forceinline__ bool factor_and_invert(const UncDev& A, const FitDev& F, const ModelEvalDev& E, int b, int lane,
                                                  double* SA, double* SL, unsigned long long& hm, Report report)
{
  const int N = A.N, M = A.M, NP = A.NP;
  double gacc, n2x;
  bool ok;
  if constexpr(FORM == FORM_J)
  {
    if constexpr(FIT)
    {
      bool bad;
      n2x = sweep_point<NMAX, SWEEP_FIT>(A.J + (size_t)b*M*N, A.x + (size_t)b*M, N, M, NP, lane, SA, SL, gacc, F.L,
                                         F.wts ? F.wts + (size_t)b*(M/F.L.fs) : nullptr, &bad);
      if(bad) n2x = __builtin_nan("");
    }
    else n2x = sweep_point<NMAX>(A.J + (size_t)b*M*N, A.x + (size_t)b*M, N, M, NP, lane, SA, SL, gacc);
    const double dg = lane < N ? SA[col_off(lane, N)] : 0.0;
    ok = __all(isfinite(n2x) && isfinite(gacc) && isfinite(dg));
  }
  else if constexpr(form_rows(FORM))
  {
    n2x = sweep_model<NMAX, rows_eval(FORM), form_src(FORM)>(E.Mdl, E.Cam, E.p + (size_t)b*N, b, N, M, M, NP, lane, SA, SL, gacc);
    const double dg = lane < N ? SA[col_off(lane, N)] : 0.0;
    ok = __all(isfinite(n2x) && isfinite(gacc) && isfinite(dg));
  }
  else
    n2x = load_products<NMAX>(A.P, b, N, NP, lane, SA, gacc, ok);
  if constexpr(FIT) { if(F.held) hm = __ballot(lane < N && F.held[(size_t)b*N + lane] != 0); }

  // ---- the factorisation at lambda[b]; a pivot <= 0 moves lambda as the solve does (dogleg.c:634-820) ----
  double lam = A.lam[b];
  if(!(lam >= 0.0)) ok = false;        // a negative or NaN lambda[b]: FAILED, written back as it came
  while(ok)
  {
    wsync();
    for(int e = lane; e < NP; e += 64) SL[e] = SA[e];
    wsync();
    if(lam > 0.0 && lane < N) SL[col_off(lane, N)] += lam;
    wsync();
    if constexpr(FIT)
    {
      if(hm)
      {
        int c = 0;
        for(int e = lane; e < NP; e += 64)
        {
          while(e >= col_off(c + 1, N)) c++;
          const int i = c + e - col_off(c, N);
          if(((hm >> c) | (hm >> i)) & 1) SL[e] = i == c ? 1.0 : 0.0;
        }
        wsync();
      }
    }
    if(chol_packed(SL, N, lane)) break;
    lam = lam == 0.0 ? LAMBDA_INITIAL : lam*10.0;
    if(!isfinite(lam)) ok = false;
  }
  report(ok, lam, n2x);
  if(!ok) return false;

  // ---- X = L^-1 in place, from the last column to the first (DTRTI2 'L'): column j of X is -X[j+1:, j+1:] L[j+1:, j] / L[j][j],
  // lane l takes row j + 1 + l ----
  for(int j = N - 1; j >= 0; j--)
  {
    const int jj = col_off(j, N), i = j + 1 + lane;
    const double d = 1.0/SL[jj];
    double s = 0.0;
    if(i < N)
    {
      for(int k = j + 1; k <= i; k++) s += SL[col_off(k, N) + i - k]*SL[jj + k - j];
      s *= -d;
    }
    wsync();
    if(lane == 0) SL[jj] = d;
    if(i < N) SL[jj + 1 + lane] = s;
    wsync();
  }
  if constexpr(FIT)
  {
    if(hm)
    {
      if((hm >> lane) & 1) SL[col_off(lane, N)] = 0.0;
      wsync();
    }
  }
  return true;
}

// sqrt(w) of row r of a problem under the fit F, outside the first sweep: from its weights wb ([M / F.L.fs] or nullptr)
// or from the loss at the callback's x (xb: [M]), the bits the first sweep multiplied that row by
__device__ __forceinline__ double fit_sqrt_w(const FitDev& F, const double* wb, const double* xb, int r)
{
  const int f = r/F.L.fs;
  if(wb) return sqrt(wb[f]);
  if(F.L.kind == DOGLEG_AMD_LOSS_TRIVIAL) return 1.0;
  double rho, w;
  loss_eval(F.L, feature_s(xb + (size_t)f*F.L.fs, F.L.fs), rho, w);
  return sqrt(w);
}

// FIT: the leverage blocks and x of the second sweep are those of the weighted rows, against a Sigma with zero held rows and
// columns; a computed scale counts the free variables only
//
// FORM_MODEL, FORM_POISSON: the second sweep forms its rows again, as the first did
template <int NMAX, int FORM, bool FIT>
__device__ void unc_problem(const UncDev& A, const FitDev& F, const ModelEvalDev& E, int b, int lane, double* S)
{
  using C = BatchCfg<NMAX>;
  const int N = A.N, M = A.M, NP = A.NP;
  double* SA = S;                      // JtJ, then Sigma
  double* SL = S + C::NP;              // the row tile of the sweeps; between them the factor and its inverse
  const double* Jb = nullptr; const double* xb = nullptr;
  [[maybe_unused]] const double* wb = nullptr;
  if constexpr(FORM == FORM_J)
  {
    Jb = A.J + (size_t)b*M*N;
    xb = A.x + (size_t)b*M;
    if constexpr(FIT) { if(F.wts) wb = F.wts + (size_t)b*(M/F.L.fs); }
  }

  double scale = 0.0;
  unsigned long long hm = 0;
  const bool stands = factor_and_invert<NMAX, FORM, FIT>(A, F, E, b, lane, SA, SL, hm, [&](bool ok, double lam, double n2x)
  {
    if(A.fac)
    {
      scale = A.scale[b];
      if(!(scale > 0.0))
      {
        // NoutlierFeatures = 0 (api_extensions.cpp: outlier_scale); NaN for a problem that failed on a non-finite x
        if constexpr(FIT)
        {
          const int NFree = N - __popcll(hm);
          scale = (double)M/(4.0*((double)(NFree + 1)*n2x/(double)(M - NFree - 1)));
        }
        else scale = (double)M/(4.0*((double)(N + 1)*n2x/(double)(M - N - 1)));
        if(lane == 0) A.scale[b] = scale;
      }
    }
    if(lane == 0) { A.lam[b] = lam; A.status[b] = ok ? DOGLEG_AMD_BATCH_UNC_OK : DOGLEG_AMD_BATCH_UNC_FAILED; }
    if(!ok)
    {
      const double nan = __builtin_nan("");
      if(A.var && lane < N) A.var[(size_t)b*N + lane] = nan;
      if(A.cov) for(int e = lane; e < N*N; e += 64) A.cov[(size_t)b*N*N + e] = nan;
      if(A.fac) for(int f = lane; f < A.NF; f += 64) A.fac[(size_t)b*A.NF + f] = nan;
    }
  });
  if(!stands) return;

  // ---- Sigma = X' X, one lane per entry: Sigma[i][j] = sum over r >= i of X[r][i] X[r][j] (i >= j) ----
  {
    int ei[C::NE], ej[C::NE];
    packed_entries<NMAX>(N, NP, lane, ei, ej);
#pragma unroll
    for(int k = 0; k < C::NE; k++)
      if(lane + 64*k < NP)
      {
        const double* ci = SL + col_off(ei[k], N); const double* cj = SL + col_off(ej[k], N) + ei[k] - ej[k];
        double s = 0.0;
        for(int r = 0; r < N - ei[k]; r++) s += ci[r]*cj[r];
        SA[lane + 64*k] = s;
      }
  }
  wsync();
  if(A.var && lane < N) A.var[(size_t)b*N + lane] = SA[col_off(lane, N)];
  if(A.cov)
    for(int e = lane; e < N*N; e += 64)
    {
      const int i = e/N;
      A.cov[(size_t)b*N*N + e] = sym_at(SA, i, e - i*N, N);
    }
  if constexpr(form_rows(FORM))
  {
    // ---- the second sweep of the model forms: the J form's tiles (T rows at the stride N | 1, lane t takes feature t), the rows
    // formed where the J form copies them.  Lane t evaluates row r0 + t, as in sweep_model, and stores it at t (N | 1); its x stays
    // in the lane: the x of feature t's rows is this lane's (fs = 1) or comes by two shuffles (fs = 2).  The loads of the next
    // tile's y, t and scale are in flight under the features' loop
    if(!A.fac) return;
    constexpr int NM = DOGLEG_BATCH_MODEL_MAX_NSTATE;
    const int fs = A.fs, NF = A.NF, NS = N | 1, Mc = NF*fs;
    int T = min(min(64, BATCH_TILE/N), (BATCH_TILE + 64)/NS);
    if(fs == 2) T &= ~1;
    const double kf = scale/8.0;
    double* tile = SL;
    const ModelDev& Md = E.Mdl;
    double p[NM];
#pragma unroll
    for(int j = 0; j < NM; j++) p[j] = j < N ? E.p[(size_t)b*N + j] : 0.0;
    constexpr int SRC = form_src(FORM);
    const double* yb = SRC == SRC_F64 ? Md.y + (size_t)b*M : nullptr;
    const double* tb = Md.t ? Md.t + (Md.t_each ? (size_t)b*M : (size_t)0) : nullptr;
    const double* sb = Md.scale ? Md.scale + (size_t)b*M : nullptr;
    double yv = 0.0, tv = 0.0, sv = 1.0;
    [[maybe_unused]] double vv = 0.0;
    const CamSrc<SRC> cs(E.Cam, b, M, Md.width);
    CamLane<SRC> cl{};
    if(lane < min(T, Mc))
    {
      if constexpr(SRC == SRC_F64) yv = yb[lane]; else cs.load(lane, cl);
      tv = tb ? tb[lane] : (double)lane;
      if(sb) sv = sb[lane];
    }
    for(int r0 = 0; r0 < Mc; r0 += T)
    {
      const int tc = min(T, Mc - r0);
      double xv = 0.0, jr[NM];
#pragma unroll
      for(int j = 0; j < NM; j++) jr[j] = 0.0;
      if constexpr(SRC != SRC_F64) cs.datum(cl, yv, vv);
      if(lane < tc)
      {
        if constexpr(form_poisson(FORM))
        {
          double dv;
          (void)poisson_row<rows_eval(FORM)>(Md.kind, p, r0 + lane, Md.width, tv, yv, vv, &xv, jr, &dv);
        }
        else dogleg_batch_model_row(Md.kind, p, r0 + lane, Md.width, tv, yv, sv, &xv, jr);
      }
      wsync();
      if(lane < tc)
      {
#pragma unroll
        for(int j = 0; j < NM; j++) if(j < N) tile[lane*NS + j] = jr[j];
      }
      wsync();
      if(r0 + T < Mc)
      {
        const int r1 = r0 + T, tn = min(T, Mc - r1);
        if(lane < tn)
        {
          if constexpr(SRC == SRC_F64) yv = yb[r1 + lane]; else cs.load(r1 + lane, cl);
          tv = tb ? tb[r1 + lane] : (double)(r1 + lane);
          if(sb) sv = sb[r1 + lane];
        }
      }
      // (every lane makes the shuffles, so that they find their sources)
      const double x0 = fs == 1 ? xv : __shfl(xv, (2*lane) & 63, 64);
      const double x1 = fs == 1 ? 0.0 : __shfl(xv, (2*lane + 1) & 63, 64);
      if(lane*fs < tc)
      {
        const size_t f = (size_t)(r0/fs + lane);
        if(fs == 1) A.fac[(size_t)b*NF + f] = feature1(SA, tile + lane*NS, N, x0, kf);
        else        A.fac[(size_t)b*NF + f] = feature2(SA, tile + 2*lane*NS, NS, N, x0, x1, kf);
      }
    }
    return;
  }
  if(FORM != FORM_J || !A.fac) return;

  // ---- the second sweep over J: tiles of T rows, row stride N | 1 in LDS (lanes read different rows: an odd stride keeps
  // them on different banks), lane t takes feature t of the tile: a = J_f Sigma J_f' against Sigma in LDS ----
  const int fs = A.fs, NF = A.NF, NS = N | 1, Mc = NF*fs;
  if constexpr(NMAX > 32)
  {
    const double kf = scale/8.0;
    double* tile = SL;
    // the classes above 32 variables: the first sweep's tile would hold 4 to 7 rows, so 4 to 7 lanes of 64 would work.  The
    // tile is the whole region the factor lay in, NP doubles: T = min(64, NP / (N | 1)) rows (24 .. 35 at <48>, 32 .. 42 at
    // <64>), copied from global memory as it lies (coalesced) with no registers held across the features' loops
    int T = min(64, C::SCR/NS);
    if(fs == 2) T &= ~1;
    for(int r0 = 0; r0 < Mc; r0 += T)
    {
      const int tc = min(T, Mc - r0), cnt = tc*N;
      const double* Jt = Jb + (size_t)r0*N;
      wsync();
      if constexpr(FIT)
      {
        // lane t holds sqrt(w) of row t of the tile; every lane makes every trip, so that the shuffle finds its source
        const double sw = lane < tc ? fit_sqrt_w(F, wb, xb, r0 + lane) : 1.0;
        for(int e = lane, r = lane/N, c = lane - r*N; e - lane < cnt; e += 64)
        {
          const double m = __shfl(sw, r & 63, 64);
          if(e < cnt) tile[r*NS + c] = Jt[e]*m;
          c += 64;
          while(c >= N) { c -= N; r++; }
        }
      }
      else
        for(int e = lane, r = lane/N, c = lane - r*N; e < cnt; e += 64)
        {
          tile[r*NS + c] = Jt[e];
          c += 64;
          while(c >= N) { c -= N; r++; }
        }
      wsync();
      if(lane*fs < tc)
      {
        const size_t f = (size_t)(r0/fs + lane);
        if constexpr(FIT)
        {
          const int r = r0 + fs*lane;
          const double x0 = fit_sqrt_w(F, wb, xb, r)*xb[r];
          if(fs == 1) A.fac[(size_t)b*NF + f] = feature1(SA, tile + lane*NS, N, x0, kf);
          else        A.fac[(size_t)b*NF + f] = feature2(SA, tile + 2*lane*NS, NS, N, x0, fit_sqrt_w(F, wb, xb, r + 1)*xb[r + 1], kf);
        }
        else if(fs == 1) A.fac[(size_t)b*NF + f] = feature1(SA, tile + lane*NS, N, xb[r0 + lane], kf);
        else             A.fac[(size_t)b*NF + f] = feature2(SA, tile + 2*lane*NS, NS, N, xb[r0 + 2*lane], xb[r0 + 2*lane + 1], kf);
      }
    }
    return;
  }
  int T = min(min(64, BATCH_TILE/N), (BATCH_TILE + 64)/NS);
  if(fs == 2) T &= ~1;
  constexpr int NL = BATCH_TILE/64;
  int po[NL];
#pragma unroll
  for(int u = 0; u < NL; u++) { const int e = lane + 64*u, r = e/N; po[u] = r*NS + e - r*N; }
  const double kf = scale/8.0;
  double* tile = SL;
  double v[NL];
  {
    const int cnt = min(T, Mc)*N;
#pragma unroll
    for(int u = 0; u < NL; u++) v[u] = lane + 64*u < cnt ? Jb[lane + 64*u] : 0.0;
  }
  for(int r0 = 0; r0 < Mc; r0 += T)
  {
    const int tc = min(T, Mc - r0);
    wsync();
    if constexpr(FIT)
    {
      // lane t holds sqrt(w) of row t of the tile (the rows behind the tile's hold 0)
      const double sw = lane < tc ? fit_sqrt_w(F, wb, xb, r0 + lane) : 1.0;
#pragma unroll
      for(int u = 0; u < NL; u++)
      {
        const double m = __shfl(sw, min((lane + 64*u)/N, 63), 64);
        if(lane + 64*u < T*N) tile[po[u]] = v[u]*m;
      }
    }
    else
    {
#pragma unroll
      for(int u = 0; u < NL; u++) if(lane + 64*u < T*N) tile[po[u]] = v[u];
    }
    wsync();
    if(r0 + T < Mc)
    {
      const int r1 = r0 + T, cnt = min(T, Mc - r1)*N;
      const double* Jn = Jb + (size_t)r1*N;
#pragma unroll
      for(int u = 0; u < NL; u++) v[u] = lane + 64*u < cnt ? Jn[lane + 64*u] : 0.0;
    }
    if(lane*fs < tc)
    {
      const size_t f = (size_t)(r0/fs + lane);
      if(fs == 1)
      {
        const double* r = tile + lane*NS;
        double a = 0.0;
        int idx = 0;
        for(int j = 0; j < N; j++)
        {
          const double rj = r[j], d = SA[idx++];
          double t0 = 0.0;
          for(int i = j + 1; i < N; i++) t0 += SA[idx++]*r[i];
          a += rj*(d*rj + 2.0*t0);
        }
        if constexpr(FIT) A.fac[(size_t)b*NF + f] = factor1(a, fit_sqrt_w(F, wb, xb, r0 + lane)*xb[r0 + lane], kf);
        else              A.fac[(size_t)b*NF + f] = factor1(a, xb[r0 + lane], kf);
      }
      else
      {
        const double* ra = tile + 2*lane*NS; const double* rb = ra + NS;
        double a00 = 0.0, a01 = 0.0, a11 = 0.0;
        int idx = 0;
        for(int j = 0; j < N; j++)
        {
          const double aj = ra[j], bj = rb[j], d = SA[idx++];
          double t0 = 0.0, t1 = 0.0;
          for(int i = j + 1; i < N; i++) { const double s = SA[idx++]; t0 += s*ra[i]; t1 += s*rb[i]; }
          a00 += aj*(d*aj + 2.0*t0); a01 += aj*(d*bj + t1) + bj*t0; a11 += bj*(d*bj + 2.0*t1);
        }
        if constexpr(FIT)
        {
          const int r = r0 + 2*lane;
          A.fac[(size_t)b*NF + f] = factor2(a00, a01, a11, fit_sqrt_w(F, wb, xb, r)*xb[r], fit_sqrt_w(F, wb, xb, r + 1)*xb[r + 1], kf);
        }
        else A.fac[(size_t)b*NF + f] = factor2(a00, a01, a11, xb[r0 + 2*lane], xb[r0 + 2*lane + 1], kf);
      }
    }
  }
}

template <int NMAX, int FORM, bool FIT>
__global__ void __launch_bounds__(64*BatchCfg<NMAX>::WPB) k_batch_uncertainty(UncDev A, FitDev F, ModelEvalDev E)
{
  constexpr int LDSW = BatchCfg<NMAX>::NP + FormCfg<NMAX, FORM>::SCR, WPB = BatchCfg<NMAX>::WPB;
  __shared__ double lds[WPB*LDSW];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x*WPB + w;
  if(b >= A.B) return;
  // the mask: b is the wave's, so the whole wave leaves together
  if(A.active && !A.active[b])
  {
    if(lane == 0) A.status[b] = DOGLEG_AMD_BATCH_UNC_SKIPPED;
    return;
  }
  unc_problem<NMAX, FORM, FIT>(A, F, E, b, lane, lds + w*LDSW);
}

// a . b over the wave, every lane ending with the same bits: the products are rounded before the butterfly.  (An FMA that took
// its lane's product into the first level's sum would round differently in the two lanes of a pair.)
__device__ inline double wave_dot(double a, double b)
{
#pragma clang fp contract(off)
  double v = a*b;
  for(int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- dogleg_amd_dense_batch_query_covariance: Var(q) = Jq Sigma_b Jq' of Nq caller-supplied query Jacobians of Q rows per
// problem, ONE launch behind one call of the batch callback.  Per wave: factor_and_invert, then per query row c the forward
// product z_c = X Jq_c' (lane i holds element i), and out[c][d] = z_c . z_d by the wave's butterfly sum: Sigma is never formed.
// The observations-only (sandwich) form Jq Sigma J_obs' J_obs Sigma Jq' (J form, nobs >= 0): G = J_obs' J_obs by a sweep of its
// own over the first nobs rows, Y_c = X' z_c (= Sigma Jq_c'), out[c][d] = Y_c' G Y_d.
// LDS of a wavefront of the query kernel: JtJ | the row tile, then the factor and X | an N-vector | G (J form) | the Q vectors
// z (or Y) of one query.  The last lie in the region of JtJ, which nobody reads once the factorisation stands, where that
// holds DOGLEG_AMD_BATCH_QUERY_MAX_ROWS rows (from <32> on), and in a region of their own below
template <int NMAX, int FORM> struct QueryCfg
{
  using C = BatchCfg<NMAX>;
  static constexpr int SCR = FormCfg<NMAX, FORM>::SCR;
  static constexpr int GB = FORM != FORM_PRODUCTS ? C::NP : 0;
  static constexpr int ZROWS = DOGLEG_AMD_BATCH_QUERY_MAX_ROWS*NMAX;
  static constexpr int ZOWN = C::NP >= ZROWS ? 0 : ZROWS;
  static constexpr int LDSW = C::NP + SCR + NMAX + GB + ZOWN;
  static_assert(sizeof(double)*C::WPB*LDSW <= 65536, "k_batch_query: the wavefronts of a workgroup need more than 64 KB of LDS");
};

// FIT: G is that of the weighted rows, X that of the free block (factor_and_invert); everything behind them is the same text
// FORM_MODEL, FORM_POISSON: G is sweep_model's JtJ over the first nobs rows, the data Nmeas apart
template <int NMAX, int FORM, bool FIT>
__device__ void query_problem(const QueryDev& A, const FitDev& F, const ModelEvalDev& E, int b, int lane, double* S)
{
  using C = BatchCfg<NMAX>;
  using QC = QueryCfg<NMAX, FORM>;
  const UncDev& U = A.U;
  const int N = U.N, Q = A.Q;
  double* SA = S;                      // JtJ
  double* SL = SA + C::NP;             // the row tile of the sweeps, then the factor and X = L^-1
  double* SV = SL + QC::SCR;           // an N-vector, read at wave-uniform addresses
  double* SG = SV + NMAX;              // G, packed as JtJ
  double* SZ = QC::ZOWN ? SG + QC::GB : SA;       // z_c (sandwich form: Y_c), row c at c N
  const size_t rows = (size_t)A.Nq*Q;
  const double* Jqb = A.Jq + (size_t)b*rows*N;
  double* ob = A.out + (size_t)b*rows*Q;

  bool sandwich = false;
  if constexpr(FORM == FORM_J)
  {
    sandwich = A.nobs >= 0;
    if(sandwich)
    {
      // sweep_point over the first nobs rows: its JtJ is G (nobs = 0: no row is read, G is exactly 0)
      double g;
      if constexpr(FIT)
        (void)sweep_point<NMAX, SWEEP_FIT>(U.J + (size_t)b*U.M*N, U.x + (size_t)b*U.M, N, A.nobs, U.NP, lane, SG, SL, g, F.L,
                                           F.wts ? F.wts + (size_t)b*(U.M/F.L.fs) : nullptr);
      else
        (void)sweep_point<NMAX>(U.J + (size_t)b*U.M*N, U.x + (size_t)b*U.M, N, A.nobs, U.NP, lane, SG, SL, g);
    }
  }
  else if constexpr(form_rows(FORM))
  {
    sandwich = A.nobs >= 0;
    if(sandwich)
    {
      double g;
      (void)sweep_model<NMAX, rows_eval(FORM), form_src(FORM)>(E.Mdl, E.Cam, E.p + (size_t)b*N, b, N, A.nobs, U.M, U.NP, lane, SG, SL, g);
    }
  }
  unsigned long long hm = 0;
  const bool stands = factor_and_invert<NMAX, FORM, FIT>(U, F, E, b, lane, SA, SL, hm, [&](bool ok, double lam, double)
  {
    if(lane == 0) { U.lam[b] = lam; U.status[b] = ok ? DOGLEG_AMD_BATCH_UNC_OK : DOGLEG_AMD_BATCH_UNC_FAILED; }
    if(!ok)
    {
      const double nan = __builtin_nan("");
      for(size_t e = lane; e < rows*Q; e += 64) ob[e] = nan;
    }
  });
  if(!stands) return;

  // the rows of Jq as they lie, lane i element i of a row (coalesced); the next row's load is in flight under the current
  // row's product
  double qn = lane < N ? Jqb[lane] : 0.0;
  for(int q = 0; q < A.Nq; q++)
  {
    for(int c = 0; c < Q; c++)
    {
      const size_t r = (size_t)q*Q + c;
      const double qv = qn;
      if(r + 1 < rows) qn = lane < N ? Jqb[(r + 1)*N + lane] : 0.0;
      wsync();
      if(lane < N) SV[lane] = qv;
      wsync();
      // z = X Jq_c': lane i sums along row i of X (consecutive lanes read consecutive doubles of a column)
      double z = 0.0;
      if(lane < N)
        for(int j = 0; j <= lane; j++) z += SL[col_off(j, N) + lane - j]*SV[j];
      if(sandwich)
      {
        // Y = X' z: lane i sums along column i of X
        wsync();
        if(lane < N) SV[lane] = z;
        wsync();
        double y = 0.0;
        if(lane < N)
        {
          const double* col = SL + col_off(lane, N) - lane;
          for(int k = lane; k < N; k++) y += col[k]*SV[k];
        }
        z = y;
      }
      if(lane < N) SZ[c*N + lane] = z;
    }
    wsync();
    // the triangle of the block, every entry once: the butterfly leaves the same bits in every lane, the lanes that own
    // [c][d] and [d][c] store them -- a bitwise symmetric block whose diagonal (plain form) is a sum of squares
    double* oq = ob + (size_t)q*Q*Q;
    for(int d = 0; d < Q; d++)
    {
      double w = lane < N ? SZ[d*N + lane] : 0.0;
      if(sandwich)
      {
        // w = G Y_d
        wsync();
        if(lane < N) SV[lane] = w;
        wsync();
        double t = 0.0;
        if(lane < N)
          for(int j = 0; j < N; j++) t += sym_at(SG, lane, j, N)*SV[j];
        w = t;
      }
      for(int c = 0; c <= d; c++)
      {
        const double zc = lane < N ? SZ[c*N + lane] : 0.0;
        const double s = wave_dot(zc, w);
        const int e = c*Q + d, f = d*Q + c;
        if(lane == (e & 63)) oq[e] = s;
        if(c != d && lane == (f & 63)) oq[f] = s;
      }
    }
    wsync();
  }
}

template <int NMAX, int FORM, bool FIT>
__global__ void __launch_bounds__(64*BatchCfg<NMAX>::WPB) k_batch_query(QueryDev A, FitDev F, ModelEvalDev E)
{
  constexpr int LDSW = QueryCfg<NMAX, FORM>::LDSW, WPB = BatchCfg<NMAX>::WPB;
  __shared__ double lds[WPB*LDSW];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x*WPB + w;
  if(b >= A.U.B) return;
  // the mask, as in k_batch_uncertainty
  if(A.U.active && !A.U.active[b])
  {
    if(lane == 0) A.U.status[b] = DOGLEG_AMD_BATCH_UNC_SKIPPED;
    return;
  }
  query_problem<NMAX, FORM, FIT>(A, F, E, b, lane, lds + w*LDSW);
}

// active: [B] or nullptr (all); a problem with active[b] == 0 starts, and stays, not live
__global__ void __launch_bounds__(256) k_batch_init(BatchDev A, const unsigned char* active)
{
  const int b = blockIdx.x*256 + threadIdx.x;
  if(b >= A.B) return;
  double* sc = A.sc + (size_t)SC_COUNT*b; int* st = A.st + (size_t)ST_COUNT*b;
  for(int k = 0; k < SC_COUNT; k++) sc[k] = 0.0;
  sc[SC_TR] = A.trustregion0;
  for(int k = 0; k < ST_COUNT; k++) st[k] = 0;
  A.live[b] = active ? (active[b] ? 1 : 0) : 1;
}

// the start of a bounded solve, behind k_batch_init: the start point of every live problem clamped into its box.  A problem with
// a NaN bound or lo > hi is FAILED here, alone: never live, no evaluation, its p not touched
__global__ void __launch_bounds__(256) k_batch_clamp(BatchDev A)
{
  const int b = blockIdx.x*256 + threadIdx.x;
  if(b >= A.B || !A.live[b]) return;
  const size_t bN = (size_t)b*A.N;
  bool ok = true;
  for(int i = 0; i < A.N; i++)
  {
    const double lo = A.lo ? A.lo[bN + i] : -INFINITY, hi = A.hi ? A.hi[bN + i] : INFINITY;
    if(!(lo <= hi)) ok = false;
  }
  if(!ok)
  {
    A.st[(size_t)ST_COUNT*b + ST_STATUS] = DOGLEG_AMD_BATCH_FAILED;
    A.live[b] = 0;
    return;
  }
  for(int i = 0; i < A.N; i++)
  {
    double p = A.p_trial[bN + i];
    if(A.lo && p < A.lo[bN + i]) p = A.lo[bN + i];
    if(A.hi && p > A.hi[bN + i]) p = A.hi[bN + i];
    A.p_trial[bN + i] = p;
  }
}

// the end of a device-resident solve: the state of every problem into the caller's arrays (what solve_locked (dense_batch.hip) does on the
// host for the host-pointer entry points).  Thread t takes element t of p, [B][N] (coalesced stores; a problem that FAILED
// or was not run keeps its input), and, for t < B, the record and the lambda of problem t.  A status of 0 after the last
// round is a problem that never was live: every live problem leaves its last round with a status.
// The robust form (weights != nullptr; the grid covers [B][NF] too): thread t takes element t of the weights, NaN for a problem
// that FAILED.
// The bounded form (A.held != nullptr): the held set at the returned point, from p, g and the bounds as the round kernel forms
// it; all 0 for a problem that FAILED.
__global__ void __launch_bounds__(256) k_batch_finish(BatchDev A, double* p, dogleg_amd_batch_result_t* results, double* lambda,
                                                      double* weights)
{
  const size_t t = (size_t)blockIdx.x*256 + threadIdx.x;
  if(t < (size_t)A.B*A.N)
  {
    const int status = A.st[(size_t)ST_COUNT*(t/A.N) + ST_STATUS];
    if(status != DOGLEG_AMD_BATCH_NOT_RUN && status != DOGLEG_AMD_BATCH_FAILED) p[t] = A.p_before[t];
    if(A.held && status != DOGLEG_AMD_BATCH_NOT_RUN)
      A.held[t] = status == DOGLEG_AMD_BATCH_FAILED ? 0 :
                  held_code(A.p_before[t], A.g[t], A.lo ? A.lo[t] : -INFINITY, A.hi ? A.hi[t] : INFINITY);
  }
  if(weights && t < (size_t)A.B*A.NF)
  {
    const int status = A.st[(size_t)ST_COUNT*(t/A.NF) + ST_STATUS];
    if(status == DOGLEG_AMD_BATCH_FAILED) weights[t] = __builtin_nan("");
    else if(status != DOGLEG_AMD_BATCH_NOT_RUN) weights[t] = A.wts[t];
  }
  if(t >= (size_t)A.B) return;
  const int* st = A.st + (size_t)ST_COUNT*t; const double* sc = A.sc + (size_t)SC_COUNT*t;
  const int status = st[ST_STATUS];
  const bool run = status != DOGLEG_AMD_BATCH_NOT_RUN;
  dogleg_amd_batch_result_t& R = results[t];
  const double lam = run ? sc[SC_LAMBDA] : 0.0;
  R.norm2_x = !run || status == DOGLEG_AMD_BATCH_FAILED ? -1.0 : sc[SC_N2X];
  R.trustregion = run ? sc[SC_TR] : 0.0; R.lambda = lam;
  R.iterations = st[ST_ITER]; R.evaluations = st[ST_EVAL]; R.status = status;
  if(lambda) lambda[t] = lam;
}

// ---- the launchers (dense_batch_dev.h).  The size class of a problem of N variables, as a type: fn(integral_constant<NMAX>)
template <class Fn> void for_size_class(int N, Fn fn)
{
  if(N <= 8)       fn(std::integral_constant<int, 8>{});
  else if(N <= 16) fn(std::integral_constant<int, 16>{});
  else if(N <= 24) fn(std::integral_constant<int, 24>{});
  else if(N <= 32) fn(std::integral_constant<int, 32>{});
  else if(N <= 48) fn(std::integral_constant<int, 48>{});
  else             fn(std::integral_constant<int, 64>{});
}
// the grid and the block follow the size class: BatchCfg<NMAX>::WPB problems per workgroup
template <int NMAX, class... Args> void launch_class(void (*kernel)(Args...), hipStream_t st, int B, const Args&... A)
{
  constexpr int WPB = BatchCfg<NMAX>::WPB;
  hipLaunchKernelGGL(kernel, dim3((B + WPB - 1)/WPB), dim3(64*WPB), 0, st, A...);
}
dim3 grid256(size_t n) { return dim3((unsigned int)((n + 255)/256)); }

} // namespace

void launch_batch_round(hipStream_t st, const BatchDev& A)
{
  for_size_class(A.N, [&](auto c) {
    constexpr int NMAX = decltype(c)::value;
    if(A.Cam.raw)
    {
      // (a camera record: the model forms with the readings as their data; calibrated or not is the instantiation, the type of
      // the readings a switch inside it)
      if constexpr(NMAX == 8)
      {
        const bool poisson = A.Mdl.likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON;
        if(A.Cam.cal)
        {
          if(poisson)
          {
            if(A.Cam.readvar)
            {
              if(A.bounded)  launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON_CALV, false, true>, st, A.B, A);
              else           launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON_CALV, false, false>, st, A.B, A);
            }
            else if(A.bounded) launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON_CAL, false, true>, st, A.B, A);
            else             launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON_CAL, false, false>, st, A.B, A);
          }
          else if(A.bounded) launch_class<NMAX>(k_batch_round<NMAX, FORM_MODEL_CAL, false, true>, st, A.B, A);
          else               launch_class<NMAX>(k_batch_round<NMAX, FORM_MODEL_CAL, false, false>, st, A.B, A);
        }
        else if(poisson)
        {
          if(A.bounded)      launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON_RAW, false, true>, st, A.B, A);
          else               launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON_RAW, false, false>, st, A.B, A);
        }
        else if(A.bounded)   launch_class<NMAX>(k_batch_round<NMAX, FORM_MODEL_RAW, false, true>, st, A.B, A);
        else                 launch_class<NMAX>(k_batch_round<NMAX, FORM_MODEL_RAW, false, false>, st, A.B, A);
      }
    }
    else if(A.Mdl.y)
    {
      // (every built-in model lies in the class of 8: the host side refuses anything else)
      if constexpr(NMAX == 8)
      {
        if(A.Mdl.likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON)
        {
          if(A.bounded)      launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON, false, true>, st, A.B, A);
          else               launch_class<NMAX>(k_batch_round<NMAX, FORM_POISSON, false, false>, st, A.B, A);
        }
        else if(A.bounded)   launch_class<NMAX>(k_batch_round<NMAX, FORM_MODEL, false, true>, st, A.B, A);
        else                 launch_class<NMAX>(k_batch_round<NMAX, FORM_MODEL, false, false>, st, A.B, A);
      }
    }
    else if(A.P.n2x)
    {
      if(A.bounded)          launch_class<NMAX>(k_batch_round<NMAX, FORM_PRODUCTS, false, true>, st, A.B, A);
      else                   launch_class<NMAX>(k_batch_round<NMAX, FORM_PRODUCTS, false, false>, st, A.B, A);
    }
    else if(A.bounded)
    {
      if(A.robust)           launch_class<NMAX>(k_batch_round<NMAX, FORM_J, true, true>, st, A.B, A);
      else                   launch_class<NMAX>(k_batch_round<NMAX, FORM_J, false, true>, st, A.B, A);
    }
    else if(A.robust)        launch_class<NMAX>(k_batch_round<NMAX, FORM_J, true, false>, st, A.B, A);
    else                     launch_class<NMAX>(k_batch_round<NMAX, FORM_J, false, false>, st, A.B, A);
  });
}
// (the model forms: the class of 8 only, as in launch_batch_round, and one instantiation with FIT for both: without a held set hm
// is 0 and NFree is N, which leaves the text without FIT)
void launch_batch_uncertainty(hipStream_t st, const UncDev& A, const FitDev& F, const ModelEvalDev& E)
{
  for_size_class(A.N, [&](auto c) {
    constexpr int NMAX = decltype(c)::value;
    if(E.Cam.raw)
    {
      if constexpr(NMAX == 8)
      {
        const bool poisson = E.Mdl.likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON;
        if(E.Cam.cal)
        {
          if(poisson && E.Cam.readvar) launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_POISSON_CALV, true>, st, A.B, A, F, E);
          else if(poisson) launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_POISSON_CAL, true>, st, A.B, A, F, E);
          else        launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_MODEL_CAL, true>, st, A.B, A, F, E);
        }
        else if(poisson) launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_POISSON_RAW, true>, st, A.B, A, F, E);
        else             launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_MODEL_RAW, true>, st, A.B, A, F, E);
      }
    }
    else if(E.Mdl.y)
    {
      if constexpr(NMAX == 8)
      {
        if(E.Mdl.likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON)
             launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_POISSON, true>, st, A.B, A, F, E);
        else launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_MODEL, true>, st, A.B, A, F, E);
      }
    }
    else if(F.fit)
    {
      if(A.P.n2x) launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_PRODUCTS, true>, st, A.B, A, F, E);
      else        launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_J, true>, st, A.B, A, F, E);
    }
    else if(A.P.n2x) launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_PRODUCTS, false>, st, A.B, A, F, E);
    else             launch_class<NMAX>(k_batch_uncertainty<NMAX, FORM_J, false>, st, A.B, A, F, E);
  });
}
void launch_batch_query(hipStream_t st, const QueryDev& A, const FitDev& F, const ModelEvalDev& E)
{
  for_size_class(A.U.N, [&](auto c) {
    constexpr int NMAX = decltype(c)::value;
    if(E.Cam.raw)
    {
      if constexpr(NMAX == 8)
      {
        const bool poisson = E.Mdl.likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON;
        if(E.Cam.cal)
        {
          if(poisson && E.Cam.readvar) launch_class<NMAX>(k_batch_query<NMAX, FORM_POISSON_CALV, true>, st, A.U.B, A, F, E);
          else if(poisson) launch_class<NMAX>(k_batch_query<NMAX, FORM_POISSON_CAL, true>, st, A.U.B, A, F, E);
          else        launch_class<NMAX>(k_batch_query<NMAX, FORM_MODEL_CAL, true>, st, A.U.B, A, F, E);
        }
        else if(poisson) launch_class<NMAX>(k_batch_query<NMAX, FORM_POISSON_RAW, true>, st, A.U.B, A, F, E);
        else             launch_class<NMAX>(k_batch_query<NMAX, FORM_MODEL_RAW, true>, st, A.U.B, A, F, E);
      }
    }
    else if(E.Mdl.y)
    {
      if constexpr(NMAX == 8)
      {
        if(E.Mdl.likelihood == DOGLEG_AMD_LIKELIHOOD_POISSON)
             launch_class<NMAX>(k_batch_query<NMAX, FORM_POISSON, true>, st, A.U.B, A, F, E);
        else launch_class<NMAX>(k_batch_query<NMAX, FORM_MODEL, true>, st, A.U.B, A, F, E);
      }
    }
    else if(F.fit)
    {
      if(A.U.P.n2x) launch_class<NMAX>(k_batch_query<NMAX, FORM_PRODUCTS, true>, st, A.U.B, A, F, E);
      else          launch_class<NMAX>(k_batch_query<NMAX, FORM_J, true>, st, A.U.B, A, F, E);
    }
    else if(A.U.P.n2x) launch_class<NMAX>(k_batch_query<NMAX, FORM_PRODUCTS, false>, st, A.U.B, A, F, E);
    else               launch_class<NMAX>(k_batch_query<NMAX, FORM_J, false>, st, A.U.B, A, F, E);
  });
}
void launch_batch_init(hipStream_t st, const BatchDev& A, const unsigned char* active)
{
  hipLaunchKernelGGL(k_batch_init, grid256((size_t)A.B), dim3(256), 0, st, A, active);
}
void launch_batch_clamp(hipStream_t st, const BatchDev& A)
{
  hipLaunchKernelGGL(k_batch_clamp, grid256((size_t)A.B), dim3(256), 0, st, A);
}
// the grid covers [B][N] and, with weights, [B][NF]
void launch_batch_finish(hipStream_t st, const BatchDev& A, double* p, dogleg_amd_batch_result_t* results, double* lambda,
                         double* weights)
{
  const size_t np = (size_t)A.B*A.N, nw = weights ? (size_t)A.B*A.NF : 0;
  hipLaunchKernelGGL(k_batch_finish, grid256(np > nw ? np : nw), dim3(256), 0, st, A, p, results, lambda, weights);
}
