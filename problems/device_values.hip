// device_values.hip -- the sparse model of device_gradcheck_problems.hip as a VALUES-ONLY model on the GPU, for the tests and
// tools of the single-problem numeric Jacobians (dogleg_amd_numeric_*).  Test plumbing: pattern, coefficients, p* and eps come
// from the caller, so a test can restate the model in numpy.  Compiled with -ffp-contract=off.
//
//   u_r = sum_t a_t (p[i_t] - p*[i_t]),  x_r = u_r + eps sin(u_r)      (u summed in index order, as k_gcp_sparse does)
//
// (a) dv_cb_values: a dogleg_callback_device_values_t, ONE launch for all copies, one thread per (copy, row).
// (b) dv_cb_naive: the naive reference of the numeric Jacobian, a dogleg_callback_device_t: per copy one launch that writes the
//     point and one launch of the values kernel for that point alone, then one thread per entry of Jt through the same
//     dogleg_numeric_step and the same subtraction and division.  The colouring is the caller's.
// (c) switches: NaN in every row of a copy that has a variable outside a given box; an undeclared dependence
//     x[r_extra] += c (p[w] - p*[w]); x[r_nan] = NaN; counters of calls, of copies (the naive reference's launches count too)
//     and of copies outside the box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include "../include/dogleg_numeric_step.h"

namespace {
struct ValuesProblem
{
  int N, M, nnz;
  int *Jp, *Ji;
  double *a, *pstar;
  double eps;
  double *box_lo, *box_hi; int box_on;   // (c) box: NaN outside
  unsigned long long* d_outside;         //     copies evaluated with a variable outside the box, counted on the device
  int r_extra, w; double c;              // (c) undeclared dependence, off: r_extra < 0
  int r_nan;                             // (c) off: r_nan < 0
  long long ncalls, ncopies;
};
struct NaiveReference
{
  ValuesProblem* P;
  int C, K, scheme;
  double delta_rel, delta_abs;
  int* colour;                           // [N], device
  double *lower, *upper;                 // [N] device, or nullptr
  double *pc, *xc;                       // [K][N], [K][M]
};

__global__ void __launch_bounds__(256) k_dv_values(ValuesProblem P, unsigned copies, const double* __restrict__ p, double* __restrict__ x)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)copies*P.M) return;
  const unsigned k = (unsigned)(idx/P.M);
  const int r = (int)(idx - (size_t)k*P.M);
  const double* pk = p + (size_t)k*P.N;
  const int t0 = P.Jp[r], t1 = P.Jp[r + 1];
  double u = 0.0;
  for(int t = t0; t < t1; t++) { const int j = P.Ji[t]; u += P.a[t]*(pk[j] - P.pstar[j]); }
  double xr = u + P.eps*sin(u);
  if(r == P.r_extra) xr += P.c*(pk[P.w] - P.pstar[P.w]);
  if(r == P.r_nan) xr = nan("");
  if(P.box_on)
  {
    bool outside = false;
    for(int j = 0; j < P.N; j++)
      if(pk[j] < P.box_lo[j] || pk[j] > P.box_hi[j]) outside = true;
    if(outside) { xr = nan(""); if(r == 0) atomicAdd(P.d_outside, 1ull); }
  }
  x[idx] = xr;
}

// copy k of the naive reference: every variable of the copy's colour at its plus or minus point
__global__ void __launch_bounds__(256) k_dv_point(int N, int C, int k, int scheme, double delta_rel, double delta_abs,
                                                  const int* __restrict__ colour, const double* __restrict__ lower,
                                                  const double* __restrict__ upper, const double* __restrict__ p,
                                                  double* __restrict__ out)
{
  const int j = blockIdx.x*256 + threadIdx.x;
  if(j >= N) return;
  double v = p[j];
  const int cj = colour[j];
  if(k >= 1 && ((k - 1) == cj || (k - 1 - C) == cj))
  {
    double tp, tm, d;
    dogleg_numeric_step(scheme, v, lower ? lower[j] : -INFINITY, upper ? upper[j] : INFINITY, delta_rel, delta_abs, &tp, &tm, &d);
    v = (k - 1) == cj ? tp : tm;
  }
  out[j] = v;
}

// one thread per entry of Jt; the row by a linear walk of Jp
__global__ void __launch_bounds__(256) k_dv_naive_J(int N, int M, int nnz, int C, int scheme, double delta_rel, double delta_abs,
                                                    const int* __restrict__ Jp, const int* __restrict__ Ji,
                                                    const int* __restrict__ colour, const double* __restrict__ lower,
                                                    const double* __restrict__ upper, const double* __restrict__ p,
                                                    const double* __restrict__ xc, double* __restrict__ x, double* __restrict__ J)
{
  const int t = blockIdx.x*256 + threadIdx.x;
  if(t < M) x[t] = xc[t];
  if(t >= nnz) return;
  int r = 0;
  while(Jp[r + 1] <= t) r++;
  const int v = Ji[t], c = colour[v];
  double tp, tm, d;
  dogleg_numeric_step(scheme, p[v], lower ? lower[v] : -INFINITY, upper ? upper[v] : INFINITY, delta_rel, delta_abs, &tp, &tm, &d);
  const double xp = xc[(size_t)(1 + c)*M + r];
  const double xm = scheme == DOGLEG_NUMERIC_STEP_CENTRAL ? xc[(size_t)(1 + C + c)*M + r] : xc[r];
  J[t] = d == 0.0 ? 0.0 : (xp - xm)/d;
}

template <class T> T* to_device(const T* h, size_t n)
{
  T* d = nullptr;
  if(hipMalloc(&d, sizeof(T)*(n ? n : 1)) != hipSuccess) return nullptr;
  if(n && h && hipMemcpy(d, h, sizeof(T)*n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
  return d;
}

void launch_values(ValuesProblem* P, const double* p_dev, double* x_dev, unsigned copies, hipStream_t st)
{
  const size_t work = (size_t)copies*P->M;
  hipLaunchKernelGGL(k_dv_values, dim3((unsigned)((work + 255)/256)), dim3(256), 0, st, *P, copies, p_dev, x_dev);
}
} // namespace

extern "C" {

void dv_free(void* h)
{
  ValuesProblem* P = (ValuesProblem*)h;
  if(!P) return;
  (void)hipFree(P->Jp); (void)hipFree(P->Ji); (void)hipFree(P->a); (void)hipFree(P->pstar);
  (void)hipFree(P->box_lo); (void)hipFree(P->box_hi); (void)hipFree(P->d_outside);
  delete P;
}
// Jp[M + 1], Ji[nnz]: the pattern of Jt; a[nnz], pstar[N]
void* dv_create(int N, int M, int nnz, const int* Jp, const int* Ji, const double* a, const double* pstar, double eps)
{
  ValuesProblem* P = new ValuesProblem();
  P->N = N; P->M = M; P->nnz = nnz; P->eps = eps; P->ncalls = P->ncopies = 0;
  P->box_on = 0; P->r_extra = -1; P->w = 0; P->c = 0.0; P->r_nan = -1;
  P->Jp = to_device(Jp, (size_t)M + 1); P->Ji = to_device(Ji, (size_t)nnz);
  P->a = to_device(a, (size_t)nnz); P->pstar = to_device(pstar, (size_t)N);
  P->box_lo = to_device((const double*)nullptr, (size_t)N); P->box_hi = to_device((const double*)nullptr, (size_t)N);
  const unsigned long long zero = 0;
  P->d_outside = to_device(&zero, 1);
  if(!P->Jp || !P->Ji || !P->a || !P->pstar || !P->box_lo || !P->box_hi || !P->d_outside)
  { fprintf(stderr, "dv_create: device allocation failed\n"); (void)hipGetLastError(); dv_free(P); return nullptr; }
  return P;
}
// lower, upper [N]; on == 0: the switch off (the arrays are then not read)
int dv_set_box(void* h, const double* lower, const double* upper, int on)
{
  ValuesProblem* P = (ValuesProblem*)h;
  P->box_on = 0;
  if(!on) return 0;
  if(hipMemcpy(P->box_lo, lower, sizeof(double)*P->N, hipMemcpyHostToDevice) != hipSuccess ||
     hipMemcpy(P->box_hi, upper, sizeof(double)*P->N, hipMemcpyHostToDevice) != hipSuccess) return -1;
  P->box_on = 1;
  return 0;
}
// a switch is off with a negative index
int dv_set_faults(void* h, int r_extra, int w, double c, int r_nan)
{
  ValuesProblem* P = (ValuesProblem*)h;
  if(r_extra >= P->M || r_nan >= P->M || (r_extra >= 0 && (w < 0 || w >= P->N))) return -1;
  P->r_extra = r_extra; P->w = r_extra >= 0 ? w : 0; P->c = c; P->r_nan = r_nan;
  return 0;
}
// copies that were evaluated with a variable outside the box, over all invocations (the box switch on)
long long dv_noutside(void* h)
{
  unsigned long long n = 0;
  if(hipMemcpy(&n, ((ValuesProblem*)h)->d_outside, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
long long dv_ncalls(void* h) { return ((ValuesProblem*)h)->ncalls; }
long long dv_ncopies(void* h) { return ((ValuesProblem*)h)->ncopies; }
void dv_reset(void* h) { ((ValuesProblem*)h)->ncalls = 0; ((ValuesProblem*)h)->ncopies = 0; }

// dogleg_callback_device_values_t
void dv_cb_values(const double* p_dev, double* x_dev, unsigned int copies, void* hip_stream, void* cookie)
{
  ValuesProblem* P = (ValuesProblem*)cookie;
  P->ncalls++; P->ncopies += copies;
  launch_values(P, p_dev, x_dev, copies, (hipStream_t)hip_stream);
}

void dv_naive_free(void* h)
{
  NaiveReference* R = (NaiveReference*)h;
  if(!R) return;
  (void)hipFree(R->colour); (void)hipFree(R->lower); (void)hipFree(R->upper); (void)hipFree(R->pc); (void)hipFree(R->xc);
  delete R;
}
// colour[N] with C colours: the caller's; lower / upper [N] host arrays or NULL.  The deltas are used as they are.
void* dv_naive_create(void* problem, const int* colour, int C, int scheme, double delta_rel, double delta_abs,
                      const double* lower, const double* upper)
{
  NaiveReference* R = new NaiveReference();
  R->P = (ValuesProblem*)problem; R->C = C; R->scheme = scheme; R->delta_rel = delta_rel; R->delta_abs = delta_abs;
  R->K = scheme == DOGLEG_NUMERIC_STEP_CENTRAL ? 2*C + 1 : C + 1;
  const size_t N = (size_t)R->P->N, M = (size_t)R->P->M;
  R->colour = to_device(colour, N);
  R->lower = lower ? to_device(lower, N) : nullptr; R->upper = upper ? to_device(upper, N) : nullptr;
  R->pc = to_device((const double*)nullptr, (size_t)R->K*N); R->xc = to_device((const double*)nullptr, (size_t)R->K*M);
  if(!R->colour || (lower && !R->lower) || (upper && !R->upper) || !R->pc || !R->xc)
  { fprintf(stderr, "dv_naive_create: device allocation failed\n"); (void)hipGetLastError(); dv_naive_free(R); return nullptr; }
  return R;
}
// dogleg_callback_device_t
void dv_cb_naive(const double* p_dev, double* x_dev, double* J_dev, void* hip_stream, void* cookie)
{
  NaiveReference* R = (NaiveReference*)cookie;
  ValuesProblem* P = R->P;
  hipStream_t st = (hipStream_t)hip_stream;
  for(int k = 0; k < R->K; k++)
  {
    double* pk = R->pc + (size_t)k*P->N;
    hipLaunchKernelGGL(k_dv_point, dim3((P->N + 255)/256), dim3(256), 0, st, P->N, R->C, k, R->scheme, R->delta_rel, R->delta_abs,
                       R->colour, R->lower, R->upper, p_dev, pk);
    P->ncalls++; P->ncopies += 1;
    launch_values(P, pk, R->xc + (size_t)k*P->M, 1u, st);
  }
  const int work = P->nnz > P->M ? P->nnz : P->M;
  hipLaunchKernelGGL(k_dv_naive_J, dim3((work + 255)/256), dim3(256), 0, st, P->N, P->M, P->nnz, R->C, R->scheme, R->delta_rel,
                     R->delta_abs, P->Jp, P->Ji, R->colour, R->lower, R->upper, p_dev, R->xc, x_dev, J_dev);
}

} // extern "C"
