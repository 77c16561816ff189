// device_gradcheck_problems.hip -- models for the tests of the Jacobian check (dogleg_amd_check_jacobian_device*), ON THE
// GPU, with switches that make the reported Jacobian or the measurements wrong in one known place.  Test plumbing like
// device_problems.hip / device_batch_problems.hip; everything the model needs (pattern, coefficients, p*, eps) comes from
// the caller, so a test can restate the model in numpy.  Compiled with -ffp-contract=off.
//
//   sparse: the model of k_ba_eval on the caller's pattern (dogleg_callback_device_t):
//             u_r = sum_t a_t (p[i_t] - p*[i_t]),  x_r = u_r + eps sin(u_r),  J_t = a_t (1 + eps cos(u_r))
//           (a) the reported J of entry t_bad multiplied by a factor
//           (b) x[r_extra] += c (p[w] - p*[w]), w not declared in that row
//           (c) x[r_nan] = NaN
//   batch:  the model of k_batch_eval with the caller's coefficients c[b][r][j] (dogleg_callback_device_batch_t):
//           (a) the reported J[b][r][v] of one (b, r, v) multiplied by a factor
// Both count their invocations; the batch also counts the live bytes that are not 1.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cmath>

namespace {
struct SparseProblem
{
  int N, M, nnz;
  int *Jp, *Ji;
  double *a, *pstar;
  double eps;
  int ncalls;
  int t_bad; double factor;          // (a), off: t_bad < 0
  int r_extra, w; double c;          // (b), off: r_extra < 0
  int r_nan;                         // (c), off: r_nan < 0
};
struct BatchProblem
{
  int B, M, N;
  double *coef, *pstar;              // [B][M][N], [B][N]
  double eps;
  int ncalls;
  int fb, fr, fv; double factor;     // (a), off: fb < 0
  unsigned long long* d_notlive;
};

// one thread per row, u summed in index order
__global__ void __launch_bounds__(256) k_gcp_sparse(SparseProblem P, const double* __restrict__ p, double* __restrict__ x,
                                                    double* __restrict__ Jx)
{
  const int r = blockIdx.x*256 + threadIdx.x;
  if(r >= P.M) return;
  const int t0 = P.Jp[r], t1 = P.Jp[r + 1];
  double u = 0.0;
  for(int t = t0; t < t1; t++) { const int j = P.Ji[t]; u += P.a[t]*(p[j] - P.pstar[j]); }
  double xr = u + P.eps*sin(u);
  if(r == P.r_extra) xr += P.c*(p[P.w] - P.pstar[P.w]);
  if(r == P.r_nan) xr = nan("");
  x[r] = xr;
  const double d = 1.0 + P.eps*cos(u);
  for(int t = t0; t < t1; t++) Jx[t] = (t == P.t_bad ? P.factor : 1.0)*(P.a[t]*d);
}

// one thread per (problem, row)
__global__ void __launch_bounds__(256) k_gcp_batch(BatchProblem P, int B, const unsigned char* __restrict__ live,
                                                   const double* __restrict__ p, double* __restrict__ x, double* __restrict__ J)
{
  const size_t idx = (size_t)blockIdx.x*256 + threadIdx.x;
  if(idx >= (size_t)B*P.M) return;
  const int b = (int)(idx / P.M), r = (int)(idx - (size_t)b*P.M);
  if(r == 0 && live[b] != 1) atomicAdd(P.d_notlive, 1ull);
  const double* cr = P.coef + idx*P.N;
  const double* pb = p + (size_t)b*P.N; const double* ps = P.pstar + (size_t)b*P.N;
  double u = 0.0;
  for(int j = 0; j < P.N; j++) u += cr[j]*(pb[j] - ps[j]);
  x[idx] = u + P.eps*sin(u);
  const double d = 1.0 + P.eps*cos(u);
  for(int j = 0; j < P.N; j++) J[idx*P.N + j] = ((b == P.fb && r == P.fr && j == P.fv) ? P.factor : 1.0)*(cr[j]*d);
}

template <class T> T* to_device(const T* h, size_t n)
{
  T* d = nullptr;
  if(hipMalloc(&d, sizeof(T)*(n ? n : 1)) != hipSuccess) return nullptr;
  if(n && hipMemcpy(d, h, sizeof(T)*n, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
  return d;
}
} // namespace

extern "C" {

void gcp_sparse_free(void* h)
{
  SparseProblem* P = (SparseProblem*)h;
  if(!P) return;
  (void)hipFree(P->Jp); (void)hipFree(P->Ji); (void)hipFree(P->a); (void)hipFree(P->pstar);
  delete P;
}
// Jp[M + 1], Ji[nnz]: the pattern of Jt; a[nnz], pstar[N]
void* gcp_sparse_create(int N, int M, int nnz, const int* Jp, const int* Ji, const double* a, const double* pstar, double eps)
{
  SparseProblem* P = new SparseProblem();
  P->N = N; P->M = M; P->nnz = nnz; P->eps = eps; P->ncalls = 0;
  P->t_bad = -1; P->factor = 1.0; P->r_extra = -1; P->w = 0; P->c = 0.0; P->r_nan = -1;
  P->Jp = to_device(Jp, (size_t)M + 1); P->Ji = to_device(Ji, (size_t)nnz);
  P->a = to_device(a, (size_t)nnz); P->pstar = to_device(pstar, (size_t)N);
  if(!P->Jp || !P->Ji || !P->a || !P->pstar)
  { fprintf(stderr, "gcp_sparse_create: device allocation failed\n"); (void)hipGetLastError(); gcp_sparse_free(P); return nullptr; }
  return P;
}
// a switch is off with a negative index
int gcp_sparse_set_faults(void* h, int t_bad, double factor, int r_extra, int w, double c, int r_nan)
{
  SparseProblem* P = (SparseProblem*)h;
  if(t_bad >= P->nnz || r_extra >= P->M || r_nan >= P->M || (r_extra >= 0 && (w < 0 || w >= P->N))) return -1;
  P->t_bad = t_bad; P->factor = factor; P->r_extra = r_extra; P->w = r_extra >= 0 ? w : 0; P->c = c; P->r_nan = r_nan;
  return 0;
}
int gcp_sparse_ncalls(void* h) { return ((SparseProblem*)h)->ncalls; }
void gcp_sparse_reset(void* h) { ((SparseProblem*)h)->ncalls = 0; }
// dogleg_callback_device_t
void gcp_cb_sparse(const double* p_dev, double* x_dev, double* J_dev, void* hip_stream, void* cookie)
{
  SparseProblem* P = (SparseProblem*)cookie;
  P->ncalls++;
  hipLaunchKernelGGL(k_gcp_sparse, dim3((P->M + 255)/256), dim3(256), 0, (hipStream_t)hip_stream, *P, p_dev, x_dev, J_dev);
}

void gcp_batch_free(void* h)
{
  BatchProblem* P = (BatchProblem*)h;
  if(!P) return;
  (void)hipFree(P->coef); (void)hipFree(P->pstar); (void)hipFree(P->d_notlive);
  delete P;
}
// coef[B][M][N], pstar[B][N]
void* gcp_batch_create(int B, int M, int N, const double* coef, const double* pstar, double eps)
{
  BatchProblem* P = new BatchProblem();
  P->B = B; P->M = M; P->N = N; P->eps = eps; P->ncalls = 0; P->fb = -1; P->fr = 0; P->fv = 0; P->factor = 1.0;
  const unsigned long long zero = 0;
  P->coef = to_device(coef, (size_t)B*M*N); P->pstar = to_device(pstar, (size_t)B*N); P->d_notlive = to_device(&zero, 1);
  if(!P->coef || !P->pstar || !P->d_notlive)
  { fprintf(stderr, "gcp_batch_create: device allocation failed\n"); (void)hipGetLastError(); gcp_batch_free(P); return nullptr; }
  return P;
}
int gcp_batch_set_fault(void* h, int b, int r, int v, double factor)
{
  BatchProblem* P = (BatchProblem*)h;
  if(b >= P->B || (b >= 0 && (r < 0 || r >= P->M || v < 0 || v >= P->N))) return -1;
  P->fb = b; P->fr = r; P->fv = v; P->factor = factor;
  return 0;
}
int gcp_batch_ncalls(void* h) { return ((BatchProblem*)h)->ncalls; }
// live bytes that were not 1, over all invocations
long long gcp_batch_notlive(void* h)
{
  unsigned long long n = 0;
  if(hipMemcpy(&n, ((BatchProblem*)h)->d_notlive, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (long long)n;
}
// dogleg_callback_device_batch_t; B problems at most as many as were created
void gcp_cb_batch(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
                  void* hip_stream, void* cookie)
{
  BatchProblem* P = (BatchProblem*)cookie;
  P->ncalls++;
  if((int)B > P->B) { fprintf(stderr, "gcp_cb_batch: %u problems asked of a batch of %d\n", B, P->B); return; }
  const size_t rows = (size_t)B*P->M;
  hipLaunchKernelGGL(k_gcp_batch, dim3((unsigned)((rows + 255)/256)), dim3(256), 0, (hipStream_t)hip_stream, *P, (int)B, live_dev,
                     p_dev, x_dev, J_dev);
}

} // extern "C"
