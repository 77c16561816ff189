// factor_users.hip -- the entry points of include/dlg_backend.h that use the factorisation held on the device after a
// solve: solves with it, leverage blocks and outlierness factors, covariance blocks and marginal variances, query
// covariance, the selected inverse.  Host orchestration only: every entry point checks its own arguments, asks
// dlg_factor_user_begin (backend.hip) whether the backend and the slot allow the call, strings kernels of
// sparse_multi.hip / kernels_dense.hip / query_cov.hip / sparse_selinv.hip together on b->stream and downloads the result.
#include "dlg_internal.h"
#include <algorithm>
#include <chrono>

namespace {
// what the argument checks in front of dlg_factor_user_begin may not look past
bool no_handle(const dlg_backend* b, int s) { return !b || s < 0 || s > 1; }

// device scratch kept by the backend: the reference's users call these entry points in loops (dogleg.c:1831-1921) -- a
// buffer that only grows, not a synchronising hipMalloc / hipFree pair per call
int grow(dlg_backend* b, DevScratch& S, size_t doubles, double** out)
{
  if(doubles > S.cap)
  {
    if(S.p) { DLG_HIP(hipStreamSynchronize(b->stream)); (void)hipFree(S.p); S = DevScratch(); }
    if(hipMalloc(&S.p, sizeof(double)*doubles) != hipSuccess) { (void)hipGetLastError(); S.p = nullptr; dlg_set_error("out of device memory"); return DLG_ERR_NOMEM; }
    S.cap = doubles;
  }
  *out = S.p;
  return DLG_OK;
}
// N x 16 columns and N x 16 interleaved right-hand sides behind them
int cols_and_il(dlg_backend* b, double** d_cols, double** d_il)
{
  const size_t blk = (size_t)b->N*sparse_multi_rhs();
  DLG_CHECK(grow(b, b->solve_scr, 2*blk, d_cols));
  *d_il = *d_cols + blk;
  return DLG_OK;
}
// doubles of scratch for the dense forward solves of nch chunks (N x 16 each): the blocks of as many chunks at a time as
// 32 << 20 doubles (256 MB) hold, at least one
size_t dense_work_doubles(const dlg_backend* b, int nch)
{
  const size_t blk = (size_t)b->N*sparse_multi_rhs();
  return std::min(std::max<size_t>(blk, ((size_t)32 << 20) / blk * blk), blk*nch);
}
int download(dlg_backend* b, double* dst, const double* src, size_t n, const char* who)
{
  if(hipMemcpyAsync(dst, src, sizeof(double)*n, hipMemcpyDeviceToHost, b->stream) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess)
  { dlg_set_error("%s: download failed", who); return DLG_ERR_HIP; }
  return DLG_OK;
}
// How the forward solves of a chunk go: sparse, on the supernodes the chunk reaches; sparse with a supernode wider than
// the blocked kernels take, or DOGLEG_AMD_LEVERAGE_SWEEP=1 (read at every call: the tests set it on a live backend), the
// full solve of every chunk; dense, the forward half of the blocked solve.
FactorRoute factor_route(const dlg_backend* b)
{
  if(b->type != DLG_SPARSE) return ROUTE_DENSE;
  return (!sparse_multi_width_ok(b) || getenv("DOGLEG_AMD_LEVERAGE_SWEEP")) ? ROUTE_SWEEP : ROUTE_REACH;
}
// The plan kept in b->cov[which] under the key it was built for.  The key differs: the stream drained, the old plan
// released, build() run and timed (P.t_plan: host seconds of the build, left alone when the plan is reused), the key
// stored.  key: route, N, the pattern and the count, then what the caller appends (the index arrays of the call).
std::vector<int> plan_key(const dlg_backend* b, FactorRoute route, int count)
{
  const uint64_t pk = b->type == DLG_SPARSE ? sparse_pattern_key(b) : 0;
  return {route, b->N, (int)(pk & 0x7fffffff), (int)((pk >> 31) & 0x7fffffff), (int)(pk >> 62), count};
}
template <class Build> int plan_refresh(dlg_backend* b, CovPlan& P, const std::vector<int>& key, Build build)
{
  if(P.key == key) return DLG_OK;
  DLG_HIP(hipStreamSynchronize(b->stream));
  cov_plan_release(P);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = build();
  if(rc != DLG_OK) { cov_plan_release(P); return rc; }
  P.t_plan = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  P.key = key;
  return DLG_OK;
}
CovPlan& cov_plan(dlg_backend* b, int which)
{
  if(!b->cov) b->cov = new CovPlan[COV_NPLAN];
  return b->cov[which];
}
} // namespace

// ------------------------------------------------- solves with the resident factor
// (JtJ + lambda I) u = rhs for nrhs right-hand sides (host, column after column, N each) with the
// factorisation held for `slot` (dlg_factorize / dlg_gauss_newton / dlg_take_step): what the
// reference does with cholmod_solve / dpotrs on ctx->factorization after the solve (dogleg.h:304-310
// hands the factor out for exactly that; its outlier / confidence code is the in-tree user,
// dogleg.c:1831-1921).  The factor stays on the device; only the vectors travel.
extern "C" int dlg_solve_with_factor(dlg_backend_t* b, int s, const double* rhs_host, double* out_host, int nrhs)
{
  const char* who = "dlg_solve_with_factor";
  if(!rhs_host || !out_host || nrhs < 0) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_factor_user_begin(b, s, who, 0));
  const size_t N = (size_t)b->N;
  double* d_out = nullptr;
  DLG_CHECK(grow(b, b->solve_scr, N, &d_out));
  for(int k = 0; k < nrhs; k++)
  {
    if(hipMemcpyAsync(b->d_work, rhs_host + k*N, sizeof(double)*N, hipMemcpyHostToDevice, b->stream) != hipSuccess)
    { dlg_set_error("%s: upload failed", who); return DLG_ERR_HIP; }
    DLG_CHECK(b->type == DLG_SPARSE ? sparse_solve(b, b->d_work, d_out) : dense_solve(b, b->d_work, d_out));
    DLG_CHECK(download(b, out_host + k*N, d_out, N, who));
  }
  return dlg_fetch_scalars(b, dlg_backend::NSCAL);      // the hand-off status of the solves' one-launch regions
}

// ---- blocked multi-right-hand-side solves ---------------------------------------
// 16 right-hand sides per pass over the factor (sparse_multi.hip / kernels_dense.hip); a sparse
// pattern with a supernode wider than the blocked kernels take falls back to one pass per column.
static int solve_block_dev(dlg_backend* b, double* d_il)
{
  return b->type == DLG_SPARSE ? sparse_solve_multi(b, d_il) : dense_solve_multi(b, d_il);
}
static bool multi_ok(dlg_backend* b) { return b->type != DLG_SPARSE || sparse_multi_width_ok(b); }
// (a sharded backend is not refused: every rank of a row-sharded solve holds the whole factor)
extern "C" int dlg_solve_multi(dlg_backend_t* b, int s, const double* rhs_host, double* out_host, int nrhs)
{
  const char* who = "dlg_solve_multi";
  if(!rhs_host || !out_host || nrhs < 0) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_factor_user_begin(b, s, who, DLG_NEEDS_UNPARTITIONED));
  if(!multi_ok(b)) return dlg_solve_with_factor(b, s, rhs_host, out_host, nrhs);
  const int MRB = sparse_multi_rhs();
  const size_t N = (size_t)b->N;
  double *d_cols = nullptr, *d_il = nullptr;
  DLG_CHECK(cols_and_il(b, &d_cols, &d_il));
  for(int c0 = 0; c0 < nrhs; c0 += MRB)
  {
    const int nc = std::min(MRB, nrhs - c0);
    if(hipMemcpyAsync(d_cols, rhs_host + c0*N, sizeof(double)*N*nc, hipMemcpyHostToDevice, b->stream) != hipSuccess)
    { dlg_set_error("%s: upload failed", who); return DLG_ERR_HIP; }
    DLG_CHECK(multi_cols_to_interleaved(b, d_cols, nc, d_il));
    DLG_CHECK(solve_block_dev(b, d_il));
    DLG_CHECK(multi_interleaved_to_cols(b, d_il, nc, d_cols));
    DLG_CHECK(download(b, out_host + c0*N, d_cols, N*nc, who));
  }
  return DLG_OK;
}
// solve the 16 interleaved right-hand sides in d_il in place (original order); d_cols: N x 16 scratch for the
// one-column-at-a-time route of a pattern too wide for the blocked kernels
static int solve_il(dlg_backend* b, double* d_il, double* d_cols, int ncols)
{
  if(multi_ok(b)) return solve_block_dev(b, d_il);
  const size_t N = (size_t)b->N;
  DLG_CHECK(multi_interleaved_to_cols(b, d_il, ncols, d_cols));
  for(int c = 0; c < ncols; c++) DLG_CHECK(sparse_solve(b, d_cols + c*N, d_cols + c*N));
  return multi_cols_to_interleaved(b, d_cols, ncols, d_il);
}
// out (N x (row1 - row0), column-major, host) = inv(JtJ + lambda I) * Jt[:, row0:row1]: the building block
// of the reference's pseudoinverse_J_dense / pseudoinverse_J_sparse (dogleg.c:1831-1921); Jt is taken
// from the slot's Jacobian on the device, nothing but the result crosses PCIe
extern "C" int dlg_pseudoinverse_chunk(dlg_backend_t* b, int s, int row0, int row1, double* out_host)
{
  const char* who = "dlg_pseudoinverse_chunk";
  if(no_handle(b, s) || !out_host || row0 < 0 || row1 < row0 || row1 > b->M) { dlg_set_error("%s: bad row range", who); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_factor_user_begin(b, s, who, DLG_NEEDS_J | DLG_NEEDS_UNSHARDED | DLG_NEEDS_UNPARTITIONED));
  const int MRB = sparse_multi_rhs();
  const size_t N = (size_t)b->N;
  double *d_cols = nullptr, *d_il = nullptr;
  DLG_CHECK(cols_and_il(b, &d_cols, &d_il));
  const bool blocked = multi_ok(b);
  for(int r = row0; r < row1; r += MRB)
  {
    const int nc = std::min(MRB, row1 - r);
    DLG_CHECK(b->type == DLG_SPARSE ? sparse_jt_chunk_interleaved(b, s, r, nc, d_il) : dense_jt_chunk_interleaved(b, s, r, nc, d_il));
    if(blocked) DLG_CHECK(solve_block_dev(b, d_il));
    DLG_CHECK(multi_interleaved_to_cols(b, d_il, nc, d_cols));
    if(!blocked)
      for(int c = 0; c < nc; c++)          // (a supernode too wide for the blocked kernels: column by column)
        DLG_CHECK(sparse_solve(b, d_cols + c*N, d_cols + c*N));
    DLG_CHECK(download(b, out_host + (size_t)(r - row0)*N, d_cols, N*nc, who));
  }
  return DLG_OK;
}

// ---- leverage blocks and outlierness factors (the reference's outlier API, dogleg.c:2294-2660) ---------------------------
// A_f = J_f (JtJ + lambda I)^-1 J_f^T of features of fs consecutive measurement rows, from the factor held for the slot and
// the slot's Jacobian on the device.  Only the forward solve is needed, A_f = V_f^T V_f with V_f = L^-1 P J_f^T: sparse, the
// forward solves of 16 rows at a time visit only the supernodes their columns reach (sparse_multi.hip), many chunks per
// launch; dense, the forward half of the blocked solve on many chunks per launch sequence.  The Gram products are summed
// on the device in a fixed order (two calls give the same bits); only nf values or blocks travel to the host.
// A sparse pattern with a supernode wider than the blocked kernels take (or DOGLEG_AMD_LEVERAGE_SWEEP=1): the full solve
// of every chunk (dlg_pseudoinverse_chunk's route) and its product with the chunk's rows of J.
static int lev_begin(dlg_backend* b, int s, int fs, const char* who)
{
  if(fs < 1 || fs > 2) { dlg_set_error("%s: feature size %d is not implemented (1 and 2 are)", who, fs); return DLG_ERR_ARG; }
  return dlg_factor_user_begin(b, s, who, DLG_NEEDS_J | DLG_NEEDS_UNSHARDED | DLG_NEEDS_UNPARTITIONED | DLG_NEEDS_PATTERN);
}
// the Gram products of every chunk through the full solve of the chunk (one slot per chunk)
static int lev_sweep(dlg_backend* b, int s, int fs, int nf, double* d_gram)
{
  const int MRB = sparse_multi_rhs(), nrow = nf*fs;
  double *d_cols = nullptr, *d_il = nullptr;
  DLG_CHECK(cols_and_il(b, &d_cols, &d_il));
  for(int ch = 0; ch*MRB < nrow; ch++)
  {
    const int nc = std::min(MRB, nrow - ch*MRB);
    DLG_CHECK(sparse_jt_chunk_interleaved(b, s, ch*MRB, nc, d_il));
    DLG_CHECK(solve_il(b, d_il, d_cols, nc));
    DLG_CHECK(lev_gram_rows(b, s, ch*MRB, nc, fs, d_il, d_gram + (size_t)ch*LEV_NP));
  }
  return DLG_OK;
}
static int lev_run(dlg_backend* b, int s, int fs, int nf, int mode, double scale, double* out_host, const char* who)
{
  DLG_CHECK(lev_begin(b, s, fs, who));
  if(nf < 0 || (long)nf*fs > b->M) { dlg_set_error("%s: %d features of %d rows do not fit %d measurements", who, nf, fs, b->M); return DLG_ERR_ARG; }
  if(nf == 0) return DLG_OK;
  if(!out_host) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  const int MRB = sparse_multi_rhs(), nch = dlg_cdiv((long)nf*fs, MRB), nt = mode == 0 ? lev_nt(fs) : 1;
  const size_t nout = (size_t)nf*nt, ngram = (size_t)nch*LEV_NP;
  double* d_buf = nullptr;
  double* d_gram = nullptr; const int* d_slot_ptr = nullptr;
  switch(factor_route(b))
  {
  case ROUTE_REACH:
    DLG_CHECK(grow(b, b->lev_scr, nout, &d_buf));
    DLG_CHECK(sparse_leverage_reach(b, s, fs, nf, &d_gram, &d_slot_ptr, nullptr));
    break;
  case ROUTE_SWEEP:
    DLG_CHECK(grow(b, b->lev_scr, nout + ngram, &d_buf));
    d_gram = d_buf + nout;
    DLG_CHECK(lev_sweep(b, s, fs, nf, d_gram));
    break;
  case ROUTE_DENSE:
    DLG_CHECK(grow(b, b->lev_scr, nout + ngram + dense_work_doubles(b, nch), &d_buf));
    d_gram = d_buf + nout;
    DLG_CHECK(dense_leverage_gram(b, s, fs, nf, d_gram + ngram, dense_work_doubles(b, nch), d_gram));
    break;
  }
  DLG_CHECK(lev_finish(b, s, nf, fs, d_slot_ptr, d_gram, scale, mode, d_buf));
  return download(b, out_host, d_buf, nout, who);
}
extern "C" int dlg_feature_leverage(dlg_backend_t* b, int s, int fs, int f0, int nf, double* A_host)
{
  if(f0 < 0 || nf < 0) { dlg_set_error("dlg_feature_leverage: bad feature range"); return DLG_ERR_ARG; }
  const int nt = (fs == 2) ? 3 : 1;
  std::vector<double> all((size_t)(f0 + nf)*nt);
  DLG_CHECK(lev_run(b, s, fs, f0 + nf, 0, 0.0, all.data(), "dlg_feature_leverage"));
  if(nf > 0) memcpy(A_host, all.data() + (size_t)f0*nt, sizeof(double)*(size_t)nf*nt);
  return DLG_OK;
}
extern "C" int dlg_outlierness_factors(dlg_backend_t* b, int s, int fs, int nf, double scale, double* factors_host)
{
  return lev_run(b, s, fs, nf, 1, scale, factors_host, "dlg_outlierness_factors");
}
extern "C" int dlg_leverage_stats(dlg_backend_t* b, int fs, long* nchunks, long* visits, int* nsn)
{
  if(!b || b->type != DLG_SPARSE || !nchunks || !visits || !nsn) { dlg_set_error("dlg_leverage_stats: bad argument"); return DLG_ERR_ARG; }
  return sparse_leverage_stats(b, fs, nchunks, visits, nsn);
}

// ---- covariance blocks Sigma = (JtJ + lambda I)^-1 with the factor held for the slot ----------------------------------
// Sigma[u, v] = (L^-1 P e_u)^T (L^-1 P e_v): only the forward solve of unit columns is needed.  Requests are packed into
// chunks of 16 distinct variables (sparse_multi.hip: cov_pack_requests); sparse, each chunk's forward solve visits only the
// supernodes on the paths from its columns to the root, many chunks per launch, and every (chunk, supernode) pair leaves
// the Gram products its chunk needs; dense, the forward half of the blocked solve from the tile of the chunks' smallest
// variable on.  k_cov_finish sums each value's slots in a fixed order and writes the blocks straight into one device
// buffer: only the requested values cross PCIe.  The plan of the last request list (and the marginal-variance plan) is kept.
// A sparse pattern with a supernode wider than the blocked kernels take, or DOGLEG_AMD_LEVERAGE_SWEEP=1: the full solve of
// every chunk's unit columns (solve_il) and its requested rows.
constexpr unsigned COV_NEEDS = DLG_NEEDS_UNSHARDED | DLG_NEEDS_UNPARTITIONED | DLG_NEEDS_PATTERN;
// the forward half of the blocked solve on all chunks of a dense plan, and their products
static int cov_dense(dlg_backend* b, const CovPlan& P)
{
  const size_t work = dense_work_doubles(b, P.K.nch);
  double* d_work = nullptr;
  DLG_CHECK(grow(b, b->lev_scr, work, &d_work));
  return dense_cov_gram(b, P, d_work, work);
}
// which 0: the requests; 1: the marginal variances
static int cov_run(dlg_backend* b, int s, int which, int nreq, const int* r0, const int* nr, const int* c0, const int* nc,
                   double* out_host, const char* who)
{
  if(no_handle(b, s) || nreq < 0) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  if(which == 0 && nreq == 0) return DLG_OK;
  if(!out_host || (which == 0 && (!r0 || !nr || !c0 || !nc))) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_factor_user_begin(b, s, who, COV_NEEDS));
  const FactorRoute route = factor_route(b);
  CovPlan& P = cov_plan(b, which);
  std::vector<int> key = plan_key(b, route, nreq);
  if(which == 0)
    for(const int* a : {r0, nr, c0, nc}) key.insert(key.end(), a, a + nreq);
  DLG_CHECK(plan_refresh(b, P, key, [&] { return cov_plan_build(b, P, route, which, nreq, r0, nr, c0, nc, who); }));
  if(route == ROUTE_REACH) DLG_CHECK(sparse_cov_reach_run(b, P));
  else if(route == ROUTE_DENSE) DLG_CHECK(cov_dense(b, P));
  else
  {
    const int MRB = sparse_multi_rhs();
    double *d_cols = nullptr, *d_il = nullptr;
    DLG_CHECK(cols_and_il(b, &d_cols, &d_il));
    for(int ch = 0; ch < P.K.nch; ch++)
    {
      int ncol = 0;
      while(ncol < MRB && P.K.var[(size_t)ch*MRB + ncol] >= 0) ncol++;
      DLG_CHECK(cov_unit_il(b, P, ch, d_il));
      DLG_CHECK(solve_il(b, d_il, d_cols, ncol));
      DLG_CHECK(cov_pick(b, P, ch, d_il));
    }
  }
  DLG_CHECK(cov_finish(b, P));
  b->cov_last = which;
  return P.ne > 0 ? download(b, out_host, P.out, (size_t)P.ne, who) : DLG_OK;
}
extern "C" int dlg_covariance_blocks(dlg_backend_t* b, int s, int nreq, const int* r0, const int* nr, const int* c0,
                                     const int* nc, double* out_host)
{
  return cov_run(b, s, 0, nreq, r0, nr, c0, nc, out_host, "dlg_covariance_blocks");
}
extern "C" int dlg_marginal_variances(dlg_backend_t* b, int s, double* var_host)
{
  return cov_run(b, s, 1, 0, nullptr, nullptr, nullptr, nullptr, var_host, "dlg_marginal_variances");
}
extern "C" int dlg_covariance_stats(dlg_backend_t* b, long* nchunks, long* visits, int* nsn)
{
  if(!b || !nchunks || !visits || !nsn) { dlg_set_error("dlg_covariance_stats: bad argument"); return DLG_ERR_ARG; }
  if(!b->cov || b->cov_last < 0) { dlg_set_error("no covariance plan has been run"); return DLG_ERR_STATE; }
  return cov_plan_stats(b, b->cov[b->cov_last], nchunks, visits, nsn);
}
// (a plan that is reused leaves the time of its build in place)
extern "C" double dlg_covariance_plan_seconds(dlg_backend_t* b)
{
  return (b && b->cov && b->cov_last >= 0) ? b->cov[b->cov_last].t_plan : -1.0;
}

// ---- query covariance Jq Sigma Jq^T (plain form) and Jq Sigma J_obs^T J_obs Sigma Jq^T (observation form) ----------------
// Var(q) = V^T V with V = L^-1 P Jq^T: the plain form needs only the forward solve of Jq's rows.  Queries (1 to 16 rows of a
// CSR) are packed whole into chunks of 16 rows (sparse_multi.hip: query_pack); sparse, each chunk's forward solve visits
// only the supernodes its rows' variables reach (k_cov_fwd_level with the rows as right-hand sides), and every (chunk,
// supernode) pair leaves the products of the chunk's queries; dense, the forward half of the blocked solve.  A sparse
// pattern with a supernode wider than the blocked kernels take, or DOGLEG_AMD_LEVERAGE_SWEEP=1: the full solve of each
// chunk (solve_il) and the products of its rows with the solved columns.  The observation form: U = Sigma Jq^T by full
// solves, then the products of (J[0:nobs] U)^T (J[0:nobs] U), QOBS_NC chunks per pass over J (query_cov.hip).  The plan is
// kept under the pattern and the index arrays; the values are uploaded at every call.  which: b->cov[2] (the public call)
// or b->cov[3] (dlg_leverage_query).  The caller has checked the arguments and called dlg_factor_user_begin.
static int qcov_run(dlg_backend* b, int s, int which, int nq, const int* qrow, const int* rowptr, const int* var,
                    const double* val, int nobs, double* out_host, const char* who)
{
  // (the key needs well-formed rows: what is not, query_pack refuses with its message)
  bool wellformed = qrow[0] >= 0;
  for(int k = 0; k < nq && wellformed; k++) wellformed = qrow[k+1] - qrow[k] >= 1 && qrow[k+1] - qrow[k] <= QCOV_MAXROWS;
  if(wellformed) wellformed = rowptr[qrow[nq]] >= rowptr[qrow[0]];
  if(!wellformed) { CovPack K; const int rc = query_pack(b->N, nq, qrow, rowptr, var, K, who); if(rc != DLG_OK) return rc; }
  const FactorRoute route = nobs >= 0 ? ROUTE_SWEEP : factor_route(b);
  CovPlan& P = cov_plan(b, which);
  const int e0 = rowptr[qrow[0]], e1 = rowptr[qrow[nq]];
  std::vector<int> key = plan_key(b, route, nq);
  key.insert(key.end(), qrow, qrow + nq + 1);
  key.insert(key.end(), rowptr + qrow[0], rowptr + qrow[nq] + 1);
  key.insert(key.end(), var + e0, var + e1);
  P.t_plan = 0.0;                            // (dlg_query_covariance_plan_seconds: 0 when the plan is reused)
  DLG_CHECK(plan_refresh(b, P, key, [&] { return query_plan_build(b, P, route, nq, qrow, rowptr, var, who); }));
  if(P.qnnz > 0) DLG_HIP(hipMemcpyAsync(P.qval, val + e0, sizeof(double)*(size_t)P.qnnz, hipMemcpyHostToDevice, b->stream));
  const int MRB = sparse_multi_rhs(), nch = P.K.nch;
  const size_t N = (size_t)b->N;
  if(route == ROUTE_REACH) DLG_CHECK(sparse_query_reach_run(b, P));
  else if(route == ROUTE_DENSE) DLG_CHECK(cov_dense(b, P));
  else if(nobs < 0)
  {
    double *d_cols = nullptr, *d_il = nullptr;
    DLG_CHECK(cols_and_il(b, &d_cols, &d_il));
    for(int ch = 0; ch < nch; ch++)
    {
      DLG_CHECK(query_rhs_il(b, P, ch, 1, d_il));
      DLG_CHECK(solve_il(b, d_il, d_cols, P.K.crow[ch+1] - P.K.crow[ch]));
      DLG_CHECK(query_gram_rows(b, P, ch, d_il));
    }
  }
  else
  {
    double *d_cols = nullptr, *d_U = nullptr;
    DLG_CHECK(grow(b, b->solve_scr, N*MRB, &d_cols));
    DLG_CHECK(grow(b, b->lev_scr, N*MRB*QOBS_NC + (size_t)QOBS_WG*QOBS_NC*MRB*MRB, &d_U));
    double* d_part = d_U + N*MRB*QOBS_NC;
    for(int ch0 = 0; ch0 < nch; ch0 += QOBS_NC)
    {
      const int nc = std::min(QOBS_NC, nch - ch0);
      DLG_CHECK(query_rhs_il(b, P, ch0, nc, d_U));
      for(int q = 0; q < nc; q++) DLG_CHECK(solve_il(b, d_U + (size_t)q*N*MRB, d_cols, P.K.crow[ch0+q+1] - P.K.crow[ch0+q]));
      DLG_CHECK(query_obs_gram(b, s, P, ch0, nc, nobs, d_U, d_part));
    }
  }
  DLG_CHECK(cov_finish(b, P));
  return P.ne > 0 ? download(b, out_host, P.out, (size_t)P.ne, who) : DLG_OK;
}
extern "C" int dlg_query_covariance(dlg_backend_t* b, int s, int nq, const int* qrow, const int* rowptr, const int* var,
                                    const double* val, int nobs, double* out_host)
{
  const char* who = "dlg_query_covariance";
  if(no_handle(b, s) || nq < 0) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  if(nq == 0) return DLG_OK;
  if(!qrow || !rowptr || !var || !val || !out_host) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  if(nobs > b->M) { dlg_set_error("%s: nobs = %d exceeds the %d measurements", who, nobs, b->M); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_factor_user_begin(b, s, who, COV_NEEDS | (nobs >= 0 ? DLG_NEEDS_J : 0)));      // (the observation form reads J)
  return qcov_run(b, s, 2, nq, qrow, rowptr, var, val, nobs, out_host, who);
}
extern "C" int dlg_query_covariance_stats(dlg_backend_t* b, long* nchunks, long* visits, int* nsn)
{
  if(!b || !nchunks || !visits || !nsn) { dlg_set_error("dlg_query_covariance_stats: bad argument"); return DLG_ERR_ARG; }
  if(!b->cov || b->cov[2].key.empty()) { dlg_set_error("no query covariance plan has been run"); return DLG_ERR_STATE; }
  return cov_plan_stats(b, b->cov[2], nchunks, visits, nsn);
}
extern "C" double dlg_query_covariance_plan_seconds(dlg_backend_t* b)
{
  return (b && b->cov && !b->cov[2].key.empty()) ? b->cov[2].t_plan : -1.0;
}
// A = Jq (JtJ + lambda I)^-1 Jq^T for a query feature: Jq fs x nstate (row-major) on the states istate .. istate + nstate - 1,
// one query of fs rows (qcov_run on its own plan)
extern "C" int dlg_leverage_query(dlg_backend_t* b, int s, const double* Jq, int istate, int nstate, int fs, double* A_host)
{
  const char* who = "dlg_leverage_query";
  DLG_CHECK(lev_begin(b, s, fs, who));
  if(!Jq || !A_host || istate < 0 || nstate < 1 || istate > b->N - nstate) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  const int qrow[2] = {0, fs};
  std::vector<int> rowptr(fs + 1), var((size_t)fs*nstate);
  for(int c = 0; c <= fs; c++) rowptr[c] = c*nstate;
  for(int c = 0; c < fs; c++) for(int j = 0; j < nstate; j++) var[(size_t)c*nstate + j] = istate + j;
  double blk[4];
  DLG_CHECK(qcov_run(b, s, 3, 1, qrow, rowptr.data(), var.data(), Jq, -1, blk, who));
  // upper triangle, row after row
  int o = 0;
  for(int i = 0; i < fs; i++) for(int k = i; k < fs; k++) A_host[o++] = blk[i*fs + k];
  return DLG_OK;
}

// ---- the selected inverse: Sigma at entries of the structure of the factor (sparse_selinv.hip).  The refusals are those
// of dlg_covariance_blocks, and an entry off the structure.
extern "C" int dlg_covariance_entries(dlg_backend_t* b, int s, long n, const int* row, const int* col, double* out_host)
{
  const char* who = "dlg_covariance_entries";
  if(no_handle(b, s) || n < 0) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  if(n == 0) return DLG_OK;
  if(!row || !col || !out_host) { dlg_set_error("%s: bad argument", who); return DLG_ERR_ARG; }
  DLG_CHECK(dlg_factor_user_begin(b, s, who, COV_NEEDS));
  return selinv_entries(b, n, row, col, out_host, who);
}
