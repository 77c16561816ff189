// sparse_selinv.hip -- the selected inverse: Sigma = (JtJ + lambda I)^-1 on the structure of the factor held on the
// device, in one sweep from the root of the supernodal tree down (the Takahashi equations), and the entry lookup of
// dlg_covariance_entries.
//
// For a supernode with own columns J and below rows B (sn_rows after the first w; the augmented row takes no part):
//   Y      = L_BJ L_JJ^-1
//   S_BJ   = -S_BB Y
//   S_JJ   = L_JJ^-T L_JJ^-1 - Y^T S_BJ
// B is a clique of the filled graph and lies in the rows of the parent (relpos[sn_prel[s]] maps it there), so S_BB is
// a part of the parent's FRONT: Sigma on rows(parent) x rows(parent), which a supernode with children writes (full square,
// column-major) into a scratch of its depth.  The sweep runs by depth from the root (a child is exactly one depth below
// its parent), so the fronts of two depths are alive at a time: a buffer per parity.
//
// Kernels (fp64, v_mfma_f64_16x16x4_f64 for the products):
//   k_selinv_prep    one launch for all supernodes, a workgroup per 16 columns of one: L_JJ^-1 [:, chunk] by a column
//                    sweep (the top block staged in LDS up to 128 columns, read from HBM above that), then
//                    Y [:, chunk] = L_BJ L_JJ^-1 [:, chunk] on the matrix cores.  Both go to Yb, laid out as Lx
//                    (top block: L_JJ^-1, below: Y).
//   k_selinv_level   two launches per depth, a wave per 16 x 16 output tile, many waves per supernode: phase 0 forms
//                    S_BJ with S_BB streamed from the parent's front through the relpos map; phase 1 forms S_JJ as one
//                    product over the rows of the panel, [L_JJ^-1; Y]^T [L_JJ^-1; -S_BJ].  Each output has one owner
//                    and every sum runs in a fixed order: the results are bitwise reproducible.
// Sibling-merged leaves (block-diagonal top) are swept as the one panel they are: L_JJ is block diagonal, so the
// members' values are theirs; Sigma between two members is formed as well but is not in the structure (the lookup
// refuses it).
#include "sparse_internal.h"
#include <algorithm>
#include <chrono>
#include <cstdint>

namespace {
constexpr int SMR = 16;                // columns per chunk of the prep kernel
constexpr int SEL_WLDS = 128;          // widest top block the prep kernel stages in LDS (packed lower triangle)
typedef double sel_v4d __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int sel_tri(int i, int j) { return i*(i + 1)/2 + j; }

size_t sel_prep_lds(int w)
{
  const size_t lt = w <= SEL_WLDS ? (size_t)((w*(w + 1)/2 + 1) & ~1) : 0;
  return sizeof(double)*(lt + (size_t)((w + 1) & ~1) + 2*(size_t)w*SMR);
}

// one (supernode, 16-column chunk) per workgroup: L_JJ^-1 e_c for the chunk's columns c, then Y = L_BJ (that)
__global__ void __launch_bounds__(TPB) k_selinv_prep(const SelTask* __restrict__ task, const int* __restrict__ sn_c0,
                                                     const int* __restrict__ sn_rowptr, const int64_t* __restrict__ sn_lx,
                                                     const double* __restrict__ Lx, double* __restrict__ Yb)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const SelTask T = task[blockIdx.x];
  const int s = T.s, cb = T.ti;
  const int w = sn_c0[s+1] - sn_c0[s], nrows = sn_rowptr[s+1] - sn_rowptr[s], r = nrows - w - 1;
  const double* L = Lx + sn_lx[s];
  double* V = Yb + sn_lx[s];
  const bool staged = w <= SEL_WLDS;
  const int tid = threadIdx.x, c = tid & (SMR - 1), g = tid >> 4;
  double* Lt = lds;
  double* dinv = Lt + (staged ? ((w*(w + 1)/2 + 1) & ~1) : 0);
  double* Ys = dinv + ((w + 1) & ~1);              // [w][16] running right-hand sides
  double* Yd = Ys + w*SMR;                         // [w][16] the solution
  if(staged)
    for(int e = tid; e < w*w; e += TPB)
    {
      const int j = e / w, i = e - j*w;
      if(i >= j) { const double v = L[i + (size_t)j*nrows]; Lt[sel_tri(i, j)] = v; if(i == j) dinv[j] = 1.0/v; }
    }
  else
    for(int j = tid; j < w; j += TPB) dinv[j] = 1.0/L[j + (size_t)j*nrows];
  for(int e = tid; e < w*SMR; e += TPB) { const int k = e / SMR; Ys[e] = (k == cb + (e & (SMR - 1))) ? 1.0 : 0.0; Yd[e] = 0.0; }
  __syncthreads();
  for(int j = cb; j < w; j++)
  {
    const double yj = Ys[j*SMR + c]*dinv[j];
    if(g == (j & 15)) Yd[j*SMR + c] = yj;
    if(staged) for(int i = j + 1 + g; i < w; i += TPB/SMR) Ys[i*SMR + c] -= Lt[sel_tri(i, j)]*yj;
    else       for(int i = j + 1 + g; i < w; i += TPB/SMR) Ys[i*SMR + c] -= L[i + (size_t)j*nrows]*yj;
    __syncthreads();
  }
  const int ncol = min(SMR, w - cb);
  for(int e = tid; e < w*ncol; e += TPB) { const int cc = e / w, k = e - cc*w; V[k + (size_t)(cb + cc)*nrows] = Yd[k*SMR + cc]; }
  // Y[:, chunk] = L_BJ Yd on the matrix cores, a wave per 16 rows (Yd is zero above row cb)
  const int lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  for(int t = wv; 16*t < r; t += TPB/64)
  {
    const int row = 16*t + mm;
    const double* Lr = L + w + min(row, r - 1);
    sel_v4d acc = {0.0, 0.0, 0.0, 0.0};
    for(int k4 = cb & ~7; k4 < w; k4 += 8)
    {
      const int ka = k4 + kq, kb = k4 + 4 + kq;
      const double a0 = (ka < w && row < r) ? Lr[(size_t)ka*nrows] : 0.0;
      const double a1 = (kb < w && row < r) ? Lr[(size_t)kb*nrows] : 0.0;
      const double b0 = (ka < w) ? Yd[ka*SMR + mm] : 0.0;
      const double b1 = (kb < w) ? Yd[kb*SMR + mm] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
    }
#pragma unroll
    for(int q = 0; q < 4; q++) { const int i = 16*t + kq + 4*q; if(i < r && mm < ncol) V[w + i + (size_t)(cb + mm)*nrows] = acc[q]; }
  }
}

// one depth of the sweep, a wave per tile task (4 a workgroup, no barriers).  phase 0: rows 16 ti.. of S_BJ, columns
// 16 tj.. ; phase 1: the tile (ti, tj), ti >= tj, of S_JJ.  Fp: the fronts of the depth above, Fs: this depth's.
// MFMA operand map (f64 16x16x4): lane (mm, kq) gives A[mm][kq] and B[kq][mm]; D[kq + 4q][mm] is register q.
__global__ void __launch_bounds__(TPB) k_selinv_level(const SelTask* __restrict__ task, int ntask, int phase,
                                                      const int* __restrict__ sn_c0, const int* __restrict__ sn_rowptr,
                                                      const int64_t* __restrict__ sn_lx, const int* __restrict__ relpos,
                                                      const int* __restrict__ par, const int* __restrict__ prel,
                                                      const int64_t* __restrict__ foff, const double* __restrict__ Fp,
                                                      double* __restrict__ Fs, const double* __restrict__ Yb,
                                                      double* __restrict__ Sx)
{
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, mm = lane & 15, kq = lane >> 4;
  const int q = blockIdx.x*(TPB/64) + wv;
  if(q >= ntask) return;
  const SelTask T = task[q];
  const int s = T.s;
  const int w = sn_c0[s+1] - sn_c0[s], nrows = sn_rowptr[s+1] - sn_rowptr[s], r = nrows - w - 1, ns = w + r;
  const double* V = Yb + sn_lx[s];
  double* S = Sx + sn_lx[s];
  const int64_t fo = foff[s];
  double* F = fo >= 0 ? Fs + fo : nullptr;
  sel_v4d acc = {0.0, 0.0, 0.0, 0.0};
  if(phase == 0)
  {
    const int p = par[s], np = sn_rowptr[p+1] - sn_rowptr[p] - 1;
    const int* pr = relpos + prel[s];
    const double* Fq = Fp + foff[p];
    const int i0 = 16*T.ti, j0 = 16*T.tj;
    const bool arow_ok = i0 + mm < r;
    const int64_t arow = pr[min(i0 + mm, r - 1)];
    const double* Vb = V + w + (size_t)min(j0 + mm, w - 1)*nrows;
    for(int k4 = 0; k4 < r; k4 += 8)
    {
      const int ka = k4 + kq, kb = k4 + 4 + kq;
      const int pa = pr[min(ka, r - 1)], pb = pr[min(kb, r - 1)];
      const double a0 = (ka < r && arow_ok) ? Fq[arow + (int64_t)pa*np] : 0.0;
      const double a1 = (kb < r && arow_ok) ? Fq[arow + (int64_t)pb*np] : 0.0;
      const double b0 = (ka < r) ? Vb[ka] : 0.0;
      const double b1 = (kb < r) ? Vb[kb] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc, 0, 0, 0);
    }
    const int j = j0 + mm;
#pragma unroll
    for(int u = 0; u < 4; u++)
    {
      const int i = i0 + kq + 4*u;
      if(i < r && j < w)
      {
        const double v = -acc[u];
        S[w + i + (size_t)j*nrows] = v;
        if(F) { F[(w + i) + (int64_t)j*ns] = v; F[j + (int64_t)(w + i)*ns] = v; }
      }
    }
    // the front's B x B block: the tasks of the first column tile copy their rows of S_BB
    if(F && T.tj == 0)
      for(int e = lane; e < 16*r; e += 64)
      {
        const int i = i0 + (e & 15), k = e >> 4;
        if(i < r) F[(w + i) + (int64_t)(w + k)*ns] = Fq[(int64_t)pr[i] + (int64_t)pr[k]*np];
      }
    return;
  }
  // S_JJ[a][b] = sum over the panel's rows k of V[k][a] * (k < w ? V[k][b] : -S[k][b]); L_JJ^-1 [k][a] is zero for k < a,
  // and a >= 16 ti
  const int a0 = 16*T.ti, b0 = 16*T.tj;
  const double* Va = V + (size_t)min(a0 + mm, w - 1)*nrows;
  const double* Vb = V + (size_t)min(b0 + mm, w - 1)*nrows;
  const double* Sb = S + (size_t)min(b0 + mm, w - 1)*nrows;
  for(int k4 = a0; k4 < ns; k4 += 8)
  {
    const int ka = k4 + kq, kb = k4 + 4 + kq;
    const double x0 = (ka < ns) ? Va[ka] : 0.0;
    const double x1 = (kb < ns) ? Va[kb] : 0.0;
    const double y0 = (ka < w) ? Vb[ka] : (ka < ns ? -Sb[ka] : 0.0);
    const double y1 = (kb < w) ? Vb[kb] : (kb < ns ? -Sb[kb] : 0.0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, acc, 0, 0, 0);
  }
  const int b = b0 + mm;
#pragma unroll
  for(int u = 0; u < 4; u++)
  {
    const int a = a0 + kq + 4*u;
    if(a < w && b < w && a >= b)
    {
      const double v = acc[u];
      S[a + (size_t)b*nrows] = v; S[b + (size_t)a*nrows] = v;
      if(F) { F[a + (int64_t)b*ns] = v; F[b + (int64_t)a*ns] = v; }
    }
  }
}

__global__ void __launch_bounds__(TPB) k_selinv_pick(long n, const int64_t* __restrict__ pos, const double* __restrict__ src,
                                                     double* __restrict__ out)
{
  const long e = (long)blockIdx.x*TPB + threadIdx.x;
  if(e < n) out[e] = src[pos[e]];
}

// position in the panels of Sigma[u][v] (variables in the caller's numbering), -1: not in the structure of the factor
int64_t sel_pos(const SymHost& H, int u, int v)
{
  const int pu = H.iperm[u], pv = H.iperm[v], c = std::min(pu, pv), rr = std::max(pu, pv);
  const int s = H.col_sn[c], c0 = H.sn_c0[s], w = H.sn_c0[s+1] - c0, nrows = H.sn_rowptr[s+1] - H.sn_rowptr[s];
  const int jc = c - c0;
  int ir;
  if(rr < c0 + w)
  {
    ir = rr - c0;
    const int b0 = H.sn_bd_ptr[s], b1 = H.sn_bd_ptr[s+1];
    if(b1 > b0)
    {
      // a block-diagonal top: the two columns must belong to the same member
      const int* m0 = H.sn_bd_col.data() + b0;
      const int* m1 = H.sn_bd_col.data() + b1;
      if(std::upper_bound(m0, m1, ir) != std::upper_bound(m0, m1, jc)) return -1;
    }
  }
  else
  {
    const int* rows = H.sn_rows.data() + H.sn_rowptr[s];
    const int* it = std::lower_bound(rows + w, rows + nrows - 1, rr);
    if(it == rows + nrows - 1 || *it != rr) return -1;
    ir = (int)(it - rows);
  }
  return H.sn_lx[s] + ir + (int64_t)jc*nrows;
}

int sel_lookup(const dlg_backend* b, long n, const int* row, const int* col, std::vector<int64_t>& pos, const char* who)
{
  const int N = b->N;
  const SymHost* H = b->type == DLG_SPARSE ? &b->sym->H : nullptr;
  pos.resize(n);
  for(long e = 0; e < n; e++)
  {
    const int u = row[e], v = col[e];
    if(u < 0 || v < 0 || u >= N || v >= N)
    { dlg_set_error("%s: entry %ld (%d, %d) is outside the %d variables", who, e, u, v, N); return DLG_ERR_ARG; }
    if(!H) { pos[e] = (int64_t)std::max(u, v) + (int64_t)std::min(u, v)*N; continue; }
    pos[e] = sel_pos(*H, u, v);
    if(pos[e] < 0)
    {
      dlg_set_error("%s: entry %ld (%d, %d) is not in the structure of the factor; take blocks off it from dlg_covariance_blocks",
                    who, e, u, v);
      return DLG_ERR_ARG;
    }
  }
  return DLG_OK;
}

// the sweep's plan, from the symbolic phase: depths, fronts, tile tasks
int sel_plan(dlg_backend* b, SelInv& X)
{
  SparseSym* Y = b->sym;
  const SymHost& H = Y->H;
  const int nsn = H.nsn;
  std::vector<int> parent(nsn, -1), dep(nsn, 0), nchild(nsn, 0), prel(nsn, -1);
  for(int s = nsn - 1; s >= 0; s--)
  {
    const int w = H.sn_c0[s+1] - H.sn_c0[s], r = H.sn_rowptr[s+1] - H.sn_rowptr[s] - w - 1;
    if(r <= 0) continue;
    const int p = H.col_sn[H.sn_rows[H.sn_rowptr[s] + w]];
    if(p <= s || H.sn_prel[s] < 0) { dlg_set_error("selected inverse: supernode %d has no map into its parent", s); return DLG_ERR_STATE; }
    parent[s] = p; dep[s] = dep[p] + 1; nchild[p]++; prel[s] = H.sn_prel[s];
  }
  int nd = 0;
  for(int s = 0; s < nsn; s++) nd = std::max(nd, dep[s] + 1);
  std::vector<std::vector<int>> by(nd);
  for(int s = 0; s < nsn; s++) by[dep[s]].push_back(s);
  std::vector<int64_t> foff(nsn, -1);
  std::vector<SelTask> prep, task;
  X.tb_ptr.assign(1, 0); X.tc_ptr.assign(1, 0);
  X.fsize[0] = X.fsize[1] = 0;
  int wmax = 1;
  for(int d = 0; d < nd; d++)
  {
    int64_t at = 0;
    for(int s : by[d])
      if(nchild[s] > 0) { const int64_t ns = H.sn_rowptr[s+1] - H.sn_rowptr[s] - 1; foff[s] = at; at += ns*ns; }
    X.fsize[d & 1] = std::max(X.fsize[d & 1], at);
    for(int s : by[d])
    {
      const int w = H.sn_c0[s+1] - H.sn_c0[s], r = H.sn_rowptr[s+1] - H.sn_rowptr[s] - w - 1;
      for(int ti = 0; 16*ti < r; ti++) for(int tj = 0; 16*tj < w; tj++) task.push_back({s, ti, tj, 0});
    }
    X.tb_ptr.push_back((int)task.size());
    for(int s : by[d])
    {
      const int w = H.sn_c0[s+1] - H.sn_c0[s];
      for(int ti = 0; 16*ti < w; ti++) for(int tj = 0; tj <= ti; tj++) task.push_back({s, ti, tj, 0});
    }
    X.tc_ptr.push_back((int)task.size());
  }
  for(int s = 0; s < nsn; s++)
  {
    const int w = H.sn_c0[s+1] - H.sn_c0[s];
    wmax = std::max(wmax, w);
    for(int cb = 0; cb < w; cb += SMR) prep.push_back({s, cb, 0, 0});
  }
  X.ndepth = nd; X.nprep = (int)prep.size();
  X.prep_lds = (int)std::max(sel_prep_lds(std::min(wmax, SEL_WLDS)), sel_prep_lds(wmax));
  DLG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_selinv_prep), hipFuncAttributeMaxDynamicSharedMemorySize, X.prep_lds));
  DLG_CHECK(upload(X.prep, prep)); DLG_CHECK(upload(X.task, task));
  DLG_CHECK(upload(X.par, parent)); DLG_CHECK(upload(X.prel, prel)); DLG_CHECK(upload(X.foff, foff));
  X.sx_n = H.lx_size;
  DLG_HIP(hipMalloc(&X.Sx, sizeof(double)*(size_t)std::max<int64_t>(X.sx_n, 1)));
  DLG_HIP(hipMalloc(&X.Yb, sizeof(double)*(size_t)std::max<int64_t>(X.sx_n, 1)));
  for(int i = 0; i < 2; i++) DLG_HIP(hipMalloc(&X.F[i], sizeof(double)*(size_t)std::max<int64_t>(X.fsize[i], 1)));
  X.sparse_ready = true;
  return DLG_OK;
}

int sel_sweep(dlg_backend* b, SelInv& X)
{
  SparseSym* Y = b->sym;
  hipStream_t st = b->stream;
  hipLaunchKernelGGL(k_selinv_prep, dim3(X.nprep), dim3(TPB), X.prep_lds, st, X.prep, Y->sn_c0, Y->sn_rowptr, Y->sn_lx, Y->Lx, X.Yb);
  for(int d = 0; d < X.ndepth; d++)
  {
    const int nb = X.tb_ptr[d+1] - X.tc_ptr[d], nc = X.tc_ptr[d+1] - X.tb_ptr[d+1];
    const int wpg = TPB/64;
    if(nb > 0)
      hipLaunchKernelGGL(k_selinv_level, dim3(dlg_cdiv(nb, wpg)), dim3(TPB), 0, st, X.task + X.tc_ptr[d], nb, 0, Y->sn_c0,
                         Y->sn_rowptr, Y->sn_lx, Y->relpos, X.par, X.prel, X.foff, X.F[(d + 1) & 1], X.F[d & 1], X.Yb, X.Sx);
    if(nc > 0)
      hipLaunchKernelGGL(k_selinv_level, dim3(dlg_cdiv(nc, wpg)), dim3(TPB), 0, st, X.task + X.tb_ptr[d+1], nc, 1, Y->sn_c0,
                         Y->sn_rowptr, Y->sn_lx, Y->relpos, X.par, X.prel, X.foff, X.F[(d + 1) & 1], X.F[d & 1], X.Yb, X.Sx);
  }
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}

void sel_free_query(SelInv& X)
{
  if(X.qpos) (void)hipFree(X.qpos);
  if(X.qout) (void)hipFree(X.qout);
  X.qpos = nullptr; X.qout = nullptr; X.qkey.clear(); X.nq = 0;
}
} // namespace

void selinv_release(dlg_backend* b)
{
  if(!b->selinv) return;
  if(b->stream) (void)hipStreamSynchronize(b->stream);
  SelInv& X = *b->selinv;
  sel_free_query(X);
  for(void* q : {(void*)X.prep, (void*)X.task, (void*)X.par, (void*)X.prel, (void*)X.foff, (void*)X.Sx, (void*)X.Yb,
                 (void*)X.F[0], (void*)X.F[1], (void*)X.dvar, (void*)X.dystart, (void*)X.Linv_rm, (void*)X.Sig, (void*)X.dwork})
    if(q) (void)hipFree(q);
  delete b->selinv;
  b->selinv = nullptr;
}

// Sigma at n entries (row[e], col[e]) into out_host.  The sweep runs on every call (the factor may have changed since);
// its plan (sparse: of the pattern) and the lookup of the last request arrays are kept.
int selinv_entries(dlg_backend* b, long n, const int* row, const int* col, double* out_host, const char* who)
{
  if(!b->selinv) b->selinv = new SelInv;
  SelInv& X = *b->selinv;
  const bool sparse = b->type == DLG_SPARSE;
  const auto t0 = std::chrono::steady_clock::now();
  bool built = false;
  if(sparse && !X.sparse_ready)
  {
    DLG_HIP(hipStreamSynchronize(b->stream));
    const int rc = sel_plan(b, X);
    if(rc != DLG_OK) { selinv_release(b); return rc; }
    built = true;
  }
  const uint64_t pk = sparse ? sparse_pattern_key(b) : 0;
  std::vector<int> key = {sparse ? 1 : 0, b->N, (int)(pk & 0x7fffffff), (int)((pk >> 31) & 0x7fffffff), (int)(pk >> 62),
                          (int)(n & 0x7fffffff), (int)(n >> 31)};
  key.insert(key.end(), row, row + n);
  key.insert(key.end(), col, col + n);
  if(X.qkey != key)
  {
    DLG_HIP(hipStreamSynchronize(b->stream));
    sel_free_query(X);
    std::vector<int64_t> pos;
    DLG_CHECK(sel_lookup(b, n, row, col, pos, who));
    DLG_CHECK(upload(X.qpos, pos));
    DLG_HIP(hipMalloc(&X.qout, sizeof(double)*(size_t)n));
    X.qkey.swap(key); X.nq = n;
    built = true;
  }
  X.t_plan = built ? std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() : 0.0;
  DLG_CHECK(sparse ? sel_sweep(b, X) : dense_selinv_run(b, X));
  hipLaunchKernelGGL(k_selinv_pick, dim3(dlg_cdiv(n, TPB)), dim3(TPB), 0, b->stream, n, X.qpos, sparse ? X.Sx : X.Sig, X.qout);
  DLG_LAUNCH_CHECK();
  if(hipMemcpyAsync(out_host, X.qout, sizeof(double)*(size_t)n, hipMemcpyDeviceToHost, b->stream) != hipSuccess ||
     hipStreamSynchronize(b->stream) != hipSuccess)
  { dlg_set_error("%s: download failed", who); return DLG_ERR_HIP; }
  return DLG_OK;
}

extern "C" int dlg_covariance_entries_stats(dlg_backend_t* b, double* plan_seconds, long* sx_values, long* front_values)
{
  if(!b || !plan_seconds || !sx_values || !front_values) { dlg_set_error("dlg_covariance_entries_stats: bad argument"); return DLG_ERR_ARG; }
  if(!b->selinv || b->selinv->qkey.empty()) { dlg_set_error("dlg_covariance_entries has not been run"); return DLG_ERR_STATE; }
  const SelInv& X = *b->selinv;
  *plan_seconds = X.t_plan;
  *sx_values = b->type == DLG_SPARSE ? (long)X.sx_n : (long)X.dn*X.dn;
  *front_values = b->type == DLG_SPARSE ? (long)(X.fsize[0] + X.fsize[1]) : 0;
  return DLG_OK;
}

// host only: the symbolic phase on a pattern and, per entry, whether it lies in the structure of the factor (in_struct[e]
// 0 / 1), and the entries of that structure (lower triangle with the diagonal; stats[0]), the front scratch of the
// sweep in doubles (stats[1]) and the widest supernode (stats[2])
extern "C" int dlg_covariance_entries_probe(int N, int M, const int* colptr, const int* rowidx, long n, const int* row,
                                            const int* col, int* in_struct, long* stats, int nstats)
{
  if(n < 0 || (n > 0 && (!row || !col || !in_struct))) { dlg_set_error("dlg_covariance_entries_probe: bad argument"); return DLG_ERR_ARG; }
  SymHost H;
  char err[512];
  if(sym_analyze(H, N, M, colptr, rowidx, 0, M, err, sizeof(err))) { dlg_set_error("symbolic analysis: %s", err); return DLG_ERR_ARG; }
  for(long e = 0; e < n; e++)
  {
    if(row[e] < 0 || col[e] < 0 || row[e] >= N || col[e] >= N)
    { dlg_set_error("dlg_covariance_entries_probe: entry %ld (%d, %d) is outside the %d variables", e, row[e], col[e], N); return DLG_ERR_ARG; }
    in_struct[e] = sel_pos(H, row[e], col[e]) >= 0;
  }
  long nnz = 0, wmax = 0;
  int64_t fr[2] = {0, 0};
  std::vector<int> dep(H.nsn, 0), nchild(H.nsn, 0);
  for(int s = H.nsn - 1; s >= 0; s--)
  {
    const long w = H.sn_c0[s+1] - H.sn_c0[s], r = H.sn_rowptr[s+1] - H.sn_rowptr[s] - w - 1;
    const int b0 = H.sn_bd_ptr[s], b1 = H.sn_bd_ptr[s+1];
    if(b1 > b0)
      for(int m = b0; m < b1; m++) { const long wm = (m + 1 < b1 ? H.sn_bd_col[m+1] : w) - H.sn_bd_col[m]; nnz += wm*(wm + 1)/2; }
    else nnz += w*(w + 1)/2;
    nnz += w*r;
    wmax = std::max(wmax, w);
    if(r > 0) { const int p = H.col_sn[H.sn_rows[H.sn_rowptr[s] + w]]; dep[s] = dep[p] + 1; nchild[p]++; }
  }
  int nd = 0;
  for(int s = 0; s < H.nsn; s++) nd = std::max(nd, dep[s] + 1);
  std::vector<int64_t> at(nd, 0);
  for(int s = 0; s < H.nsn; s++)
    if(nchild[s] > 0) { const int64_t ns = H.sn_rowptr[s+1] - H.sn_rowptr[s] - 1; at[dep[s]] += ns*ns; }
  for(int d = 0; d < nd; d++) fr[d & 1] = std::max(fr[d & 1], at[d]);
  const long v[] = { nnz, (long)(fr[0] + fr[1]), wmax };
  for(int i = 0; i < nstats && i < 3; i++) stats[i] = v[i];
  return DLG_OK;
}
