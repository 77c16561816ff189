// sparse_factor.hip -- K5: level-scheduled supernodal Cholesky on gfx950,
// replaces cholmod_factorize[_p] (dogleg.c:659-664).  Per elimination-tree level: panel
// factorisation (k_factor_level), then the updates of the ancestors by the level's panels.
#include "sparse_internal.h"
#include "panel_factor.h"
#include "factor_tail.h"

namespace {
// -DDLG_FL_PROFILE: phase clocks of workgroup 0 of every factor launch (tools only)
#ifdef DLG_FL_PROFILE
constexpr int FL_PROF_WG = 4096;       // workgroups per level whose phase clocks are kept
__device__ long long g_fl_prof[32*FL_PROF_WG*8];
__device__ long long g_fl_add[FL_PROF_WG*4];          // the children's adds of the one-launch region: see mf_add_children
#define FL_ADD_STAMP(k) do { if(HANDOFF && threadIdx.x == 0 && blockIdx.x < FL_PROF_WG) g_fl_add[blockIdx.x*4 + (k)] = wall_clock64(); } while(0)
#define FL_STAMP(k) do { if(threadIdx.x == 0 && blockIdx.x < FL_PROF_WG) g_fl_prof[((prof_lvl & 31)*FL_PROF_WG + blockIdx.x)*8 + (k)] = wall_clock64(); } while(0)      // 100 MHz, one clock for the chip
#else
#define FL_STAMP(k)
#define FL_ADD_STAMP(k)
#endif

// multifrontal region: add the update matrices of the children of a supernode into its LDS
// panel P (entries whose column is one of the supernode's own columns) and into its own update
// matrix Wt (the others; zeroed here).  The region stores NEGATED update matrices W = -U, so
// both destinations are plain additions.  The symbolic phase lists the destination of every
// entry of every child (mf_dst: element offset from P; bit 15: offset into a Wt kept in HBM),
// padded to whole batches with a scratch slot, so the kernel is a pure stream: a low-occupancy
// wave pays ~4 cycles per instruction of any kind, and a dependent global load costs
// microseconds up here -- all loads of a batch (MF_SLOTS entries per thread) are issued
// together.  One child at a time: inside a child no two entries share a destination, so the
// sums are in child order.
template <int NT, bool UT_LDS, bool HANDOFF = false>
__device__ __forceinline__ void mf_add_children(double* P, double* Wt, int ntri, int nch, int ch0,
                                                MfChild rc, const MfChild* __restrict__ mf_rec,
                                                const double* uscr, const uint16_t* __restrict__ mf_dst, int tid,
                                                int* pr_flag = nullptr, int pr_epoch = 0, DlgHandoff ho = DlgHandoff{nullptr, 0, 0}, int z0 = 0)
{
  constexpr int MF_SLOTS = (NT >= 512) ? 20 : 16;      // 512 threads: up to 10240 entries (a 139-row update matrix) in one round
  const int lane = tid & 63;
  // (z0 .. ntri: the entries this workgroup sums -- all of them, or a replica's own stretch of an update matrix kept in HBM)
  for(int e = z0 + tid; e < ntri; e += NT) Wt[e] = 0.0;
  __syncthreads();
  for(int k = 0; k < nch; k++)
  {
    if(k > 0 && (k & 63) == 0) rc = mf_rec[ch0 + k + min(lane, nch - k - 1)];
    const int npad = __builtin_amdgcn_readlane(rc.npad, k & 63);
    const int64_t uo = ((int64_t)__builtin_amdgcn_readlane((int)(rc.u_off >> 32), k & 63) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)rc.u_off, k & 63);
    const int64_t dof = ((int64_t)__builtin_amdgcn_readlane((int)(rc.dst_off >> 32), k & 63) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)rc.dst_off, k & 63);
    const double* Wc = uscr + uo + tid;
    const uint16_t* D = mf_dst + dof + tid;
    // the destinations of the first round are static data (cold in HBM, ~2 us away): on their way BEFORE the
    // wait for the child, so that behind its flag only the update matrix itself is fetched
    unsigned d[MF_SLOTS];
#pragma unroll
    for(int u = 0; u < MF_SLOTS; u++) d[u] = (u*NT < npad) ? D[u*NT] : 0u;
    if(HANDOFF)
    {
      // persistent top region: wait for THIS child's flags only (the children of this launch; the others
      // finished with the launch before) -- one flag per replica of the child, each of which hands over its
      // tile columns of the update matrix.  The symbolic phase lists the children by expected time of
      // arrival, the latest last: the early ones are added while the late one is still at work, and the
      // order of the sums stays what the list says.
      const int cr = __builtin_amdgcn_readlane(rc.rsv, k & 63);
      const int ci = cr & 0xfffff, cn = cr >> 20;          // (cr < 0: not in this launch, cn < 0)
      if(tid < cn)
      {
        int spins = 0;
        while(__hip_atomic_load(pr_flag + ci + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != pr_epoch + ho.skew)
        {
          __builtin_amdgcn_s_sleep(1);
          if(++spins > ho.spins) { atomicOr(ho.status, DLG_HANDOFF_FACTOR); break; }      // a child that never arrives: report (its own status word: not a pivot), do not hang
        }
      }
      __syncthreads();
      if(k == 0) FL_ADD_STAMP(0);
      if(k == nch - 1) FL_ADD_STAMP(2);
    }
    for(int e0 = 0; e0 < npad; e0 += NT*MF_SLOTS)      // npad is a multiple of 1024: whole rounds of NT
    {
      double v[MF_SLOTS], old[MF_SLOTS];
      if(e0 > 0)
      {
#pragma unroll
        for(int u = 0; u < MF_SLOTS; u++) if(e0 + u*NT < npad) d[u] = D[e0 + u*NT];
      }
#pragma unroll
      for(int u = 0; u < MF_SLOTS; u++)
        if(e0 + u*NT < npad)
        {
          // persistent top region: the child wrote these bytes in this launch (write-through stores,
          // see k_factor_level) -- read them around this CU's L1
          // (a global_ load: the hand-off is not measured for flat_ ones)
          typedef const __attribute__((address_space(1))) double* gptr_t;
          v[u] = HANDOFF ? __hip_atomic_load((gptr_t)(Wc + e0 + u*NT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : Wc[e0 + u*NT];
        }
      if(UT_LDS)
      {
#pragma unroll
        for(int u = 0; u < MF_SLOTS; u++) if(e0 + u*NT < npad) old[u] = P[d[u]];
#pragma unroll
        for(int u = 0; u < MF_SLOTS; u++) if(e0 + u*NT < npad) P[d[u]] = old[u] + v[u];
      }
      else
      {
        // the update matrix lives in HBM: each of its entries gets an atomic add (fire and forget,
        // no read round trip).  A child adds to an address at most once and the barrier orders the
        // children's instruction streams; the adds of one CU to one address reach L2 through the
        // same queue in that order (waiting for L2's acknowledgement before every barrier --
        // s_waitcnt vmcnt(0) -- was measured: it doubles this phase).  With sliced fronts no supernode of
        // config #4 comes here any more; the run-to-run bit tests that pin this path are
        // tests/test_scale_gpu.py::test_update_matrices_summed_in_hbm_are_bitwise_reproducible_config4
        // (slices off: 23 update matrices of the region summed here) and ..._config5.
#pragma unroll
        for(int u = 0; u < MF_SLOTS; u++) if(e0 + u*NT < npad) old[u] = P[(d[u] & 0x8000) ? 0 : d[u]];
#pragma unroll
        for(int u = 0; u < MF_SLOTS; u++)
          if(e0 + u*NT < npad)
          {
            if(d[u] & 0x8000) unsafeAtomicAdd(Wt + (d[u] & 0x7fff), v[u]);
            else P[d[u]] = old[u] + v[u];
          }
      }
    }
    __syncthreads();
    if(k == 0) FL_ADD_STAMP(1);
  }
}

// The usual case of the one-launch region -- two children, each update matrix one round of loads, everything
// staged in LDS -- with the second child's loads on their way while the first is being added.  Both children of
// a supernode on the critical chain arrive together; added one after the other they cost two memory round trips
// and a poll in between (2.5 + 1.3 + 2.4 us measured).  Here every thread, once the first child's loads are out,
// reads the second child's flags itself: if they are up (a thread's own finding: its loads come after its own
// look at the flags, nobody else's), its half of that child's entries is fetched while it adds the first child's.
// The order of the sums is the list's, as before: first child, workgroup barrier, second child.
template <int NT>
__device__ __forceinline__ void mf_add_two_pipelined(double* P, double* Wt, int nzero, MfChild rc, const double* uscr,
                                                     const uint16_t* __restrict__ mf_dst, int tid,
                                                     int* pr_flag, int pr_epoch, DlgHandoff ho)
{
  constexpr int H = 10;                    // entries per thread and half (two halves = one round of 20*NT)
  constexpr bool HANDOFF = true;           // (the profile build's stamps ask)
  (void)HANDOFF;
  typedef const __attribute__((address_space(1))) double* gptr_t;
  for(int e = tid; e < nzero; e += NT) Wt[e] = 0.0;
  const int npA = __builtin_amdgcn_readlane(rc.npad, 0), npB = __builtin_amdgcn_readlane(rc.npad, 1);
  auto rl64 = [&](int64_t v, int l) { return ((int64_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, l); };
  const double* WA = uscr + rl64(rc.u_off, 0) + tid; const double* WB = uscr + rl64(rc.u_off, 1) + tid;
  const uint16_t* DA = mf_dst + rl64(rc.dst_off, 0) + tid; const uint16_t* DB = mf_dst + rl64(rc.dst_off, 1) + tid;
  const int crA = __builtin_amdgcn_readlane(rc.rsv, 0), crB = __builtin_amdgcn_readlane(rc.rsv, 1);
  const int ciA = crA & 0xfffff, cnA = crA >> 20, ciB = crB & 0xfffff, cnB = crB >> 20;
  const int want = pr_epoch + ho.skew;
  auto wait_flags = [&](int ci, int cn) {
    if(tid < cn)
    {
      int spins = 0;
      while(__hip_atomic_load(pr_flag + ci + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want)
      {
        __builtin_amdgcn_s_sleep(1);
        if(++spins > ho.spins) { atomicOr(ho.status, DLG_HANDOFF_FACTOR); break; }
      }
    } };
  auto load_child = [&](const double* W, int np, double (&x)[H], double (&y)[H]) {
#pragma unroll
    for(int u = 0; u < H; u++) x[u] = (u*NT < np) ? __hip_atomic_load((gptr_t)(W + u*NT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
    for(int u = 0; u < H; u++) y[u] = ((H + u)*NT < np) ? __hip_atomic_load((gptr_t)(W + (H + u)*NT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  };
  auto add_half = [&](const unsigned* d, int np, int u0, const double (&v)[H]) {
    double old[H];
#pragma unroll
    for(int u = 0; u < H; u++) old[u] = P[d[u0 + u]];
#pragma unroll
    for(int u = 0; u < H; u++) if((u0 + u)*NT < np) P[d[u0 + u]] = old[u] + v[u];
  };
  // destinations of both children: static data, on their way before any wait
  unsigned dA[2*H], dB[2*H];
#pragma unroll
  for(int u = 0; u < 2*H; u++) { dA[u] = (u*NT < npA) ? DA[u*NT] : 0u; dB[u] = (u*NT < npB) ? DB[u*NT] : 0u; }
  // Wave 0 waits for the first child and looks at the second child's flags in the same loads (lanes 8 ..): where BOTH are
  // up when the first one is -- or one more look later: the children of a balanced tree finish together, and since the
  // short last blocks of the 66-column separators went to the vector pipe that is the rule at the top of config #4 --
  // all entries of both update matrices are fetched in ONE round of loads; one behind the other they are two round trips
  // (8 - 9 us from the last flag to "children added" at the root, profiles/r05_top_of_tree_levels.txt).  The sums keep
  // their order either way: first child, barrier, second child.
  __shared__ int s_both;
  if(tid < 64)
  {
    int spins = 0;
    const bool la = tid < cnA, lb = tid >= 8 && tid < 8 + cnB;
    bool ball = false;
    for(;;)
    {
      const int va = la ? __hip_atomic_load(pr_flag + ciA + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
      const int vb = lb ? __hip_atomic_load(pr_flag + ciB + (tid - 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
      ball = __all(vb == want);
      if(__all(va == want)) break;
      __builtin_amdgcn_s_sleep(1);
      if(++spins > ho.spins) { if(tid == 0) atomicOr(ho.status, DLG_HANDOFF_FACTOR); ball = false; break; }
    }
#ifndef DLG_ADD_NO_GRACE
    if(!ball && cnB > 0 && spins <= ho.spins)
    {
      // (one more look: a second child a few hundred nanoseconds behind the first is worth that wait -- it saves a round trip)
      const int vb = lb ? __hip_atomic_load(pr_flag + ciB + (tid - 8), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
      ball = __all(vb == want);
    }
#endif
#ifdef DLG_ADD_NO_BOTH
    ball = false;
#endif
    if(tid == 0) s_both = (ball && cnB > 0) ? 1 : 0;
  }
  __syncthreads();                         // (also: Wt is zero everywhere)
  FL_ADD_STAMP(0);
  double vX[H], vY[H], bX[H], bY[H];
  if(s_both)
  {
    load_child(WA, npA, vX, vY);
    load_child(WB, npB, bX, bY);
    add_half(dA, npA, 0, vX); add_half(dA, npA, H, vY);
    __syncthreads();                       // the first child is in, in every thread's entries
    FL_ADD_STAMP(1);
    FL_ADD_STAMP(2);
#ifdef DLG_FL_PROFILE
    if(threadIdx.x == 0 && blockIdx.x < FL_PROF_WG) g_fl_add[blockIdx.x*4 + 3] = 2000 + 10*cnB;
#endif
    add_half(dB, npB, 0, bX); add_half(dB, npB, H, bY);
    __syncthreads();
    return;
  }
  // The second child is still at work: the first child's entries, and behind their first half every thread's own look at
  // the second child's flags -- if they are up (a thread's own finding: its loads come after its own look at the flags,
  // nobody else's), its half of that child's entries is fetched while it adds the first child's second half.
  load_child(WA, npA, vX, vY);
  add_half(dA, npA, 0, vX);
  int fl[8];
#pragma unroll
  for(int q = 0; q < 8; q++) fl[q] = (q < cnB) ? __hip_atomic_load(pr_flag + ciB + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : want;
  add_half(dA, npA, H, vY);
  bool bup = true;
#pragma unroll
  for(int q = 0; q < 8; q++) bup = bup && fl[q] == want;
  if(bup) load_child(WB, npB, bX, bY);
  __syncthreads();                         // the first child is in, in every thread's entries
  FL_ADD_STAMP(1);
#ifdef DLG_FL_PROFILE
  if(threadIdx.x == 0 && blockIdx.x < FL_PROF_WG) g_fl_add[blockIdx.x*4 + 3] = 1000 + (bup ? 1 : 0) + 10*cnB + 100*(fl[0] == want);
#endif
  if(!bup) wait_flags(ciB, cnB);           // (a polling lane that saw them up itself has nothing to wait for)
  __syncthreads();
  FL_ADD_STAMP(2);
  if(!bup) load_child(WB, npB, bX, bY);
  add_half(dB, npB, 0, bX); add_half(dB, npB, H, bY);
  __syncthreads();
}

// factor one supernode panel per workgroup in LDS (column-major, even leading dimension).
// One workgroup per work item (FwItem) = (supernode, slice [r0,r1) of its below rows): the LDS
// panel holds the w x w top block plus the slice (up to ~160 KB); slices of one supernode factor
// the top block redundantly (identical arithmetic), slice 0 publishes it (top_scr, k_copy_top).
// The arithmetic is in panel_factor.h:
//   * regular panels, >= 256 threads: panel_factor_mfma -- per 8 columns wave 0 brings the
//     diagonal row tile up to date on the matrix cores, factors the 8x8 block in registers and
//     publishes it while the other waves update the remaining row tiles; barrier; every thread
//     solves its row; barrier;
//   * 128 threads: panel_factor (same steps, all waves factor the block redundantly);
//   * sibling-merged leaves (block-diagonal top): no sweep at all; unsliced ones in a compact
//     layout that never stages the (almost empty) top block (bd_compact_*), sliced ones through
//     panel_factor_blockdiag.
// mode 1 / 2: the (unsliced) panel's update matrix U = B B' comes straight out of LDS afterwards;
// mode 2 (multifrontal region) first adds the children's update matrices (mf_add_children), leaves
// them in U as well and stores W = -U.  U is staged behind the panel in LDS when both fit.
// The panel is copied in and out thread = (row, column group), CP_FLIGHT columns in flight.
// LEAF: every work item of the launch is an unsliced block-diagonal panel in the compact layout (a level
// of merged leaves) -- the paths of the other kinds of panel are compiled out, which brings the kernel
// under 128 registers: 4 workgroups per CU instead of 3.
template <int NT, bool LEAF = false>
__global__ void __launch_bounds__(NT, LEAF ? 4 : 1) k_factor_level(const FwItem* __restrict__ items,
                                                     const MfChild* __restrict__ mf_rec,
                                                     const int* __restrict__ sn_bd_col,
                                                     const uint16_t* __restrict__ mf_dst,
                                                     double* __restrict__ Lx,
                                                     double* __restrict__ top_scr,
                                                     int* __restrict__ info,
                                                     double* uscr, int mode,
                                                     int* pr_flag, int pr_epoch, DlgHandoff ho, int64_t pr_acc,
                                                     double* __restrict__ leaf_rd)
{
  extern __shared__ __attribute__((aligned(16))) double P[];
  __shared__ int sbad, s_skip;
  constexpr int DS = LEAF ? 4 : 8;             // doubles per column of the factored member blocks (compact layout)
  constexpr int CP_FLIGHT = LEAF ? 16 : 32;
#ifdef DLG_FL_PROFILE
  const int prof_lvl = mode >> 8;
  FL_STAMP(0);
#endif
  const bool stage_leaf_u = (mode & 4) != 0;    // childless supernodes may stage U in LDS too (host: no occupancy loss)
  const bool b16 = (mode & 16) != 0;            // panel_factor_b16 (blocks of 16, the diagonal tile in registers)
  // FMODE_LEAN_ROWS (LEAF only): of the rows below the member blocks only the augmented row goes back to the panel -- the
  // others stay the assembly's W, whose one reader inside a step, the backward solve, takes L_below' x = L_tt^-1 (W' x)
  // from them (k_solve_bwd_level: rows_raw); the members' reciprocal pivots are left in leaf_rd for the readers that
  // need L_below itself (k_leaf_rows_materialize)
  const bool lean_rows = LEAF && (mode & 32) != 0;
  mode &= 3;
  const FwItem it = items[blockIdx.x];
  const int r0 = it.r0, w = it.w, nrows = it.nrows;
  double* G = Lx + it.lx;
  const int tid = threadIdx.x, lane = tid & 63;
  const int nloc = w + (it.r1 - r0);          // rows held by this workgroup
  const int shift = r0;                        // local row i >= w  <->  panel row i + shift
  const int64_t top = it.top;
  const int mb = nloc - w, ntri = mb*(mb + 1)/2;
  // compact layout for unsliced block-diagonal panels (the merged point leaves): the top block is
  // almost all zeros and is never staged -- LDS holds the rows below it (Pb[i + j*ldp], i >= w) and
  // the factored member blocks (Dg), see panel_factor.h
  const bool cmp = it.nbd > 0 && top < 0;
  const int ldp = cmp ? ((mb + 1) & ~1) : ((nloc + 1) & ~1);
  double* Pb = cmp ? P - w : P;
  const int row0c = cmp ? w : 0;               // first row that is staged
  const bool has_u = mode != 0 && top < 0;
  // the update matrix is staged in LDS where it fits: behind the panel, its last columns in the unused
  // strict upper triangle of the top block if need be (it.jsp, sym_w_split)
  // (sliced: a replica of the one-launch region that keeps only its own columns of the update matrix -- the
  // packed entries [eA, eB) -- behind the panel; the host sized the LDS for it)
  const bool sliced = !LEAF && it.sliced != 0;
  const bool u_lds = has_u && (sliced || ((it.nch > 0 || stage_leaf_u) &&
                     (cmp ? (size_t)(ldp*w + ntri + 1 + DS*w)*sizeof(double) <= (size_t)FAC_LDS_BUDGET : it.jsp >= 0)));   // + the scratch slot of mf_dst
  const int usp = (u_lds && !cmp && !sliced) ? it.jsp : mb;          // first column kept up there (mb: none)
  const int sl_pad = sliced ? (it.eA & 1) : 0;            // (keeps packed index and LDS index of one parity: 16-byte copies)
  const int nlin = sliced ? it.eB - it.eA + sl_pad : usp*mb - usp*(usp - 1)/2;              // doubles behind the panel
  double* Ug = has_u ? uscr + it.u_off : nullptr;
  double* Us = P + ldp*w;                                 // what is behind the panel ...
  const int ush = sliced ? sl_pad - it.eA : 0;            // ... holds packed index e at Us[e + ush]
  double* Dg = Us + (u_lds ? nlin + 1 : 0);
  // (LEAF: members of at most 4 columns, supernodes of at most 64 -- sparse_factor_setup: less LDS per
  // workgroup, which is what lets a fourth one onto the CU)
  __shared__ int s_mcol[LEAF ? 68 : 260];
  __shared__ double s_rdiag[LEAF ? 64 : 256];
  MfChild rc = {0, 0, 0, 0};
  const bool mf_acc = !LEAF && mode == 2 && it.nch > 0;
  if(mf_acc) rc = mf_rec[it.ch0 + min(lane, it.nch - 1)];     // on its way during the panel copy
  // (s_skip: a launch before this one found a non-positive pivot -- the factorisation is going to be
  // thrown away by the lambda loop, dogleg.c:656-677: nothing to do here but to let the parent go on)
  if(tid == 0) { sbad = 0x7fffffff; s_skip = __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0x7fffffff; }
  // one-launch region: its last workgroup (dispatched last: all of them are on their CUs) opens the gate
  // behind which the second stream holds the Cauchy step's pass over J (the word behind the items' flags;
  // a matter of timing only -- that pass depends on nothing this launch computes)
  if(pr_flag && tid == 0 && blockIdx.x == gridDim.x - 1)
    __hip_atomic_store(pr_flag + gridDim.x, pr_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if(cmp)
  {
    __syncthreads();
    // (a workgroup of a factorisation that is not going to be used -- failed pivot in an earlier launch, abandoned
    // (sparse_abandon_enqueued), or found doomed by the look at the diagonal (sparse_factorize) -- leaves before it loads
    // anything and, above all, before the members are factored IN PLACE below: the panels stay the assembly's)
    if(s_skip)
    {
      if(pr_flag && tid == 0) __hip_atomic_store(pr_flag + blockIdx.x, pr_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    bd_compact_members<NT, DS>(G, nrows, w, tid, sn_bd_col + it.bd0, it.nbd, it.bdw, s_mcol, s_rdiag, Dg, &sbad, it.col0);
  }
  // LEAF: the rows below the top block are ONE linear image in LDS (column j at P + j ldp, ldp even): they come in by
  // loads that write LDS themselves (16 bytes a lane, a wave-instruction fills 128 consecutive doubles of the image, the
  // lane's source address is its own) -- all of a panel's loads are in flight at once and no register holds a value.
  // Through registers, sixteen columns a thread at a time, the copy was two dependent round trips and 9.8 of a leaf
  // workgroup's 26.8 us (tools/prof_factor.sh).  (A pad row reads the first entry of the next column: never used.)
  // (thread = (panel row, column group) of the copies through registers: rows padded to whole waves, the remaining threads
  // take further columns)
  const int cp_rows = min(NT, (nloc - row0c + 63) & ~63), cp_ng = NT/cp_rows, cp_g = tid/cp_rows;
  // The same for a whole unsliced panel (rows 0 .. nloc of every column, column j at P + j ldp): the first level of the
  // one-launch region waits for nothing but this copy (8.2 us of its 28, profiles/r05_top_of_tree_levels.txt).
#ifndef DLG_LEAF_NO_GLDS
  if((LEAF && cmp) || (!LEAF && !cmp && !sliced && shift == 0))
  {
    const int ntot = ldp*w;
    const double* g0 = cmp ? G + (w + shift) : G;
    for(int k = tid >> 6; 128*k < ntot; k += NT/64)
    {
      const int e = 128*k + 2*lane;
      if(e < ntot)
      {
        const int j = e / ldp, r = e - j*ldp;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(g0 + (size_t)j*nrows + r),
                                         (__attribute__((address_space(3))) void*)(P + 128*k), 16, 0, 0);
      }
    }
  }
  else
#endif
  {
  for(int i = row0c + tid - cp_g*cp_rows; i < nloc && cp_g < cp_ng; i += cp_rows)
  {
    const double* gp = G + (i < w ? i : i + shift);
    for(int j0 = cp_g; j0 < w; j0 += CP_FLIGHT*cp_ng)
    {
      double v[CP_FLIGHT];
#pragma unroll
      for(int u = 0; u < CP_FLIGHT; u++) v[u] = (j0 + u*cp_ng < w) ? gp[(size_t)(j0 + u*cp_ng)*nrows] : 0.0;
#pragma unroll
      for(int u = 0; u < CP_FLIGHT; u++) if(j0 + u*cp_ng < w) Pb[i + (j0 + u*cp_ng)*ldp] = v[u];
    }
  }
  }
  // (persistent top region: the panel is in LDS already; the children's flags are awaited one by one in
  // mf_add_children)
  __syncthreads();
  FL_STAMP(1);
  // Replicas of a supernode all read its panel from HBM and ONE of them writes the factored panel back: the last one
  // (highest workgroup index: the others were dispatched before it), and only after every other replica has said that
  // its copy is in LDS -- a replica that finds no CU until late (a chip shared with other launches) would otherwise
  // read a panel that is factored already.  The word: -epoch = "panel read", epoch = "done" (what the parent waits for).
  const int nrep = (pr_flag && it.rsv2 > 1) ? it.rsv2 : 1;
  if(nrep > 1 && it.rep < nrep - 1 && tid == 0) __hip_atomic_store(pr_flag + blockIdx.x, -pr_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if(s_skip)
  {
    if(pr_flag && tid == 0) __hip_atomic_store(pr_flag + blockIdx.x, pr_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if(mf_acc && usp < mb)
    for(int jw = usp + (tid >> 6); jw < mb; jw += NT/64)
      for(int i = lane; i < mb - jw; i += 64) P[(mb - jw)*ldp + i] = 0.0;      // (the barrier is in mf_add_children)
  if(mf_acc)
  {
    // (two children, one round of loads each: the second child's loads overlap the first child's adds)
    const bool two = NT >= 512 && it.nch == 2 && __builtin_amdgcn_readlane(rc.npad, 0) <= 20*NT && __builtin_amdgcn_readlane(rc.npad, 1) <= 20*NT &&
                     (__builtin_amdgcn_readlane(rc.rsv, 0) >> 20) <= 8 && (__builtin_amdgcn_readlane(rc.rsv, 1) >> 20) <= 8;
    if(pr_flag && u_lds && two) mf_add_two_pipelined<NT>(P, Us, nlin, rc, uscr, mf_dst, tid, pr_flag, pr_epoch, ho);
    else if(pr_flag && u_lds) mf_add_children<NT, true, true>(P, Us, nlin, it.nch, it.ch0, rc, mf_rec, uscr, mf_dst, tid, pr_flag, pr_epoch, ho);
    // (replicas of a supernode whose update matrix is summed in HBM: each owns the packed entries [eA, eB) -- its tile
    // columns --, its destination lists drop everything else of the children that is not a panel entry)
    else if(pr_flag)     mf_add_children<NT, false, true>(P, Ug + pr_acc, (nrep > 1 && !sliced) ? it.eB : ntri, it.nch, it.ch0, rc, mf_rec, uscr, mf_dst, tid, pr_flag, pr_epoch, ho,
                                                          (nrep > 1 && !sliced) ? it.eA : 0);
    else if(u_lds)  mf_add_children<NT, true >(P, Us, nlin, it.nch, it.ch0, rc, mf_rec, uscr, mf_dst, tid);
    else            mf_add_children<NT, false>(P, Ug, ntri, it.nch, it.ch0, rc, mf_rec, uscr, mf_dst, tid);
  }
  FL_STAMP(2);
  if(cmp) bd_compact_rows<NT, DS>(Pb, ldp, nloc, w, tid, it.nbd, s_mcol, s_rdiag, Dg, it.bdw);
  else if(LEAF) { }
  else if(it.nbd > 0) panel_factor_blockdiag<NT>(P, ldp, nloc, w, tid, sn_bd_col + it.bd0, it.nbd, &sbad, it.col0, s_mcol, s_rdiag);
  else if(NT >= 256 && b16 && nloc <= 16*PF_B16_MAXT) panel_factor_b16<(NT >= 256 ? NT : 256)>(P, ldp, nloc, w, tid, &sbad, it.col0);
  else if(NT >= 256) panel_factor_mfma<(NT >= 256 ? NT : 256)>(P, ldp, nloc, w, tid, &sbad, it.col0);
  else         panel_factor<NT, true, true>(P, ldp, nloc, w, tid, &sbad, it.col0);
  FL_STAMP(3);
  if(r0 == 0 && it.rep == 0 && tid == 0 && sbad != 0x7fffffff) atomicMin(info, sbad);
  // U = B B' (mode 2: W = children's sum - B B'): lower 16x16 tiles on the matrix cores, both
  // operands read from the panel (factor_tail_tiles above).  The lower triangle of tiles is dealt
  // out in column-major tile order, in chunks of consecutive tiles: every round gives each wave one
  // chunk, all chunks of a round within one tile of each other -- the two waves of a SIMD share its
  // matrix core, so the tail is only as fast as the busiest SIMD.
  if(has_u)
  {
    const int T = (mb + 15) >> 4;
    const int wv = tid >> 6;
    double* Ud = u_lds ? Us : Ug;              // in place behind the panel (+ ush), or straight to the scratch
    constexpr int NWV = NT/64;
    constexpr int SY_G = (NT >= 512) ? 6 : 4;
    constexpr int TKD = LEAF ? 2 : 4;          // k-steps of operands in flight (factor_tail.h; the leaf instantiation has 128 registers)
    // (a replica of the one-launch region forms the tile columns [tj0, tj1) only: tiles [tlo, thi) in
    // column-major tile order; every tile has its own accumulator chain, so who forms it changes no bit)
    const int tjA = min(it.tj0, T), tjB = min(it.tj1, T);
    const int tlo = tjA*T - tjA*(tjA - 1)/2, thi = tjB*T - tjB*(tjB - 1)/2;
    const int ntiles = thi - tlo;
    const int rounds = (ntiles + NWV*SY_G - 1)/(NWV*SY_G), nchunks = rounds*NWV;
    const bool w_hbm = mf_acc && !u_lds;
    const bool st_wt = pr_flag != nullptr && !u_lds;
    const int ush_t = u_lds ? ush : 0;
    const int64_t acc_shift = st_wt ? pr_acc : 0;
    for(int c = wv; c < nchunks; c += NWV)
    {
      // (32-bit: c*ntiles < 2^31 by far; a 64-bit division is some hundred instructions in front of the products)
      const int t0 = tlo + (int)((unsigned)(c*ntiles)/(unsigned)nchunks), t1 = tlo + (int)((unsigned)((c + 1)*ntiles)/(unsigned)nchunks);
      switch(t1 - t0)
      {
        case 1: factor_tail_tiles<1, TKD>(Pb, ldp, w, mb, T, t0, Ud, mode, w_hbm, mf_acc, lane, acc_shift, st_wt, usp, P, ush_t); break;
        case 2: factor_tail_tiles<2, TKD>(Pb, ldp, w, mb, T, t0, Ud, mode, w_hbm, mf_acc, lane, acc_shift, st_wt, usp, P, ush_t); break;
        case 3: factor_tail_tiles<3, TKD>(Pb, ldp, w, mb, T, t0, Ud, mode, w_hbm, mf_acc, lane, acc_shift, st_wt, usp, P, ush_t); break;
        case 4: factor_tail_tiles<4, TKD>(Pb, ldp, w, mb, T, t0, Ud, mode, w_hbm, mf_acc, lane, acc_shift, st_wt, usp, P, ush_t); break;
        case 5: if(SY_G >= 5) factor_tail_tiles<(SY_G >= 5 ? 5 : 1), TKD>(Pb, ldp, w, mb, T, t0, Ud, mode, w_hbm, mf_acc, lane, acc_shift, st_wt, usp, P, ush_t); break;
        case 6: if(SY_G >= 6) factor_tail_tiles<(SY_G >= 6 ? 6 : 1), TKD>(Pb, ldp, w, mb, T, t0, Ud, mode, w_hbm, mf_acc, lane, acc_shift, st_wt, usp, P, ush_t); break;
        default: break;
      }
    }
    if(u_lds) __syncthreads();
  }
  FL_STAMP(4);
  if(u_lds)
  {
    typedef __attribute__((address_space(1))) double* gwptr_t;
    // the part behind the panel.  Persistent top region: the parent reads W in this same launch --
    // 16-byte write-through stores (the slots are 16-byte aligned and padded to an even length),
    // drained by every wave before the flag goes up
    // (a replica: the columns [jA, jB) of its tile columns -- a contiguous stretch [eA, eB) of the packed triangle)
    const int jA = min(16*it.tj0, mb), jB = min(it.tj1, 1 << 20) >= ((mb + 15) >> 4) ? mb : 16*it.tj1;
    const int jAl = min(jA, usp), jBl = min(jB, usp);
    const int eA = jAl*mb - jAl*(jAl - 1)/2, eB = jBl*mb - jBl*(jBl - 1)/2;
    if(pr_flag)
    {
      const int eA2 = (eA + 1) & ~1, eB2 = eB & ~1;
      for(int e = eA2 + 2*tid; e < eB2; e += 2*NT)
      {
        const dlg_v2d v2 = *reinterpret_cast<const dlg_v2d*>(Us + (e + ush));
        asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(Ug + e), "v"(v2) : "memory");
      }
      if(tid == 0 && eA < eA2 && eA < eB) __hip_atomic_store((gwptr_t)(Ug + eA), Us[eA + ush], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if(tid == 1 && eB2 < eB && eB2 >= eA2) __hip_atomic_store((gwptr_t)(Ug + eB2), Us[eB2 + ush], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    else for(int e = eA + tid; e < eB; e += NT) Ug[e] = Us[e + ush];
    // the columns kept in the top block's upper triangle
    for(int jw = max(usp, jA) + (tid >> 6); jw < jB; jw += NT/64)
    {
      const double* src = P + (mb - jw)*ldp;
      double* dst = Ug + tri_col(jw, mb) + jw;
      for(int i = lane; i < mb - jw; i += 64)
      {
        if(pr_flag) __hip_atomic_store((gwptr_t)(dst + i), src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else dst[i] = src[i];
      }
    }
  }
  if(pr_flag)
  {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if(tid == 0) __hip_atomic_store(pr_flag + blockIdx.x, pr_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  FL_STAMP(7);
  const bool store_panel = it.rep == nrep - 1;       // the panel is the last replica's to store
  if(nrep > 1 && store_panel)
  {
    if(tid < nrep - 1)
    {
      int spins = 0;
      for(;;)
      {
        const int v = __hip_atomic_load(pr_flag + ((int)blockIdx.x - (nrep - 1) + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if(v == pr_epoch || v == -pr_epoch) break;
        __builtin_amdgcn_s_sleep(1);
        if(++spins > ho.spins) { atomicOr(ho.status, DLG_HANDOFF_FACTOR); break; }
      }
    }
    __syncthreads();
  }
  if(LEAF && cmp && lean_rows)
  {
    for(int j = tid; j < w; j += NT)
    {
      G[(size_t)j*nrows + (nloc - 1 + shift)] = Pb[(nloc - 1) + j*ldp];
      leaf_rd[it.col0 + j] = s_rdiag[j];
    }
  }
  else
  for(int i = row0c + tid - cp_g*cp_rows; i < nloc && cp_g < cp_ng && store_panel; i += cp_rows)
  {
    // rows below the top block go back to the panel; the top block too unless the supernode is
    // cut into slices (then slice 0 parks it in top_scr, see k_copy_top) or it was never staged
    double* gp; size_t gs;
    if(i >= w)        { gp = G + (i + shift); gs = (size_t)nrows; }
    else if(top < 0)  { gp = G + i; gs = (size_t)nrows; }
    else if(r0 == 0)  { gp = top_scr + top + i; gs = (size_t)w; }
    else continue;
    // (where the top block's upper triangle held part of W, only its lower triangle goes back)
    const int jend = (usp < mb && i < w) ? i + 1 : w;
    for(int j0 = cp_g; j0 < jend; j0 += 16*cp_ng)
    {
      double v[16];
#pragma unroll
      for(int u = 0; u < 16; u++) v[u] = (j0 + u*cp_ng < jend) ? Pb[i + (j0 + u*cp_ng)*ldp] : 0.0;
#pragma unroll
      for(int u = 0; u < 16; u++) if(j0 + u*cp_ng < jend) gp[(size_t)(j0 + u*cp_ng)*gs] = v[u];
    }
  }
  FL_STAMP(5);
#ifdef DLG_FL_PROFILE
  if(threadIdx.x == 0 && blockIdx.x < FL_PROF_WG)
    g_fl_prof[((prof_lvl & 31)*FL_PROF_WG + blockIdx.x)*8 + 6] = (long long)w | ((long long)nrows << 12) | ((long long)it.nch << 24) | ((long long)(u_lds ? 1 : 0) << 36) | ((long long)(has_u ? 1 : 0) << 37) | ((long long)(it.r1 - it.r0) << 40) | ((long long)(it.rep & 15) << 52) | ((long long)(it.pad & 63) << 56);
#endif
}
// publish the top blocks of the multi-slice supernodes
__global__ void __launch_bounds__(TPB) k_copy_top(const int* __restrict__ ms_sn, const int* __restrict__ sn_c0,
                                                  const int* __restrict__ sn_rowptr,
                                                  const int64_t* __restrict__ sn_lx,
                                                  const int64_t* __restrict__ sn_top,
                                                  double* __restrict__ Lx,
                                                  const double* __restrict__ top_scr, const int* __restrict__ info)
{
  // (a factorisation that broke down or was found doomed: the scratch holds an EARLIER factorisation's top blocks -- they
  // must not land in panels that sparse_assemble may take over as the assembly left them)
  if(*info != 0x7fffffff) return;
  const int s = ms_sn[blockIdx.x];
  const int w = sn_c0[s+1] - sn_c0[s];
  const int nrows = sn_rowptr[s+1] - sn_rowptr[s];
  double* G = Lx + sn_lx[s];
  const double* T = top_scr + sn_top[s];
  for(int e = threadIdx.x; e < w*w; e += TPB) { const int j = e / w, i = e - j*w; G[i + (size_t)j*nrows] = T[e]; }
}

// L_below = W L_tt^-T of the merged leaves a lean leaf launch left as W (k_factor_level, FMODE_LEAN_ROWS), for the readers
// of the factor other than the backward solve.  One workgroup per leaf: the rows below the member blocks into the leaf
// kernel's LDS image, the factored member blocks from the panel and their reciprocal pivots from leaf_rd (what the leaf
// launch held in LDS at this point), bd_compact_rows -- the arithmetic and the bits of the write-back the leaf launch
// left out --, and the rows go back.  The augmented row (the last one) is the factorisation's already: not stored.
template <int NT>
__global__ void __launch_bounds__(NT) k_leaf_rows_materialize(const FwItem* __restrict__ items,
                                                              double* __restrict__ Lx, const double* __restrict__ leaf_rd,
                                                              const int* __restrict__ info)
{
  // (the factor is that of a factorisation that broke down or was given up: its leaf workgroups left before they factored
  // a member -- nothing here is a factor's, and the panels stay what sparse_assemble may take over; see k_copy_top)
  if(*info != 0x7fffffff) return;
  extern __shared__ __attribute__((aligned(16))) double P[];
  constexpr int DS = 4;                        // (the leaf instantiation's: members of at most 4 columns)
  __shared__ int s_mcol[68];
  __shared__ double s_rdiag[64];
  const FwItem it = items[blockIdx.x];
  const int w = it.w, nrows = it.nrows, tid = threadIdx.x;
  // (every item of a lean level is an unsliced block-diagonal panel of at most 64 columns whose members have one common
  // width of at most 4, it.bdw: fac_level_params, L.leaf -- the leaf instantiation's own premise)
  double* G = Lx + it.lx;
  const int mb = nrows - w, ldp = (mb + 1) & ~1;
  double* Pb = P - w;
  double* Dg = P + ldp*w;
  for(int m = tid; m <= it.nbd; m += NT) s_mcol[m] = (m < it.nbd) ? m*it.bdw : w;
  for(int j = tid; j < w; j += NT) s_rdiag[j] = leaf_rd[it.col0 + j];
  __syncthreads();
  for(int m = tid; m < it.nbd; m += NT)
  {
    const int c0 = s_mcol[m], nb = s_mcol[m + 1] - c0;
    for(int c = 0; c < nb; c++)
      for(int q = 0; q <= c && q < DS; q++) Dg[(c0 + c)*DS + q] = G[(c0 + c) + (size_t)(c0 + q)*nrows];
  }
  for(int e = tid; e < mb*w; e += NT) { const int j = e / mb, i = e - j*mb; P[i + j*ldp] = G[(size_t)j*nrows + w + i]; }
  __syncthreads();
  bd_compact_rows<NT, DS>(Pb, ldp, nrows, w, tid, it.nbd, s_mcol, s_rdiag, Dg, it.bdw);
  __syncthreads();
  for(int e = tid; e < (mb - 1)*w; e += NT) { const int j = e / (mb - 1), i = e - j*(mb - 1); G[(size_t)j*nrows + w + i] = P[i + j*ldp]; }
}

// cooperative variant of the update for heavy sources (wide panels): the whole
// workgroup works on one sub-task at a time, thread per source row, the nc x wd
// block of the source rows that sit in the target columns staged in LDS.  The
// target panel is updated in HBM; a barrier orders consecutive sub-tasks.
__global__ void __launch_bounds__(TPB) k_update_coop(int unit0, const int* __restrict__ uw_item,
                                                     const int* __restrict__ uw_s0,
                                                     const int* __restrict__ uw_s1,
                                                     const int64_t* __restrict__ uw_part,
                                                     const int* __restrict__ ui_t,
                                                     const int* __restrict__ ui_col,
                                                     const int* __restrict__ ui_nc,
                                                     const SymSub* __restrict__ usub,
                                                     const int* __restrict__ relpos,
                                                     const int* __restrict__ sn_rowptr,
                                                     const int64_t* __restrict__ sn_lx,
                                                     double* __restrict__ Lx,
                                                     double* __restrict__ upart, const int* __restrict__ info)
{
  // (a factorisation that has broken down -- or was found doomed by the look at the diagonal, sparse_host.hip -- is not
  // worth finishing, and the panels stay what the assembly left: sparse_assemble takes them over for the next lambda)
  if(*info != 0x7fffffff) return;

  __shared__ __attribute__((aligned(16))) double Bs[256*8];
  const int unit = unit0 + blockIdx.x;
  const int item = uw_item[unit];
  const int t = ui_t[item], col = ui_col[item], nc = ui_nc[item];
  const int nrows_t = sn_rowptr[t+1] - sn_rowptr[t];
  const int s0 = uw_s0[unit], s1 = uw_s1[unit];
  const int64_t part = uw_part[unit];
  double* dst = (part < 0) ? (Lx + sn_lx[t] + (int64_t)col*nrows_t) : (upart + part);
  const double sgn = (part < 0) ? -1.0 : 1.0;
  const int tid = threadIdx.x;
  if(part >= 0)
  {
    for(int e = tid; e < nrows_t*nc; e += TPB) dst[e] = 0.0;
    __syncthreads();
  }
  for(int st = s0; st < s1; st++)
  {
    const SymSub U = usub[st];
    const double* Ld = Lx + U.src;
    const int* rel = relpos + U.rel;
    const int ld = U.nrows_d;
    batched_copy<TPB, 8>(U.wd*8, tid,
                         [&](int e) { const int c = e & 7, q = e >> 3; return (c < nc) ? Ld[c + (size_t)q*ld] : 0.0; },
                         [&](int e, double v) { Bs[e] = v; });
    __syncthreads();
    for(int i = tid; i < U.m; i += TPB)
    {
      double sacc[8];
#pragma unroll
      for(int c = 0; c < 8; c++) sacc[c] = 0.0;
#pragma unroll 4
      for(int q = 0; q < U.wd; q++)
      {
        const double ai = Ld[i + (size_t)q*ld];
        const double2 b0 = *reinterpret_cast<const double2*>(&Bs[q*8]);
        const double2 b1 = *reinterpret_cast<const double2*>(&Bs[q*8 + 2]);
        const double2 b2 = *reinterpret_cast<const double2*>(&Bs[q*8 + 4]);
        const double2 b3 = *reinterpret_cast<const double2*>(&Bs[q*8 + 6]);
        sacc[0] += ai*b0.x; sacc[1] += ai*b0.y; sacc[2] += ai*b1.x; sacc[3] += ai*b1.y;
        sacc[4] += ai*b2.x; sacc[5] += ai*b2.y; sacc[6] += ai*b3.x; sacc[7] += ai*b3.y;
      }
      const int cmax = (i < nc - 1) ? i : nc - 1;
      const int r = rel[i];
#pragma unroll
      for(int c = 0; c < 8; c++) if(c <= cmax) dst[r + c*nrows_t] += sgn*sacc[c];
    }
    __syncthreads();
  }
}

// ---- two-phase update of a level with many small sources -------------------------------
// Phase 1: U_d = B_d B_d' for every source d of the level (B_d = the mb rows below its diagonal
// block, wd columns), packed lower triangle (tri_col), into the scratch.
// One workgroup per source: B_d is staged in LDS once (k-major, zero padded to whole tiles),
// the lower 16x16 tiles are produced by v_mfma_f64_16x16x4_f64 with both operands read from
// LDS; a wave owns whole tile columns so the B operand is read once per k-step.
template <int NT>
__global__ void __launch_bounds__(NT) k_update_syrk(const int* __restrict__ lvl_sn,
                                                    const int* __restrict__ sn_c0,
                                                    const int* __restrict__ sn_rowptr,
                                                    const int64_t* __restrict__ sn_lx,
                                                    const int64_t* __restrict__ u_off,
                                                    const double* __restrict__ Lx,
                                                    double* __restrict__ uscr, int KC)
{
  extern __shared__ __attribute__((aligned(16))) double Bs[];
  constexpr int NW = NT/64, TPW = 8;            // waves, tiles per wave (kept in registers)
  const int d = lvl_sn[blockIdx.x];
  const int wd = sn_c0[d+1] - sn_c0[d], nrows = sn_rowptr[d+1] - sn_rowptr[d], mb = nrows - wd;
  const double* Ld = Lx + sn_lx[d] + wd;
  double* U = uscr + u_off[d];
  const int T = (mb + 15) >> 4, MB16 = T*16;
  const int LDB = ((mb + 31)/32)*32 + 16, K4 = (wd + 3) & ~3;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jn = lane & 15, kq = lane >> 4;
  // this wave's tiles: flat index over the lower tiles (column by column), round robin
  const int ntiles = T*(T + 1)/2;
  int aoff[TPW], boff[TPW];
#pragma unroll
  for(int q = 0; q < TPW; q++)
  {
    int rem = w + q*NW, tj = 0;
    if(rem < ntiles) { while(rem >= T - tj) { rem -= T - tj; tj++; } }
    else { rem = 0; tj = 0; }
    aoff[q] = 16*(tj + rem); boff[q] = 16*tj;
  }
  const int nmine = (ntiles - w + NW - 1)/NW;           // tiles of this wave (<= TPW by construction)
  dlg_v4d c4[TPW];
#pragma unroll
  for(int q = 0; q < TPW; q++) c4[q] = (dlg_v4d){0.0, 0.0, 0.0, 0.0};
  for(int k0 = 0; k0 < K4; k0 += KC)
  {
    const int kc = min(KC, K4 - k0);
    if(k0 > 0) __syncthreads();
    batched_copy<NT, 8>(kc*MB16, tid,
                        [&](int e) { const int k = k0 + e / MB16, i = e % MB16; return (k < wd && i < mb) ? Ld[i + (size_t)k*nrows] : 0.0; },
                        [&](int e, double v) { const int k = e / MB16, i = e - k*MB16; Bs[k*LDB + i] = v; });
    __syncthreads();
    const double* base = Bs + kq*LDB + jn;
#pragma unroll 2
    for(int kk = 0; kk < kc; kk += 4)
    {
#pragma unroll
      for(int q = 0; q < TPW; q++)
        if(q < nmine)
          c4[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(base[kk*LDB + aoff[q]], base[kk*LDB + boff[q]], c4[q], 0, 0, 0);
    }
  }
#pragma unroll
  for(int q = 0; q < TPW; q++)
    if(q < nmine)
    {
      const int j = boff[q] + jn;
#pragma unroll
      for(int r = 0; r < 4; r++)
      {
        const int i = aoff[q] + kq + 4*r;
        if(i < mb && j <= i) U[tri_col(j, mb) + i] = c4[q][r];
      }
    }
}
// Phase 2: a work unit (chunk of the sub-tasks of one target column block) adds the column
// blocks of the U_d it is fed from into wave-private LDS slabs (waves take sub-tasks round
// robin), sums the slabs in wave order and applies / stores the result like the other update
// kernels.
constexpr int GATHER_FLIGHT = 4;        // sub-tasks whose loads are in flight together
template <int NT>
__global__ void __launch_bounds__(NT) k_update_gather(int unit0, const GatherUnit* __restrict__ units,
                                                       const SymSub* __restrict__ usub,
                                                       const int64_t* __restrict__ usub_u,
                                                       const int* __restrict__ relpos,
                                                       double* __restrict__ Lx,
                                                       double* __restrict__ upart,
                                                       const double* __restrict__ uscr, int nw,
                                                       int* __restrict__ info,
                                                       const int* __restrict__ fin_gate = nullptr, int fin_epoch = 0, int* fin_status = nullptr)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int s_skip;
  // (fin on the side, sparse_assemble.hip: the partial-sum stages of the target panels may still run on the second
  // stream -- the word is fetched now and looked at in front of the first access to a target panel)
  int fin_seen = fin_epoch;
  if(fin_gate && threadIdx.x == 0) fin_seen = __hip_atomic_load(fin_gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if(threadIdx.x == 0)
  {
    s_skip = *info != 0x7fffffff;      // a failed factorisation is not worth finishing
  }
  // (one flat record: the chain unit -> item -> target supernode -> its rows cost three dependent loads
  // in front of the first barrier)
  const GatherUnit U0 = units[unit0 + blockIdx.x];
  const int nc = U0.nc, nrows_t = U0.nrows_t, s0 = U0.s0, s1 = U0.s1;
  double* Lt = Lx + U0.lt;
  const int64_t part = U0.part;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = nrows_t*nc;
  for(int e = tid; e < slab*nw; e += NT) lds[e] = 0.0;
  __syncthreads();
  if(s_skip) return;
  if(w < nw)
  {
    double* acc = lds + (size_t)w*slab;
    // the records of this wave's sub-tasks (s0 + w, s0 + w + nw, ...): lane l fetches record l of
    // the current batch of 64 with one load per field, the loop broadcasts them with readlane;
    // GATHER_FLIGHT sub-tasks are in flight at a time
    const int nmine = (s1 - s0 - w + nw - 1)/nw;
    for(int k0 = 0; k0 < nmine; k0 += 64)
    {
      const int stl = s0 + w + (k0 + min(lane, nmine - k0 - 1))*nw;
      const SymSub R = usub[stl];
      const int64_t ru = usub_u[stl];
      const int r_rel = R.rel, r_mb = R.nrows_d - R.wd, r_m = R.m;
      const int r_ulo = (int)(uint32_t)ru, r_uhi = (int)(ru >> 32);
      const int nb = min(64, nmine - k0);
      for(int k = 0; k < nb; k += GATHER_FLIGHT)
      {
        int relv[GATHER_FLIGHT], mbv[GATHER_FLIGHT], mv[GATHER_FLIGHT], mmax = 0;
        const double* Uv[GATHER_FLIGHT];
#pragma unroll
        for(int g = 0; g < GATHER_FLIGHT; g++)
        {
          const int kg = min(k + g, nb - 1);
          relv[g] = __builtin_amdgcn_readlane(r_rel, kg);
          mbv[g] = __builtin_amdgcn_readlane(r_mb, kg);
          mv[g] = (k + g < nb) ? __builtin_amdgcn_readlane(r_m, kg) : 0;
          Uv[g] = uscr + (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(r_uhi, kg) << 32) | (uint32_t)__builtin_amdgcn_readlane(r_ulo, kg));
          mmax = max(mmax, mv[g]);
        }
        int mv2[GATHER_FLIGHT];          // rows of the sub-block (>= 1), also its packed column stride
#pragma unroll
        for(int g = 0; g < GATHER_FLIGHT; g++) mv2[g] = max(mv[g], 1);
        for(int i0 = 0; i0 < mmax; i0 += 64)
        {
          const int i = i0 + lane;
          const int cmax = (i < nc - 1) ? i : nc - 1;
          int ig[GATHER_FLIGHT], rg[GATHER_FLIGHT];
          double v[GATHER_FLIGHT][8];
#pragma unroll
          for(int g = 0; g < GATHER_FLIGHT; g++) { ig[g] = min(i, max(mv[g], 1) - 1); rg[g] = relpos[relv[g] + ig[g]]; }
#pragma unroll
          for(int g = 0; g < GATHER_FLIGHT; g++)
#pragma unroll
            for(int c = 0; c < 8; c++)
              if(c < nc) { const int cc = min(min(c, cmax), ig[g]); v[g][c] = Uv[g][ig[g] + cc*(mv2[g] - 1) - cc*(cc - 1)/2]; }   // packed lower triangle, column cc of the sub-block
#pragma unroll
          for(int g = 0; g < GATHER_FLIGHT; g++)
#pragma unroll
            for(int c = 0; c < 8; c++)
              if(c < nc) { if(i < mv[g] && c <= cmax) acc[rg[g] + c*nrows_t] += v[g][c]; }
        }
      }
    }
  }
  if(fin_gate && tid == 0)
    for(int spins = 0; fin_seen != fin_epoch; spins++)
    {
      if(spins > (1 << 21)) { atomicOr(fin_status, DLG_HANDOFF_FACTOR); break; }       // (never in order: reported, not hung)
      __builtin_amdgcn_s_sleep(8);
      fin_seen = __hip_atomic_load(fin_gate, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    }
  __syncthreads();
  // the slab goes out eight entries per thread at a time: the reads of the panel are in flight together
  for(int e0 = tid; e0 < slab; e0 += 8*NT)
  {
    double old[8], tot[8];
#pragma unroll
    for(int u = 0; u < 8; u++) old[u] = (part < 0 && e0 + u*NT < slab) ? Lt[e0 + u*NT] : 0.0;
#pragma unroll
    for(int u = 0; u < 8; u++)
    {
      tot[u] = 0.0;
      if(e0 + u*NT < slab) for(int k = 0; k < nw; k++) tot[u] += lds[(size_t)k*slab + e0 + u*NT];
    }
#pragma unroll
    for(int u = 0; u < 8; u++)
      if(e0 + u*NT < slab) { if(part < 0) Lt[e0 + u*NT] = old[u] - tot[u]; else upart[part + e0 + u*NT] = tot[u]; }
  }
}

// fp64-MFMA variant of the update for heavy sources.  The unit's work is cut into pieces
// (sub-task, 16*UPD_TILES source rows); wave w of the nw active waves takes pieces w, w+nw, ... and
// accumulates into its private LDS slab (nrows_t x nc), so no barrier orders the pieces; the
// slabs are summed in wave order at the end.  One piece:
//   C[i][j] = sum_k Ld[i][k] * Ld[j][k],   i = the piece's source rows (MFMA row tiles of 16), j < nc <= 8
// with v_mfma_f64_16x16x4_f64: A[m][k] = Ld[row tile][4 columns], B[k][n] = Ld[n][4 columns]
// (n >= nc: zero); both operands are read straight from the source panel (column-major:
// 16 consecutive rows per column are one 128-byte segment).
constexpr int UPD_TILES = 6;          // MFMA row tiles (16 source rows each) per piece
__global__ void __launch_bounds__(TPB) k_update_mfma(int unit0, const int* __restrict__ uw_item,
                                                     const int* __restrict__ uw_s0,
                                                     const int* __restrict__ uw_s1,
                                                     const int64_t* __restrict__ uw_part,
                                                     const int* __restrict__ ui_t,
                                                     const int* __restrict__ ui_col,
                                                     const int* __restrict__ ui_nc,
                                                     const SymSub* __restrict__ usub,
                                                     const int* __restrict__ relpos,
                                                     const int* __restrict__ sn_rowptr,
                                                     const int64_t* __restrict__ sn_lx,
                                                     double* __restrict__ Lx,
                                                     double* __restrict__ upart, int nw, const int* __restrict__ info)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // (a factorisation that has broken down -- or was found doomed by the look at the diagonal, sparse_host.hip -- is not
  // worth finishing, and the panels stay what the assembly left: sparse_assemble takes them over for the next lambda)
  if(*info != 0x7fffffff) return;

  const int unit = unit0 + blockIdx.x;
  const int item = uw_item[unit];
  const int t = ui_t[item], col = ui_col[item], nc = ui_nc[item];
  const int nrows_t = sn_rowptr[t+1] - sn_rowptr[t];
  double* Lt = Lx + sn_lx[t] + (int64_t)col*nrows_t;
  const int s0 = uw_s0[unit], s1 = uw_s1[unit];
  const int64_t part = uw_part[unit];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = nrows_t*nc;
  for(int e = tid; e < slab*nw; e += TPB) lds[e] = 0.0;
  __syncthreads();
  if(w < nw)
  {
    double* acc = lds + (size_t)w*slab;
    const int jn = lane & 15, kq = lane >> 4;
    const int jc = min(jn, nc - 1);
    int piece = 0;
    for(int st = s0; st < s1; st++)
    {
      const SymSub U = usub[st];
      const double* Ld = Lx + U.src;
      const int* rel = relpos + U.rel;
      const int ld = U.nrows_d, wd = U.wd, m = U.m;
      for(int mt0 = 0; mt0 < m; mt0 += 16*UPD_TILES, piece++)
      {
        if(piece % nw != w) continue;
        const int ntile = min(UPD_TILES, (m - mt0 + 15) >> 4);
        const int relv0 = rel[min(mt0 + lane, m - 1)], relv1 = rel[min(mt0 + 64 + lane, m - 1)];
        dlg_v4d c4[UPD_TILES];
#pragma unroll
        for(int q = 0; q < UPD_TILES; q++) c4[q] = (dlg_v4d){0.0, 0.0, 0.0, 0.0};
        int ia[UPD_TILES];
        bool va[UPD_TILES];
#pragma unroll
        for(int q = 0; q < UPD_TILES; q++) { const int i = mt0 + 16*q + jn; va[q] = i < m; ia[q] = min(i, m - 1); }
        // 16 source columns (4 MFMA k-steps) per round: all loads of a round are issued before
        // its first product; rows / columns past the end are clamped and zeroed
        for(int kk = 0; kk < wd; kk += 16)
        {
          double a[4][UPD_TILES], b[4];
#pragma unroll
          for(int h = 0; h < 4; h++)
          {
            const int k = kk + 4*h + kq;
            const size_t co = (size_t)min(k, wd - 1)*ld;
            b[h] = Ld[jc + co];
#pragma unroll
            for(int q = 0; q < UPD_TILES; q++) a[h][q] = Ld[ia[q] + co];
          }
#pragma unroll
          for(int h = 0; h < 4; h++)
          {
            const bool kok = kk + 4*h + kq < wd;
            const double bv = (kok && jn < nc) ? b[h] : 0.0;
#pragma unroll
            for(int q = 0; q < UPD_TILES; q++)
              if(q < ntile) c4[q] = __builtin_amdgcn_mfma_f64_16x16x4f64((kok && va[q]) ? a[h][q] : 0.0, bv, c4[q], 0, 0, 0);
          }
        }
        // D[i'][j]: this lane holds rows i' = kq + 4r of every tile, column j = jn
#pragma unroll
        for(int q = 0; q < UPD_TILES; q++)
          if(q < ntile)
          {
#pragma unroll
            for(int r = 0; r < 4; r++)
            {
              const int il = 16*q + kq + 4*r, i = mt0 + il;
              const int rr = il < 64 ? __builtin_amdgcn_ds_bpermute(4*il, relv0) : __builtin_amdgcn_ds_bpermute(4*(il - 64), relv1);
              const int cmax = (i < nc - 1) ? i : nc - 1;
              if(i < m && jn <= cmax) acc[rr + jn*nrows_t] += c4[q][r];
            }
          }
      }
    }
  }
  __syncthreads();
  for(int e = tid; e < slab; e += TPB)
  {
    double tot = 0.0;
    for(int k = 0; k < nw; k++) tot += lds[(size_t)k*slab + e];
    if(part < 0) Lt[e] -= tot; else upart[part + e] = tot;
  }
}

// apply the updates of all source supernodes of one level to their ancestors.
// One workgroup per work unit = a chunk of the sub-tasks of one item
// (target supernode t, one var-block of its columns).  nw waves each own a
// private LDS slab (nrows_t x nc) and walk the unit's sub-tasks round-robin;
// the slabs are summed in wave order.  A single-chunk item subtracts the sum
// from the target panel; a multi-chunk item (e.g. a dense last block that every
// supernode updates) stores it as a partial slab for k_update_fin.
// nw == 0: the slab does not fit LDS; the workgroup accumulates in HBM.
__global__ void __launch_bounds__(TPB) k_update_level(int unit0, const int* __restrict__ uw_item,
                                                      const int* __restrict__ uw_s0,
                                                      const int* __restrict__ uw_s1,
                                                      const int64_t* __restrict__ uw_part,
                                                      const int* __restrict__ ui_t,
                                                      const int* __restrict__ ui_col,
                                                      const int* __restrict__ ui_nc,
                                                      const SymSub* __restrict__ usub,
                                                      const int* __restrict__ relpos,
                                                      const int* __restrict__ sn_rowptr,
                                                      const int64_t* __restrict__ sn_lx,
                                                      double* __restrict__ Lx,
                                                      double* __restrict__ upart, int nw, const int* __restrict__ info)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // (a factorisation that has broken down -- or was found doomed by the look at the diagonal, sparse_host.hip -- is not
  // worth finishing, and the panels stay what the assembly left: sparse_assemble takes them over for the next lambda)
  if(*info != 0x7fffffff) return;

  const int unit = unit0 + blockIdx.x;
  const int item = uw_item[unit];
  const int t = ui_t[item], col = ui_col[item], nc = ui_nc[item];
  const int nrows_t = sn_rowptr[t+1] - sn_rowptr[t];
  double* Lt = Lx + sn_lx[t] + (int64_t)col*nrows_t;
  const int s0 = uw_s0[unit], s1 = uw_s1[unit];
  const int64_t part = uw_part[unit];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int slab = nrows_t*nc;

  if(nw > 0)
  {
    for(int e = tid; e < slab*nw; e += TPB) lds[e] = 0.0;
    __syncthreads();
    if(w < nw && s0 + w < s1)
    {
      double* acc = lds + (size_t)w*slab;
      SymSub cur = usub[s0 + w];
      for(int st = s0 + w; st < s1; st += nw)
      {
        const SymSub U = cur;
        if(st + nw < s1) cur = usub[st + nw];          // prefetch the next record
        const double* Ld = Lx + U.src;
        const int* rel = relpos + U.rel;
        const int ld = U.nrows_d;
        for(int i = lane; i < U.m; i += 64)
        {
          const int cmax = (i < nc - 1) ? i : nc - 1;
          double sacc[8];
#pragma unroll
          for(int c = 0; c < 8; c++) sacc[c] = 0.0;
          for(int q = 0; q < U.wd; q++)
          {
            const double ai = Ld[i + (size_t)q*ld];
#pragma unroll
            for(int c = 0; c < 8; c++) if(c <= cmax) sacc[c] += ai*Ld[c + (size_t)q*ld];
          }
          const int r = rel[i];
#pragma unroll
          for(int c = 0; c < 8; c++) if(c <= cmax) acc[r + c*nrows_t] += sacc[c];
        }
      }
    }
    __syncthreads();
    for(int e = tid; e < slab; e += TPB)
    {
      double tot = 0.0;
      for(int k = 0; k < nw; k++) tot += lds[(size_t)k*slab + e];
      if(part < 0) Lt[e] -= tot; else upart[part + e] = tot;
    }
  }
  else
  {
    double* dst = (part < 0) ? Lt : upart + part;
    const double sgn = (part < 0) ? -1.0 : 1.0;
    if(part >= 0) { for(int e = tid; e < slab; e += TPB) dst[e] = 0.0; __syncthreads(); }
    for(int st = s0; st < s1; st++)
    {
      const SymSub U = usub[st];
      const double* Ld = Lx + U.src;
      const int* rel = relpos + U.rel;
      const int ld = U.nrows_d;
      for(int i = tid; i < U.m; i += TPB)
      {
        const int cmax = (i < nc - 1) ? i : nc - 1;
        const int r = rel[i];
        for(int c = 0; c <= cmax; c++)
        {
          double sacc = 0.0;
          for(int q = 0; q < U.wd; q++) sacc += Ld[i + (size_t)q*ld]*Ld[c + (size_t)q*ld];
          dst[r + c*nrows_t] += sgn*sacc;
        }
      }
      __syncthreads();
    }
  }
}
// sum the partial slabs of a multi-chunk item and apply them.  grid.y workgroups share the
// elements of a slab in chunks of E; within a workgroup the partials are dealt to G = 256/E
// thread groups, each keeping four loads in flight.  The summation order is fixed by (G, n)
// alone, so the result is deterministic.
__global__ void __launch_bounds__(TPB) k_update_fin(int f0, const int* __restrict__ uf_item,
                                                    const int* __restrict__ uf_n,
                                                    const int64_t* __restrict__ uf_off,
                                                    const int* __restrict__ ui_t,
                                                    const int* __restrict__ ui_col,
                                                    const int* __restrict__ ui_nc,
                                                    const int* __restrict__ sn_rowptr,
                                                    const int64_t* __restrict__ sn_lx,
                                                    double* __restrict__ Lx,
                                                    const double* __restrict__ upart, const int* __restrict__ info)
{
  __shared__ double sh[TPB];
  // (a factorisation that has broken down -- or was found doomed by the look at the diagonal, sparse_host.hip -- is not
  // worth finishing, and the panels stay what the assembly left: sparse_assemble takes them over for the next lambda)
  if(*info != 0x7fffffff) return;

  const int f = f0 + blockIdx.x;
  const int item = uf_item[f], n = uf_n[f];
  const int t = ui_t[item], col = ui_col[item], nc = ui_nc[item];
  const int nrows_t = sn_rowptr[t+1] - sn_rowptr[t];
  double* Lt = Lx + sn_lx[t] + (int64_t)col*nrows_t;
  const int slab = nrows_t*nc;
  const double* src = upart + uf_off[f];
  const int E = (slab >= 32) ? 32 : 8;
  const int G = TPB/E;
  const int el = threadIdx.x % E, g = threadIdx.x / E;
  for(int ebase = blockIdx.y*E; ebase < slab; ebase += gridDim.y*E)
  {
    const int e = ebase + el;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
    if(e < slab)
    {
      const double* q = src + e;
      int k = g;
      for(; k + 3*G < n; k += 4*G)
      {
        t0 += q[(size_t)k*slab];         t1 += q[(size_t)(k + G)*slab];
        t2 += q[(size_t)(k + 2*G)*slab]; t3 += q[(size_t)(k + 3*G)*slab];
      }
      for(; k < n; k += G) t0 += q[(size_t)k*slab];
    }
    __syncthreads();
    sh[threadIdx.x] = (t0 + t1) + (t2 + t3);
    __syncthreads();
    if(g == 0 && e < slab)
    {
      double sacc = 0.0;
      for(int k = 0; k < G; k++) sacc += sh[k*E + el];
      Lt[e] -= sacc;
    }
  }
}

} // namespace

// the one dispatch over the instantiations of k_factor_level (leaf: the lean one, 256 threads only; the compiler
// lays the kernels out in the order they are first named: <256> in front of <256, true>)
static void launch_factor_level(int nt, bool leaf, int grid, int lds, hipStream_t st, const SparseSym* Y, const FwItem* items,
                                const MfChild* rec, const uint16_t* dst, int fmode, int* fl, int ep, DlgHandoff ho, int64_t pacc,
                                double* leaf_rd = nullptr)
{
#define DLG_FL_LAUNCH(...) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_factor_level<__VA_ARGS__>), dim3(grid), dim3(nt), lds, st, \
                                              items, rec, Y->sn_bd_col, dst, Y->Lx, Y->top_scr, Y->d_info, Y->uscr, fmode, fl, ep, ho, pacc, leaf_rd)
  if(nt == 128) DLG_FL_LAUNCH(128);
  else if(nt == 256 && !leaf) DLG_FL_LAUNCH(256);
  else if(nt == 256) DLG_FL_LAUNCH(256, true);
  else { nt = 512; DLG_FL_LAUNCH(512); }
#undef DLG_FL_LAUNCH
}
constexpr int FMODE_B16 = 16;      // panel_factor_b16 where the panel has at most 512 rows: every launch asks for it
constexpr int FMODE_LEAN_ROWS = 32;      // a level of merged leaves: the rows below the member blocks stay the assembly's (k_factor_level: lean_rows)

// the levels of region R, the first of which is l, in one launch (its epoch is the caller's: ++R.epoch)
static void launch_region(dlg_backend* b, const PrRegion& R, int l)
{
  SparseSym* Y = b->sym;
  const int fmode = 2 + 4*R.stage + FMODE_B16 + 256*(l & 31);
  const int64_t pacc = Y->pr_acc ? (int64_t)(Y->pr_acc - Y->uscr) : 0;
  launch_factor_level(Y->fac.nt[l], false, R.nwg, R.lds, b->stream, Y, R.item, R.rec, R.dst, fmode, R.flag, R.epoch,
                      dlg_handoff(b, 1 << 21), pacc);
}

// a region's schedule on the device (R.level0 >= H.nlevels: there is none)
static int region_upload(dlg_backend* b, PrRegion& R, const RegionPlan& P)
{
  SparseSym* Y = b->sym;
  R.level0 = P.level0; R.level1 = P.level1; R.lds = P.lds; R.stage = P.stage; R.nwg = P.nwg;
  if(P.level0 >= Y->H.nlevels) return DLG_OK;
  if(!R.item) { DLG_CHECK(upload(R.item, P.item)); Y->allocs.push_back(R.item); }
  if(!R.rec)  { DLG_CHECK(upload(R.rec, P.rec));   Y->allocs.push_back(R.rec); }
  if(!R.dst)  { DLG_CHECK(upload(R.dst, P.dst));   Y->allocs.push_back(R.dst); }
  return DLG_OK;
}
// ... and its flags: one per workgroup of the region + the fork gate
static int region_flags(dlg_backend* b, PrRegion& R)
{
  SparseSym* Y = b->sym;
  if(R.level0 >= Y->H.nlevels || R.flag) return DLG_OK;
  DLG_HIP(hipMalloc(&R.flag, sizeof(int)*((size_t)R.nwg + 1)));
  Y->allocs.push_back(R.flag);
  DLG_HIP(hipMemsetAsync(R.flag, 0, sizeof(int)*((size_t)R.nwg + 1), b->stream));
  R.epoch = 0;
  return DLG_OK;
}

// launch parameters of K5: the plan (sparse_region.cpp) and what it needs on the device
int sparse_factor_setup(dlg_backend* b)
{
  SparseSym* Y = b->sym;
  const SymHost& H = Y->H;
  const RegionKnobs K = region_knobs_env(b->ncu);
  char err[256];
  if(fac_level_params(H, Y->fac, err, sizeof(err))) { dlg_set_error("%s", err); return DLG_ERR_ARG; }
  if(!Y->uw_flat && !H.uw_item.empty())
  {
    std::vector<GatherUnit> fl(H.uw_item.size());
    for(size_t u = 0; u < fl.size(); u++)
    {
      const int item = H.uw_item[u], t = H.ui_t[item];
      const int nr = H.sn_rowptr[t+1] - H.sn_rowptr[t];
      fl[u] = GatherUnit{ H.sn_lx[t] + (int64_t)H.ui_col[item]*nr, H.uw_part[u], H.uw_s0[u], H.uw_s1[u], nr, H.ui_nc[item] };
    }
    DLG_CHECK(upload(Y->uw_flat, fl)); Y->allocs.push_back(Y->uw_flat);
  }
  // A subtree partition has TWO regions: the rank's own levels up to the cut (lo: a cut that leaves at least two multifrontal
  // levels below it) and, behind the sum over the ranks, the replicated levels above it (top, as on one rank).
  const bool part = H.part_nranks > 1;
  const RegionPlan top = region_plan(H, Y->fac, part ? H.cut_level + 1 : 1, H.nlevels - 1, K);
  DLG_CHECK(region_upload(b, Y->top, top));
  bool acc_any = top.acc_any;
  Y->lo.level0 = H.nlevels;
  if(part && H.cut_level >= 2 && K.lower)
  {
    const RegionPlan lo = region_plan(H, Y->fac, 1, H.cut_level, K);
    DLG_CHECK(region_upload(b, Y->lo, lo));
    acc_any = acc_any || lo.acc_any;
  }
  // update matrices of a region that do not fit LDS are summed (atomics) in a shadow of the scratch,
  // so that the slot the parent reads only ever sees write-through stores
  if(acc_any && !Y->pr_acc)
  {
    DLG_HIP(hipMalloc(&Y->pr_acc, sizeof(double)*(size_t)std::max<int64_t>(1, H.uscr_size)));
    Y->allocs.push_back(Y->pr_acc);
  }
  DLG_CHECK(region_flags(b, Y->top));
  DLG_CHECK(region_flags(b, Y->lo));
  // The levels whose leaf launch may leave the rows below the member blocks as the assembly wrote them: the lean
  // instantiation, launched on its own (not inside a region), and nothing of the level's updates reads those rows from the
  // panel -- the update matrices come out of the launch's LDS copy (syrk_fused) or there are none.
  // DOGLEG_AMD_LEAF_STORE_ROWS=1: no level does (the write-back of all rows, for A/B runs and the tests).
  // (sparse_solve_setup, which runs behind this, takes a level back whose backward launch could not honour it)
  const bool store_rows = env_int("DOGLEG_AMD_LEAF_STORE_ROWS", 0) != 0, sym_debug = getenv("DOGLEG_AMD_SYM_DEBUG") != nullptr;
  Y->leaf_lean.assign(H.nlevels, 0);
  for(int l = 0; l < H.nlevels && !store_rows; l++)
  {
    const bool own_launch = l < Y->top.level0 && !(l >= Y->lo.level0 && l <= Y->lo.level1);
    const int nu = H.uw_lvl_ptr[l+1] - H.uw_lvl_ptr[l];
    const bool rows_unread = nu == 0 || (H.upd_syrk[l] && Y->fac.upd_nw[l] > 0 && Y->fac.syrk_fused[l]);
    Y->leaf_lean[l] = (Y->fac.leaf[l] && own_launch && rows_unread) ? 1 : 0;
    if(sym_debug) fprintf(stderr, "factor level %d: lean leaf rows %d\n", l, (int)Y->leaf_lean[l]);
  }
  if(!Y->leaf_rd) { DLG_HIP(hipMalloc(&Y->leaf_rd, sizeof(double)*2*(size_t)std::max(1, H.N))); Y->allocs.push_back(Y->leaf_rd); }
  Y->leaf_rows.reset();
  // the kernels that ask for more dynamic LDS than the default: the first four the factor budget, the rest the common one
  const void* const big_lds[] = { (const void*)&k_factor_level<128>, (const void*)&k_factor_level<256>, (const void*)&k_factor_level<256, true>,
                                  (const void*)&k_factor_level<512>, (const void*)&k_leaf_rows_materialize<256>, (const void*)&k_update_level, (const void*)&k_update_syrk<256>,
                                  (const void*)&k_update_syrk<1024>, (const void*)&k_update_gather<TPB>, (const void*)&k_update_mfma };
  for(int i = 0; i < 10; i++) DLG_HIP(hipFuncSetAttribute(big_lds[i], hipFuncAttributeMaxDynamicSharedMemorySize, i < 5 ? FAC_LDS_BUDGET : LDS_BUDGET));
  return DLG_OK;
}

#ifdef DLG_FL_PROFILE
// per level: the workgroup that finishes last (its phases) and the mean over the recorded workgroups
extern "C" void dlg_fl_profile_dump(int nlevels)
{
  std::vector<long long> h(32*FL_PROF_WG*8);
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_fl_prof), sizeof(long long)*h.size());
  for(int l = 0; l < nlevels && l < 32; l++)
  {
    int nwg = 0, last = -1; long long t0 = 0, tend = 0; double mean[5] = {0, 0, 0, 0, 0};
    for(int g = 0; g < FL_PROF_WG; g++)
    {
      const long long* q = &h[(l*FL_PROF_WG + g)*8];
      if(q[5] == 0) continue;
      nwg++;
      if(t0 == 0 || q[0] < t0) t0 = q[0];
      if(q[5] > tend) { tend = q[5]; last = g; }
      for(int k = 0; k < 5; k++) mean[k] += (double)(q[k+1] - q[k]);
    }
    if(nwg == 0) continue;
    // a persistent launch: the timeline of its last workgroups (the top of the tree), 10 ns units
    for(int g = FL_PROF_WG - 1, shown = 0; g >= 0 && shown < (getenv("DLG_FL_DUMP_ALL") ? FL_PROF_WG : 20); g--)
    {
      const long long* q = &h[(l*FL_PROF_WG + g)*8];
      if(q[5] == 0 || q[7] == 0) continue;
      shown++;
      {
        std::vector<long long> ha(FL_PROF_WG*4);
        static bool got = false; static std::vector<long long> hadd;
        if(!got) { hadd.resize(FL_PROF_WG*4); hipMemcpyFromSymbol(hadd.data(), HIP_SYMBOL(g_fl_add), sizeof(long long)*hadd.size()); got = true; }
        if(hadd[g*4 + 0]) fprintf(stderr, "   add %3d: child0 seen %6lld child0 added %6lld last child seen %6lld dbg %lld\n", g, hadd[g*4] - t0, hadd[g*4 + 1] - t0, hadd[g*4 + 2] - t0, hadd[g*4 + 3]);
      }
      fprintf(stderr, "   wg %3d (w %3lld rows %4lld nch %lld u_lds %lld lvl %lld rep %lld): start %6lld flag up %6lld panel in %6lld added %6lld factored %6lld tail %6lld flag+stored %6lld\n",
              g, q[6] & 4095, (q[6] >> 12) & 4095, (q[6] >> 24) & 4095, (q[6] >> 36) & 1, (q[6] >> 56) & 63, (q[6] >> 52) & 15, q[0] - t0, q[7] - t0, q[1] - t0, q[2] - t0, q[3] - t0, q[4] - t0, q[5] - t0);
    }
    const long long* q = &h[(l*FL_PROF_WG + last)*8];
    fprintf(stderr, "level %2d: %3d wg, span %7lld | last wg %3d (w %3lld rows %4lld slice %4lld nch %2lld u_lds %lld has_u %lld): start +%6lld load %6lld add %6lld factor %6lld tail %6lld store %6lld | mean: load %6.0f add %6.0f factor %6.0f tail %6.0f store %6.0f\n",
            l, nwg, tend - t0, last, q[6] & 4095, (q[6] >> 12) & 4095, (q[6] >> 40) & 4095, (q[6] >> 24) & 4095, (q[6] >> 36) & 1, (q[6] >> 37) & 1,
            q[0] - t0, q[1] - q[0], q[2] - q[1], q[3] - q[2], q[4] - q[3], q[5] - q[4],
            mean[0]/nwg, mean[1]/nwg, mean[2]/nwg, mean[3]/nwg, mean[4]/nwg);
  }
  std::vector<long long> z(h.size(), 0);
  hipMemcpyToSymbol(HIP_SYMBOL(g_fl_prof), z.data(), sizeof(long long)*z.size());
}
#endif
// K5: level-scheduled supernodal Cholesky (launches only; the caller reads the pivot flag)
int sparse_factor_levels(dlg_backend* b, int part)
{
  SparseSym* Y = b->sym;
  const SymHost& H = Y->H;
  hipStream_t st = b->stream;
  // A factorisation enqueued ahead of the caller's decision (step.hip, step_prepare) comes in two parts where its
  // first launch is a level of its own: part 1 = that launch (the leaf level), part 2 = everything behind it.  Same
  // launches in the same order on the same stream as part 0.
  const bool split = Y->top.level0 > 0 && H.nlevels >= 2 && H.part_nranks <= 1 && H.fw_lvl_ptr[1] > H.fw_lvl_ptr[0];
  if(part == 2 && !split) return DLG_OK;
  if(part != 2)
  {
  if(H.part_nranks > 1 && H.cut_level < 0) DLG_CHECK(sparse_partition_reduce(b));     // nothing below the cut
  // (fin on the side, sparse_assemble.hip: the partial-sum stages of the ancestors' panels may still be on the second
  // stream -- level 0 does not touch those panels; whatever follows it does)
  if(Y->top.level0 == 0 || H.nlevels < 2) DLG_CHECK(sparse_fin_side_gate(b));
  }
  for(int l = 0; l < H.nlevels; l++)
  {
    const bool launched_before = part == 2 && l == 0;      // (the level's factor launch is on the stream: part 1)

    const int n = H.fw_lvl_ptr[l+1] - H.fw_lvl_ptr[l];
    // from the first level that cannot fill the chip on, the factorisation is latency-bound:
    // independent work (the Cauchy step's pass over J) may run beside it
    const bool gate_here = (l == Y->top.level0 && Y->top.flag) || (l == Y->lo.level0 && Y->lo.flag);      // (no event on this stream: the launch opens a gate)
    if(l > 0 && n < 256 && !gate_here) dlg_fork_point(b);
    if(l == Y->lo.level0 && Y->lo.flag)
    {
      // a subtree partition: the rank's own levels up to the cut in one launch (sparse_factor_setup, region "lo")
      PrRegion& R = Y->lo;
      ++R.epoch;
      if(l > 0 && n < 256) dlg_fork_gate(b, R.flag + R.nwg, R.epoch);
      {
        DlgRegionTurn turn(b);            // (held for the launch only: the sum over the ranks behind it blocks in the caller's hook)
        launch_region(b, R, l);
      }
      l = R.level1;                                 // (= the cut: everything below it is done)
      if(H.part_nranks > 1 && l == H.cut_level) { DLG_LAUNCH_CHECK(); DLG_CHECK(sparse_partition_reduce(b)); }
      continue;
    }
    if(l == Y->top.level0)
    {
      // the persistent top region: every remaining level in one launch (sparse_factor_setup)
      PrRegion& R = Y->top;
      ++R.epoch;
      // (the gate goes up with the region's LAST workgroup -- the top of the tree, on the chip once the populous levels below
      // it have drained --, however many supernodes the region's first level has: with `n < 256` asked for here too, config #5
      // -- 285 supernodes on level 1 -- never forked, and its Cauchy pass ran beside the backward solve instead)
      if(gate_here && l > 0) dlg_fork_gate(b, R.flag + R.nwg, R.epoch);
      DlgRegionTurn turn(b);
      launch_region(b, R, l);
      break;
    }
    if(n > 0 && !launched_before)
    {
      // (a level of merged leaves that may keep its rows below as the assembly's: the buffer's state says so from here on,
      // whatever becomes of this factorisation -- a workgroup that gives up has not touched its rows either)
      const int rd_slot = Y->leaf_lean[l] ? Y->leaf_rows.slot(Y->Lx) : -1;
      const bool lean = rd_slot >= 0;
      const int fmode = ((l >= H.mf_level0) ? 2 : Y->fac.syrk_fused[l]) + 4*Y->fac.stage[l] + FMODE_B16 + (lean ? FMODE_LEAN_ROWS : 0) + 256*(l & 31);
      launch_factor_level(Y->fac.nt[l], Y->fac.leaf[l], n, Y->fac.lds[l], st, Y, Y->fw_item + H.fw_lvl_ptr[l], Y->mf_rec, Y->mf_dst,
                          fmode, (int*)nullptr, 0, DlgHandoff{nullptr, 0, 0}, (int64_t)0, lean ? Y->leaf_rd + (size_t)rd_slot*H.N : (double*)nullptr);
      if(lean) Y->leaf_rows.factored_lean(Y->Lx);
      else if(Y->fac.leaf[l]) Y->leaf_rows.factored_full(Y->Lx);
    }
    if(part == 1 && split && l == 0) { Y->fac_pending = true; DLG_LAUNCH_CHECK(); return DLG_OK; }
    // (behind the leaf level's factor kernel, in front of its updates: the gather kernel looks at the word itself,
    // in front of anything else a one-wave kernel waits for it)
    const int nu = H.uw_lvl_ptr[l+1] - H.uw_lvl_ptr[l];
    const bool gather_next = nu > 0 && H.upd_syrk[l] && Y->fac.upd_nw[l] > 0;
    const int fin_ep = (l == 0 && gather_next) ? Y->fin_side_owed : 0;
    if(fin_ep) Y->fin_side_owed = 0;
    if(l == 0) DLG_CHECK(sparse_fin_side_gate(b));
    if(gather_next)
    {
      const int ns = H.xl_ptr[l+1] - H.xl_ptr[l];
      if(Y->fac.syrk_fused[l] || ns == 0) { /* phase 1 was done by the factor kernel */ }
      else if(Y->fac.syrk_nt[l] == 256)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_syrk<256>), dim3(ns), dim3(256), Y->fac.syrk_lds[l], st,
                           Y->xl_sn + H.xl_ptr[l], Y->sn_c0, Y->sn_rowptr, Y->sn_lx, Y->u_off, Y->Lx, Y->uscr,
                           Y->fac.syrk_kc[l]);
      else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_syrk<1024>), dim3(ns), dim3(1024), Y->fac.syrk_lds[l], st,
                           Y->xl_sn + H.xl_ptr[l], Y->sn_c0, Y->sn_rowptr, Y->sn_lx, Y->u_off, Y->Lx, Y->uscr,
                           Y->fac.syrk_kc[l]);
      // (one wave per unit, all units resident at once, was measured: 78 us against 48 with up to four
      // waves sharing a unit's sub-tasks)
      hipLaunchKernelGGL(HIP_KERNEL_NAME(k_update_gather<TPB>), dim3(nu), dim3(TPB), Y->fac.upd_lds[l], st, H.uw_lvl_ptr[l],
                         Y->uw_flat, Y->usub, Y->usub_u, Y->relpos, Y->Lx, Y->upart, Y->uscr,
                         Y->fac.upd_nw[l], Y->d_info,
                         fin_ep ? (const int*)(Y->fin_flag + 1) : (const int*)nullptr, fin_ep,
                         reinterpret_cast<int*>(b->d_scal + (dlg_backend::NSCAL - 2)));
    }
    else if(nu > 0 && Y->fac.upd_coop[l] == 2)
      hipLaunchKernelGGL(k_update_mfma, dim3(nu), dim3(TPB), Y->fac.upd_lds[l], st, H.uw_lvl_ptr[l],
                         Y->uw_item, Y->uw_s0, Y->uw_s1, Y->uw_part, Y->ui_t, Y->ui_col, Y->ui_nc,
                         Y->usub, Y->relpos, Y->sn_rowptr, Y->sn_lx, Y->Lx, Y->upart, Y->fac.upd_nw[l], (const int*)Y->d_info);
    else if(nu > 0 && Y->fac.upd_coop[l])
      hipLaunchKernelGGL(k_update_coop, dim3(nu), dim3(TPB), 0, st, H.uw_lvl_ptr[l],
                         Y->uw_item, Y->uw_s0, Y->uw_s1, Y->uw_part, Y->ui_t, Y->ui_col, Y->ui_nc,
                         Y->usub, Y->relpos, Y->sn_rowptr, Y->sn_lx, Y->Lx, Y->upart, (const int*)Y->d_info);
    else if(nu > 0)
      hipLaunchKernelGGL(k_update_level, dim3(nu), dim3(TPB), Y->fac.upd_lds[l], st, H.uw_lvl_ptr[l],
                         Y->uw_item, Y->uw_s0, Y->uw_s1, Y->uw_part, Y->ui_t, Y->ui_col, Y->ui_nc,
                         Y->usub, Y->relpos, Y->sn_rowptr, Y->sn_lx, Y->Lx, Y->upart, Y->fac.upd_nw[l], (const int*)Y->d_info);
    const int nfz = H.uf_lvl_ptr[l+1] - H.uf_lvl_ptr[l];
    if(nfz > 0)
      hipLaunchKernelGGL(k_update_fin, dim3(nfz, Y->fac.fin_ny[l]), dim3(TPB), 0, st, H.uf_lvl_ptr[l], Y->uf_item, Y->uf_n,
                         Y->uf_off, Y->ui_t, Y->ui_col, Y->ui_nc, Y->sn_rowptr, Y->sn_lx, Y->Lx,
                         Y->upart, (const int*)Y->d_info);
    // subtree partition: everything below the cut is done -- the sum over the ranks, then the replicated top
    if(H.part_nranks > 1 && l == H.cut_level) { DLG_LAUNCH_CHECK(); DLG_CHECK(sparse_partition_reduce(b)); }
  }
  if(!H.ms_sn.empty())
    hipLaunchKernelGGL(k_copy_top, dim3((unsigned)H.ms_sn.size()), dim3(TPB), 0, st, Y->ms_sn, Y->sn_c0,
                       Y->sn_rowptr, Y->sn_lx, Y->sn_top, Y->Lx, Y->top_scr, (const int*)Y->d_info);
  DLG_LAUNCH_CHECK();
  return DLG_OK;
}

// The readers of the merged leaves' L_below other than the backward solve are behind this: dlg_factor_user_begin calls it for
// the blocked solves, the reach sweeps and the selected inverse, sparse_solve for the forward solve of another right-hand side: where the current factor's leaf launch
// ran lean, L_below is stored over W now, on the backend's stream, once (the buffer's state says when: leaf_rows_state.h).
int sparse_leaf_rows_materialize(dlg_backend* b)
{
  SparseSym* Y = b->sym;
  if(!Y || !Y->Lx || !Y->leaf_rows.raw(Y->Lx)) return DLG_OK;
  const SymHost& H = Y->H;
  const int slot = Y->leaf_rows.slot(Y->Lx);
  for(int l = 0; l < H.nlevels; l++)
  {
    const int n = H.fw_lvl_ptr[l+1] - H.fw_lvl_ptr[l];
    if(!Y->leaf_lean[l] || n == 0) continue;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_leaf_rows_materialize<256>), dim3(n), dim3(256), Y->fac.lds[l], b->stream,
                       Y->fw_item + H.fw_lvl_ptr[l], Y->Lx, Y->leaf_rd + (size_t)slot*H.N, (const int*)Y->d_info);
  }
  DLG_LAUNCH_CHECK();
  Y->leaf_rows.materialize(Y->Lx);
  return DLG_OK;
}
// {lean leaf launches, materialisations, 1 if the current factor's leaf rows are the assembly's still, levels that may run lean}
extern "C" int dlg_sparse_leaf_rows_stats(dlg_backend_t* b, long* stats, int nstats)
{
  if(!b || !b->sym || !stats) { dlg_set_error("no symbolic analysis yet"); return DLG_ERR_STATE; }
  const SparseSym* Y = b->sym;
  long lean = 0;
  for(char c : Y->leaf_lean) lean += c;
  const long v[] = { Y->leaf_rows.lean_launches, Y->leaf_rows.materialized, Y->leaf_rows.raw(Y->Lx) ? 1L : 0L, lean };
  for(int i = 0; i < nstats && i < 4; i++) stats[i] = v[i];
  return DLG_OK;
}

// Host only (no GPU): the plan of the one-launch region for a pattern as a chip with `ncu` compute units would get it,
// checked (region_check); stats as include/dlg_backend.h lists them.  DLG_ERR_STATE with a message on a violation.
extern "C" int dlg_sparse_region_probe(int N, int M, const int* colptr, const int* rowidx, int ncu, long* stats, int nstats)
{
  SymHost H;
  char err[512];
  if(sym_analyze(H, N, M, colptr, rowidx, 0, M, err, sizeof(err))) { dlg_set_error("symbolic analysis: %s", err); return DLG_ERR_ARG; }
  const RegionKnobs K = region_knobs_env(ncu);
  FacLevels L;
  if(fac_level_params(H, L, err, sizeof(err))) { dlg_set_error("%s", err); return DLG_ERR_ARG; }
  const RegionPlan R = region_plan(H, L, 1, H.nlevels - 1, K);
  long checked[2];
  if(region_check(H, R, checked, err, sizeof(err))) { dlg_set_error("%s", err); return DLG_ERR_STATE; }
  const long v[] = { (long)R.level0, (long)(H.fw_lvl_ptr[H.nlevels] - H.fw_lvl_ptr[std::min(R.level0, H.nlevels)]),
                     (long)R.nwg, (long)R.lds, checked[0], checked[1], (long)region_plan_hash(R), (long)fac_levels_hash(L) };
  for(int i = 0; i < nstats && i < 8; i++) stats[i] = v[i];
  return DLG_OK;
}
