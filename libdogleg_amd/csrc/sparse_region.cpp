// sparse_region.cpp -- see sparse_region.h.  Pure host code (no HIP).
#include "sparse_region.h"
#include "fnv.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace {
constexpr int FAC_LDS = SYM_FAC_LDS_BUDGET;
// doubles of a panel of `rows` rows and w columns in LDS: even leading dimension; unsliced block-diagonal tops
// (merged leaves, cmp) use the compact layout that never stages the top block (k_factor_level: cmp)
long panel_doubles(long w, long rows, bool cmp, bool leaf)
{
  return cmp ? ((rows - w + 1) & ~1L)*w + (leaf ? 4 : 8)*w : ((rows + 1) & ~1L)*w;
}

// T tile columns (tile counts T - t) in at most `want` contiguous shares, the largest share as small as
// possible: share r is [cut[r], cut[r+1])
std::vector<int> cut_tile_columns(int T, int want)
{
  std::vector<int> cut;
  for(int cap = (T*(T + 1)/2 + want - 1)/std::max(want, 1); ; cap++)
  {
    cut.assign(1, 0);
    int load = 0;
    for(int t = 0; t < T; t++)
    {
      if(load > 0 && load + (T - t) > cap) { cut.push_back(t); load = 0; }
      load += T - t;
    }
    cut.push_back(T);
    if((int)cut.size() - 1 <= want) break;
  }
  return cut;
}

// a child's record as the region's launch reads it: the first workgroup of the child | its replicas << 20
int child_workgroups(int rsv, const std::vector<int>& first, const std::vector<int>& count)
{
  return (rsv >= 0 && first[rsv] >= 0) ? (first[rsv] | (count[rsv] << 20)) : -1;
}

// The children records and destination lists of a replica that owns the columns [jA, jB) of its update matrix:
// a panel entry goes to the panel, entry (jw + df, jw) of an owned column to own(jw, df), everything else
// (and the padding) to `drop`.  Returns the replica's ch0.
template <class OwnF>
int write_children(const SymHost& H, const FwItem& it, long jA, long jB, long drop, OwnF own, const std::vector<int>& first,
                   const std::vector<int>& count, std::vector<MfChild>& rec, std::vector<uint16_t>& dst)
{
  const long ldp = (it.nrows + 1) & ~1L;
  const int ch0_new = (int)rec.size();
  for(int k = 0; k < it.nch; k++)
  {
    MfChild rc = H.mf_rec[it.ch0 + k];
    const int c = H.mf_child[it.ch0 + k];
    const int mc = (H.sn_rowptr[c+1] - H.sn_rowptr[c]) - (H.sn_c0[c+1] - H.sn_c0[c]);
    const int* map = &H.relpos[H.sn_prel[c]];
    const int nc = mc*(mc + 1)/2;
    rc.dst_off = (int64_t)dst.size();
    rc.rsv = child_workgroups(rc.rsv, first, count);
    dst.reserve(dst.size() + rc.npad);
    for(int j = 0; j < mc; j++)
      for(int q = j; q < mc; q++)
      {
        const long fi = map[q], fj = map[j], jw = fj - it.w;
        const long d = (fj < it.w) ? fi + fj*ldp : (jw >= jA && jw < jB) ? own(jw, fi - fj) : drop;
        dst.push_back((uint16_t)d);
      }
    for(int e = nc; e < rc.npad; e++) dst.push_back((uint16_t)drop);
    rec.push_back(rc);
  }
  return ch0_new;
}

} // namespace

RegionKnobs region_knobs_env(int ncu)
{
  RegionKnobs K;
  K.ncu = ncu;
  // (the cap counts SUPERNODES, five times the CUs: with replicas a region holds more workgroups than the chip has CUs
  // anyway.  The backward solve keeps twice the CUs: its region runs from the root DOWN, the populous levels last.)
  K.cap = env_int("DOGLEG_AMD_PERSIST_MAX", 5*ncu);
  K.rmax = std::max(1, std::min(8, env_int("DOGLEG_AMD_FRONT_REPLICAS", 8)));
  K.slices = !getenv("DOGLEG_AMD_NO_FRONT_SLICES"); K.persist = !getenv("DOGLEG_AMD_NO_PERSIST");
  K.lower = !getenv("DOGLEG_AMD_NO_LOWER_REGION"); K.timing = getenv("DOGLEG_AMD_TIMING") != nullptr;
  return K;
}

int fac_level_params(const SymHost& H, FacLevels& L, char* err, size_t len)
{
  for(auto* v : {&L.lds, &L.leaf, &L.stage, &L.upd_coop, &L.upd_lds, &L.upd_nw, &L.syrk_lds, &L.syrk_fused}) v->assign(H.nlevels, 0);
  L.nt.assign(H.nlevels, 512); L.syrk_nt.assign(H.nlevels, 256); L.syrk_kc.assign(H.nlevels, 4); L.fin_ny.assign(H.nlevels, 1);
  const bool leaf_kernel = !getenv("DOGLEG_AMD_NO_LEAF_KERNEL"), debug = getenv("DOGLEG_AMD_SYM_DEBUG") != nullptr;
  for(int l = 0; l < H.nlevels; l++)
  {
    long maxp = 0, maxw = 0, maxr = 0;
    for(int i = H.lvl_ptr[l]; i < H.lvl_ptr[l+1]; i++) maxw = std::max(maxw, (long)(H.sn_c0[H.lvl_sn[i]+1] - H.sn_c0[H.lvl_sn[i]]));
    // all work items unsliced block-diagonal panels (merged leaves) outside the multifrontal region, members of at most 4
    // columns, at most 64 columns in all, and 256 threads: the lean instantiation (k_factor_level<256, true>)
    bool all = leaf_kernel && H.fw_lvl_ptr[l+1] > H.fw_lvl_ptr[l] && l < H.mf_level0;
    for(int i = H.fw_lvl_ptr[l]; i < H.fw_lvl_ptr[l+1]; i++)
    {
      const FwItem& it = H.fw_item[i];
      if(!(it.nbd > 0 && it.top < 0 && it.bdw > 0 && it.bdw <= 4 && it.w <= 64)) all = false;
      maxr = std::max(maxr, (long)it.w + (it.r1 - it.r0));
    }
    L.nt[l] = (maxr <= 128) ? 128 : (maxr <= 256 ? 256 : 512);
    L.leaf[l] = (all && L.nt[l] == 256) ? 1 : 0;
    for(int i = H.fw_lvl_ptr[l]; i < H.fw_lvl_ptr[l+1]; i++)
    {
      const int s = H.fw_sn[i];
      const long wv = H.sn_c0[s+1] - H.sn_c0[s];
      const long nloc = wv + (H.fw_r1[i] - H.fw_r0[i]);
      const bool cmp = H.sn_bd_ptr[s+1] > H.sn_bd_ptr[s] && H.sn_top[s] < 0;
      const long p = panel_doubles(wv, nloc, cmp, L.leaf[l]) + (cmp ? 1 : 0);
      if(p > maxp) maxp = p;
    }
    if(l >= H.mf_level0) L.nt[l] = env_int("DOGLEG_AMD_MF_NT", 512);
    L.upd_coop[l] = (maxw > 8) ? 1 : 0;           // heavy sources: matrix-core / cooperative update kernels
    if(maxp*8 > FAC_LDS) { snprintf(err, len, "internal error: a factor slice does not fit LDS (%ld doubles)", maxp); return 1; }
    L.lds[l] = (int)(maxp*8);
    long maxslab = 0;
    for(int it = H.ui_lvl_ptr[l]; it < H.ui_lvl_ptr[l+1]; it++)
      maxslab = std::max(maxslab, (long)(H.sn_rowptr[H.ui_t[it]+1] - H.sn_rowptr[H.ui_t[it]])*H.ui_nc[it]);
    long finslab = 0;
    for(int f = H.uf_lvl_ptr[l]; f < H.uf_lvl_ptr[l+1]; f++)
      finslab = std::max(finslab, (long)(H.sn_rowptr[H.ui_t[H.uf_item[f]]+1] - H.sn_rowptr[H.ui_t[H.uf_item[f]]])*H.ui_nc[H.uf_item[f]]);
    L.fin_ny[l] = (int)std::min(64L, std::max(1L, (finslab + 31)/32));
    int nw = 0;
    if(maxslab > 0) { nw = (int)((long)SYM_LDS_BUDGET/(maxslab*8)); if(nw > 4) nw = 4; }
    L.upd_nw[l] = nw;
    L.upd_lds[l] = (int)(maxslab*8*nw);
    // heavy sources: 2 = matrix-core update kernel (needs the target slabs in LDS), 1 = cooperative
    // kernel accumulating in HBM (also selectable with DOGLEG_AMD_NO_UPDATE_MFMA for testing)
    if(L.upd_coop[l] && nw > 0 && !getenv("DOGLEG_AMD_NO_UPDATE_MFMA")) L.upd_coop[l] = 2;
    if(H.upd_syrk[l])
    {
      long ldbmax = 0, k4max = 0, tmax = 0;
      for(int i = H.lvl_ptr[l]; i < H.lvl_ptr[l+1]; i++)
      {
        const int d = H.lvl_sn[i];
        const long wd = H.sn_c0[d+1] - H.sn_c0[d], mb = H.sn_rowptr[d+1] - H.sn_rowptr[d] - wd;
        ldbmax = std::max(ldbmax, ((mb + 31)/32)*32 + 16); k4max = std::max(k4max, (wd + 3)/4*4);
        tmax = std::max(tmax, (mb + 15)/16);
      }
      long kc = (65536/(ldbmax*8)) & ~3L;            // source columns staged per round (<= 64 KB of LDS)
      if(kc > k4max) kc = k4max;
      L.syrk_kc[l] = (int)kc;
      L.syrk_lds[l] = (int)(kc*ldbmax*8);
      L.syrk_nt[l] = (tmax*(tmax + 1)/2 <= 32) ? 256 : 1024;
      // no supernode of the level is cut into slices: the factor kernel forms the U_d itself
      bool unsliced = true;
      for(int i = H.lvl_ptr[l]; i < H.lvl_ptr[l+1]; i++) if(H.sn_top[H.lvl_sn[i]] >= 0) unsliced = false;
      L.syrk_fused[l] = (unsliced && nw > 0 && !getenv("DOGLEG_AMD_NO_SYRK_FUSE")) ? 1 : 0;
    }
    if(l >= H.mf_level0 || L.syrk_fused[l])
    {
      // room for the update matrix behind the panel where both fit (the kernel's rule and, for supernodes with children, the
      // symbolic phase's).  Childless supernodes only stage it if that does not cost the level a resident workgroup per CU.
      long with_children = L.lds[l], leaves = L.lds[l];
      for(int i = H.lvl_ptr[l]; i < H.lvl_ptr[l+1]; i++)
      {
        const int s = H.lvl_sn[i];
        const long wv = H.sn_c0[s+1] - H.sn_c0[s], nr = H.sn_rowptr[s+1] - H.sn_rowptr[s], mb = nr - wv;
        const bool cmp = H.sn_bd_ptr[s+1] > H.sn_bd_ptr[s] && H.sn_top[s] < 0;
        const long pan = panel_doubles(wv, nr, cmp, L.leaf[l]);
        const int jsp = cmp ? (int)mb : sym_w_split(wv, nr);      // the kernel's rule (sym_w_split: part of W may sit in the top block's upper triangle)
        const long need = (pan + (jsp >= 0 ? sym_w_linear(mb, jsp) : mb*(mb + 1)/2) + 1)*8;
        const long need0 = (pan + 1)*8;          // at least the scratch slot behind the panel
        const long want = (need <= FAC_LDS && jsp >= 0) ? need : need0;
        const bool has_children = l >= H.mf_level0 && H.mf_cptr[s+1] > H.mf_cptr[s];
        if(has_children) with_children = std::max(with_children, want); else leaves = std::max(leaves, want);
      }
      const long base = std::max((long)L.lds[l], with_children);
      const long per_cu0 = 163840/(base + 3584), per_cu1 = 163840/(std::max(base, leaves) + 3584);
      L.stage[l] = (per_cu1 == per_cu0) ? 1 : 0;
      L.lds[l] = (int)(L.stage[l] ? std::max(base, leaves) : base);
    }
    if(debug)
      fprintf(stderr, "factor level %d: %d supernodes, dynamic LDS %d bytes, update matrices staged %d, leaf instantiation %d, gather: %d waves, %d bytes\n",
              l, H.lvl_ptr[l+1] - H.lvl_ptr[l], L.lds[l], (int)L.stage[l], (int)L.leaf[l], L.upd_nw[l], L.upd_lds[l]);
  }
  return 0;
}

// One-launch region: the last levels of the multifrontal region as ONE launch, workgroups
// in level order -- a workgroup only ever waits for lower-numbered ones, so in-order dispatch cannot deadlock.
// Conditions: unsliced supernodes, update matrices staged in LDS, one block size, no update units.
RegionPlan region_plan(const SymHost& H, const FacLevels& L, int lo_min, int hi, const RegionKnobs& K)
{
  RegionPlan R;
  R.level0 = H.nlevels;
  if(!K.persist || H.nlevels < 2 || hi < lo_min) return R;
  const int ncu = K.ncu;
  const bool slice_ok = K.slices;
  int total = 0, l0 = hi + 1, lds = 0, stage = 1;
  const int nt = L.nt[hi];
  for(int l = hi; l >= std::max(1, lo_min); l--)
  {
    const int n = H.fw_lvl_ptr[l+1] - H.fw_lvl_ptr[l];
    if(l < H.mf_level0) break;
    if(n == 0 || total + n > K.cap || L.nt[l] != nt || L.lds[l] <= 0) break;
    if(H.uw_lvl_ptr[l+1] > H.uw_lvl_ptr[l] || H.uf_lvl_ptr[l+1] > H.uf_lvl_ptr[l]) break;
    if(std::any_of(&H.fw_item[H.fw_lvl_ptr[l]], &H.fw_item[H.fw_lvl_ptr[l]] + n,
                   [](const FwItem& it) { return it.top >= 0 || it.r0 != 0 || it.nbd > 0; })) break;
    stage = stage && L.stage[l]; total += n; l0 = l; lds = std::max(lds, L.lds[l]);
  }
  if(hi + 1 - l0 < 2) return R;
  R.level0 = l0; R.level1 = hi; R.stage = stage;
  if(K.timing)
    fprintf(stderr, "libdogleg_amd: one-launch region of the factorisation: levels %d..%d of %d (%d supernodes, ", l0, hi, H.nlevels, total);
  // Replicas: a supernode of a level with fewer supernodes than CUs is given to several workgroups -- the same sweep
  // on the same data, the same bits --, each of which forms and publishes only its share of the update matrix's tile
  // columns.  A level gets replicas while it and its neighbour level still fit the chip together.
  std::vector<int> first(H.fw_item.size(), -1), count(H.fw_item.size(), 0);
  // the region's own children records and destination lists: the symbolic phase's, behind them those of the replicas
  R.rec = H.mf_rec; R.dst = H.mf_dst;
  long lds_need = lds;
  // A level holds more workgroups than CUs are free when its turn comes: the ones that find a CU late should be the
  // ones with slack.  Its supernodes are listed by the estimated time their subtree is done, the latest first (columns
  // swept in blocks of 16, rows, a constant for the children's sum and the hand-off); no arithmetic depends on the order.
  std::vector<double> est(H.fw_item.size(), 0.0);
  std::vector<int> item_of_sn(H.nsn, -1);
  for(int l = R.level0; l <= hi; l++)
    for(int i = H.fw_lvl_ptr[l]; i < H.fw_lvl_ptr[l+1]; i++) item_of_sn[H.fw_sn[i]] = i;
  for(int l = R.level0; l <= hi; l++)
  {
    const int n = H.fw_lvl_ptr[l+1] - H.fw_lvl_ptr[l];
    std::vector<int> order(n);
    for(int k = 0; k < n; k++) order[k] = H.fw_lvl_ptr[l] + k;
    for(int i : order)
    {
      const FwItem& fi = H.fw_item[i];
      double e0 = 0.0;
      for(int k = 0; k < fi.nch; k++) { const int ci = item_of_sn[H.mf_child[fi.ch0 + k]]; if(ci >= 0) e0 = std::max(e0, est[ci]); }
      est[i] = e0 + 3.0*((fi.w + 15)/16) + 0.02*fi.nrows + 9.0;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b2) { return est[a] > est[b2]; });
    // (the first level of the region is its most populous one, and the Cauchy step's pass over J runs beside
    // it: replicas there cost more in CUs than they save -- only what does not fit LDS whole is sliced)
    const int rl = std::max(1, std::min(K.rmax, (ncu/2)/std::max(n, 1)));
    // (the first level's supernodes whose panel is at least 70 % of the level's largest get a second workgroup, while CUs are left)
    const int l1_pct = (l == R.level0 && rl == 1) ? 70 : 0;
    long l1_max = 0; int l1_left = std::max(0, ncu - n);
    if(l1_pct > 0) for(int i = H.fw_lvl_ptr[l]; i < H.fw_lvl_ptr[l+1]; i++) l1_max = std::max(l1_max, (long)H.fw_item[i].nrows*H.fw_item[i].w);
    for(int i : order)
    {
      FwItem it = H.fw_item[i];
      const int mb = it.nrows - it.w, T = (mb + 15) >> 4;
      int rl_i = rl;
      if(l1_pct > 0 && l1_left > 0 && (long)it.nrows*it.w*100 >= l1_max*l1_pct) { rl_i = 2; l1_left--; }
      const long pan = panel_doubles(it.w, it.nrows, false, false), room = FAC_LDS/8 - pan - 2;
      const bool has_w = mb > 0 && it.u_off >= 0;
      // the packed entries [e(r), e(r+1)) of the update matrix belong to share r of `cut`
      std::vector<int> cut;
      auto col = [&](int t) { return std::min<long>(16L*t, mb); };
      // an update matrix that does not fit LDS whole (it.jsp < 0) fits in slices: two replicas at least
      int want = has_w ? std::min(rl_i, T) : 1;
      if(has_w && it.jsp < 0 && slice_ok) want = std::max(want, std::min(2, T));
      int nrep = 1;
      for(; want <= std::min(8, std::max(T, 1)); want++)
      {
        cut = cut_tile_columns(T, want);
        nrep = std::max(1, (int)cut.size() - 1);
        if(nrep == 1 || !slice_ok) break;
        bool fits = true;
        for(int r = 0; r < nrep; r++)
          if(sym_w_linear(mb, col(cut[r+1])) - sym_w_linear(mb, col(cut[r])) + 1 > room) fits = false;
        if(fits) break;
        nrep = 1;                                   // (more, narrower slices)
      }
      bool hbm_rep = false;
      // one workgroup (or replicas that each stage the whole update matrix: DOGLEG_AMD_NO_FRONT_SLICES)
      if((nrep == 1 || !slice_ok) && it.jsp < 0)
      {
        nrep = 1;
        if(has_w && it.nch > 0) R.acc_any = true;
        // An update matrix that is summed in HBM gets replicas too: each sweeps the panel and OWNS a stretch of tile
        // columns in HBM -- it sums the children's entries of that stretch only, forms B B' of those tiles, publishes them
        const int want_h = (has_w && slice_ok) ? std::min(std::min(rl_i, T), 8) : 1;      // (at least 2 / 3 / 4 of them also on the populous levels: 336 / 330 / 326 steps/s against 338)
        if(want_h > 1)
        {
          cut = cut_tile_columns(T, want_h);
          nrep = std::max(1, (int)cut.size() - 1);
          hbm_rep = nrep > 1;
        }
      }
      first[i] = (int)R.item.size(); count[i] = nrep;
      for(int r = 0; r < nrep; r++)
      {
        it = H.fw_item[i];
        it.rep = r; it.tj0 = (nrep == 1) ? 0 : cut[r]; it.tj1 = (nrep == 1 || r == nrep - 1) ? (1 << 20) : cut[r+1];
        it.rsv2 = nrep;      // (the LAST replica stores the panel, once the others have read it: k_factor_level)
        it.pad = l;          // (the level: for the profile build's dump)
        if(hbm_rep || (nrep > 1 && slice_ok))
        {
          // [eA, eB): the stretch of the packed triangle this replica zeroes, sums and forms (k_factor_level)
          const long jA = col(it.tj0), jB = (r == nrep - 1) ? mb : col(it.tj1);
          const long eA = sym_w_linear(mb, jA), eB = sym_w_linear(mb, jB);
          it.eA = (int)eA; it.eB = (int)eB;
          if(hbm_rep)
          {
            // (not `sliced`: nothing of the update matrix is in LDS; what is not the replica's goes to the scratch slot)
            it.sliced = 0;
            lds_need = std::max(lds_need, (pan + 2)*8);
            it.ch0 = write_children(H, it, jA, jB, pan, [&](long jw, long df) { return 0x8000 | (sym_w_linear(mb, jw) + df); },
                                    first, count, R.rec, R.dst);
          }
          else
          {
            const long slp = eA & 1, wt = pan + slp;
            it.sliced = 1;
            lds_need = std::max(lds_need, (pan + slp + (eB - eA) + 2)*8);
            it.ch0 = write_children(H, it, jA, jB, wt + (eB - eA), [&](long jw, long df) { return wt + (sym_w_linear(mb, jw) - eA) + df; },
                                    first, count, R.rec, R.dst);
          }
        }
        R.item.push_back(it);
      }
    }
  }
  // (the records of the symbolic phase: the children's workgroups in this launch)
  for(size_t k = 0; k < H.mf_rec.size(); k++) R.rec[k].rsv = child_workgroups(R.rec[k].rsv, first, count);
  R.nwg = (int)R.item.size();
  R.lds = (int)std::max<long>(lds, lds_need);
  if(K.timing) fprintf(stderr, "%d workgroups, %d bytes of LDS, multifrontal from level %d)\n", R.nwg, R.lds, H.mf_level0);
  return R;
}

// Everything the kernel takes on trust: every destination inside the workgroup's LDS, the slices of a supernode's
// replicas covering its update matrix exactly once, children listed before their parents.
int region_check(const SymHost& H, const RegionPlan& R, long* stats, char* err, size_t len)
{
  long nsliced = 0, nhbm = 0;
  auto fail = [&](const char* what, size_t g) { snprintf(err, len, "one-launch region: %s (workgroup %zu)", what, g); return 1; };
  std::vector<long> covered;
  for(size_t g = 0; g < R.item.size(); g++)
  {
    const FwItem& it = R.item[g];
    const long mb = it.nrows - it.w, pan = panel_doubles(it.w, it.nrows, false, false), ntri = mb*(mb + 1)/2;
    const long T = (mb + 15) >> 4;
    // [eA, eB) is the packed stretch of the tile columns [tj0, tj1)
    const long jA = std::min<long>(16L*it.tj0, mb), jB = it.tj1 >= T ? mb : std::min<long>(16L*it.tj1, mb);
    const bool stretch_ok = it.eA == jA*mb - jA*(jA - 1)/2 && it.eB == jB*mb - jB*(jB - 1)/2;
    if(it.rep == 0) covered.assign((size_t)std::max<long>(T, 1), 0);
    for(long t = std::min<long>(it.tj0, T); t < std::min<long>(it.tj1, T); t++) covered[(size_t)t]++;
    long lds_end;
    if(it.sliced)
    {
      nsliced++;
      if(!stretch_ok) return fail("slice bounds do not match its tile columns", g);
      lds_end = pan + (it.eA & 1) + (it.eB - it.eA) + 1;             // + the scratch slot
    }
    else
    {
      if(it.jsp < 0 && mb > 0 && it.u_off >= 0)
      {
        if(it.rep == 0) nhbm++;
        // (replicas of an update matrix that is summed in HBM own the packed entries [eA, eB): their tile columns)
        if(it.rsv2 > 1) { if(!stretch_ok) return fail("an HBM replica's stretch does not match its tile columns", g); }
        else if(it.tj0 != 0 || it.tj1 < T) return fail("a single workgroup that does not form the whole update matrix", g);
      }
      // (the kernel stages the whole update matrix behind the panel when the supernode has children, or the launch stages the childless ones' too)
      const bool staged = it.jsp >= 0 && mb > 0 && it.u_off >= 0 && (it.nch > 0 || R.stage);
      lds_end = pan + (staged ? sym_w_linear(mb, it.jsp) : 0) + 1;
    }
    if(lds_end*8 > R.lds) return fail("its LDS need exceeds the launch's", g);
    if(R.lds > FAC_LDS) return fail("the launch's LDS exceeds the budget", g);
    for(int k = 0; k < it.nch; k++)
    {
      if((size_t)(it.ch0 + k) >= R.rec.size()) return fail("children record out of range", g);
      const MfChild& rc2 = R.rec[it.ch0 + k];
      if(rc2.rsv >= 0)
      {
        const long ci = rc2.rsv & 0xfffff, cn = rc2.rsv >> 20;
        if(cn < 1 || ci + cn > (long)g) return fail("a child's workgroups do not precede their parent", g);
      }
      if(rc2.dst_off < 0 || (size_t)(rc2.dst_off + rc2.npad) > R.dst.size()) return fail("destination list out of range", g);
      if(rc2.u_off < 0 || rc2.u_off + rc2.npad > H.uscr_size) return fail("a child's update matrix outside the scratch", g);
      for(long e = 0; e < rc2.npad; e++)
      {
        const long d = R.dst[(size_t)(rc2.dst_off + e)];
        if(it.sliced || it.jsp >= 0) { if(d >= pan + (it.sliced ? (it.eA & 1) + (it.eB - it.eA) : sym_w_linear(mb, it.jsp)) + 1) return fail("a destination behind the workgroup's LDS", g); }
        else if(!(d & 0x8000) ? d >= pan + 1 : (d & 0x7fff) > ntri) return fail("a destination outside panel / update matrix", g);
        else if((d & 0x8000) && it.rsv2 > 1 && ((d & 0x7fff) < it.eA || (d & 0x7fff) >= it.eB)) return fail("an HBM replica adds to an entry it does not own", g);
      }
    }
    const bool last = g + 1 == R.item.size() || R.item[g + 1].rep == 0;
    if(last && mb > 0 && it.u_off >= 0)
      for(long t = 0; t < T; t++) if(covered[(size_t)t] != 1) return fail("a tile column of the update matrix is not formed exactly once", g);
  }
  if(stats) { stats[0] = nsliced; stats[1] = nhbm; }
  return 0;
}

uint64_t region_plan_hash(const RegionPlan& R)
{
  Fnv f;
  f.add(R.level0, R.lds, R.stage, R.nwg);
  for(const FwItem& it : R.item)
    f.add(it.s, it.r0, it.r1, it.w, it.nrows, it.col0, it.bd0, it.nbd, it.lx, it.top, it.u_off, it.ch0, it.nch, it.bdw, it.jsp,
          it.rep, it.tj0, it.tj1, it.pad, it.sliced, it.eA, it.eB, it.rsv2);
  for(const MfChild& r : R.rec) f.add(r.u_off, r.dst_off, r.npad, r.rsv);
  for(uint16_t d : R.dst) f.add(d);
  return f.h;
}

uint64_t fac_levels_hash(const FacLevels& L)
{
  Fnv f;
  for(size_t l = 0; l < L.nt.size(); l++)
    f.add(L.nt[l], L.lds[l], L.leaf[l], L.stage[l], L.upd_coop[l], L.upd_lds[l], L.upd_nw[l],
          L.syrk_lds[l], L.syrk_nt[l], L.syrk_kc[l], L.syrk_fused[l], L.fin_ny[l]);
  return f.h;
}
