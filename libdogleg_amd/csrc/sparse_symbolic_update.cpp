// sparse_symbolic_update.cpp -- step 8 of the symbolic phase (see sparse_symbolic_internal.h): the factor update
// schedule.  Which levels form the multifrontal region, the row maps of every supernode into its ancestors, the
// sub-tasks, items and work units of the levels below the region, the two-phase levels, and the flat records the
// factor kernels read (FwItem, MfChild, mf_dst).  Pure host code (no HIP).
#include "sparse_symbolic_internal.h"
#include <cstdio>

namespace {

// one factor-update sub-task before it is packed: rows [ka, ..) of source d update block position q of target t
struct Sub { int lvl, t, q, d, ka, rel; };

// multifrontal region: the levels from mf_level0 up, provided none of their supernodes is
// cut into slices or has more than MF_MAXM rows below its diagonal block (one workgroup
// adds a child's whole update matrix).  DOGLEG_AMD_MF_LEVEL: lowest level allowed in the
// region, < 0 turns it off.
int mf_region_level0(const SymHost& S, const SymKnobs& K)
{
  int level0 = S.nlevels;
  {
    const int mf_req = K.mf_level, mf_maxm = 255;
    for(int l = S.nlevels - 1; mf_req >= 0 && l >= mf_req; l--)
    {
      bool ok = true;
      for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1] && ok; i++)
      {
        const int d = S.lvl_sn[i];
        const int mb = S.sn_rowptr[d+1] - S.sn_rowptr[d] - (S.sn_c0[d+1] - S.sn_c0[d]);
        if(S.sn_top[d] >= 0 || mb > mf_maxm) ok = false;
      }
      if(!ok) break;
      level0 = l;
    }
  }
  return level0;
}

// the row maps (relpos) of every supernode into the ancestors it updates -- inside the multifrontal region into
// its parent only --, and one sub-task per (source, target var-block) below the region
int update_subtasks(const SymHost& S, const SymFront& F, SymUpdate& R, std::vector<Sub>& subs, std::vector<int>& sn_parent,
                    char* err, int errlen)
{
  const int nsn = S.nsn;
  R.sn_prel.assign(nsn, -1);
  sn_parent.assign(nsn, -1);
  for(int d = 0; d < nsn; d++)
  {
    const std::vector<int>& bl = F.below(d);
    if(bl.empty()) continue;
    const bool mf_src = S.sn_level[d] >= R.mf_level0;
    const int wd = S.sn_c0[d+1] - S.sn_c0[d];
    const int nrows_d = S.sn_rowptr[d+1] - S.sn_rowptr[d];
    size_t i = 0;
    int krow = wd;                       // row index in d of block bl[i]
    while(i < bl.size())
    {
      const int t = F.sn_of_b[bl[i]];
      const int k0 = krow;
      const int relbase = (int)R.relpos.size();
      // positions of rows k0.. of d inside t: walk the remaining blocks
      {
        const std::vector<int>& tl = F.below(t);
        size_t tp = 0;
        for(size_t ii = i; ii < bl.size(); ii++)
        {
          const int q = bl[ii];
          int off;
          if(q >= F.sn_b0[t] && q < F.sn_b0[t+1]) off = F.colstart[q] - S.sn_c0[t];
          else
          {
            while(tp < tl.size() && tl[tp] < q) tp++;
            if(tp >= tl.size() || tl[tp] != q)
              SYM_FAIL("internal error: structure of supernode %d not nested in ancestor %d", d, t);
            off = F.belowoff[F.belowoff_ptr[t] + (int)tp];
          }
          for(int a = 0; a < F.w[F.border[q]]; a++) R.relpos.push_back(off + a);
        }
      }
      R.relpos.push_back(S.sn_rowptr[t+1] - S.sn_rowptr[t] - 1);      // augmented row -> augmented row
      if((int)R.relpos.size() - relbase != nrows_d - k0) SYM_FAIL("internal error: relpos size mismatch");
      if(k0 == wd) { sn_parent[d] = t; R.sn_prel[d] = relbase; }
      if(mf_src)
      {
        // only the map into the parent is needed: the update travels up the tree from there
        while(i < bl.size() && F.sn_of_b[bl[i]] == t) { krow += F.w[F.border[bl[i]]]; i++; }
        break;
      }
      // one sub-task per target var-block (another rank's supernode is not a source here)
      while(i < bl.size() && F.sn_of_b[bl[i]] == t)
      {
        if(F.mine(S, d)) subs.push_back({S.sn_level[d], t, bl[i], d, krow, relbase + (krow - k0)});
        krow += F.w[F.border[bl[i]]];
        i++;
      }
    }
  }
  return 0;
}

// levels with many small sources use the two-phase update
void two_phase_levels(const SymHost& S, const SymKnobs& K, SymUpdate& R)
{
  const int nsn = S.nsn;
  R.upd_syrk.assign(S.nlevels, 0); R.u_off.assign(nsn, -1); R.uscr_size = 0;
  const int syrk_min = K.syrk_min;
  for(int l = 0; l < R.mf_level0; l++)
  {
    const int n = S.lvl_ptr[l+1] - S.lvl_ptr[l];
    if(syrk_min <= 0 || n < syrk_min) continue;
    bool ok = true;
    for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1] && ok; i++)
    {
      const int d = S.lvl_sn[i];
      const int64_t wd = S.sn_c0[d+1] - S.sn_c0[d], mb = S.sn_rowptr[d+1] - S.sn_rowptr[d] - wd;
      if(mb > 240 || wd <= 8) ok = false;        // <= 15 x 15 tiles of 16 rows: 8 tiles per wave, 16 waves
    }
    if(!ok) continue;
    R.upd_syrk[l] = 1;
    int64_t off = 0;
    for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1]; i++)
    {
      const int d = S.lvl_sn[i];
      const int64_t mb = S.sn_rowptr[d+1] - S.sn_rowptr[d] - (S.sn_c0[d+1] - S.sn_c0[d]);
      R.u_off[d] = off; off += mb*mb;
    }
    R.uscr_size = std::max(R.uscr_size, off);
  }
}

// the children lists of the multifrontal region, their update matrices' slots, and per child where every entry goes
void mf_children(const SymHost& S, const std::vector<int>& sn_parent, SymUpdate& R)
{
  const int nsn = S.nsn;
  // the update matrices of the multifrontal region live until the parent has read them
  R.mf_cptr.assign(nsn + 1, 0);
  for(int d = 0; d < nsn; d++)
    if(S.sn_level[d] >= R.mf_level0)
    {
      const int64_t mb = S.sn_rowptr[d+1] - S.sn_rowptr[d] - (S.sn_c0[d+1] - S.sn_c0[d]);
      R.u_off[d] = R.uscr_size; R.uscr_size += (mb*(mb + 1)/2 + 1) & ~(int64_t)1;     // 16-byte aligned slots
      if(sn_parent[d] >= 0) R.mf_cptr[sn_parent[d] + 1]++;
    }
  for(int t = 0; t < nsn; t++) R.mf_cptr[t+1] += R.mf_cptr[t];
  R.mf_child.resize(R.mf_cptr[nsn]);
  {
    std::vector<int> nx(R.mf_cptr.begin(), R.mf_cptr.end() - 1);
    for(int d = 0; d < nsn; d++)
      if(S.sn_level[d] >= R.mf_level0 && sn_parent[d] >= 0) R.mf_child[nx[sn_parent[d]]++] = d;
  }
  // children in the order of their expected time of arrival, the latest last: a parent adds the early
  // ones while the late one is still at work (k_factor_level, one-launch region).  The estimate: the
  // longest chain below (and including) a supernode, a supernode counting panel rows x columns.
  {
    std::vector<double> chain(nsn, 0.0);
    for(int l = 0; l < S.nlevels; l++)
      for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1]; i++)
      {
        const int t = S.lvl_sn[i];
        double below = 0.0;
        for(int k = R.mf_cptr[t]; k < R.mf_cptr[t+1]; k++) below = std::max(below, chain[R.mf_child[k]]);
        chain[t] = below + (double)(S.sn_rowptr[t+1] - S.sn_rowptr[t])*(S.sn_c0[t+1] - S.sn_c0[t]);
      }
    for(int t = 0; t < nsn; t++)
      std::stable_sort(R.mf_child.begin() + R.mf_cptr[t], R.mf_child.begin() + R.mf_cptr[t+1],
                       [&](int a, int b) { return chain[a] < chain[b]; });
  }
  R.mf_rec.resize(R.mf_child.size());
  for(int t = 0; t < nsn; t++)
  {
    if(R.mf_cptr[t+1] == R.mf_cptr[t]) continue;
    // layout of t's factor workgroup (k_factor_level): panel with an even leading dimension,
    // the update matrix behind it when both (and one scratch double) fit in LDS
    const int w = S.sn_c0[t+1] - S.sn_c0[t], nrows = S.sn_rowptr[t+1] - S.sn_rowptr[t], mb = nrows - w;
    const int ldp = (nrows + 1) & ~1;
    const int jsp = sym_w_split(w, nrows);            // -1: the update matrix stays in HBM
    const bool u_lds = jsp >= 0;
    const int nlin = u_lds ? (int)sym_w_linear(mb, jsp) : 0;
    const int wt_off = u_lds ? ldp*w : 0x8000, trash = ldp*w + nlin;
    for(int k = R.mf_cptr[t]; k < R.mf_cptr[t+1]; k++)
    {
      const int c = R.mf_child[k];
      const int mc = S.sn_rowptr[c+1] - S.sn_rowptr[c] - (S.sn_c0[c+1] - S.sn_c0[c]);
      const int* map = &R.relpos[R.sn_prel[c]];
      const int nc = mc*(mc + 1)/2, npad = (nc + 1023) & ~1023;
      R.mf_rec[k].u_off = R.u_off[c]; R.mf_rec[k].dst_off = (int64_t)R.mf_dst.size();
      R.mf_rec[k].npad = npad; R.mf_rec[k].rsv = 0;
      R.mf_dst.reserve(R.mf_dst.size() + npad);
      for(int j = 0; j < mc; j++)
        for(int i = j; i < mc; i++)
        {
          const int fi = map[i], fj = map[j];
          const int jw = fj - w;
          const int d = (fj < w) ? fi + fj*ldp
                      : (u_lds && jw >= jsp) ? (mb - jw)*ldp + (fi - fj)          // in the top block's upper triangle
                      : wt_off + jw*mb - jw*(jw - 1)/2 + (fi - fj);
          R.mf_dst.push_back((uint16_t)d);
        }
      for(int e = nc; e < npad; e++) R.mf_dst.push_back((uint16_t)trash);
    }
  }
  R.uscr_size += 1024;                 // the padded tail of the last child is read (and dropped)
}

// one flat record per factor work item
void fw_items(const SymHost& S, SymUpdate& R)
{
  const int nsn = S.nsn;
  R.fw_item.resize(S.fw_sn.size());
  // the work item of every child (persistent top region of the factorisation: its flag); -1: none here
  {
    std::vector<int> sn_item(nsn, -1);
    for(size_t k = 0; k < S.fw_sn.size(); k++) if(sn_item[S.fw_sn[k]] < 0) sn_item[S.fw_sn[k]] = (int)k;
    for(size_t k = 0; k < R.mf_rec.size(); k++) R.mf_rec[k].rsv = sn_item[R.mf_child[k]];
  }
  for(size_t k = 0; k < S.fw_sn.size(); k++)
  {
    const int s2 = S.fw_sn[k];
    FwItem& it = R.fw_item[k];
    it.s = s2; it.r0 = S.fw_r0[k]; it.r1 = S.fw_r1[k]; it.w = S.sn_c0[s2+1] - S.sn_c0[s2];
    it.nrows = S.sn_rowptr[s2+1] - S.sn_rowptr[s2]; it.col0 = S.sn_c0[s2];
    it.bd0 = S.sn_bd_ptr[s2]; it.nbd = S.sn_bd_ptr[s2+1] - S.sn_bd_ptr[s2];
    it.lx = S.sn_lx[s2]; it.top = S.sn_top[s2]; it.u_off = R.u_off[s2];
    it.ch0 = R.mf_cptr[s2]; it.nch = R.mf_cptr[s2+1] - R.mf_cptr[s2];
    it.bdw = 0; it.jsp = sym_w_split(it.w, it.nrows);
    it.rep = 0; it.tj0 = 0; it.tj1 = 1 << 20; it.pad = 0; it.sliced = 0; it.eA = 0; it.eB = 0; it.rsv2 = 0;
    if(it.nbd > 0)
    {
      // members of equal width (the usual case: points): no list lookup in the kernel
      const int* mc = &S.sn_bd_col[it.bd0];
      const int wd0 = (it.nbd > 1 ? mc[1] : it.w) - mc[0];
      bool same = mc[0] == 0;
      for(int m = 0; m < it.nbd && same; m++) if(((m + 1 < it.nbd) ? mc[m+1] : it.w) - mc[m] != wd0) same = false;
      if(same) it.bdw = wd0;
    }
  }
}

// sub-tasks sorted by (level, target, block) and grouped into items; returns the level of every item
std::vector<int> update_items(const SymHost& S, const SymFront& F, std::vector<Sub>& subs, SymUpdate& R)
{
  std::sort(subs.begin(), subs.end(), [](const Sub& a, const Sub& b) {
    if(a.lvl != b.lvl) return a.lvl < b.lvl;
    if(a.t != b.t) return a.t < b.t;
    if(a.q != b.q) return a.q < b.q;
    return a.d < b.d; });
  R.ui_lvl_ptr.assign(S.nlevels + 1, 0);
  R.ui_ptr.push_back(0);
  std::vector<int> item_lvl;
  for(size_t i = 0; i < subs.size(); i++)
  {
    const Sub& u = subs[i];
    const bool newitem = (i == 0) || subs[i-1].lvl != u.lvl || subs[i-1].t != u.t || subs[i-1].q != u.q;
    if(newitem)
    {
      if(i != 0) R.ui_ptr.push_back((int)i);
      R.ui_t.push_back(u.t);
      R.ui_col.push_back(F.colstart[u.q] - S.sn_c0[u.t]);
      R.ui_nc.push_back(F.w[F.border[u.q]]);
      R.ui_lvl_ptr[u.lvl + 1]++;
      item_lvl.push_back(u.lvl);
    }
    const int nrows_d = S.sn_rowptr[u.d+1] - S.sn_rowptr[u.d];
    SymSub ss;
    ss.src = S.sn_lx[u.d] + u.ka; ss.rel = u.rel; ss.nrows_d = nrows_d;
    ss.wd = S.sn_c0[u.d+1] - S.sn_c0[u.d]; ss.m = nrows_d - u.ka;
    R.usub.push_back(ss);
    if(R.upd_syrk[u.lvl])
    {
      const int64_t mb = nrows_d - ss.wd, k0 = u.ka - ss.wd;
      R.usub_u.push_back(R.u_off[u.d] + k0*mb - k0*(k0 - 1)/2);      // packed lower triangle: diagonal of column k0
    }
    else R.usub_u.push_back(-1);
  }
  if(!subs.empty()) R.ui_ptr.push_back((int)subs.size());
  for(int l = 0; l < S.nlevels; l++) R.ui_lvl_ptr[l+1] += R.ui_lvl_ptr[l];
  return item_lvl;
}

void update_units(const SymHost& S, const std::vector<int>& item_lvl, SymUpdate& R)
{
  // work units
  R.uw_lvl_ptr.assign(S.nlevels + 1, 0); R.uf_lvl_ptr.assign(S.nlevels + 1, 0);
  R.upart_size = 0;
  const int nitems = (int)R.ui_t.size();
  // chunking by estimated cost: a light sub-task (narrow source) counts 1, a
  // heavy one counts by its thread-iterations; a unit is closed at UNIT_COST
  const int unit_cost = 1024;
  const int unit_cost_gather = std::max(1, unit_cost/64);
  std::vector<int> cuts;
  for(int it = 0; it < nitems; it++)
  {
    const int s0 = R.ui_ptr[it], s1 = R.ui_ptr[it+1];
    const int lvl = item_lvl[it];
    const int t = R.ui_t[it];
    const int64_t slab = (int64_t)(S.sn_rowptr[t+1] - S.sn_rowptr[t])*R.ui_nc[it];
    cuts.clear(); cuts.push_back(s0);
    long acc = 0;
    for(int st = s0; st < s1; st++)
    {
      const SymSub& u = R.usub[st];
      const long c = R.upd_syrk[lvl] ? unit_cost_gather : ((u.wd <= 8) ? 1 : 64 + (long)u.wd*((u.m + 255)/256));
      if(acc > 0 && acc + c > unit_cost) { cuts.push_back(st); acc = 0; }
      acc += c;
    }
    cuts.push_back(s1);
    const int nch = (int)cuts.size() - 1;
    if(nch <= 1)
    {
      R.uw_item.push_back(it); R.uw_s0.push_back(s0); R.uw_s1.push_back(s1); R.uw_part.push_back(-1);
      R.uw_lvl_ptr[lvl + 1]++;
    }
    else
    {
      R.uf_item.push_back(it); R.uf_n.push_back(nch); R.uf_off.push_back(R.upart_size);
      R.uf_lvl_ptr[lvl + 1]++;
      for(int k = 0; k < nch; k++)
      {
        R.uw_item.push_back(it); R.uw_s0.push_back(cuts[k]); R.uw_s1.push_back(cuts[k+1]);
        R.uw_part.push_back(R.upart_size + (int64_t)k*slab);
        R.uw_lvl_ptr[lvl + 1]++;
      }
      R.upart_size += (int64_t)nch*slab;
    }
  }
  for(int l = 0; l < S.nlevels; l++) { R.uw_lvl_ptr[l+1] += R.uw_lvl_ptr[l]; R.uf_lvl_ptr[l+1] += R.uf_lvl_ptr[l]; }
}

} // namespace

int sym_update_schedule(const SymHost& S, const SymFront& F, const SymKnobs& K, SymUpdate& R, char* err, int errlen)
{
  R.mf_level0 = mf_region_level0(S, K);
  std::vector<Sub> subs;
  std::vector<int> sn_parent;
  if(update_subtasks(S, F, R, subs, sn_parent, err, errlen)) return 1;
  two_phase_levels(S, K, R);
  mf_children(S, sn_parent, R);
  fw_items(S, R);
  const std::vector<int> item_lvl = update_items(S, F, subs, R);
  update_units(S, item_lvl, R);
  return 0;
}

void SymUpdate::into(SymHost& S)
{
  S.mf_level0 = mf_level0;
  S.sn_prel = std::move(sn_prel);
  S.relpos = std::move(relpos);
  S.mf_cptr = std::move(mf_cptr);
  S.mf_child = std::move(mf_child);
  S.upd_syrk = std::move(upd_syrk);
  S.u_off = std::move(u_off);
  S.usub_u = std::move(usub_u);
  S.uscr_size = uscr_size;
  S.upart_size = upart_size;
  S.mf_rec = std::move(mf_rec);
  S.mf_dst = std::move(mf_dst);
  S.fw_item = std::move(fw_item);
  S.ui_lvl_ptr = std::move(ui_lvl_ptr);
  S.ui_t = std::move(ui_t);
  S.ui_col = std::move(ui_col);
  S.ui_nc = std::move(ui_nc);
  S.ui_ptr = std::move(ui_ptr);
  S.usub = std::move(usub);
  S.uw_lvl_ptr = std::move(uw_lvl_ptr);
  S.uw_item = std::move(uw_item);
  S.uw_s0 = std::move(uw_s0);
  S.uw_s1 = std::move(uw_s1);
  S.uf_lvl_ptr = std::move(uf_lvl_ptr);
  S.uf_item = std::move(uf_item);
  S.uf_n = std::move(uf_n);
  S.uw_part = std::move(uw_part);
  S.uf_off = std::move(uf_off);
}
