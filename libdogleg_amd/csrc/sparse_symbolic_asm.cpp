// sparse_symbolic_asm.cpp -- step 9b of the symbolic phase (see sparse_symbolic_internal.h): the JtJ assembly schedule.
// Pure host code (no HIP).
// Column-block centric: a task owns (a group of) the output blocks (I,J) of ONE
// column block J and walks the row-blocks that contain J in batches: a batch's
// Jacobian rows are staged in LDS once and feed every block of that column.
#include "sparse_symbolic_internal.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <numeric>

namespace {

constexpr int ACC_CAP = 256, SLOT_CAP = 32, STAGE_CAP = 512, TASK_BATCHES = 16;
constexpr int RHO_PER_BATCH = 32, PAIRS_PER_BATCH = 256;
constexpr int KG_PER_TASK_T = 64, KG_PER_TASK_P = 256;

// one column block J on its way through the builder: its row list [r0, r1) of rrb, its elimination position, its
// supernode t, the panel's leading dimension, J's first column inside the panel, its width; rider: second pass
struct Col { int J, r0, r1, qJ, t, ld, lc, nJ; bool is_rider; };

struct AsmBuilder
{
  const SymHost& S; const SymFront& front; const SymKnobs& K; SymAssembly& out;
  char* err; int errlen;
  const int nvb, nrb;
  const bool use_mfma;
  std::vector<int> rptr, rrb, rx;          // var-block v: its local row-blocks rrb[rptr[v] .. rptr[v+1]) in row order, rx: v's place in each
  // layout id of every row-block: number of blocks, their widths and offsets inside a row
  std::vector<int> rb_layout;
  std::vector<int> slot_of, slot_stamp;
  struct SlotTmp { int I; int64_t dest; int nI; int diag; };
  std::vector<SlotTmp> slots;
  std::vector<int> grp_of, acc_of;            // per slot: group id, accumulator offset inside the group
  std::map<std::vector<int>, int> shape_ids;
  std::vector<int> tseen, pseen, fin_of;
  struct Ord { int I, nI, offI; bool P; };
  struct Cls { std::vector<int> es; std::vector<Ord> ords; int MP, MT, nP, nT, shape, slot0, acc_size, rider, pq;
               int lay, xJ; uint64_t mask; };
  std::vector<int> mtask_acc;          // accumulator size of every MFMA task (parallel to asm_mtask)
  std::vector<int> mtask_blk, mtask_rider;   // ... its column block, the rider it carries (-1: none)
  std::vector<Cls> classes;
  std::vector<int> cnt_same, key;
  std::vector<std::vector<int64_t>> fin_lists;
  // riders: dense column blocks whose only output block is their own diagonal
  std::vector<int> rb_host, rb_rider;
  std::vector<char> is_rider_blk;
  std::vector<std::vector<int64_t>> rider_parts;

  AsmBuilder(const SymHost& S_, const SymFront& F_, const SymKnobs& K_, SymAssembly& R_, char* err_, int errlen_)
    : S(S_), front(F_), K(K_), out(R_), err(err_), errlen(errlen_), nvb(F_.nvb), nrb(F_.nrb), use_mfma(K_.asm_mfma != 0),
      slot_of(nvb, -1), slot_stamp(nvb, -1), tseen(nvb, -1), pseen(nvb, -1), fin_of(nvb, -1),
      rb_host(nrb, -1), rb_rider(nrb, -1), is_rider_blk(nvb, 0), rider_parts(nvb) {}

  void row_lists();
  void riders();
  bool mfma_column(const Col& c);
  bool mfma_classes(const Col& c);
  bool mfma_ordinals(const Col& c);
  void mfma_shape(Cls& C, const Col& c);
  void mfma_emit(Cls& C, const Col& c, int64_t panel);
  void mfma_partials(const Col& c, int first_task);
  int  column_blocks();
  int  scalar_column(const Col& c);
  void sort_runs();
  void fin_stages();
  void sentinel();
  int  run();
};

// the row lists per var-block and the layout id of every row-block
void AsmBuilder::row_lists()
{
  rptr.assign(nvb + 1, 0);
  for(const RowBlock& b : front.rbs) if(b.local) for(int x = 0; x < b.nvb; x++) rptr[front.rb_vb[b.vptr + x] + 1]++;
  for(int v = 0; v < nvb; v++) rptr[v+1] += rptr[v];
  rrb.resize(rptr[nvb]); rx.resize(rptr[nvb]);
  {
    std::vector<int> nx(rptr.begin(), rptr.end() - 1);
    for(int bi = 0; bi < nrb; bi++)
    {
      const RowBlock& b = front.rbs[bi];
      if(!b.local) continue;
      for(int x = 0; x < b.nvb; x++) { const int v = front.rb_vb[b.vptr + x]; rrb[nx[v]] = bi; rx[nx[v]] = x; nx[v]++; }
    }
  }
  // layout id of every row-block: number of blocks, their widths and offsets inside a row
  rb_layout.assign(nrb, -1);
  {
    std::map<std::vector<int>, int> ids;
    std::vector<int> k, kprev;
    int prev = -1;
    for(int bi = 0; bi < nrb; bi++)
    {
      const RowBlock& b = front.rbs[bi];
      k.clear();
      for(int x = 0; x < b.nvb; x++) { k.push_back(front.w[front.rb_vb[b.vptr + x]]); k.push_back(front.rb_off[b.vptr + x]); }
      if(prev >= 0 && k == kprev) { rb_layout[bi] = prev; continue; }
      auto it = ids.find(k);
      if(it == ids.end()) it = ids.emplace(k, (int)ids.size()).first;
      rb_layout[bi] = prev = it->second; kprev = k;
    }
  }
}

// riders: dense column blocks whose only output block is their own diagonal
void AsmBuilder::riders()
{
  if(use_mfma && K.rider_min > 0)
    for(int Jr = 0; Jr < nvb; Jr++)
    {
      if(rptr[Jr+1] - rptr[Jr] < K.rider_min) continue;
      bool last_everywhere = true;
      for(int e = rptr[Jr]; e < rptr[Jr+1] && last_everywhere; e++)
      {
        const RowBlock& b = front.rbs[rrb[e]];
        for(int x = 0; x < b.nvb; x++) if(front.bpos[front.rb_vb[b.vptr + x]] > front.bpos[Jr]) { last_everywhere = false; break; }
      }
      if(!last_everywhere) continue;
      is_rider_blk[Jr] = 1;
      for(int e = rptr[Jr]; e < rptr[Jr+1]; e++)
      {
        const int bi = rrb[e];
        const RowBlock& b = front.rbs[bi];
        int host = -1, best = 0;           // the other block of the row with the longest row list
        for(int x = 0; x < b.nvb; x++)
        {
          const int I = front.rb_vb[b.vptr + x];
          if(I == Jr) continue;
          const int cnt = rptr[I+1] - rptr[I];
          if(cnt > best || (cnt == best && host >= 0 && front.bpos[I] < front.bpos[host])) { best = cnt; host = I; }
        }
        rb_host[bi] = host; rb_rider[bi] = host >= 0 ? Jr : -1;
      }
    }
}

// ---- MFMA path.  The row-blocks of a column block J are partitioned into classes of
// identical row layout (AsmShape); inside a class every block (I,J) is either persistent
// (same I in every row-block) or transient (all I different).  J qualifies when every
// transient block receives exactly one contribution overall.
bool AsmBuilder::mfma_column(const Col& c)
{
  if(!mfma_classes(c) || !mfma_ordinals(c)) return false;
  const int64_t panel = S.sn_lx[c.t] + (int64_t)c.lc*c.ld;
  const int first_task = (int)out.asm_mtask.size();
  for(Cls& C : classes) { mfma_shape(C, c); mfma_emit(C, c, panel); }
  mfma_partials(c, first_task);
  return true;
}

// 1. classes of identical layout: same row layout id, same position of J in the row, same set
//    of blocks eliminated after J, same rider
bool AsmBuilder::mfma_classes(const Col& c)
{
  const int J = c.J, r0 = c.r0, r1 = c.r1, qJ = c.qJ; const bool is_rider = c.is_rider;
  classes.clear();
  int last_cls = -1;
  for(int e = r0; e < r1; e++)
  {
    const int bi = rrb[e];
    const RowBlock& b = front.rbs[bi];
    if(is_rider && rb_host[bi] >= 0) continue;             // carried by another column block's tasks
    uint64_t mask = 0;
    if(is_rider) mask = 1;                                  // a rider is the last block of its rows
    else
    {
      if(b.nvb > 64) return false;
      for(int x = 0; x < b.nvb; x++) if(front.bpos[front.rb_vb[b.vptr + x]] >= qJ) mask |= 1ull << x;
    }
    const int rider = rb_host[bi] == J ? rb_rider[bi] : -1;
    // a rider only reads its own block: rows with the same offset of that block are one class,
    // whatever else they contain
    const int lay = is_rider ? front.rb_off[b.vptr + rx[e]] : rb_layout[bi], xJ = is_rider ? 0 : rx[e];
    int c = -1;
    if(last_cls >= 0 && classes[last_cls].lay == lay && classes[last_cls].xJ == xJ &&
       classes[last_cls].mask == mask && classes[last_cls].rider == rider) c = last_cls;
    else
      for(size_t q = 0; q < classes.size(); q++)
        if(classes[q].lay == lay && classes[q].xJ == xJ && classes[q].mask == mask && classes[q].rider == rider) { c = (int)q; break; }
    if(c < 0)
    {
      if(classes.size() >= (is_rider ? 4096u : 64u)) return false;
      c = (int)classes.size(); classes.emplace_back();
      Cls& C = classes.back();
      C.lay = lay; C.xJ = xJ; C.mask = mask; C.rider = rider;
      for(int x = 0; x < b.nvb; x++)
      { const int I = front.rb_vb[b.vptr + x]; if(front.bpos[I] >= qJ) C.ords.push_back({I, front.w[I], front.rb_off[b.vptr + x], true}); }
    }
    classes[c].es.push_back(e); last_cls = c;
  }
  return true;
}

// 2. persistent / transient blocks of every class
bool AsmBuilder::mfma_ordinals(const Col& c)
{
  const int J = c.J, qJ = c.qJ, nJ = c.nJ; const bool is_rider = c.is_rider;
  for(Cls& C : classes)
  {
    const int nord = (int)C.ords.size();
    cnt_same.assign(nord, 0);
    for(int e : C.es)
    {
      const RowBlock& b = front.rbs[rrb[e]];
      int k = 0;
      for(int x = 0; x < b.nvb; x++)
      { const int I = front.rb_vb[b.vptr + x]; if(front.bpos[I] < qJ) continue; if(I == C.ords[k].I) cnt_same[k]++; k++; }
    }
    C.MP = C.MT = C.nP = C.nT = 0;
    for(int k = 0; k < nord; k++)
    {
      C.ords[k].P = cnt_same[k] == (int)C.es.size();
      if(C.ords[k].P) { C.MP += C.ords[k].nI; C.nP++; pseen[C.ords[k].I] = J; } else { C.MT += C.ords[k].nI; C.nT++; }
    }
    if(C.MP > 16 || C.MT > 16) return false;
    // window of row columns the kernel stages in LDS
    int lo = front.rb_off[front.rbs[rrb[C.es[0]]].vptr + rx[C.es[0]]], hi = lo + nJ;
    for(const Ord& o : C.ords) { lo = std::min(lo, o.offI); hi = std::max(hi, o.offI + o.nI); }
    if(hi - lo > 64 && !is_rider) return false;
    if(hi - lo > 255) return false;
  }
  for(const Cls& C : classes)
  {
    if(C.nT == 0) continue;
    for(int e : C.es)
    {
      const RowBlock& b = front.rbs[rrb[e]];
      int k = 0;
      for(int x = 0; x < b.nvb; x++)
      {
        const int I = front.rb_vb[b.vptr + x];
        if(front.bpos[I] < qJ) continue;
        if(!C.ords[k].P) { if(tseen[I] == J || pseen[I] == J) return false; tseen[I] = J; }
        k++;
      }
    }
  }
  return true;
}

// 3. the shape record of a class: looked up by its key, made if it is new
void AsmBuilder::mfma_shape(Cls& C, const Col& c)
{
  const int J = c.J, nJ = c.nJ;
  const int offJ = front.rb_off[front.rbs[rrb[C.es[0]]].vptr + rx[C.es[0]]];
  key.assign(1, nJ); key.push_back(offJ);
  for(const Ord& o : C.ords) { key.push_back(o.nI); key.push_back(o.offI); key.push_back(o.P); key.push_back(o.I == C.rider); }
  auto it = shape_ids.find(key);
  if(it != shape_ids.end()) C.shape = it->second;
  else
  {
    AsmShape sh; memset(&sh, 0, sizeof(sh));
    for(int m = 0; m < 16; m++) { sh.pcol[m] = sh.tcol[m] = -1; sh.tj[m] = 0xFF; }
    int mp = 0, mt = 0, ip = 0, jt = 0;
    for(const Ord& o : C.ords)
    {
      for(int a = 0; a < o.nI; a++)
        if(o.P) { sh.pcol[mp] = (int16_t)(o.offI + a); sh.pslot[mp] = (uint8_t)ip; sh.pa[mp] = (uint8_t)a; mp++; }
        else    { sh.tcol[mt] = (int16_t)(o.offI + a); sh.tj[mt] = (uint8_t)jt; sh.ta[mt] = (uint8_t)a; mt++; }
      if(o.P && o.I == C.rider) { sh.offR = (uint16_t)o.offI; sh.nJr = (uint8_t)o.nI; sh.rslot = (uint8_t)ip; }
      if(o.P && o.I == J) sh.dslot = (uint8_t)ip;
      if(o.P) ip++; else jt++;
    }
    { int mp2 = 0, acc = 0;
      for(const Ord& o : C.ords) if(o.P)
      { for(int a = 0; a < o.nI; a++) { sh.paccoff[mp2] = (uint8_t)(acc + a); sh.pnI[mp2] = (uint8_t)o.nI; mp2++; } acc += o.nI*nJ; } }
    int lo = offJ, hi = offJ + nJ;
    for(const Ord& o : C.ords) { lo = std::min(lo, o.offI); hi = std::max(hi, o.offI + o.nI); }
    sh.col0 = (uint16_t)lo; sh.ncopy = (uint8_t)(hi - lo);
    for(int m = 0; m < 16; m++) { if(sh.pcol[m] >= 0) sh.pcol[m] -= lo; if(sh.tcol[m] >= 0) sh.tcol[m] -= lo; }
    if(sh.nJr > 0) sh.offR -= lo;
    out.asm_lds_len = std::max(out.asm_lds_len, ((hi - lo + 15)/16)*16 + 2);
    sh.offJ = (uint16_t)(offJ - lo); sh.nJ = (uint8_t)nJ; sh.MP = (uint8_t)C.MP; sh.MT = (uint8_t)C.MT;
    sh.nT = (uint8_t)C.nT; sh.smax = (uint8_t)std::min(4, 16/nJ);
    C.shape = (int)out.asm_shape.size(); out.asm_shape.push_back(sh); shape_ids[key] = C.shape;
  }
}

// 4. the slots, tasks and k-groups of a class
void AsmBuilder::mfma_emit(Cls& C, const Col& c, int64_t panel)
{
  const int J = c.J, qJ = c.qJ, ld = c.ld, nJ = c.nJ;
  const int smax = C.nT > 0 ? std::min(4, 16/nJ) : 4;
  const int kg_cap = C.nT > 0 ? KG_PER_TASK_T : KG_PER_TASK_P;
  C.slot0 = (int)out.asm_slot.size(); C.acc_size = 0;
  for(const Ord& o : C.ords) if(o.P)
  {
    AsmSlot sl; sl.dest = slots[slot_of[o.I]].dest; sl.ld = ld; sl.accoff = (uint16_t)C.acc_size;
    sl.nI = (uint8_t)o.nI; sl.diag = (uint8_t)(o.I == J);
    out.asm_slot.push_back(sl); C.acc_size += o.nI*nJ;
  }
  C.pq = (int)out.asm_pdest.size();
  for(const Ord& o : C.ords) if(o.P) out.asm_pdest.push_back((int)(slots[slot_of[o.I]].dest - panel));
  bool task_open = false, kg_open = false;
  int kg_rows = 0, kg_slots = 0, kg_in_task = 0;
  auto close_kg = [&]() {
    if(!kg_open) return;
    AsmKG& g = out.asm_kg.back();
    g.meta |= (uint32_t)kg_slots << 8 | 1u << 11; kg_open = false;
    // at most two transient destinations: they ride in the record
    const int nent = kg_slots*C.nT;
    if(C.nT > 0 && nent <= 2 && g.tq + nent <= (int)out.asm_tdest.size())
    { for(int q = 0; q < nent; q++) g.td[q] = out.asm_tdest[g.tq + q]; g.meta |= 1u << 13; } };
  auto close_task = [&]() { close_kg(); if(task_open) { out.asm_mtask.back().kg1 = (int)out.asm_kg.size(); task_open = false; } };
  auto open_kg = [&]() {
    AsmKG g; g.base[0] = g.base[1] = g.base[2] = g.base[3] = -1; g.tq = (int)out.asm_tdest.size(); g.meta = 0;
    g.xr[0] = g.xr[1] = g.xr[2] = g.xr[3] = 0;
    g.td[0] = g.td[1] = 0;
    out.asm_kg.push_back(g); kg_open = true; kg_rows = 0; kg_slots = 0; kg_in_task++; };
  for(int e : C.es)
  {
    const RowBlock& b = front.rbs[rrb[e]];
    const bool fits = kg_open && kg_rows + b.nrows <= 4 && kg_slots < smax;
    const int need_kg = b.nrows > 4 ? 2 : (fits ? 0 : 1);
    if(!task_open || kg_in_task + need_kg > kg_cap)
    {
      close_task();
      AsmMTask T; T.kg0 = (int)out.asm_kg.size(); T.kg1 = -1; T.slot0 = C.slot0; T.shape = C.shape; T.ld = ld;
      T.pq = C.pq; T.panel = panel; T.part = -1; T.rpart = -1; T.jvar = -1; T.pad = 0;
      mtask_acc.push_back(C.acc_size); mtask_blk.push_back(J); mtask_rider.push_back(C.rider);
      if(C.rider >= 0)
      {
        const int nr = front.w[C.rider];
        T.rpart = out.asm_part_size; out.asm_part_size += nr*nr;
        rider_parts[C.rider].push_back(T.rpart);
      }
      out.asm_mtask.push_back(T); task_open = true; kg_in_task = 0;
    }
    const int base = b.lbase;
    if(b.nrows > 4)
    {
      close_kg();
      const int tq = (int)out.asm_tdest.size();
      for(int h = 0; h < 2; h++)
      {
        open_kg(); out.asm_kg.back().tq = tq;
        for(int r = 4*h; r < std::min(b.nrows, 4*h + 4); r++)
        { out.asm_kg.back().base[r - 4*h] = base + r*b.len; out.asm_kg.back().xr[r - 4*h] = b.lr0 + r; }
        kg_slots = 1;
        if(h == 0) { out.asm_kg.back().meta |= 1u << 8; kg_open = false; }    // no store yet: the block continues
        else close_kg();
      }
    }
    else
    {
      if(!(kg_open && kg_rows + b.nrows <= 4 && kg_slots < smax)) { close_kg(); open_kg(); }
      for(int r = 0; r < b.nrows; r++)
      {
        out.asm_kg.back().base[kg_rows] = base + r*b.len; out.asm_kg.back().xr[kg_rows] = b.lr0 + r;
        out.asm_kg.back().meta |= (uint32_t)kg_slots << (2*kg_rows);
        kg_rows++;
      }
      kg_slots++;
    }
    if(C.nT > 0)
    {
      int k = 0;
      for(int x = 0; x < b.nvb; x++)
      {
        const int I = front.rb_vb[b.vptr + x];
        if(front.bpos[I] < qJ) continue;
        if(!C.ords[k].P) out.asm_tdest.push_back((int)(slots[slot_of[I]].dest - panel));
        k++;
      }
    }
  }
  close_task();
}

// 5. several tasks: persistent blocks go through partials, summed per destination block
void AsmBuilder::mfma_partials(const Col& c, int first_task)
{
  const int J = c.J, t = c.t, ld = c.ld, lc = c.lc, nJ = c.nJ; const bool is_rider = c.is_rider;
  const int ntask = (int)out.asm_mtask.size() - first_task;
  const bool carried = is_rider && !rider_parts[J].empty();
  if(ntask > 1 || carried)
  {
    const int fin0 = (int)out.asm_fin2.size();
    fin_lists.clear();
    for(int k = first_task; k < first_task + ntask; k++)
    {
      AsmMTask& T = out.asm_mtask[k];
      T.part = out.asm_part_size; out.asm_part_size += mtask_acc[k];
    }
    for(const Cls& C : classes)
    {
      int sidx = 0;
      for(const Ord& o : C.ords) if(o.P)
      {
        const AsmSlot& sl = out.asm_slot[C.slot0 + sidx]; sidx++;
        int f;
        if(fin_of[o.I] >= fin0 && fin_of[o.I] < (int)out.asm_fin2.size() && out.asm_fin2[fin_of[o.I]].dest == sl.dest) f = fin_of[o.I];
        else
        {
          f = (int)out.asm_fin2.size(); fin_of[o.I] = f;
          AsmFin2 F; F.dest = sl.dest; F.ld = ld; F.list0 = 0; F.nlist = 0; F.nI = sl.nI; F.nJ = (uint8_t)nJ;
          F.diag = sl.diag; F.to_part = 0;
          out.asm_fin2.push_back(F); fin_lists.emplace_back();
        }
        for(int k = first_task; k < first_task + ntask; k++)
        {
          const AsmMTask& T = out.asm_mtask[k];
          if(T.slot0 == C.slot0) fin_lists[f - fin0].push_back(T.part + sl.accoff);
        }
      }
    }
    if(carried)
    {
      if(fin_lists.empty())          // every row of the rider is carried by other tasks
      {
        AsmFin2 F; F.dest = S.sn_lx[t] + lc + (int64_t)lc*ld; F.ld = ld; F.list0 = 0; F.nlist = 0;
        F.nI = F.nJ = (uint8_t)nJ; F.diag = 1; F.to_part = 0;
        out.asm_fin2.push_back(F); fin_lists.emplace_back();
      }
      fin_lists[0].insert(fin_lists[0].begin(), rider_parts[J].begin(), rider_parts[J].end());
    }
    for(size_t f = 0; f < fin_lists.size(); f++)
    {
      out.asm_fin2[fin0 + f].list0 = (int)out.asm_fin2_list.size();
      out.asm_fin2[fin0 + f].nlist = (int)fin_lists[f].size();
      out.asm_fin2_list.insert(out.asm_fin2_list.end(), fin_lists[f].begin(), fin_lists[f].end());
    }
  }
}

// every column block with rows: its output blocks, then the MFMA schedule or, failing that, the scalar one
int AsmBuilder::column_blocks()
{
  for(int pass = 0; pass < 2; pass++)          // pass 1: the riders (rows nobody carried + the carried partials)
  for(int J = 0; J < nvb; J++)
  {
    const int r0 = rptr[J], r1 = rptr[J+1];
    if(r0 == r1 || (int)is_rider_blk[J] != pass) continue;
    const int qJ = front.bpos[J], t = front.sn_of_b[qJ];
    const int ld = S.sn_rowptr[t+1] - S.sn_rowptr[t];
    const int lc = front.colstart[qJ] - S.sn_c0[t];
    const int nJ = front.w[J];
    // distinct I's with pos(I) >= pos(J), in first-seen order
    slots.clear();
    for(int e = r0; e < r1; e++)
    {
      const RowBlock& b = front.rbs[rrb[e]];
      for(int x = 0; x < b.nvb; x++)
      {
        const int I = front.rb_vb[b.vptr + x];
        if(front.bpos[I] < qJ || slot_stamp[I] == J) continue;
        slot_stamp[I] = J; slot_of[I] = (int)slots.size();
        int64_t dest;
        if(I == J) dest = S.sn_lx[t] + lc + (int64_t)lc*ld;
        else
        {
          const int ro = front.rowoff_in(t, front.bpos[I]);
          if(ro < 0) SYM_FAIL("internal error: JtJ block (%d,%d) missing from the factor structure", front.bpos[I], qJ);
          dest = S.sn_lx[t] + ro + (int64_t)lc*ld;
        }
        slots.push_back({I, dest, front.w[I], I == J ? 1 : 0});
      }
    }
    const Col c{J, r0, r1, qJ, t, ld, lc, nJ, pass == 1};
    if(use_mfma && mfma_column(c)) continue;
    if(pass == 1) SYM_FAIL("internal error: no assembly schedule for dense column block %d", J);
    if(scalar_column(c)) return 1;
  }
  return 0;
}

// a column block on the scalar (LDS accumulator) kernel: groups of slots, tasks of batches of row-blocks
int AsmBuilder::scalar_column(const Col& c)
{
  const int J = c.J, r0 = c.r0, r1 = c.r1, qJ = c.qJ, ld = c.ld, nJ = c.nJ;
  // this block falls back to the LDS kernel: the riders it would have carried keep their own tasks
  for(int e = r0; e < r1; e++) if(rb_host[rrb[e]] == J) { rb_host[rrb[e]] = -2; rb_rider[rrb[e]] = -1; }
  // groups of slots that fit the LDS accumulator
  grp_of.assign(slots.size(), 0); acc_of.assign(slots.size(), 0);
  int ngrp = 0;
  {
    int acc = 0, cnt = 0;
    for(size_t k = 0; k < slots.size(); k++)
    {
      const int sz = slots[k].nI*nJ;
      if(cnt > 0 && (acc + sz > ACC_CAP || cnt >= SLOT_CAP)) { ngrp++; acc = 0; cnt = 0; }
      grp_of[k] = ngrp; acc_of[k] = acc; acc += sz; cnt++;
    }
    ngrp++;
  }
  for(int g = 0; g < ngrp; g++)
  {
    // slot table of the group
    const int slot0 = (int)out.asm_slot.size();
    int acc_size = 0, nslots = 0;
    for(size_t k = 0; k < slots.size(); k++) if(grp_of[k] == g)
    {
      AsmSlot sl; sl.dest = slots[k].dest; sl.ld = ld; sl.accoff = (uint16_t)acc_of[k];
      sl.nI = (uint8_t)slots[k].nI; sl.diag = (uint8_t)slots[k].diag;
      out.asm_slot.push_back(sl); nslots++; acc_size = acc_of[k] + slots[k].nI*nJ;
    }
    // rho records with at least one pair in this group, batched by staged size
    const int first_task = (int)out.asm_ctask.size();
    bool task_open = false, batch_open = false;
    std::vector<int> seq0, seq;
    int nb_in_task = 0, stage_used = 0, rho_in_batch = 0, pairs_in_batch = 0;
    auto close_batch = [&]() { if(batch_open) { out.asm_batch.back().rho1 = (int)out.asm_rho.size(); batch_open = false; } };
    auto close_task = [&]() {
      close_batch();
      if(task_open) { out.asm_ctask.back().batch1 = (int)out.asm_batch.size(); task_open = false; } };
    for(int e = r0; e < r1; e++)
    {
      const RowBlock& b = front.rbs[rrb[e]];
      int npairs = 0;
      for(int x = 0; x < b.nvb; x++)
      { const int I = front.rb_vb[b.vptr + x]; if(front.bpos[I] >= qJ && grp_of[slot_of[I]] == g) npairs++; }
      if(npairs == 0) continue;
      const int cnt = b.nrows*b.len;
      const bool direct = cnt > STAGE_CAP;
      const int need = direct ? 0 : cnt;
      if(batch_open && (stage_used + need > STAGE_CAP || rho_in_batch >= RHO_PER_BATCH ||
                        pairs_in_batch + npairs > PAIRS_PER_BATCH)) close_batch();
      if(!batch_open)
      {
        if(!task_open || nb_in_task >= TASK_BATCHES)
        {
          close_task();
          AsmTask T; T.batch0 = (int)out.asm_batch.size(); T.batch1 = -1; T.slot0 = slot0;
          T.nslots = (uint16_t)nslots; T.nJ = (uint8_t)nJ; T.pad = 0; T.acc_size = acc_size; T.pad2 = 0; T.part = -1;
          T.pad = 1;                       // uniform until a row-block with another block sequence shows up
          out.asm_ctask.push_back(T); task_open = true; nb_in_task = 0; seq0.clear();
        }
        out.asm_batch.push_back({(int)out.asm_rho.size(), -1}); batch_open = true; stage_used = 0; nb_in_task++;
        rho_in_batch = 0; pairs_in_batch = 0;
      }
      AsmRho R; R.base = b.lbase; R.pair0 = (int)out.asm_pair.size(); R.len = (uint16_t)b.len;
      R.offJ = (uint16_t)front.rb_off[b.vptr + rx[e]]; R.stage_off = direct ? (uint16_t)0xFFFF : (uint16_t)stage_used;
      R.nrows = (uint8_t)b.nrows; R.pad = 0;
      out.asm_rho.push_back(R);
      stage_used += need; rho_in_batch++; pairs_in_batch += npairs;
      seq.clear();
      for(int x = 0; x < b.nvb; x++)
      { const int I = front.rb_vb[b.vptr + x]; if(front.bpos[I] >= qJ && grp_of[slot_of[I]] == g) seq.push_back(front.w[I]); }
      if(seq0.empty()) { seq0 = seq; int tot = 0; for(int q : seq) tot += q*nJ; if(tot > 128) out.asm_ctask.back().pad = 0; }
      else if(seq != seq0) out.asm_ctask.back().pad = 0;
      if(npairs > PAIRS_PER_BATCH) SYM_FAIL("a measurement row touches too many variable blocks (%d)", npairs);
      for(int x = 0; x < b.nvb; x++)
      {
        const int I = front.rb_vb[b.vptr + x];
        if(front.bpos[I] < qJ || grp_of[slot_of[I]] != g) continue;
        AsmPair P; P.offI = (uint16_t)front.rb_off[b.vptr + x];
        P.acc_nI = (uint16_t)(acc_of[slot_of[I]] | ((front.w[I] - 1) << 12));
        out.asm_pair.push_back(P);
      }
    }
    close_task();
    // multi-task groups: partial accumulators + finalize entry
    const int ntask = (int)out.asm_ctask.size() - first_task;
    if(ntask > 1)
    {
      AsmFin F; F.slot0 = slot0; F.nslots = nslots; F.acc_size = acc_size; F.nparts = ntask;
      F.part0 = out.asm_part_size; F.nJ = nJ;
      out.asm_cfin.push_back(F);
      for(int k = 0; k < ntask; k++) out.asm_ctask[first_task + k].part = out.asm_part_size + (int64_t)k*acc_size;
      out.asm_part_size += (int64_t)ntask*acc_size;
    }
  }
  return 0;
}

// group the MFMA tasks by shape (their k-groups move with them) and cut the sequence into
// runs: a wave loads the shape's lane constants once and streams the k-groups of several
// small tasks back to back
void AsmBuilder::sort_runs()
{
  {
    const int nt = (int)out.asm_mtask.size();
    std::vector<int> order(nt);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return out.asm_mtask[a].shape < out.asm_mtask[b].shape; });
    // (the runs are cut first -- consecutive tasks of one shape, at most RUN_KG k-groups --, and every run's k-groups are
    // padded with empty ones to a multiple of the kernel's unroll: the kernel then never looks past the end of its run
    // inside an iteration (four scalar compares and a select a k-group).  An empty k-group behind a task's last one has
    // no rows, no slots and no end: it costs a product of zeros.)
    const int RUN_KG = 32;
    std::vector<AsmMTask> tasks2; tasks2.reserve(nt);
    std::vector<AsmKG> kg2; kg2.reserve(out.asm_kg.size() + out.asm_kg.size()/8);
    out.asm_run.clear();
    for(int q = 0; q < nt; )
    {
      AsmRun R; R.task0 = q; R.kg0 = (int)kg2.size();
      const int shape0 = out.asm_mtask[order[q]].shape;
      int nkg = 0;
      do
      {
        AsmMTask T = out.asm_mtask[order[q]];
        const int k0 = (int)kg2.size();
        kg2.insert(kg2.end(), out.asm_kg.begin() + T.kg0, out.asm_kg.begin() + T.kg1);
        kg2.back().meta |= 1u << 12;             // last k-group of its task
        nkg += T.kg1 - T.kg0;
        T.kg0 = k0; T.kg1 = (int)kg2.size();
        tasks2.push_back(T);
        q++;
      }
      while(q < nt && out.asm_mtask[order[q]].shape == shape0 &&
            nkg + (out.asm_mtask[order[q]].kg1 - out.asm_mtask[order[q]].kg0) <= RUN_KG);
      while(((int)kg2.size() - R.kg0) % ASM_KG_ALIGN != 0)
      {
        AsmKG g; g.base[0] = g.base[1] = g.base[2] = g.base[3] = -1; g.tq = 0; g.meta = 1u << 13;      // (no slots; "destinations in the record": none)
        g.xr[0] = g.xr[1] = g.xr[2] = g.xr[3] = 0; g.td[0] = g.td[1] = 0;
        kg2.push_back(g);
      }
      R.task1 = q; R.kg1 = (int)kg2.size();
      out.asm_run.push_back(R);
    }
    out.asm_mtask.swap(tasks2); out.asm_kg.swap(kg2);
    // Jt*x beside JtJ: which task records every var-block sums (task order)
    {
      std::vector<std::vector<int>> ent(nvb);
      for(int kk = 0; kk < nt; kk++)
      {
        const int k = order[kk], J = mtask_blk[k], R = mtask_rider[k];
        ent[J].push_back(16*kk);
        if(R >= 0) ent[R].push_back(16*kk + front.w[J]);
      }
      out.asm_jtx_ok = use_mfma && out.asm_ctask.empty() && nt > 0;
      out.jf_ptr.assign(1, 0); out.jf_ent.clear(); out.jf_var0.resize(nvb); out.jf_w.resize(nvb);
      out.jf_short.clear(); out.jf_long.clear();
      for(int v = 0; v < nvb; v++)
      {
        out.jf_ent.insert(out.jf_ent.end(), ent[v].begin(), ent[v].end());
        out.jf_ptr.push_back((int)out.jf_ent.size());
        out.jf_var0[v] = S.vb_start[v]; out.jf_w[v] = front.w[v];
        if(front.w[v] > 16 || (ent[v].empty() && rptr[v+1] > rptr[v])) out.asm_jtx_ok = false;
        if(ent[v].empty()) continue;                 // no rows: its entries of Jt*x stay zero
        // a single record that is the block's own task (not a ride on another block's): the kernel
        // writes Jt*x itself
        if(ent[v].size() == 1 && (ent[v][0] & 15) == 0) { out.asm_mtask[ent[v][0] >> 4].jvar = S.vb_start[v]; continue; }
        if(ent[v].size() <= 64) out.jf_short.push_back(v); else out.jf_long.push_back(v);
      }
    }
    // persistent destinations, 16 per task in task order (the kernel prefetches them by task index)
    {
      std::vector<int> pd2((size_t)nt*16, 0);
      for(int k = 0; k < nt; k++)
        for(int q = 0; q < 16 && out.asm_mtask[k].pq + q < (int)out.asm_pdest.size(); q++)
          pd2[(size_t)k*16 + q] = out.asm_pdest[out.asm_mtask[k].pq + q];
      out.asm_pdest.swap(pd2);
    }
    // (do all k-groups that store transient blocks carry the destinations themselves?)
    out.asm_td_inline = true;
    for(const AsmMTask& T : out.asm_mtask)
      if(out.asm_shape[T.shape].MT > 0)
        for(int g = T.kg0; g < T.kg1; g++)
          if(((out.asm_kg[g].meta >> 8) & 7) > 0 && (!(out.asm_kg[g].meta & (1u << 13)) || !(out.asm_kg[g].meta & (1u << 11)))) out.asm_td_inline = false;     // (... and stores them: no row-block of more than four rows)
    // (Tried: an XCD-aware launch order -- runs sorted by the position in J of the first row they
    // read, the sorted list cut into 8 segments laid out on the workgroups s, s + 8, ..., so that the
    // two readers of a stretch of J, its points' tasks and its cameras' tasks, meet in one XCD's L2.
    // Measured slower: 120.7 us against 112.6 on config #4, 1.17 ms against 1.07 on config #5 -- the
    // kernel is bound by instruction issue around the K = 4 MFMAs, not by the second pass over J, and
    // the shape-sorted order balances the long camera runs better.)
  }
}

// long lists are summed hierarchically: chunks of 64 partials -> intermediate partials.
// Stages run in order; inside a stage the entries with <= 64 partials come first
// (one wave each), then the longer ones (one workgroup each).
void AsmBuilder::fin_stages()
{
  {
    std::vector<AsmFin2> cur; cur.swap(out.asm_fin2);
    std::vector<int64_t> lst; lst.swap(out.asm_fin2_list);
    std::vector<std::vector<AsmFin2>> stages;
    std::vector<AsmFin2> inter;
    for(int depth = 0; depth < 8; depth++)
    {
      inter.clear();
      for(AsmFin2& F : cur)
      {
        if(F.nlist <= 256) continue;
        const int e = F.nI*F.nJ, nch = (F.nlist + 63)/64;
        const int new0 = (int)lst.size();
        std::vector<int64_t> news;
        for(int c = 0; c < nch; c++)
        {
          AsmFin2 X = F; X.to_part = 1; X.dest = out.asm_part_size; out.asm_part_size += e;
          X.list0 = F.list0 + 64*c; X.nlist = std::min(64, F.nlist - 64*c);
          inter.push_back(X); news.push_back(X.dest);
        }
        lst.insert(lst.end(), news.begin(), news.end());
        F.list0 = new0; F.nlist = nch;
      }
      stages.push_back(cur);
      if(inter.empty()) break;
      cur = inter;
      // the intermediates just created must run BEFORE the entries that consume them
    }
    // stages were collected consumer-first: emit them in reverse
    for(int sidx = (int)stages.size() - 1; sidx >= 0; sidx--)
    {
      std::vector<AsmFin2>& st = stages[sidx];
      std::stable_partition(st.begin(), st.end(), [](const AsmFin2& f) { return f.nlist <= 64; });
      int ns = 0; for(const AsmFin2& f : st) if(f.nlist <= 64) ns++;
      out.fin2_stage.push_back((int)out.asm_fin2.size()); out.fin2_stage.push_back(ns); out.fin2_stage.push_back((int)st.size() - ns);
      out.asm_fin2.insert(out.asm_fin2.end(), st.begin(), st.end());
    }
    out.asm_fin2_list.swap(lst);
  }
}

// sentinel so that rho[i+1].pair0 closes the pair list of the last rho
void AsmBuilder::sentinel()
{
  AsmRho R; memset(&R, 0, sizeof(R)); R.pair0 = (int)out.asm_pair.size(); out.asm_rho.push_back(R);
}

int AsmBuilder::run()
{
  out.asm_part_size = 0;
  out.asm_ts_off = K.asm_mfma == 2;
  row_lists();
  riders();
  if(column_blocks()) return 1;
  sort_runs();
  fin_stages();
  sentinel();
  return 0;
}

} // namespace

int sym_assembly_schedule(const SymHost& S, const SymFront& F, const SymKnobs& K, SymAssembly& R, char* err, int errlen)
{
  return AsmBuilder(S, F, K, R, err, errlen).run();
}

void SymAssembly::into(SymHost& S)
{
  S.asm_rho = std::move(asm_rho);
  S.asm_pair = std::move(asm_pair);
  S.asm_slot = std::move(asm_slot);
  S.asm_batch = std::move(asm_batch);
  S.asm_ctask = std::move(asm_ctask);
  S.asm_cfin = std::move(asm_cfin);
  S.asm_shape = std::move(asm_shape);
  S.asm_kg = std::move(asm_kg);
  S.asm_mtask = std::move(asm_mtask);
  S.asm_fin2 = std::move(asm_fin2);
  S.asm_fin2_list = std::move(asm_fin2_list);
  S.asm_lds_len = asm_lds_len;
  S.asm_td_inline = asm_td_inline;
  S.asm_ts_off = asm_ts_off;
  S.asm_jtx_ok = asm_jtx_ok;
  S.jf_ptr = std::move(jf_ptr);
  S.jf_ent = std::move(jf_ent);
  S.jf_var0 = std::move(jf_var0);
  S.jf_w = std::move(jf_w);
  S.jf_short = std::move(jf_short);
  S.jf_long = std::move(jf_long);
  S.fin2_stage = std::move(fin2_stage);
  S.asm_run = std::move(asm_run);
  S.asm_pdest = std::move(asm_pdest);
  S.asm_tdest = std::move(asm_tdest);
  S.asm_part_size = asm_part_size;
}
