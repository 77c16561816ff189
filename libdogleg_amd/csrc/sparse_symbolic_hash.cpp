// sparse_symbolic_hash.cpp -- sym_hash: every field of a SymHost in one 64-bit FNV-1a, records field by field
// (AsmFin::pad is the one field sym_analyze never writes: it stays out).  Pins the symbolic phase bit for bit
// (tests/test_library_cpu.py, profiles/symbolic_refactor.md).
#include "sparse_symbolic.h"
#include "fnv.h"
#include <cstring>

namespace {

struct SymHasher : Fnv
{
  // a vector: its length, then every element through `one`
  template <class T, class F> void vec(const std::vector<T>& v, F one) { add(v.size()); for(const T& x : v) one(x); }
  template <class T> void ints(const std::vector<T>& v) { vec(v, [&](T x) { add(x); }); }
  template <class T, size_t n> void arr(const T (&a)[n]) { for(size_t i = 0; i < n; i++) add(a[i]); }
};

} // namespace

uint64_t sym_hash(const SymHost& S)
{
  SymHasher f;
  f.add(S.N, S.M, S.nnz, S.row0, S.row1, S.part_rank, S.part_nranks, S.cut_level);
  f.ints(S.sn_owner); f.ints(S.xl_ptr); f.ints(S.xl_sn); f.ints(S.part_rows);
  f.add(S.nvb); f.ints(S.vb_start); f.ints(S.perm); f.ints(S.iperm);
  f.add(S.nsn); f.ints(S.sn_c0); f.ints(S.sn_rowptr); f.ints(S.sn_rows); f.ints(S.sn_lx); f.ints(S.sn_scr); f.ints(S.sn_level);
  f.add(S.nlevels); f.ints(S.lvl_ptr); f.ints(S.lvl_sn); f.ints(S.sn_bd_ptr); f.ints(S.sn_bd_col);
  f.ints(S.fw_lvl_ptr); f.ints(S.fw_sn); f.ints(S.fw_r0); f.ints(S.fw_r1); f.ints(S.sn_top); f.ints(S.ms_sn);
  f.add(S.top_size); f.ints(S.diagpos); f.ints(S.col_sn); f.add(S.lx_size, S.scr_size, S.max_panel);
  f.ints(S.ui_lvl_ptr); f.ints(S.ui_t); f.ints(S.ui_col); f.ints(S.ui_nc); f.ints(S.ui_ptr);
  f.vec(S.usub, [&](const SymSub& u) { f.add(u.src, u.rel, u.nrows_d, u.wd, u.m); });
  f.ints(S.relpos);
  f.ints(S.uw_lvl_ptr); f.ints(S.uw_item); f.ints(S.uw_s0); f.ints(S.uw_s1); f.ints(S.uw_part);
  f.ints(S.uf_lvl_ptr); f.ints(S.uf_item); f.ints(S.uf_n); f.ints(S.uf_off); f.add(S.upart_size);
  f.ints(S.upd_syrk); f.ints(S.u_off); f.ints(S.usub_u); f.add(S.uscr_size);
  f.add(S.mf_level0); f.ints(S.mf_cptr); f.ints(S.mf_child); f.ints(S.sn_prel);
  f.vec(S.fw_item, [&](const FwItem& i) {
    f.add(i.s, i.r0, i.r1, i.w, i.nrows, i.col0, i.bd0, i.nbd, i.lx, i.top, i.u_off, i.ch0, i.nch, i.bdw, i.jsp,
          i.rep, i.tj0, i.tj1, i.pad, i.sliced, i.eA, i.eB, i.rsv2); });
  f.vec(S.mf_rec, [&](const MfChild& c) { f.add(c.u_off, c.dst_off, c.npad, c.rsv); });
  f.ints(S.mf_dst);
  f.vec(S.oblk, [&](const SymOutBlock& o) { f.add(o.dest, o.ld, o.var0, o.nI, o.nJ, o.diag, o.pad, o.pad2); });
  f.vec(S.contrib, [&](const SymContrib& c) { f.add(c.base, c.r0, c.len, c.nrows, c.pad, c.offI, c.offJ); });
  f.vec(S.jtx_task, [&](const SymTask& t) { f.add(t.blk, t.c0, t.c1, t.part, t.var0, t.nI); });
  f.ints(S.jtx_fin_ptr); f.ints(S.jtx_fin_blk); f.add(S.jtx_nparts, S.jtx_covers_all);
  f.vec(S.asm_rho, [&](const AsmRho& r) { f.add(r.base, r.pair0, r.len, r.offJ, r.stage_off, r.nrows, r.pad); });
  f.vec(S.asm_pair, [&](const AsmPair& p) { f.add(p.offI, p.acc_nI); });
  f.vec(S.asm_slot, [&](const AsmSlot& s) { f.add(s.dest, s.ld, s.accoff, s.nI, s.diag); });
  f.vec(S.asm_batch, [&](const AsmBatch& b) { f.add(b.rho0, b.rho1); });
  f.vec(S.asm_ctask, [&](const AsmTask& t) { f.add(t.batch0, t.batch1, t.slot0, t.nslots, t.nJ, t.pad, t.acc_size, t.pad2, t.part); });
  f.vec(S.asm_cfin, [&](const AsmFin& c) { f.add(c.slot0, c.nslots, c.acc_size, c.nparts, c.part0, c.nJ); });
  f.vec(S.asm_shape, [&](const AsmShape& s) {
    f.arr(s.pcol); f.arr(s.tcol); f.arr(s.pslot); f.arr(s.pa); f.arr(s.tj); f.arr(s.ta);
    f.add(s.offJ, s.nJ, s.MP, s.MT, s.nT, s.smax, s.pad, s.offR, s.nJr, s.rslot, s.col0, s.ncopy, s.dslot);
    f.arr(s.paccoff); f.arr(s.pnI); });
  f.vec(S.asm_kg, [&](const AsmKG& g) { f.arr(g.base); f.add(g.tq, g.meta); f.arr(g.xr); f.arr(g.td); });
  f.vec(S.asm_mtask, [&](const AsmMTask& t) { f.add(t.kg0, t.kg1, t.slot0, t.shape, t.ld, t.pq, t.panel, t.part, t.rpart, t.jvar, t.pad); });
  f.vec(S.asm_fin2, [&](const AsmFin2& x) { f.add(x.dest, x.ld, x.list0, x.nlist, x.nI, x.nJ, x.diag, x.to_part); });
  f.ints(S.asm_fin2_list);
  f.add(S.asm_lds_len, S.asm_td_inline, S.asm_ts_off, S.asm_jtx_ok);
  f.ints(S.jf_ptr); f.ints(S.jf_ent); f.ints(S.jf_var0); f.ints(S.jf_w); f.ints(S.jf_short); f.ints(S.jf_long);
  f.ints(S.fin2_stage);
  f.vec(S.asm_run, [&](const AsmRun& r) { f.add(r.task0, r.task1, r.kg0, r.kg1); });
  f.ints(S.asm_pdest); f.ints(S.asm_tdest); f.add(S.asm_part_size);
  f.ints(S.rl_ptr); f.ints(S.rl_pos);
  int64_t flops; memcpy(&flops, &S.factor_flops, sizeof(flops));     // the double's bits
  f.add(S.nnz_JtJ_lower, S.nnz_L, flops);
  return f.h;
}
