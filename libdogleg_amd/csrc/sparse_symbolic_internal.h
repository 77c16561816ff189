// sparse_symbolic_internal.h -- what the phases of sym_analyze hand each other.  Host code only: included by the
// sparse_symbolic*.cpp files, by no kernel file.
//
//   front (sparse_symbolic.cpp, one thread, in this order): blocks, block graph, ordering, block factorisation,
//     supernodes, layout, subtree partition, factor work list.  They fill the SymFront below and the members of
//     SymHost that describe the factor's structure.
//   schedules (four threads): sym_update_schedule (8, sparse_symbolic_update.cpp), sym_jtx_lists (9a) and
//     sym_solve_gather (10, sparse_symbolic.cpp), sym_assembly_schedule (9b, sparse_symbolic_asm.cpp).  Each reads the
//     SymHost the front left and what it needs of the SymFront and the knobs through const references, and fills a
//     record of its own with the SymHost members it owns; sym_analyze moves them into the SymHost after the join.
#pragma once
#include "sparse_symbolic.h"
#include <algorithm>

// every environment knob of the symbolic phase, read once by sym_knobs_env before any work (unset or empty: the default)
struct SymKnobs
{
  int slice_cap;      // DOGLEG_AMD_SLICE_CAP: doubles of a row slice (top block + its rows) of a panel too large for LDS; as
                      // much of the 160 KB as one workgroup can get, so that fewer slices repeat the top block's factorisation
  int nd_leaf;        // DOGLEG_AMD_ND_LEAF: weight from which the nested dissection stops and orders by minimum degree
  bool lds_split;     // DOGLEG_AMD_LDS_SPLIT: cut a chain whose panel would not fit LDS whole (0: row-sliced separators outside the
                      // multifrontal region, a path of its own, kept under test on config #5)
  int mf_level;       // DOGLEG_AMD_MF_LEVEL: lowest level allowed in the multifrontal region, < 0 turns it off
  int syrk_min;       // DOGLEG_AMD_SYRK_MIN: supernodes from which a level uses the two-phase update
  int asm_mfma;       // DOGLEG_AMD_ASM_MFMA: 0: no MFMA assembly, 2: with the four masked transient stores a k-group
  int rider_min;      // DOGLEG_AMD_RIDER_MIN: rows from which a dense column block rides on other blocks' tasks
  int debug;          // DOGLEG_AMD_SYM_DEBUG: 1: the per-level dump, >= 2: wall time of every step, on stderr
};
SymKnobs sym_knobs_env();

struct RowBlock { int r0, nrows, len, base, vptr, nvb; bool local; int lbase, lr0; };   // lbase / lr0: first value / first row in the rank-local arrays

struct Graph
{
  int n = 0;
  std::vector<int> ptr, adj;      // CSR, no self loops, sorted
  std::vector<int> w;             // node weights (variables per block)
  std::vector<long> wdeg;         // weighted degree
};

// what steps 1 to 7, the partition and the work list hand to the schedules, beside the SymHost members they fill
struct SymFront
{
  int N = 0, nvb = 0, nrb = 0, nsn = 0, part_rank = 0;
  std::vector<RowBlock> rbs;                // row-blocks; the var-blocks of row-block b and their offsets inside a row:
  std::vector<int> rb_vb, rb_off;           // rb_vb / rb_off[b.vptr .. b.vptr + b.nvb)
  std::vector<int> w;                       // [nvb] variables of every var-block
  std::vector<int> border, bpos;            // elimination position -> var-block and back
  std::vector<std::vector<int>> st;         // [nvb] structure of a block column: the positions below it, ascending
  std::vector<int> colstart;                // [nvb+1] scalar position of a block position
  std::vector<int> sn_b0, sn_of_b;          // [nsn+1] first block position of a supernode; [nvb] supernode of a block position
  std::vector<int> sn_parent0;              // [nsn] parent in the supernodal elimination tree, -1: a root
  std::vector<int> belowoff_ptr, belowoff;  // per supernode: row offset in its panel of every block below it

  // block-level structure below supernode s: that of its last block column
  const std::vector<int>& below(int s) const { return st[sn_b0[s+1] - 1]; }
  // row offset of block position q inside supernode t's row list (-1 if absent)
  int rowoff_in(int t, int q) const
  {
    if(q >= sn_b0[t] && q < sn_b0[t+1]) return colstart[q] - colstart[sn_b0[t]];
    const std::vector<int>& bl = below(t);
    auto it = std::lower_bound(bl.begin(), bl.end(), q);
    if(it == bl.end() || *it != q) return -1;
    return belowoff[belowoff_ptr[t] + (int)(it - bl.begin())];
  }
  // does this rank work on supernode s (above the cut: every rank does)
  bool mine(const SymHost& S, int s) const { return S.sn_owner[s] < 0 || S.sn_owner[s] == part_rank; }
};

// ---- the schedules' results: the SymHost members each one owns (names, types and defaults as in SymHost)
struct SymUpdate            // 8
{
  int mf_level0 = 0;
  std::vector<int> sn_prel, relpos, mf_cptr, mf_child;
  std::vector<char> upd_syrk;
  std::vector<int64_t> u_off, usub_u;
  int64_t uscr_size = 0, upart_size = 0;
  std::vector<MfChild> mf_rec;
  std::vector<uint16_t> mf_dst;
  std::vector<FwItem> fw_item;
  std::vector<int> ui_lvl_ptr, ui_t, ui_col, ui_nc, ui_ptr;
  std::vector<SymSub> usub;
  std::vector<int> uw_lvl_ptr, uw_item, uw_s0, uw_s1, uf_lvl_ptr, uf_item, uf_n;
  std::vector<int64_t> uw_part, uf_off;
  void into(SymHost& S);
};
struct SymJtx               // 9a
{
  std::vector<SymOutBlock> oblk;
  std::vector<SymContrib> contrib;
  std::vector<SymTask> jtx_task;
  std::vector<int> jtx_fin_ptr, jtx_fin_blk;
  int jtx_nparts = 0;
  bool jtx_covers_all = false;
  void into(SymHost& S);
};
struct SymAssembly          // 9b
{
  std::vector<AsmRho> asm_rho;
  std::vector<AsmPair> asm_pair;
  std::vector<AsmSlot> asm_slot;
  std::vector<AsmBatch> asm_batch;
  std::vector<AsmTask> asm_ctask;
  std::vector<AsmFin> asm_cfin;
  std::vector<AsmShape> asm_shape;
  std::vector<AsmKG> asm_kg;
  std::vector<AsmMTask> asm_mtask;
  std::vector<AsmFin2> asm_fin2;
  std::vector<int64_t> asm_fin2_list;
  int asm_lds_len = 0;
  bool asm_td_inline = false, asm_ts_off = false, asm_jtx_ok = false;
  std::vector<int> jf_ptr, jf_ent, jf_var0, jf_w, jf_short, jf_long, fin2_stage;
  std::vector<AsmRun> asm_run;
  std::vector<int> asm_pdest, asm_tdest;
  int64_t asm_part_size = 0;
  void into(SymHost& S);
};
struct SymGather            // 10
{
  std::vector<int> rl_ptr, rl_pos;
  void into(SymHost& S);
};

// (the two that can fail: 0, or nonzero with a message in err)
int sym_update_schedule(const SymHost& S, const SymFront& F, const SymKnobs& K, SymUpdate& R, char* err, int errlen);
void sym_jtx_lists(const SymHost& S, const SymFront& F, SymJtx& R);
int sym_assembly_schedule(const SymHost& S, const SymFront& F, const SymKnobs& K, SymAssembly& R, char* err, int errlen);
void sym_solve_gather(const SymHost& S, SymGather& R);

#define SYM_FAIL(...) do { snprintf(err, errlen, __VA_ARGS__); return 1; } while(0)
