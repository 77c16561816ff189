// leaf_rows_state.h -- which panel buffers still hold the ASSEMBLED rows below their merged leaves' member blocks.
// The lean leaf launch of the factorisation (sparse_factor.hip, k_factor_level<256, true> with FMODE_LEAN_ROWS) factors
// the member blocks in place and stores the augmented row, but leaves the other rows below as the assembly wrote them
// (W); L_below = W L_tt^-T is formed only for the readers that need it (k_leaf_rows_materialize).  The state belongs to
// the BUFFER: it is kept by buffer address, so it follows every exchange of the two panel buffers (sparse_assemble's
// adoption of the speculative assembly, sparse_restore_factor) and a factor that is held (sparse_hold_factor keeps the
// buffer's address) without any code at those places.  Plain C++, no HIP: tests/c/leaf_rows_state_main.cpp walks it.
#pragma once

struct LeafRowsState
{
  static constexpr int NBUF = 2;            // a backend has two panel buffers (Lx, Lx_spec)
  const void* buf[NBUF] = {nullptr, nullptr};
  bool raw_[NBUF] = {false, false};
  long lean_launches = 0, materialized = 0;         // leaf launches in the lean mode; runs of the materialisation kernel

  // the buffer's slot, given out at first sight and kept (-1: a third buffer, which no backend has)
  int slot(const void* p)
  {
    for(int i = 0; i < NBUF; i++) if(buf[i] == p) return i;
    for(int i = 0; i < NBUF; i++) if(!buf[i]) { buf[i] = p; return i; }
    return -1;
  }
  bool raw(const void* p) const
  {
    for(int i = 0; i < NBUF; i++) if(buf[i] == p && p) return raw_[i];
    return false;
  }
  // an assembly into p, a clear of p: whatever its rows were, they are a factorisation's no more
  void assembled(const void* p) { const int i = slot(p); if(i >= 0) raw_[i] = false; }
  // the lean leaf launch ran on p
  void factored_lean(const void* p) { const int i = slot(p); if(i >= 0) { raw_[i] = true; lean_launches++; } }
  // the leaf launch ran on p with the write-back of all rows
  void factored_full(const void* p) { const int i = slot(p); if(i >= 0) raw_[i] = false; }
  // L_below was stored over W
  void materialize(const void* p) { const int i = slot(p); if(i >= 0 && raw_[i]) { raw_[i] = false; materialized++; } }
  void reset() { *this = LeafRowsState(); }
};
