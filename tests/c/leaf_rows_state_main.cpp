// The state of the merged leaves' rows below their member blocks (libdogleg_amd/csrc/leaf_rows_state.h: plain C++, no
// HIP), walked through what the host code does with the two panel buffers: assemble -> factor (lean) -> exchange of
// the buffers -> hold -> restore -> materialise.  Built with -fsanitize=address,undefined by
// tests/test_leaf_rows_cpu.py; prints "ok" and returns 0, or says which step went wrong.
#include "leaf_rows_state.h"
#include <cstdio>
#include <utility>
#include <vector>

static int fails = 0;
#define CHECK(c) do { if(!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); fails++; } } while(0)

int main()
{
  std::vector<double> A(8), B(8), C(8);
  double *Lx = A.data(), *Lx_spec = B.data();
  LeafRowsState S;
  CHECK(!S.raw(Lx) && !S.raw(Lx_spec) && !S.raw(nullptr));

  // point 0: assembled in place, factored lean
  S.assembled(Lx);
  CHECK(S.slot(Lx) == 0 && !S.raw(Lx));
  S.factored_lean(Lx);
  CHECK(S.raw(Lx) && S.lean_launches == 1);

  // point 1: assembled beside the evaluation into the other buffer, adopted (pointer swap) while point 0's factor is held
  S.assembled(Lx_spec);
  CHECK(S.slot(Lx_spec) == 1 && !S.raw(Lx_spec) && S.raw(Lx));
  double* held = Lx;                                   // sparse_hold_factor
  std::swap(Lx, Lx_spec);                              // sparse_assemble adopts
  CHECK(!S.raw(Lx) && S.raw(Lx_spec) && S.raw(held));
  S.factored_lean(Lx);
  CHECK(S.raw(Lx) && S.raw(held) && S.lean_launches == 2);

  // the trial point is rejected: the held factor comes back (sparse_restore_factor), raw as it was left
  std::swap(Lx, Lx_spec);
  CHECK(Lx == held && S.raw(Lx));
  // a user of the held factor: materialised once, idempotent
  S.materialize(Lx);
  CHECK(!S.raw(Lx) && S.materialized == 1);
  S.materialize(Lx);
  CHECK(!S.raw(Lx) && S.materialized == 1);
  // the dropped factor in the spare buffer is still raw until the buffer is cleared
  CHECK(S.raw(Lx_spec));
  S.assembled(Lx_spec);                                // clear_panels
  CHECK(!S.raw(Lx_spec));

  // the write-back of all rows (DOGLEG_AMD_LEAF_STORE_ROWS, or a level that may not run lean)
  S.assembled(Lx); S.factored_full(Lx);
  CHECK(!S.raw(Lx));
  S.materialize(Lx);
  CHECK(S.materialized == 1);
  // a factorisation stopped before its first launch: assembled, never factored -- nothing to form
  S.assembled(Lx);
  CHECK(!S.raw(Lx));

  // a third buffer has no slot: the host launches the full write-back for it
  CHECK(S.slot(C.data()) == -1);
  S.factored_lean(C.data());
  CHECK(!S.raw(C.data()) && S.lean_launches == 2);

  // a new pattern: nothing carries over, the slots are given out again
  S.factored_lean(Lx);
  S.reset();
  CHECK(!S.raw(Lx) && S.lean_launches == 0 && S.slot(C.data()) == 0);

  if(fails) return 1;
  printf("ok\n");
  return 0;
}
