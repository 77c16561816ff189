"""The batches of the bounded products solve's tests (tests/test_dense_products_batch_bounds_cpu.py, _gpu.py): ragged batches of
the synthetic problems, M[b] = ragged_M(B, Mmin, Mmax) of tests/batch_products_oracle.py, seeds 1 .. B, set "diverse", bounds by
bounds_between of tests/test_dense_batch_bounds_gpu.py (its docstring: half way between start and optimum, on the variables i = b
mod 3 or on every variable), stopping thresholds STOP_OVER (1e-6, that docstring too).  The reference is
tests/batch_bounds_oracle.py::solve_one with the trivial loss on tests/batch_oracle.py::HostProblem(M[b], N, seed, ...): it is per
problem, so a ragged batch needs nothing new.

Every batch was checked on the CPU with the oracle alone: the smallest decision margin over its problems is above MARGIN_FLOOR =
1e-6, no problem is left out, and the margin each batch gave is recorded here and asserted to 5 % before anything is compared.
Test infrastructure: nothing of the library under test computes a number here."""
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import LOSS_TRIVIAL
from tests import batch_bounds_oracle as bb
from tests import batch_oracle as bo
from tests import batch_products_oracle as po
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_bounds_gpu as tbd
from tests import test_dense_batch_gpu as tb

MARGIN_FLOOR = tb.MARGIN_FLOOR
SETNAME = "diverse"
STOP_OVER = tbd.STOP_OVER

# the ragged parity batches: (N, (Mmin, Mmax), B): (every variable bounded, the margin recorded, problems that end with a held
# variable)
PARITY = {
    (6, (20, 90), 65): (False, 8.117e-4, 65),
    (6, (20, 90), 33): (False, 1.676e-3, 33),
}
# one batch of CLASS_B per edge of a size class: (N, (Mmin, Mmax)): (every variable bounded, margin, problems that end held)
CLASS_B = 5
CLASSES = {
    (1, (5, 9)): (False, 7.805e-2, 2),
    (8, (20, 40)): (False, 8.046e-3, 5),
    (9, (30, 60)): (False, 3.162e-4, 5),
    (16, (50, 90)): (False, 7.097e-3, 5),
    (17, (40, 80)): (False, 2.351e-2, 5),
    (24, (60, 100)): (False, 2.575e-3, 5),
    (25, (60, 100)): (False, 1.335e-2, 5),
    (32, (70, 120)): (False, 4.364e-3, 5),
    (33, (70, 120)): (False, 2.413e-3, 5),
    (48, (103, 150)): (False, 4.491e-3, 5),
    (49, (103, 150)): (False, 6.365e-5, 5),
    (64, (128, 160)): (True, 8.474e-5, 5),
}


def all_batches():
    """(N, (Mmin, Mmax), B, every, margin, held problems) of every batch above"""
    return [(N, rg, B) + v for (N, rg, B), v in PARITY.items()] + [(N, rg, CLASS_B) + v for (N, rg), v in CLASSES.items()]


def params(over=STOP_OVER):
    return tb.params(SETNAME, **dict(over))


@functools.lru_cache(maxsize=None)
def oracle_batch(N, ragged, B, every=False, over=STOP_OVER, frac=0.5):
    """(the bounded oracle's solves, lo (B, N), hi (B, N), M (B,)) of the ragged batch; cached: the tests share batches.  p* is the
    optimum of the unbounded oracle under the set's own parameters, the bounded solve runs under `over`"""
    eps, noise, spread, _ = tb.SETS[SETNAME]
    loss = ro.Loss(LOSS_TRIVIAL, 1.0, 1)
    Ms = po.ragged_M(B, *ragged)
    out, los, his = [], [], []
    for b in range(B):
        hp = bo.HostProblem(int(Ms[b]), N, 1 + b, eps, noise, spread)
        free = ro.solve_one(hp, tb.params(SETNAME), loss)
        lo, hi = tbd.bounds_between(hp.p0(), free["p"], b, every, frac)
        out.append(bb.solve_one(hp, tb.params(SETNAME, **dict(over)), loss, lo, hi))
        los.append(lo)
        his.append(hi)
        hp.dp.close()
    lo, hi = np.array(los), np.array(his)
    lo.setflags(write=False)
    hi.setflags(write=False)
    return out, lo, hi, Ms


def margin_of(orc):
    return min(r["margin"] for r in orc)


def held_problems(orc):
    return sum(bool(o["held"].any()) for o in orc)


def assert_margin(orc, recorded, what):
    """the floor, then the recorded figure to 5 %: before anything is compared"""
    m = margin_of(orc)
    print(f"{what}: smallest decision margin of the oracle's solves {m:.3g} (recorded {recorded:.3g})")
    assert m > MARGIN_FLOOR, f"{what}: margin {m:.3g}: the seeds no longer keep the decisions off the rounding edges"
    assert abs(m - recorded) <= 0.05 * recorded, "the generator or the oracle changed: choose the batches again"
