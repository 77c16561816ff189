"""The cases of the bounded device solve's tests (tests/test_device_bounds_cpu.py, tests/test_device_bounds_gpu.py): problems,
parameters, bounds, the NumPy oracle's solve of each (tests/batch_bounds_oracle.py's solve_one on problems/device_robust.py's
OffsetHostModel, cached: the tests share them) and the smallest decision margin the oracle recorded for it.  Built as
tests/device_robust_cases.py is, whose problems and parameters it takes.

The bounds are bounds_between of tests/test_dense_batch_bounds_gpu.py: with p* the optimum the UNBOUNDED oracle finds from the
start point p0 under the case's own parameters and loss, every third variable (i = 0 mod 3) gets a bound at p*_i + frac (p0_i -
p*_i), a lower bound where the start lies above the optimum and an upper bound where it lies below: the start is feasible, the
unbounded optimum is not.

The cases were chosen on the CPU, with the oracle alone, such that every margin (the plain loop's decisions and those of the
held set, the clip and the fallback) is above MARGIN_FLOOR = 1e-6 -- no case is left out of a comparison; the margin is written
beside the case and asserted to 5 % before anything is compared.
  mild, frac 0.5, device_robust_cases.params(): the solve runs into the bounds and holds them; a few clipped steps, no fallback.
    The trivial loss runs without planted offsets, Huber (featureSize 2) with device_robust_cases' planted ones.
    BAProblem(12, 120, 720) is used with seed 3: seeds 1, 2, 5, 6 and 8 give negative margins at a 1e-6 stop.
  every branch, BAProblem(5, 20, 60, eps=1.5, p0_spread=2.0), frac 0.25, trustregion0 = 1000, both thresholds 1e-5,
    max_iterations = 30: fallbacks, rejected trials that are stepped again with held variables, all three kinds of step.
    Seed 1 (branch1) has one fallback whose p + alpha d lands on the bound or one ulp short of it by the last bit of the Cauchy
    step: the library puts the component that sets alpha on its bound either way, and so does the oracle
    (tests/batch_bounds_oracle.fallback_step, whose two margins -- is the step cut, which component lands -- are counted)."""
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import LOSS_TRIVIAL, LOSS_HUBER, BatchLoss
from problems.device_robust import OffsetHostModel
from tests import batch_bounds_oracle as bb
from tests import batch_robust_oracle as ro
from tests import device_robust_cases as dc
from tests import oracle_api as oa
from tests.test_dense_batch_bounds_gpu import bounds_between

MARGIN_FLOOR = 1e-6
BRANCH_OVER = dict(trustregion0=1000.0, update_threshold=1e-5, Jt_x_threshold=1e-5, max_iterations=30)

# name: (constructor, arguments, keywords, frac, parameter overrides, loss kind, featureSize)
CASES = {
    "ba_small": dc.PROBLEMS["ba_small"] + (0.5, {}, "trivial", 1),
    "ba_small_huber": dc.PROBLEMS["ba_small"] + (0.5, {}, "huber", 2),
    "dense_small": dc.PROBLEMS["dense_small"] + (0.5, {}, "trivial", 1),
    "dense_medium": dc.PROBLEMS["dense_medium"] + (0.5, {}, "trivial", 1),
    "ba_medium3": (oa.BAProblem, (12, 120, 720), dict(seed=3, eps=0.4, p0_spread=0.6), 0.5, {}, "trivial", 1),
    "branch2": (oa.BAProblem, (5, 20, 60), dict(seed=2, eps=1.5, p0_spread=2.0), 0.25, BRANCH_OVER, "trivial", 1),
    "branch4": (oa.BAProblem, (5, 20, 60), dict(seed=4, eps=1.5, p0_spread=2.0), 0.25, BRANCH_OVER, "trivial", 1),
    "branch1": (oa.BAProblem, (5, 20, 60), dict(seed=1, eps=1.5, p0_spread=2.0), 0.25, BRANCH_OVER, "trivial", 1),
    "parked_a": dc.PROBLEMS["parked_a"] + (0.5, {}, "trivial", 1),
    "parked_b": dc.PROBLEMS["parked_b"] + (0.5, {}, "trivial", 1),
}

# the margin recorded, and what the oracle's solve went through: variables held at the end, steps with a clamped component,
# fallbacks, rejected trials stepped again with held variables
MARGINS = {
    "ba_small": 4.10e-3, "ba_small_huber": 3.16e-3, "dense_small": 0.180, "dense_medium": 0.0514, "ba_medium3": 2.82e-4,
    "branch2": 1.16e-3, "branch4": 1.02e-3, "branch1": 2.85e-4, "parked_a": 9.61e-4, "parked_b": 2.29e-4,
}
RECORDED = {
    "ba_small": dict(held=28, clipped=2, fallbacks=0, held_resteps=0),
    "ba_small_huber": dict(held=31, clipped=5, fallbacks=0, held_resteps=0),
    "dense_small": dict(held=2, clipped=1, fallbacks=0, held_resteps=0),
    "dense_medium": dict(held=16, clipped=1, fallbacks=0, held_resteps=0),
    "ba_medium3": dict(held=133, clipped=3, fallbacks=0, held_resteps=0),
    "branch2": dict(held=8, clipped=17, fallbacks=9, held_resteps=5),
    "branch4": dict(held=22, clipped=29, fallbacks=14, held_resteps=5),
    "branch1": dict(held=26, clipped=29, fallbacks=13, held_resteps=6),
    "parked_a": dict(held=112, clipped=3, fallbacks=0, held_resteps=0),
    "parked_b": dict(held=109, clipped=3, fallbacks=0, held_resteps=0),
}
SPARSE = tuple(n for n in CASES if CASES[n][0] is oa.BAProblem and not n.startswith("parked"))
DENSE = tuple(n for n in CASES if CASES[n][0] is oa.DenseProblem)


def problem(name):
    """a fresh instance (the caller closes it)"""
    ctor, args, kw = CASES[name][:3]
    return ctor(*args, **kw)


def params(name, **over):
    return dc.params(**{**CASES[name][4], **over})


def loss_pair(name):
    """(the oracle's Loss, the library's BatchLoss or None for least squares)"""
    kind, fs = CASES[name][5:7]
    if kind == "trivial":
        return ro.Loss(LOSS_TRIVIAL, 0.0, 1), None
    assert kind == "huber"
    return ro.Loss(LOSS_HUBER, dc.SCALE, fs), BatchLoss(LOSS_HUBER, dc.SCALE, fs)


def offsets(name):
    """(M,) added to x: device_robust_cases' planted offsets of the problem's seed with a loss, zeros without"""
    prob = problem(name)
    M = prob.M
    prob.close()
    kind, fs = CASES[name][5:7]
    if kind == "trivial":
        return np.zeros(M)
    from problems.batch_offsets import planted_offsets
    return planted_offsets(1, M, fs, dc.FRACTION, dc.SIZE, CASES[name][2]["seed"])[0][0]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(the bounded oracle's solve_one, lo, hi, the unbounded oracle's solve) of the case (read only: the tests share it)"""
    prob = problem(name)
    hm = OffsetHostModel(prob, offsets(name))
    loss = loss_pair(name)[0]
    free = ro.solve_one(hm, params(name), loss)
    lo, hi = bounds_between(hm.p0(), free["p"], 0, False, CASES[name][3])
    out = bb.solve_one(hm, params(name), loss, lo, hi)
    prob.close()
    return out, lo, hi, free


def assert_margin(name):
    o = oracle(name)[0]
    m, recorded = o["margin"], MARGINS[name]
    print(f"{name}: smallest decision margin of the oracle's solve {m:.3g} (recorded {recorded:.3g}), {o['iterations']} accepted "
          f"steps, {o['evaluations']} evaluations, status {o['status']}, {int(np.count_nonzero(o['held']))} held, {o['clipped']} "
          f"clipped steps, {o['fallbacks']} fallbacks, {o['held_steps']} steps with a held variable ({o['held_resteps']} behind a "
          f"rejected trial), kinds of step {sorted(o['step_types'])}")
    assert m > MARGIN_FLOOR, f"{name}: margin {m:.3g}: the case no longer keeps the decisions off the rounding edges"
    assert abs(m - recorded) <= 0.05 * recorded, "the generator or the oracle changed: choose the case again"
    return o
