"""The cases of the robust device solve's tests (tests/test_device_robust_cpu.py, tests/test_device_robust_gpu.py): problems,
parameters, planted outliers, the NumPy oracle's solve of each (tests/batch_robust_oracle.py, cached: the tests share them) and
the smallest decision margin the oracle recorded for it.

The seeds were chosen on the CPU, with the oracle alone, such that every case's margin is above MARGIN_FLOOR = 1e-6 -- the
scheme and the floor of tests/test_dense_batch_robust_gpu.py: no case is left out, the margin is written beside the case and
asserted to 5 % before anything is compared.  Parameters: trustregion0 = 3, max_iterations = 30, update_threshold =
Jt_x_threshold = 1e-6 (with the planted outliers F is dominated by their rho, so the last steps of a solve to 1e-8 improve F
by less than its rounding error and their gain ratios are noise on any implementation: negative margins), loss scale 0.05,
5 % of the features displaced by +-1.0 (problems/batch_offsets.py's planted_offsets with the problem's seed).
Seed 4 of the (12, 120, 720) shape gives negative margins for Huber and soft-L1: it is not used.

The parked-backend sequence (patterns A, A, B of equal N, M and nnz: one camera less, two points more) is that of
tests/test_device_eval_gpu.py at a smaller size, (9, 100, 700) and (8, 102, 700) with N = 354: the oracle's Cholesky is a
Python loop over the columns and takes half a minute a solve at that test's N = 1338."""
import functools

from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY
from problems.batch_offsets import planted_offsets
from problems.device_robust import OffsetHostModel
from tests import batch_robust_oracle as ro
from tests import oracle_api as oa

MARGIN_FLOOR = 1e-6
SCALE, FRACTION, SIZE = 0.05, 0.05, 1.0
KINDS = {"trivial": LOSS_TRIVIAL, "huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}

# name: (constructor, arguments, keywords); the seed also chooses the planted features
PROBLEMS = {
    "ba_small": (oa.BAProblem, (5, 20, 60), dict(seed=1, eps=0.4, p0_spread=0.6)),            # N 96, M 120, nnz 1 800
    "ba_medium": (oa.BAProblem, (12, 120, 720), dict(seed=5, eps=0.4, p0_spread=0.6)),        # N 438, M 1 440, nnz 21 600
    "dense_small": (oa.DenseProblem, (), dict(M=60, N=6, seed=1)),
    "dense_medium": (oa.DenseProblem, (), dict(M=600, N=48, seed=1)),
    "parked_a": (oa.BAProblem, (9, 100, 700), dict(seed=21, eps=0.4, p0_spread=0.5)),         # N 354, M 1 400, nnz 12 600
    "parked_b": (oa.BAProblem, (8, 102, 700), dict(seed=22, eps=0.4, p0_spread=0.5)),
}

# (problem, featureSize, loss): the margin recorded
MARGINS = {
    ("ba_small", 1, "trivial"): 0.228, ("ba_small", 1, "huber"): 0.00239, ("ba_small", 1, "soft_l1"): 0.762, ("ba_small", 1, "cauchy"): 0.607,
    ("ba_small", 2, "trivial"): 0.226, ("ba_small", 2, "huber"): 0.00531, ("ba_small", 2, "soft_l1"): 0.162, ("ba_small", 2, "cauchy"): 0.298,
    ("ba_small", 3, "trivial"): 0.223, ("ba_small", 3, "huber"): 0.00504, ("ba_small", 3, "soft_l1"): 0.19, ("ba_small", 3, "cauchy"): 0.274,
    ("ba_small", 4, "trivial"): 0.203, ("ba_small", 4, "huber"): 0.00554, ("ba_small", 4, "soft_l1"): 0.752, ("ba_small", 4, "cauchy"): 0.306,
    ("ba_medium", 2, "trivial"): 0.0178, ("ba_medium", 2, "huber"): 0.000109, ("ba_medium", 2, "soft_l1"): 0.107, ("ba_medium", 2, "cauchy"): 0.297,
    ("dense_small", 2, "trivial"): 0.25, ("dense_small", 2, "huber"): 0.0476, ("dense_small", 2, "soft_l1"): 0.265, ("dense_small", 2, "cauchy"): 0.265,
    ("dense_medium", 2, "trivial"): 0.236, ("dense_medium", 2, "huber"): 0.0325, ("dense_medium", 2, "soft_l1"): 0.272, ("dense_medium", 2, "cauchy"): 0.281,
    ("parked_a", 2, "huber"): 0.00682, ("parked_a", 2, "cauchy"): 0.296, ("parked_b", 2, "huber"): 0.0262, ("parked_b", 2, "cauchy"): 0.0127,
}


def problem(name):
    """a fresh instance (the caller closes it)"""
    ctor, args, kw = PROBLEMS[name]
    return ctor(*args, **kw)


def params(**over):
    prm = oa.default_params()
    prm.trustregion0 = 3.0
    prm.max_iterations = 30
    prm.update_threshold = prm.Jt_x_threshold = 1e-6
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def loss_of(kind, fs):
    return BatchLoss(KINDS[kind], SCALE, fs)


def offsets(name, fs):
    """(off (M,), planted (M // fs,) bool)"""
    prob = problem(name)
    M = prob.M
    prob.close()
    off, planted = planted_offsets(1, M, fs, FRACTION, SIZE, PROBLEMS[name][2]["seed"])
    return off[0], planted[0]


@functools.lru_cache(maxsize=None)
def oracle(name, fs, kind):
    """the oracle's solve_one of the case (read only: the tests share it)"""
    prob = problem(name)
    out = ro.solve_one(OffsetHostModel(prob, offsets(name, fs)[0]), params(), ro.Loss(KINDS[kind], SCALE, fs))
    prob.close()
    return out


def assert_margin(case):
    o = oracle(*case)
    m, recorded = o["margin"], MARGINS[case]
    print(f"{case}: smallest decision margin of the oracle's solve {m:.3g} (recorded {recorded:.3g}), {o['iterations']} accepted "
          f"steps, {o['evaluations']} evaluations, status {o['status']}")
    assert m > MARGIN_FLOOR, f"{case}: margin {m:.3g}: the seed no longer keeps the decisions off the rounding edges"
    assert abs(m - recorded) <= 0.05 * recorded, "the generator or the oracle changed: choose the seed again"
    return o
