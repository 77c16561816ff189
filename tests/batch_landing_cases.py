"""The fallback's landing (step 6 of the bounded batch loop, include/dogleg.h above dogleg_amd_optimize_dense_batch_bounded): the
cases the landing tests share, CPU and GPU.  The oracle is tests/batch_bounds_oracle.py (fallback_step states the rule).

1. A linear family whose landing is the same on every implementation.  J = [[1, 0.9375], [0, 0.3125]], y = (0.140625, 0.375),
   p0 = 0, upper = (inf, u), trustregion0 = 10.  Every entry is a short dyadic number, so JtJ = [[1, 0.9375], [0.9375, 0.9765625]],
   Jt x = (-0.140625, -0.2490234375), g'g and g'Hg are exact in any order of summation, contracted or not; k = -g'g / g'Hg and
   u / d_1 are single divisions, min(1, tr / |cauchy|) is 1, and 0 + alpha d_1 has one rounding either way.  The first step is the
   Gauss-Newton step (-0.984375, 1.2); clipped at u its expected improvement is negative, so the fallback is taken and cut at u.
   Whether round(round(u / d_1) d_1) falls short of u depends on u alone: LANDING_U lists 16 bounds drawn by
   default_rng(1).uniform(0.05, 0.2, 600) with the class NumPy's sum gives each.  One ulp short the variable is on no bound, is
   not held at the next point, the next fallback is cut at alpha ~ 1e-16 and the solve stops on update_threshold at p_0 ~ 0.064,
   where the bounded optimum has p_0 ~ 0.034: what the landing rule removes.
   embedded(N, at) puts the pair at variables (at, at + 1) of N: the other variables get identity rows and data 0, so g = 0 and
   d = 0 there and they decide nothing.
2. Batches of the built-in models, least squares and Poisson, whose bounded solves take fallbacks that are cut at a bound: their
   rows go through exp, so no landing can be predicted bit for bit, but the rule makes the landing a decision with a margin
   like any other.  The seeds were chosen on the CPU with the oracle alone: FIT_SEEDS[form, case] lists the seed of problem b;
   problem b has the bounds of phase b mod 6 of the form's own tables (tests/batch_models_np.py, tests/batch_poisson_oracle.py).
   The 1D kinds have abscissae of their own per problem (t_mode "each")."""
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import LOSS_TRIVIAL, MODEL_GAUSS1D, MODEL_GAUSS2D, MODEL_NSTATE, LIKELIHOOD_POISSON
from problems.batch_linear import LinearHostProblem, exact_bounded_solution
from tests import batch_bounds_oracle as bb
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_gpu as tb

MARGIN_FLOOR = tb.MARGIN_FLOOR
KKT_TOL = 1e-9

# ---------------------------------------------------------------- 1. the linear family
PAIR_J = np.array([[1.0, 0.9375], [0.0, 0.3125]])
PAIR_Y = np.array([0.140625, 0.375])
TRUSTREGION0 = 10.0
LANDING_U = (
    (0.11349896734588635, "short"), (0.059352436872481346, "short"), (0.08018048010869967, "short"),
    (0.11340753604181561, "short"), (0.05367360162400448, "short"), (0.05689807710057735, "short"),
    (0.1187119340729179, "short"), (0.07474908919227316, "short"), (0.10756032166776114, "short"),
    (0.1267732437050385, "on"), (0.19256955444889035, "on"), (0.07162394190794506, "on"), (0.09677471780157282, "on"),
    (0.0746760899711152, "beyond"), (0.061562571275080816, "beyond"), (0.10714723089396314, "beyond"),
)
SIZES = (2, 8, 9, 17, 33, 49, 64)          # one per size class, 8 twice: the pair alone and among others


def placements(N):
    """where the pair sits: the first two variables and the last two (the landing in the last lanes; at N = 64 bit 63 of the
    held ballot)"""
    return (0,) if N == 2 else (0, N - 2)


def params():
    prm = tb.params("default")
    prm.trustregion0 = TRUSTREGION0
    return prm


def embedded(N, at, u):
    """(A (N, N), y (N,), p0 (N,), lo (N,), hi (N,)) of the pair at variables (at, at + 1) under the upper bound u"""
    A, y = np.eye(N), np.zeros(N)
    A[at:at + 2, at:at + 2] = PAIR_J
    y[at:at + 2] = PAIR_Y
    hi = np.full(N, np.inf)
    hi[at + 1] = u
    return A, y, np.zeros(N), np.full(N, -np.inf), hi


@functools.lru_cache(maxsize=None)
def linear_batch(N, at):
    """(A (16, N, N), y (16, N), p0, lo, hi) of LANDING_U; read only: the tests share it"""
    return tuple(np.array(a) for a in zip(*[embedded(N, at, u) for u, _ in LANDING_U]))


@functools.lru_cache(maxsize=None)
def linear_oracle(N, at, landing="bound"):
    """the oracle's solves of linear_batch(N, at); read only"""
    A, y, p0, lo, hi = linear_batch(N, at)
    return [bb.solve_one(LinearHostProblem(A[b], y[b], p0[b]), params(), ro.Loss(LOSS_TRIVIAL), lo[b], hi[b], landing=landing)
            for b in range(len(LANDING_U))]


@functools.lru_cache(maxsize=None)
def exact_pair(u):
    """the bounded optimum of the pair (by enumeration of the active sets)"""
    return exact_bounded_solution(PAIR_J, PAIR_Y, np.full(2, -np.inf), np.array([np.inf, u]))


def exact_embedded(N, at, u):
    p = np.zeros(N)
    p[at:at + 2] = exact_pair(u)
    return p


# ---------------------------------------------------------------- 2. the model batches
FIT_B = mz.B
FIT_CASES = ((MODEL_GAUSS1D, 65), (MODEL_GAUSS2D, (7, 7)))
POISSON_LEVEL = "high"
MIN_LANDINGS = 8
# the seed of problem b.  Problems b = 0, 6, .. and b = 3, 9, .. (the phases that take fallbacks) get the first seeds of 1 .. 400
# (Poisson: 1 .. 1600) whose solve under that phase's bounds has a cut landing, while there are any; the others the first seeds
# not used yet.  Every solve ends in JTX or SMALL_STEP with its smallest margin above 10 MARGIN_FLOOR (Poisson: and the cost's
# rounding allowance below COST_TOL); tests/test_dense_batch_landing_cpu.py asserts what the batches contain
FIT_SEEDS = {
    ("model", (MODEL_GAUSS1D, 65)): (
        4, 1, 2, 79, 3, 5, 12, 6, 7, 327, 8, 9, 19, 10, 11, 13, 14, 15, 41, 16, 17, 18, 20, 21, 44, 22, 23, 24, 25, 26, 50, 27, 28, 29,
        30, 31, 51, 32, 33, 34, 35, 36, 75, 37, 38, 39, 40, 42, 82, 43, 45, 46, 47, 48, 84, 49, 52, 53, 54, 55, 126, 56, 57, 58, 59),
    ("model", (MODEL_GAUSS2D, (7, 7))): (
        34, 1, 2, 101, 3, 4, 40, 5, 6, 150, 7, 8, 47, 9, 10, 11, 12, 13, 59, 14, 15, 16, 17, 18, 76, 19, 20, 21, 22, 23, 121, 24, 25,
        26, 27, 28, 131, 29, 30, 31, 32, 33, 140, 35, 36, 37, 38, 39, 204, 41, 42, 43, 44, 45, 350, 46, 48, 49, 50, 51, 356, 52, 53,
        54, 55),
    ("poisson", (MODEL_GAUSS1D, 65)): (
        29, 1, 2, 564, 3, 4, 138, 5, 6, 594, 7, 8, 160, 9, 10, 1443, 11, 12, 282, 13, 14, 15, 16, 17, 306, 18, 19, 20, 21, 22, 478,
        23, 24, 25, 26, 27, 655, 28, 30, 31, 32, 33, 709, 34, 35, 36, 37, 38, 803, 39, 40, 41, 42, 43, 843, 44, 45, 46, 47, 48, 1076,
        49, 50, 51, 52),
    ("poisson", (MODEL_GAUSS2D, (7, 7))): (
        30, 1, 2, 287, 3, 4, 115, 5, 6, 371, 7, 8, 118, 9, 10, 424, 11, 12, 121, 13, 14, 1023, 15, 16, 140, 17, 18, 19, 20, 21, 446,
        22, 23, 24, 25, 26, 508, 27, 28, 29, 31, 32, 907, 33, 34, 35, 36, 37, 1064, 38, 39, 40, 41, 42, 1114, 43, 44, 45, 46, 47,
        1198, 48, 49, 50, 51),
}


def fit_problem(form, case, seed):
    """dict(y, p0, truth, t) of one seed: tests/batch_models_np.problem with abscissae per problem for the 1D kinds; form
    "poisson": the truth and the start moved to the count level POISSON_LEVEL and Poisson data, as
    tests/batch_poisson_oracle.problem does it (with the abscissae, which that one does not take)"""
    kind, _ = case
    q = mz.problem(case, seed, t_mode=None if mz.is_2d(kind) else "each")
    if form == "model":
        return q
    N = MODEL_NSTATE[kind]
    M, w, _ = mz.case_shape(case)
    fac, off = po.LEVELS[POISSON_LEVEL]
    truth, p0 = q["truth"].copy(), q["p0"].copy()
    p0[0] *= fac
    p0[N - 1] *= off / truth[N - 1]
    truth[0] *= fac
    truth[N - 1] = off
    f, _ = mz.model_eval(kind, truth, np.zeros(M), q["t"], None, w)
    rng = np.random.default_rng([37, kind, M, w, int(seed)])
    return dict(y=rng.poisson(f).astype(np.float64), p0=p0, truth=truth, t=q["t"], scale=None)


def fit_bounds(form, case, phase, truth):
    return (mz if form == "model" else po).bounds_of(case, phase, truth)


def fit_params(form):
    return mz.params() if form == "model" else po.params()


def fit_solve(form, case, seed, phase, landing="bound"):
    """the oracle's bounded solve of one seed under the bounds of a phase"""
    q = fit_problem(form, case, seed)
    hp = mz.HostModel(case[0], q["y"], q["p0"], q["t"], None, mz.case_shape(case)[1])
    lo, hi = fit_bounds(form, case, phase, q["truth"])
    if form == "model":
        return bb.solve_one(hp, fit_params(form), ro.Loss(LOSS_TRIVIAL, 1.0, 1), lo, hi, landing=landing)
    return po.solve_one(hp, fit_params(form), LIKELIHOOD_POISSON, lo, hi, landing=landing)


def fit_batch(form, case):
    """the arrays of a batch, with the keys of tests/batch_models_np.batch"""
    kind, _ = case
    M, w, h = mz.case_shape(case)
    seeds = FIT_SEEDS[form, case]
    ps = [fit_problem(form, case, s) for s in seeds]
    los, his = zip(*[fit_bounds(form, case, b % 6, ps[b]["truth"]) for b in range(len(seeds))])
    each = not mz.is_2d(kind)
    return dict(kind=kind, M=M, width=w, height=h, y=np.array([q["y"] for q in ps]), p0=np.array([q["p0"] for q in ps]),
                truth=np.array([q["truth"] for q in ps]), t=np.array([q["t"] for q in ps]) if each else None, scale=None,
                lo=np.array(los), hi=np.array(his), t_mode="each" if each else None)


@functools.lru_cache(maxsize=None)
def fit_oracle(form, case, landing="bound"):
    """the oracle's solves of fit_batch(form, case); read only: the tests share it"""
    return [fit_solve(form, case, s, b % 6, landing) for b, s in enumerate(FIT_SEEDS[form, case])]
