"""The shapes at which tests/test_dense_batch_shapes_gpu.py runs dense_batch.hip, with what the oracle alone says about
them; tests/test_dense_batch_shapes_cpu.py asserts all of it without a GPU.  Test infrastructure: the CPU oracle
(tests/batch_oracle.py through the cached oracle_batch of tests/test_dense_batch_gpu.py) and the host reference of
tests/test_dense_batch_uncertainty_gpu.py; nothing of the library under test computes a number in here.

The margins are the smallest decision margin of the B problems seed0 .. seed0 + B - 1 (batch_oracle.margin), found with
batch_oracle.find_seed0 against MARGIN_FLOOR = 1e-6; seed0 = 1 passed at every shape under both parameter sets."""
import functools

import numpy as np

from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu

# ---------------------------------------------------------------- restated from libdogleg_amd/csrc/dense_batch.hip
BATCH_TILE = 256                        # doubles of J staged per tile (64 of x lie behind them)


def size_class(N):
    """NMAX of the k_batch_round / k_batch_uncertainty instantiation that launch_batch_round / launch_batch_uncertainty pick"""
    return 8 if N <= 8 else 16 if N <= 16 else 24 if N <= 24 else 32


def n_packed(N):
    """entries of the packed triangle: the loops `for(e = lane; e < NP; e += 64)` make ceil(NP / 64) passes"""
    return N * (N + 1) // 2


def T(N):
    """rows per tile of sweep_point"""
    return min(64, BATCH_TILE // N)


def T2(N, fs):
    """rows per tile of the second sweep of unc_problem (row stride N | 1 in LDS)"""
    t = min(T(N), (BATCH_TILE + 64) // (N | 1))
    return t & ~1 if fs == 2 else t


# ---------------------------------------------------------------- the cases
B, SEED0 = 65, 1                        # 16 whole workgroups and one wavefront alone in the 17th
# (N, M): {set: the margin the search recorded}
CASES = {
    (1, 5): {"diverse": 1.21e-2, "default": 1.70e-2},        # T 64: one partial tile
    (2, 9): {"diverse": 8.91e-3, "default": 3.04e-2},        # T 64: one partial tile
    (5, 103): {"diverse": 1.06e-2, "default": 3.14e-3},      # T 51: 2 tiles + 1 row
    (8, 32): {"diverse": 7.26e-5, "default": 1.09e-2},       # T 32: exactly one tile
    (8, 33): {"diverse": 5.19e-3, "default": 3.54e-2},       # T 32: 1 tile + 1 row
    (9, 55): {"diverse": 3.96e-3, "default": 1.40e-2},       # T 28: 1 tile + 27 rows
    (16, 50): {"diverse": 8.41e-2, "default": 1.55e-2},      # T 16: 3 tiles + 2 rows
    (17, 40): {"diverse": 2.30e-2, "default": 5.96e-3},      # T 15: 2 tiles + 10 rows
    (24, 73): {"diverse": 9.57e-3, "default": 7.50e-3},      # T 10: 7 tiles + 3 rows
    (25, 81): {"diverse": 2.91e-3, "default": 7.31e-5},      # T 10: 8 tiles + 1 row
    (31, 47): {"diverse": 5.35e-3, "default": 2.76e-2},      # T 8: 5 tiles + 7 rows
}
# one measurement of one state: a case of its own
ONE_BY_ONE = {(1, 1): {"diverse": 8.21e-3, "default": 8.67e-2}}
# the uncertainty call: M > N + 1 (the scale is computed); (17, 41) for (17, 40): an odd M beside the even T2(17, 2) = 14;
# (11, 47): T2 23 -> 22 under featureSize 2, and an odd M
UNC_CASES = [(1, 5), (2, 9), (5, 103), (8, 32), (8, 33), (9, 55), (11, 47), (16, 50), (17, 41), (24, 73), (25, 81), (31, 47)]
UNC_B = B
UNC_ZERO_SHAPE, UNC_ZERO_COLUMN = (24, 73), 17         # the lambda loop of the uncertainty kernel, 3 problems of 32
# rejected trials under the "hard" set: (N, M): (seed0, B, the margin recorded, rejected trials in the oracle's solves)
RETRY = {(32, 70): (1, 33, 7.70e-3, 2), (24, 73): (1195, 33, 1.07e-2, 1)}
# a zero column in problems 3, 17, 30 of 32: (N, M): (column, the margin recorded)
ZERO_COLUMN = {(24, 73): (17, 7.83e-3), (32, 70): (31, 1.30e-2)}
ZERO_B, ZERO_CHOSEN = 32, (3, 17, 30)
# M < N under "default", seeds 1 .. 16, max_iterations 6: (N, M): the margin recorded.  Compared to 1e-3 in p (cond(JtJ +
# 1e-10 I) ~ 1e11), so the margin has to stand a decade over that: UNDER_MARGIN_FLOOR.  (24, 9), margin 1.3e-3, does not
# and is left out; (20, 9) runs the <24> instantiation in its place.
UNDER = {(10, 6): 1.11e-1, (20, 9): 2.50e-1}
UNDER_LEFT_OUT = {(24, 9): 1.30e-3}
UNDER_B, UNDER_OVER, UNDER_MARGIN_FLOOR, UNDER_P_TOL = 16, (("max_iterations", 6),), 1e-2, 1e-3
# bit for bit, whatever the order and the neighbours
NEIGHBOUR_SHAPES, NEIGHBOUR_B, NEIGHBOUR_ALONE = [(24, 73), (31, 47)], 257, (0, 100, 256)


def under_oracle(shape):
    N, M = shape
    return tb.oracle_batch(N, M, 1, UNDER_B, "default", UNDER_OVER)


@functools.lru_cache(maxsize=None)
def zero_oracle(shape):
    return tb.zero_column_oracle(tb.params("default"), ZERO_B, ZERO_CHOSEN, ZERO_COLUMN[shape][0], shape)


def recorded(m, want):
    """a margin against the one the search recorded, the way test_parity_over_a_batch asserts it"""
    return abs(m - want) <= 0.05 * want


# ---------------------------------------------------------------- how far the host reference itself can be trusted
@functools.lru_cache(maxsize=None)
def host_agreement(shape):
    """at the oracle's end points of the "default" problems 1 .. UNC_B of `shape`: the reference Sigma (the oracle's packed
    Cholesky, tu.ref_sigma) against LAPACK's inverse of J'J in the scaled measure of tu.check_against_reference, the factors
    of the one against the factors of the other for both feature sizes, and what the conditioning is:
    dict(sigma, factors, cond, leverage, mindet, n_dbl_max)"""
    N, M = shape
    orc = tb.oracle_batch(N, M, SEED0, UNC_B, "default")
    out = dict(sigma=0.0, factors=0.0, cond=0.0, leverage=0.0, mindet=np.inf, n_dbl_max=0)
    for b, o in enumerate(orc):
        assert o["lambda_"] == 0.0
        x, J, S = tu.reference(N, M, SEED0 + b, o["p"], 0.0)
        G = J.T @ J
        S2 = np.linalg.inv(G)
        d = np.sqrt(np.diag(S))
        out["sigma"] = max(out["sigma"], float(np.max(np.abs(S2 - S) / np.outer(d, d))))
        out["cond"] = max(out["cond"], float(np.linalg.cond(G)))
        H = J @ S @ J.T
        out["leverage"] = max(out["leverage"], float(np.max(np.diag(H))))
        out["mindet"] = min([out["mindet"], float(np.min(np.abs(1.0 - np.diag(H))))]
                            + [abs(float(np.linalg.det(H[f:f + 2, f:f + 2] - np.eye(2)))) for f in range(0, M - 1, 2)])
        sc = tu.ref_scale(M, N, float(x @ x))
        for fs in (1, 2):
            f1, f2 = tu.ref_factors(S, x, J, fs, sc), tu.ref_factors(S2, x, J, fs, sc)
            out["n_dbl_max"] += int((f1 == tu.DBL_MAX).sum() + (f2 == tu.DBL_MAX).sum())
            out["factors"] = max(out["factors"],
                                 float(np.max(np.abs(f1 - f2) / np.maximum(np.abs(f1), tu.FAC_ATOL / tu.FAC_RTOL))))
    return out
