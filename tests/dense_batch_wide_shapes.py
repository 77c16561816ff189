"""The shapes at which tests/test_dense_batch_wide_gpu.py runs the size classes <48> and <64> of dense_batch.hip (problems
of 33 .. 64 variables), with what the oracle alone says about them; tests/test_dense_batch_wide_cpu.py asserts all of it
without a GPU.  Test infrastructure, as tests/dense_batch_shapes.py: the CPU oracles (tests/batch_oracle.py,
tests/batch_products_oracle.py) and the host reference of tests/test_dense_batch_uncertainty_gpu.py; nothing of the library
under test computes a number in here.

Every batch is B = 33 problems, seeds 1 .. 33: 16 workgroups of two problems and one wavefront alone in the 17th at <48>,
33 workgroups of one at <64>.  The margins are the smallest decision margin of the batch's problems (batch_oracle.margin),
all above MARGIN_FLOOR = 1e-6."""
import functools

import numpy as np

from tests import dense_batch_shapes as ds
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu
from tests import batch_products_oracle as po

# ---------------------------------------------------------------- restated from libdogleg_amd/csrc/dense_batch.hip
BATCH_TILE = ds.BATCH_TILE


def size_class(N):
    """NMAX of the instantiation that launch_round / launch_uncertainty choose"""
    return ds.size_class(N) if N <= 32 else 48 if N <= 48 else 64


def problems_per_workgroup(N):
    """BatchCfg<NMAX>::WPB"""
    return {48: 2, 64: 1}.get(size_class(N), 4)


def T(N):
    """rows per tile of sweep_point: unchanged, 256 doubles"""
    return ds.T(N)


def T2(N, fs):
    """rows per tile of the second sweep of unc_problem: above 32 variables the tile is the SCR region of the class, NP(NMAX)
    doubles, rows at stride N | 1"""
    if N <= 32:
        return ds.T2(N, fs)
    t = min(64, ds.n_packed(size_class(N)) // (N | 1))
    return t & ~1 if fs == 2 else t


# ---------------------------------------------------------------- the cases
B, SEED0 = 33, 1
# (N, M): {set: the margin recorded}; T = 7 / 6 / 5 / 5 / 4 / 4
CASES = {
    (33, 70): {"diverse": 2.6e-3, "default": 7.6e-3},        # <48>, T 7: exactly 10 tiles
    (40, 97): {"diverse": 1.03e-2, "default": 2.49e-2},      # <48>, T 6: 16 tiles + 1 row
    (48, 100): {"diverse": 8.32e-3, "default": 5.88e-2},     # <48>, T 5: exactly 20 tiles
    (49, 103): {"diverse": 1.75e-2, "default": 9.28e-3},     # <64>, T 5: 20 tiles + 3 rows
    (63, 131): {"diverse": 8.25e-4, "default": 3.11e-2},     # <64>, T 4: 32 tiles + 3 rows
    (64, 128): {"diverse": 4.98e-3, "default": 3.43e-3},     # <64>, T 4: exactly 32 tiles
}
# rejected trials under the "hard" set: (N, M): (the margin recorded, rejected trials in the oracle's solves)
RETRY = {(33, 70): (3.16e-4, 2), (64, 128): (4.73e-3, 1)}
# the other two shapes of the issue's table that reject a trial (asserted on the CPU only)
RETRY_CPU_ONLY = {(40, 97): (1.04e-2, 1), (63, 131): (8.61e-4, 1)}
# a zero column (the last) in problems 3, 17, 30 of 32, "default": (N, M): (column, the margin recorded)
ZERO_COLUMN = {(48, 100): (47, 5.88e-2), (64, 128): (63, 3.43e-3)}
ZERO_B, ZERO_CHOSEN = ds.ZERO_B, ds.ZERO_CHOSEN
# M < N under "default", seeds 1 .. 16, max_iterations 6: (N, M): the margin recorded (floor 1e-2, p to 1e-3)
UNDER = {(40, 12): 0.196, (64, 20): 0.25}
UNDER_B, UNDER_OVER, UNDER_MARGIN_FLOOR, UNDER_P_TOL = ds.UNDER_B, ds.UNDER_OVER, ds.UNDER_MARGIN_FLOOR, ds.UNDER_P_TOL
# bit for bit, whatever the order and the neighbours: B = 65, problems 0, 32, 64 alone.  <64> runs 65 workgroups of one;
# (48, 100) is there for <48>, whose 33rd workgroup is half empty
NEIGHBOUR_SHAPES, NEIGHBOUR_B, NEIGHBOUR_ALONE = [(48, 100), (49, 103), (64, 128)], 65, (0, 32, 64)
# the uncertainty call: the six shapes; (40, 97), (49, 103), (63, 131) have an odd M
UNC_CASES = sorted(CASES)
UNC_ZERO_SHAPE, UNC_ZERO_COLUMN = (48, 100), 47
UNC_NAN_SHAPE, UNC_NAN_B, UNC_NAN_BAD = (64, 128), 8, (1, 5, 7)
# the products form: the J-form shapes of N = 33, 48, 64 (the same problems, so the J form's margins), and per N one
# ragged batch, M from N + 7 to 2 N + 12: N: ((Mmin, Mmax), {set: the margin recorded})
PRODUCTS_SHAPES = [(33, 70), (48, 100), (64, 128)]
RAGGED = {
    33: ((40, 78), {"diverse": 4.70e-3, "default": 7.86e-2}),
    48: ((55, 108), {"diverse": 3.29e-3, "default": 3.37e-2}),
    64: ((71, 140), {"diverse": 3.62e-3, "default": 1.17e-2}),
}
# the Jacobian check of a batch callback
GRADCHECK_SHAPE, GRADCHECK_B, GRADCHECK_FAULT = (64, 70), 3, (2, 69, 63)        # (problem, measurement, variable)
REFUSED_NSTATE = 65

recorded = ds.recorded


def under_oracle(shape):
    N, M = shape
    return tb.oracle_batch(N, M, 1, UNDER_B, "default", UNDER_OVER)


@functools.lru_cache(maxsize=None)
def zero_oracle(shape):
    return tb.zero_column_oracle(tb.params("default"), ZERO_B, ZERO_CHOSEN, ZERO_COLUMN[shape][0], shape)


def ragged_oracle(N, setname):
    return po.oracle_batch(N, 0, SEED0, B, setname, ragged=RAGGED[N][0])


# ---------------------------------------------------------------- how far the host reference itself can be trusted
@functools.lru_cache(maxsize=None)
def host_agreement(shape):
    """ds.host_agreement on the B = 33 problems of `shape`: the reference Sigma (the oracle's packed Cholesky) against
    LAPACK's inverse of J'J in the scaled measure of tu.check_against_reference, the factors of the one against the factors
    of the other for both feature sizes, and the conditioning: dict(sigma, factors, cond, leverage, mindet, n_dbl_max,
    lambda_max)"""
    N, M = shape
    orc = tb.oracle_batch(N, M, SEED0, B, "default")
    out = dict(sigma=0.0, factors=0.0, cond=0.0, leverage=0.0, mindet=np.inf, n_dbl_max=0, lambda_max=0.0)
    for b, o in enumerate(orc):
        out["lambda_max"] = max(out["lambda_max"], o["lambda_"])
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
