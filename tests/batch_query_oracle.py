"""The host side of the batch query-covariance tests (tests/test_dense_batch_query_gpu.py, ..._cpu.py): the cases, the points,
the query Jacobians and the expected Jq Sigma Jq^T / Jq Sigma Jobs^T Jobs Sigma Jq^T, all from HostProblem.eval(p[b]) at the
very p[b] handed to the library.  Nothing of the library under test computes a number here.

The points: the CPU oracle's solve of every problem from its p0 with the default parameters (lambda = 0 at every one of
them), so the cases are the same with and without a GPU.  Sigma by two independent host routes: ref_sigma of
tests/test_dense_batch_uncertainty_gpu.py (the oracle's packed JtJ, orc_dpptrf_L, orc_dpptrs_L on unit columns) -- the
reference of the GPU tests -- and np.linalg.inv(J^T J + lambda I) (LAPACK's LU), compared by tests/test_dense_batch_query_cpu.py.

Test infrastructure only."""
import functools

import numpy as np

from tests import oracle_api as oa
from tests import batch_oracle as bo
from tests.test_dense_batch_uncertainty_gpu import ref_sigma

EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
TOL = 1e-9                      # max |out - ref|_cd / sqrt(ref_cc ref_dd): the scaled tolerance of the covariance tests
B, NQ, SEED0 = 9, 3, 1          # 9 problems: not a multiple of any number of problems per workgroup (4, 2, 1 ... and 9 of 1)
QROWS = (1, 2, 16)
# one shape per size class of the kernels
PLAIN_SHAPES = [(3, 12), (6, 40), (16, 96), (24, 60), (32, 64), (48, 100), (64, 130)]
# ((N, M), Nobservations): the edges of the sweep's tile of 256 doubles (42 rows of 6), and one case inside at <48> and <64>
SANDWICH_CASES = [((6, 40), 0), ((6, 40), 1), ((6, 40), 39), ((6, 40), 40),
                  ((6, 90), 42), ((6, 90), 43), ((6, 90), 84), ((6, 90), 85),
                  ((48, 100), 37), ((64, 130), 71)]
ZERO_ROW = (4, 1)               # (problem, query) whose last row is all zero: the padding rule


def host_problem(N, M, seed, zero_col=-1):
    return bo.HostProblem(M, N, int(seed), EPS, NOISE, SPREAD, zero_col)


@functools.lru_cache(maxsize=None)
def solved(N, M, nb=B, seed0=SEED0):
    """(seeds, p (nb, N), [J_b]): the oracle's end point of every problem and its Jacobian there; lambda is 0 at all of them"""
    seeds = np.arange(seed0, seed0 + nb)
    p, Js = np.zeros((nb, N)), []
    for b, s in enumerate(seeds):
        hp = host_problem(N, M, s)
        r = bo.solve_one(hp, oa.default_params(), want_margin=False)
        assert r["norm2_x"] >= 0 and r["lambda_"] == 0.0
        p[b] = r["p"]
        Js.append(hp.eval(np.ascontiguousarray(p[b]))[1].copy())
        hp.dp.close()
    p.setflags(write=False)
    return seeds, p, Js


@functools.lru_cache(maxsize=None)
def queries(nb, Nq, Q, N, seed=7):
    """Jq (nb, Nq, Q, N) from a seeded normal distribution; the last row of query ZERO_ROW is all zero where it exists"""
    Jq = np.random.default_rng([seed, nb, Nq, Q, N]).standard_normal((nb, Nq, Q, N))
    zb, zq = ZERO_ROW
    if zb < nb and zq < Nq:
        Jq[zb, zq, Q - 1] = 0.0
    Jq.setflags(write=False)
    return Jq


def sigma_inv(J, lam):
    """the second host route: LAPACK's general inverse"""
    return np.linalg.inv(J.T @ J + lam * np.eye(J.shape[1]))


def blocks(Jq_b, S, Jobs=None):
    """the expected blocks (Nq, Q, Q) of one problem from its Sigma"""
    if Jobs is None:
        return np.stack([q @ S @ q.T for q in Jq_b])
    return np.stack([q @ S @ Jobs.T @ Jobs @ S @ q.T for q in Jq_b])


@functools.lru_cache(maxsize=None)
def expected(N, M, Q, nobs=-1, Nq=NQ, nb=B, route="oracle"):
    """(nb, Nq, Q, Q): nobs < 0 the plain form, otherwise the observations-only form over the first nobs rows"""
    _, _, Js = solved(N, M, nb)
    Jq = queries(nb, Nq, Q, N)
    sig = ref_sigma if route == "oracle" else sigma_inv
    ref = np.stack([blocks(Jq[b], sig(Js[b], 0.0), None if nobs < 0 else Js[b][:nobs]) for b in range(nb)])
    ref.setflags(write=False)
    return ref


def scaled_error(out, ref):
    """max over the blocks of |out - ref|_cd / sqrt(ref_cc ref_dd).  Where ref_cc ref_dd is 0 (a zero row of Jq, or
    Nobservations = 0) the expected entry is exactly 0 and so must `out` be: inf otherwise"""
    out, ref = np.asarray(out).reshape(-1, *ref.shape[-2:]), np.asarray(ref).reshape(-1, *ref.shape[-2:])
    worst = 0.0
    for o, r in zip(out, ref):
        d = np.sqrt(np.abs(np.diag(r)))
        den = np.outer(d, d)
        zero = den == 0.0
        if np.any(o[zero] != 0.0) or not np.all(np.isfinite(o)):
            return np.inf
        if np.any(~zero):
            worst = max(worst, float(np.max(np.abs(o - r)[~zero] / den[~zero])))
    return worst
