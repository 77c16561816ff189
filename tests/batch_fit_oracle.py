"""The host side of the tests of the ..._fit uncertainty and query calls (tests/test_dense_batch_fit_gpu.py, ..._cpu.py): the
cases, the points, the held patterns and a NumPy reference of what include/dogleg.h writes above dogleg_amd_batch_fit_t, all
from HostProblem.eval / OffsetHostProblem.eval at the very p[b] handed to the library.  Nothing of the library under test
computes a number here.

The problems: the "default" set of tests/test_dense_batch_gpu.py with the planted outliers of tests/test_dense_batch_robust_gpu.py
(a tenth of the weight features displaced by 50 x the noise).  The points: the robust NumPy oracle's solve of every problem (its
p, lambda and weights), so the cases are the same with and without a GPU.

The reference of problem b, with w_f given or rho'(s_f) of the loss at x: rows times sqrt(w_f), H = J~' J~, A = H + lambda I
with the held rows and columns replaced by the identity's.  Sigma by two independent routes: "oracle", the C oracle's packed
Cholesky (orc_dpptrf_L, orc_dpptrs_L on unit columns) of the masked A with the held rows and columns cleared afterwards -- the
reference of the GPU tests --, and "inv", LAPACK's general inverse of the compacted free block scattered into zeros.  The
factors, a computed scale and both query forms follow the formulas of the header from that Sigma.

Test infrastructure only."""
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import LOSS_TRIVIAL, dptr
from problems.batch_offsets import OffsetHostProblem
from tests import oracle_api as oa
from tests import batch_oracle as bo
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_robust_gpu as rt

DBL_MAX = np.finfo(np.float64).max
SETNAME = "default"
B = 5                           # a batch of 5: not a multiple of the 4 or 2 problems of a workgroup
NQ, Q = 2, 3
# (N, M, fs of the factors, lfs of the weights, loss): one shape per size class of the kernels, M a multiple of lfs that leaves a
# ragged last tile at the weighted sweep's tile height T' = T - T mod lfs, T = min(64, 256 / N).  With lfs = 4 the classes above 32
# have T' = 4 and no M that is a multiple of lfs leaves a ragged tile: (48, 104) is the case of lfs 4 / fs 2 there, on whole tiles
CASES = [(3, 12, 1, 1, "huber"), (8, 36, 2, 4, "soft_l1"), (13, 40, 1, 2, "cauchy"), (24, 52, 2, 4, "huber"),
         (32, 68, 2, 2, "soft_l1"), (48, 102, 1, 2, "cauchy"), (48, 104, 2, 4, "huber"), (64, 134, 2, 2, "soft_l1")]
RAGGED = [c for c in CASES if c[:2] != (48, 104)]
HELD_PATTERNS = ("none", "first", "last", "third", "all_but_one", "all")
# the planted batch of tests/test_dense_batch_robust_gpu.py, every loss
PLANTED_SHAPE, PLANTED_LFS, PLANTED_B = rt.PARITY_SHAPE, rt.PARITY_FS, 9


def loss_of(kind, lfs):
    """(the oracle's loss, the library's BatchLoss)"""
    return ro.Loss(rt.KINDS[kind], rt.scale_of(SETNAME, lfs, rt.NEAR), lfs), rt.loss_of(kind, SETNAME, lfs, rt.NEAR)


def held_pattern(name, nb, N):
    """(nb, N) uint8, nonzero = held"""
    h = np.zeros((nb, N), dtype=np.uint8)
    i = np.arange(N)
    for b in range(nb):
        if name == "first":
            h[b, 0] = 1
        elif name == "last":
            h[b, N - 1] = 2
        elif name == "third":
            h[b, i % 3 == b % 3] = 1
        elif name == "all_but_one":
            h[b, i != b % N] = 2
        elif name == "all":
            h[b] = 1
    return h


def host_problem(N, M, lfs, seed, b, nb, zero_col=-1):
    """problem b of a planted batch of nb on the host"""
    eps, noise, spread, _ = tb.SETS[SETNAME]
    hp = bo.HostProblem(M, N, int(seed), eps, noise, spread, zero_col)
    return OffsetHostProblem(hp, rt.offsets_of(nb, M, lfs, SETNAME)[b])


@functools.lru_cache(maxsize=None)
def points(N, M, lfs, kind, nb=B):
    """(seeds, p (nb, N), lambda (nb,), weights (nb, M / lfs)) of the robust oracle's solves of the planted batch"""
    seeds = tuple(range(1, 1 + nb))
    orc = rt.oracle_batch(N, M, lfs, kind, seeds, SETNAME, rt.NEAR, True, rt.PLANTED_OVER)
    assert all(o["norm2_x"] >= 0 for o in orc)
    out = (np.array([o["p"] for o in orc]), np.array([float(o["lambda_"]) for o in orc]), np.array([o["weights"] for o in orc]))
    for a in out:
        a.setflags(write=False)
    return (seeds,) + out


@functools.lru_cache(maxsize=None)
def evaluated(N, M, lfs, kind, nb=B):
    """[(x, J)] of the batch at points()"""
    seeds, p, _, _ = points(N, M, lfs, kind, nb)
    out = []
    for b, s in enumerate(seeds):
        hp = host_problem(N, M, lfs, s, b, nb)
        x, J = hp.eval(np.ascontiguousarray(p[b]))
        out.append((x.copy(), J.copy()))
        hp.close()
    return out


def weighted_rows(x, J, lfs, w):
    sw = np.repeat(np.sqrt(w), lfs)
    return sw * x, sw[:, None] * J


def masked(H, lam, held):
    """H + lambda I with the held rows and columns those of the identity"""
    A = H + lam * np.eye(len(H))
    h = np.asarray(held) != 0
    A[h, :] = 0.0
    A[:, h] = 0.0
    A[h, h] = 1.0
    return A


def lambda_used(H, lam, held):
    """the lambda at which the masked matrix factorises: the solve's schedule"""
    while ro.cholesky(masked(H, lam, held)) is None:
        lam = ro.LAMBDA_INITIAL if lam == 0.0 else lam * 10.0
        assert np.isfinite(lam)
    return lam


def sigma(H, lam, held, route="oracle"):
    """Sigma with exact zeros in the held rows and columns"""
    N = len(H)
    h = np.asarray(held) != 0
    S = np.zeros((N, N))
    if route == "inv":
        f = np.flatnonzero(~h)
        if len(f):
            S[np.ix_(f, f)] = np.linalg.inv((H + lam * np.eye(N))[np.ix_(f, f)])
        return S
    A = masked(H, lam, held)
    O = oa.oracle()
    ap = np.ascontiguousarray(A[np.triu_indices(N)])            # row-major packed upper
    assert O.orc_dpptrf_L(N, dptr(ap)) == 0
    for c in np.flatnonzero(~h):
        e = np.zeros(N)
        e[c] = 1.0
        O.orc_dpptrs_L(N, dptr(ap), dptr(e))
        S[:, c] = e
    S[h, :] = 0.0
    return S


def scale_of(M, N_free, norm2_xt):
    return M / (4.0 * ((N_free + 1) * norm2_xt / (M - N_free - 1)))


def factors(S, xt, Jt, fs, scale):
    """include/dogleg.h above dogleg_getOutliernessFactors with A_f = J~_f Sigma J~_f^T and x~_f"""
    k = scale / 8.0
    out = np.zeros(len(xt) // fs)
    for f in range(len(out)):
        Jf, xf = Jt[f * fs:(f + 1) * fs], xt[f * fs:(f + 1) * fs]
        A = Jf @ S @ Jf.T
        if fs == 1:
            den = 1.0 - A[0, 0]
            out[f] = DBL_MAX if abs(den) < 1e-8 else xf[0] * xf[0] / den * k
        else:
            Mx = A - np.eye(2)
            det = Mx[0, 0] * Mx[1, 1] - Mx[0, 1] * Mx[1, 0]
            if abs(det) < 1e-8:
                out[f] = DBL_MAX
            else:
                Bm = np.linalg.inv(Mx)
                out[f] = float(xf @ (Bm + Bm @ Bm) @ xf) * k
    return out


def blocks(Jq_b, S, Jobs=None):
    if Jobs is None:
        return np.stack([q @ S @ q.T for q in Jq_b])
    G = Jobs.T @ Jobs
    return np.stack([q @ S @ G @ S @ q.T for q in Jq_b])


def reference(x, J, lam, held, lfs=1, w=None, loss=None, fs=1, scale=None, Jq=None, nobs=-1, route="oracle"):
    """what the fit calls give for one problem: dict(S, var, factors, scale, w, cond, and, with Jq (Nq, Q, N), blocks)
    w: the weights (M / lfs,), or None: from loss (a tests/batch_robust_oracle.py Loss, or None: unweighted)"""
    M, N = J.shape
    if w is None:
        w = np.ones(M // lfs) if loss is None or loss.kind == LOSS_TRIVIAL else loss.rho_w(loss.s(x))[1]
    xt, Jt = weighted_rows(x, J, lfs, w)
    H = Jt.T @ Jt
    S = sigma(H, lam, held, route)
    free = np.flatnonzero(np.asarray(held) == 0)
    out = dict(S=S, var=np.diag(S).copy(), w=w, xt=xt, Jt=Jt,
               cond=float(np.linalg.cond((H + lam * np.eye(N))[np.ix_(free, free)])) if len(free) else 1.0)
    out["scale"] = scale_of(M, len(free), float(xt @ xt)) if scale is None else scale
    out["factors"] = factors(S, xt, Jt, fs, out["scale"])
    if Jq is not None:
        out["blocks"] = blocks(Jq, S, None if nobs < 0 else Jt[:nobs])
    return out


@functools.lru_cache(maxsize=None)
def queries(nb, N, seed=11):
    Jq = np.random.default_rng([seed, nb, N]).standard_normal((nb, NQ, Q, N))
    Jq.setflags(write=False)
    return Jq


def cov_error(cov, S, held):
    """max |cov - S|_ij / sqrt(S_ii S_jj) over the free block; inf unless every held row and column of cov is exactly +0.0"""
    h = np.asarray(held) != 0
    z = np.concatenate([cov[h, :].ravel(), cov[:, h].ravel()])
    if np.any(z != 0.0) or np.any(np.signbit(z)):
        return np.inf
    f = np.flatnonzero(~h)
    if not len(f):
        return 0.0
    d = np.sqrt(np.diag(S)[f])
    return float(np.max(np.abs(cov - S)[np.ix_(f, f)] / np.outer(d, d)))
