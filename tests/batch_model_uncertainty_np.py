"""What the tests of the fused uncertainty and query calls of the built-in models share (tests/test_dense_batch_model_uncertainty_
cpu.py, _gpu.py): the names of the four entry points, the batches with their data variants, the NumPy rows of either likelihood
and the covariance they give, and the constructed singular problem of the lambda loop.  The Gauss batches are those of
tests/batch_models_np.py, the Poisson ones those of tests/batch_poisson_oracle.py."""
import numpy as np

from libdogleg_amd.ctypes_defs import LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON, MODEL_GAUSS2D, MODEL_NSTATE
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po

NAMES = ("dogleg_amd_dense_batch_model_uncertainty", "dogleg_amd_dense_batch_model_uncertainty_device",
         "dogleg_amd_dense_batch_model_query_covariance", "dogleg_amd_dense_batch_model_query_covariance_device")
LIKELIHOODS = (LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON)
LK_NAMES = {LIKELIHOOD_GAUSS: "gauss", LIKELIHOOD_POISSON: "poisson"}
LEVEL = "high"               # the Poisson tables of the bit-for-bit tests (every case; "low" joins them against NumPy)
LAMBDA_INITIAL = 1e-10       # dense_batch_kernels.hip


def variants(case, likelihood):
    """(t_mode, with_scale) of a case's data: those of tests/test_dense_batch_model_gpu.py, a scale with GAUSS only"""
    if mz.is_2d(case[0]):
        return [(None, False), (None, True)] if likelihood == LIKELIHOOD_GAUSS else [(None, False)]
    if likelihood == LIKELIHOOD_GAUSS:
        return [(None, False), (None, True), ("shared", False), ("each", True)]
    return [(None, False), ("shared", False), ("each", False)]


def poisson_batch(case, level=LEVEL, t_mode=None, nb=mz.B):
    """the batch of a Poisson table with the abscissae of a data variant: batch_poisson_oracle.batch (t_mode None: exactly that),
    the truth and the start those of batch_models_np.problem for these abscissae at the level's counts"""
    table = (case, level)
    if t_mode is None:
        return po.batch(table, nb=nb)
    kind, _ = case
    N = MODEL_NSTATE[kind]
    M, w, h = mz.case_shape(case)
    seed0 = po.SEED0.get(table, 1)
    fac, off = po.LEVELS[level]
    ps = []
    for b in range(nb):
        q = mz.problem(case, seed0 + b, t_mode)
        truth, p0 = q["truth"].copy(), q["p0"].copy()
        p0[0] *= fac
        p0[N - 1] *= off / truth[N - 1]
        truth[0] *= fac
        truth[N - 1] = off
        f, _ = mz.model_eval(kind, truth, np.zeros(M), q["t"], None, w)
        rng = np.random.default_rng([31, kind, M, w, int(seed0 + b), 0 if level == "high" else 1])
        ps.append(dict(y=rng.poisson(f).astype(np.float64), p0=p0, truth=truth, t=q["t"]))
    los, his = zip(*[po.bounds_of(case, b, ps[b]["truth"]) for b in range(nb)])
    t = ps[0]["t"] if t_mode == "shared" else np.array([q["t"] for q in ps])
    return dict(kind=kind, M=M, width=w, height=h, y=np.array([q["y"] for q in ps]), p0=np.array([q["p0"] for q in ps]),
                truth=np.array([q["truth"] for q in ps]), t=t, scale=None, lo=np.array(los), hi=np.array(his), t_mode=t_mode)


def batch_of(case, likelihood, t_mode=None, with_scale=False, nb=mz.B):
    if likelihood == LIKELIHOOD_GAUSS:
        return mz.batch(case, nb=nb, t_mode=t_mode, with_scale=with_scale)
    assert not with_scale
    return poisson_batch(case, t_mode=t_mode, nb=nb)


def rows_np(bt, b, p, likelihood):
    """(x (M,), J (M, N)) of problem b at p: the adapter's rows, or those of the Fisher callback"""
    hp = mz.host_model(bt, b)
    if likelihood == LIKELIHOOD_GAUSS:
        return hp.eval(p)
    f, G = po.model_values(hp, p)
    with np.errstate(all="ignore"):
        q = 1.0 / np.sqrt(f)
        return (f - hp.y) * q, G * q[:, None]


def sigma_np(bt, b, p, lam, held, likelihood):
    """(J'J + lam I)^-1 on the free variables of problem b, zeros in the held rows and columns; and the free mask"""
    N = p.shape[0]
    _, J = rows_np(bt, b, p, likelihood)
    free = np.ones(N, dtype=bool) if held is None else np.asarray(held) == 0
    S = np.zeros((N, N))
    if free.any():
        S[np.ix_(free, free)] = np.linalg.inv((J.T @ J + lam * np.eye(N))[np.ix_(free, free)])
    return S, free


def singular_batch(likelihood, nb=3):
    """GAUSS2D 7 x 7 problems whose amplitude is exactly 0 at the point of the call: the columns of x0, y0 and sigma of J vanish, so
    J'J is singular and the first pivot of those columns is an exact 0.  f = c > 0: feasible under either likelihood.  Returns
    (the batch, the points)"""
    case = (MODEL_GAUSS2D, (7, 7))
    bt = batch_of(case, likelihood, nb=nb)
    p = bt["truth"].copy()
    p[:, 0] = 0.0
    return bt, p
