"""The CPU oracle applied to every problem of a products batch: one oa.oracle_solve("products", ...) each, packed upper,
with a host products callback that wraps batch_oracle.HostProblem.eval on the problem's own M[b] rows (DenseProblem(Mb, ...)
is the first Mb rows of DenseProblem(Mmax, ...) of the same seed) and reduces them with the oracle's own primitives
(orc_norm2, orc_dense_Jt_x, orc_dense_JtJ_packed_upper).  The result dict and the decision margin are those of
tests/batch_oracle.py, reused by import.  Test infrastructure: nothing of the library under test computes a number here."""
import ctypes as C
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import (CB_PRODUCTS, BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS,
                                       dptr)
from tests import oracle_api as oa
from tests import batch_oracle as bo

# name: (eps, noise, p0_spread, trustregion0) -- the sets of tests/test_dense_batch_gpu.py
SETS = {"diverse": (0.9, 0.01, 2.0, 1.0), "default": (0.3, 0.01, 0.5, 1.0e3), "hard": (0.95, 0.01, 6.0, 1.0e3)}
MARGIN_FLOOR = 1e-6


def params(setname, **over):
    """the parameters of a set, packed upper (what the oracle's products solve is run with)"""
    prm = oa.default_params()
    prm.trustregion0 = SETS[setname][3]
    prm.JtJ_packed = prm.JtJ_upper = True
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def ragged_M(B, Mmin, Mmax):
    """M[b] = Mmin + 7 b mod (Mmax - Mmin + 1)"""
    return Mmin + (7 * np.arange(B)) % (Mmax - Mmin + 1)


class HostProductsProblem:
    """HostProblem(M, N, seed, ...) behind a dogleg_callback_dense_products_t, packed upper"""

    def __init__(self, M, N, seed, eps, noise, p0_spread, zero_col=-1):
        self.hp = bo.HostProblem(M, N, seed, eps, noise, p0_spread, zero_col)
        self.M, self.N = M, N
        O = oa.oracle()
        hp = self.hp

        def products(p, norm2x, xtJ, JtJ, cookie):
            x, J = hp.eval(np.ctypeslib.as_array(p, shape=(N,)).copy())
            J = np.ascontiguousarray(J)
            norm2x[0] = O.orc_norm2(dptr(x), M)
            O.orc_dense_Jt_x(xtJ, dptr(J), dptr(x), M, N)
            C.memset(JtJ, 0, 8 * (N * (N + 1) // 2))           # (the primitive accumulates)
            O.orc_dense_JtJ_packed_upper(JtJ, dptr(J), M, N)

        self._keep = CB_PRODUCTS(products)
        self.cb, self.cookie = C.cast(self._keep, C.c_void_p), None

    def p0(self):
        return self.hp.p0()

    def eval(self, p):
        return self.hp.eval(p)

    def close(self):
        self.hp.dp.close()


def solve_one(pp, prm, want_margin=True):
    """the products oracle on one problem: the dict of batch_oracle.solve_one"""
    p0 = pp.p0()
    r, p, tr = oa.oracle_solve("products", p0, pp.N, 0, 0, pp.cb, pp.cookie, prm, capacity=1024)
    trials = tr.trials()
    assert tr.c.ntrials <= tr.capacity
    iters = sum(1 for t in trials if t["accepted"] == 1)
    x, J = pp.eval(p)
    gmax_end = float(np.max(np.abs(J.T @ x)))
    if not trials:
        status = BATCH_JTX if gmax_end <= prm.Jt_x_threshold else BATCH_MAX_ITERATIONS
        trust, lam = prm.trustregion0, 0.0
    else:
        last = trials[-1]
        lam = last["lambda_"]
        if last["accepted"] == 2:
            status, trust = BATCH_SMALL_STEP, last["trustregion_before"]
        elif last["accepted"] == 1:
            status, trust = (BATCH_JTX if gmax_end <= prm.Jt_x_threshold else BATCH_MAX_ITERATIONS), last["trustregion_after"]
        else:
            status, trust = BATCH_TRUSTREGION, last["trustregion_after"]
    out = dict(p=p, norm2_x=r, trustregion=trust, lambda_=lam, iterations=iters, evaluations=tr.ncallbacks, status=status,
               step_types={t["step_type"] for t in trials}, rejected=sum(1 for t in trials if t["accepted"] == 0))
    if want_margin:
        out["margin"] = bo.margin(pp, prm, p0, tr, trials)
    return out


def solve_batch(Ms, N, seeds, eps, noise, p0_spread, prm, zero_cols=None, want_margin=True):
    """one products-oracle solve per problem; Ms: one M for all or one per problem; zero_cols: {problem: column}"""
    seeds = list(seeds)
    Ms = np.broadcast_to(Ms, (len(seeds),))
    res = []
    for b, s in enumerate(seeds):
        pp = HostProductsProblem(int(Ms[b]), N, int(s), eps, noise, p0_spread, (zero_cols or {}).get(b, -1))
        res.append(solve_one(pp, prm, want_margin))
        pp.close()
    return res


@functools.lru_cache(maxsize=None)
def oracle_batch(N, M, seed0, B, setname, over=(), ragged=None, zero=None):
    """the products oracle on problems seed0 .. seed0 + B - 1 (cached: several tests share a batch).  ragged: (Mmin, Mmax)
    in place of M; zero: (chosen problems, column)"""
    eps, noise, spread, _ = SETS[setname]
    Ms = M if ragged is None else ragged_M(B, *ragged)
    zero_cols = None if zero is None else {b: zero[1] for b in zero[0]}
    return solve_batch(Ms, N, range(seed0, seed0 + B), eps, noise, spread, params(setname, **dict(over)), zero_cols)


# ---------------------------------------------------------------- the cases and the margins recorded for them
B, B_SMALL = 257, 65
# (N, M): (B, {set: margin})
PARITY = {
    (3, 12): (B, {"diverse": 2.05e-3, "default": 3.22e-3}),
    (6, 40): (B, {"diverse": 2.71e-4, "default": 1.06e-2}),
    (16, 96): (B, {"diverse": 1.71e-2, "default": 1.39e-2}),
    (7, 37): (B, {"diverse": 6.73e-4, "default": 8.04e-4}),
    (32, 200): (B_SMALL, {"diverse": 3.01e-3, "default": 1.68e-3}),
    # the four size classes, and a triangle loaded in one pass (NP <= 64) or in several
    (1, 1): (B_SMALL, {"diverse": 8.21e-3, "default": 8.67e-2}),
    (1, 5): (B_SMALL, {"diverse": 1.21e-2, "default": 1.70e-2}),
    (2, 9): (B_SMALL, {"diverse": 8.91e-3, "default": 3.04e-2}),
    (8, 32): (B_SMALL, {"diverse": 7.26e-5, "default": 1.09e-2}),
    (9, 55): (B_SMALL, {"diverse": 3.96e-3, "default": 1.40e-2}),
    (16, 50): (B_SMALL, {"diverse": 8.41e-2, "default": 1.55e-2}),
    (17, 40): (B_SMALL, {"diverse": 2.30e-2, "default": 5.96e-3}),
    (24, 73): (B_SMALL, {"diverse": 9.57e-3, "default": 7.50e-3}),
    (25, 81): (B_SMALL, {"diverse": 2.91e-3, "default": 7.31e-5}),
    (31, 47): (B_SMALL, {"diverse": 5.35e-3, "default": 2.76e-2}),
    (32, 70): (B_SMALL, {"diverse": 1.46e-2, "default": 1.30e-2}),
}
# N: ((Mmin, Mmax), {set: margin}), B problems
RAGGED = {
    6: ((9, 40), {"diverse": 2.71e-4, "default": 1.98e-2}),
    16: ((20, 96), {"diverse": 7.96e-3, "default": 7.39e-3}),
    3: ((5, 12), {"diverse": 1.02e-2, "default": 3.22e-3}),
}
HARD_SHAPE, HARD_SEED0, HARD_B, HARD_MARGIN, HARD_REJECTED, HARD_EVALS = (6, 40), 897, 257, 4.51e-4, 3, (4, 8)
# a zero column in problems 3, 17, 30 of 32, "default": (N, M): (column, margin)
ZERO_COLUMN = {(24, 73): (17, 7.83e-3), (32, 70): (31, 1.30e-2)}
ZERO_B, ZERO_CHOSEN = 32, (3, 17, 30)


def recorded(m, want):
    """a margin against the one recorded, to 5 % as tests/test_dense_batch_gpu.py asserts it"""
    return abs(m - want) <= 0.05 * want


def assert_margin(orc, what, want=None):
    m = min(r["margin"] for r in orc)
    print(f"{what}: smallest decision margin of the oracle's solves {m:.3g}")
    assert m > MARGIN_FLOOR, f"{what}: margin {m:.3g}: the seeds no longer keep the decisions off the rounding edges"
    if want is not None:
        assert recorded(m, want), f"{what}: margin {m:.3g}, recorded {want:.3g}: the generator changed"
    return m
