"""The CPU oracle applied to every problem of a batch, one oa.oracle_solve("dense", ...) each, with what a batch result
is compared against (end point, norm2_x, trust region, lambda, iterations, evaluations, status) and the smallest
decision margin of each solve, computed from the oracle's trace alone.  Test infrastructure (tests/test_dense_batch_gpu.py,
tools/batch_bench.py's single-thread baseline)."""
import ctypes as C

import numpy as np

from libdogleg_amd.ctypes_defs import (CB_DENSE, BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS,
                                       dptr)
from tests import oracle_api as oa


class HostProblem:
    """DenseProblem(M, N, seed, ...) of problems.c as the oracle's host callback; zero_col >= 0: the model with
    column zero_col of J exactly zero (a small wrapper round synth_cb_dense: that variable held at p*, its column
    cleared), the host side of problems/device_batch_problems.hip's MODE_ZERO_COLUMN."""

    def __init__(self, M, N, seed, eps, noise, p0_spread, zero_col=-1):
        self.dp = oa.DenseProblem(M, N, seed=seed, eps=eps, noise=noise, p0_spread=p0_spread)
        self.M, self.N, self.zero_col = M, N, zero_col
        if zero_col < 0:
            self.cb, self.cookie, self._keep = self.dp.cb, self.dp.cookie, None
        else:
            pstar = np.zeros(N)
            self.dp.lib.synth_pstar(self.dp.h, dptr(pstar))
            lib, h = self.dp.lib, self.dp.h

            def wrapped(p, x, J, cookie):
                q = np.ctypeslib.as_array(p, shape=(N,)).copy()
                q[zero_col] = pstar[zero_col]
                lib.synth_cb_dense(dptr(q), x, J, h)
                np.ctypeslib.as_array(J, shape=(M, N))[:, zero_col] = 0.0

            self._keep = CB_DENSE(wrapped)
            self.cb, self.cookie = C.cast(self._keep, C.c_void_p), None

    def p0(self):
        return self.dp.p0()

    def eval(self, p):
        x, J = self.dp.eval(p) if self.zero_col < 0 else (np.zeros(self.M), np.zeros((self.M, self.N)))
        if self.zero_col >= 0:
            self._keep(dptr(np.ascontiguousarray(p, dtype=np.float64)), dptr(x), dptr(J), None)
        return x, J


def solve_one(hp, prm, want_margin=True):
    """the oracle on one problem: dict(p, norm2_x, trustregion, lambda_, iterations, evaluations, status, margin,
    step_types, rejected)"""
    p0 = hp.p0()
    r, p, tr = oa.oracle_solve("dense", p0, hp.N, hp.M, 0, hp.cb, hp.cookie, prm, capacity=1024)
    trials = tr.trials()
    assert tr.c.ntrials <= tr.capacity
    iters = sum(1 for t in trials if t["accepted"] == 1)
    x, J = hp.eval(p)
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
        out["margin"] = margin(hp, prm, p0, tr, trials)
    return out


def margin(hp, prm, p0, tr, trials):
    """the smallest decision margin of a solve, from the oracle's trace: the relative gap of norm2_cauchy (and of
    norm2_gn where the Gauss-Newton step was formed) to trustregion^2, |rho - t| for t in {0, the decrease threshold,
    the increase threshold} less the rounding error of rho itself, and the relative gaps of max|step| to update_threshold, of |Jt x|_inf to Jt_x_threshold
    (start point and every accepted point) and of the trust region to trustregion_threshold after a rejection"""
    def rel(a, b):
        return abs(a - b) / abs(b) if b != 0 else abs(a)

    def gmax(p):
        x, J = hp.eval(p)
        return float(np.max(np.abs(J.T @ x)))

    m = [rel(gmax(p0), prm.Jt_x_threshold)]
    for i, t in enumerate(trials):
        tr2 = t["trustregion_before"] ** 2
        m.append(rel(t["norm2_cauchy"], tr2))
        if t["step_type"] != 0:
            m.append(rel(t["norm2_gn"], tr2))
        m.append(rel(float(np.max(np.abs(tr.step[i]))), prm.update_threshold))
        if t["accepted"] in (0, 1):
            # rho = (norm2x_before - norm2x_after) / expected: each norm2 is a sum of M squares with a relative rounding
            # error of at most M eps, whatever the order of summation, so two correct implementations may differ in rho by
            # rho_err; that much of the gap does not count
            rho_err = 2.0 * hp.M * np.finfo(float).eps * t["norm2x_before"] / abs(t["expected_improvement"])
            m += [abs(t["rho"] - th) - rho_err
                  for th in (0.0, prm.trustregion_decrease_threshold, prm.trustregion_increase_threshold)]
        if t["accepted"] == 1:
            m.append(rel(gmax(tr.p_trial[i]), prm.Jt_x_threshold))
        if t["accepted"] == 0:
            m.append(rel(t["trustregion_after"], prm.trustregion_threshold))
    return min(m)


def solve_batch(M, N, seeds, eps, noise, p0_spread, prm, zero_cols=None, want_margin=True):
    """one oracle solve per problem of a batch; zero_cols: {problem: column} (MODE_ZERO_COLUMN)"""
    res = []
    for b, s in enumerate(seeds):
        hp = HostProblem(M, N, int(s), eps, noise, p0_spread, (zero_cols or {}).get(b, -1))
        res.append(solve_one(hp, prm, want_margin))
        hp.dp.close()
    return res


def find_seed0(M, N, B, eps, noise, p0_spread, prm, floor=1e-6, start=1, tries=200000):
    """the first seed0 >= start for which the problems seed0 .. seed0 + B - 1 all have a margin above `floor`: the margins of
    single seeds are computed once, the window slides over them.  (seed0, smallest margin of the window)"""
    marg = {}

    def get(s):
        if s not in marg:
            hp = HostProblem(M, N, s, eps, noise, p0_spread)
            marg[s] = solve_one(hp, prm)["margin"]
            hp.dp.close()
        return marg[s]

    s0 = start
    while s0 < start + tries:
        bad = next((s for s in range(s0 + B - 1, s0 - 1, -1) if get(s) <= floor), None)
        if bad is None:
            return s0, min(marg[s] for s in range(s0, s0 + B))
        s0 = bad + 1
    raise RuntimeError("no seed0 found")
