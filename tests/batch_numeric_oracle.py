"""The numeric Jacobians of a batch restated for the tests: the step rule of include/dogleg_numeric_step.h in numpy (every
operation one rounded float64 operation, in the header's order, so the restatement matches bit for bit), what the adapter's two
kernels must produce from given copies, and NumericHostProblem -- DenseProblem of problems.c as a host callback whose J is the
difference quotient of synth_cb_dense's x -- for the CPU oracle.  Test infrastructure."""
import ctypes as C

import numpy as np

from libdogleg_amd.ctypes_defs import CB_DENSE, NUMERIC_FORWARD, NUMERIC_CENTRAL, NUMERIC_DELTA_DEFAULT, dptr
from tests import oracle_api as oa


def deltas(scheme, delta_rel=0.0, delta_abs=0.0):
    """the deltas in force: both <= 0 selects the scheme's default for both"""
    if delta_rel <= 0.0 and delta_abs <= 0.0:
        return NUMERIC_DELTA_DEFAULT[scheme], NUMERIC_DELTA_DEFAULT[scheme]
    return delta_rel, delta_abs


def step(scheme, p, lo, hi, delta_rel, delta_abs):
    """(tp, tm, d) of the step rule, elementwise over arrays (lo / hi: arrays, -inf / +inf without bounds)"""
    p, lo, hi = (np.asarray(a, dtype=np.float64) for a in (p, lo, hi))
    with np.errstate(invalid="ignore", over="ignore"):
        h = np.float64(delta_rel) * np.abs(p) + np.float64(delta_abs)
        up, dn = p + h, p - h
        if scheme == NUMERIC_CENTRAL:
            tp = np.where(up > hi, hi, up)
            tm = np.where(dn < lo, lo, dn)
            return tp, tm, tp - tm
        tp = np.where(up > hi, np.where(dn < lo, lo, dn), up)
        return tp, p.copy(), tp - p


def copies(scheme, p, lo, hi, delta_rel, delta_abs):
    """(p_copies (K, B, N), divisor (B, N)) for p (B, N): copy 0 is p, copy 1 + j has variable j at its plus point, copy
    1 + N + j (central) at its minus point"""
    B, N = p.shape
    lo = np.full_like(p, -np.inf) if lo is None else lo
    hi = np.full_like(p, np.inf) if hi is None else hi
    tp, tm, d = step(scheme, p, lo, hi, delta_rel, delta_abs)
    K = 2 * N + 1 if scheme == NUMERIC_CENTRAL else N + 1
    pc = np.repeat(p[None], K, axis=0)
    for j in range(N):
        pc[1 + j, :, j] = tp[:, j]
        if scheme == NUMERIC_CENTRAL:
            pc[1 + N + j, :, j] = tm[:, j]
    return pc, d


def jacobian(scheme, xc, d):
    """J (B, M, N) from the copies' x (K, B, M) and the divisors (B, N): one subtraction and one IEEE division per entry, exact
    zeros where the divisor is 0"""
    K, B, M = xc.shape
    N = d.shape[1]
    xp = xc[1:1 + N]
    xm = xc[1 + N:1 + 2 * N] if scheme == NUMERIC_CENTRAL else np.repeat(xc[0:1], N, axis=0)
    dd = d.T[:, :, None]                                    # (N, B, 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (xp - xm) / dd
    q = np.where(dd == 0.0, 0.0, q)
    return np.ascontiguousarray(np.transpose(q, (1, 2, 0)))


class NumericHostProblem:
    """DenseProblem(M, N, seed, ...) of problems.c as the oracle's host callback with the NUMERIC Jacobian of the step rule:
    x from synth_cb_dense at p and at the perturbed points, J by jacobian().  lower / upper (N,) or None.  ulp_rng: a numpy
    Generator -- every x the model returns is then moved by -1, 0 or +1 ulp at random, to see what last-bit differences of
    sin between two implementations may change."""

    def __init__(self, M, N, seed, eps, noise, p0_spread, scheme=NUMERIC_CENTRAL, delta_rel=0.0, delta_abs=0.0, lower=None,
                 upper=None, ulp_rng=None):
        self.dp = oa.DenseProblem(M, N, seed=seed, eps=eps, noise=noise, p0_spread=p0_spread)
        self.M, self.N, self.scheme = M, N, scheme
        self.delta_rel, self.delta_abs = deltas(scheme, delta_rel, delta_abs)
        self.lo = np.full(N, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64)
        self.hi = np.full(N, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
        self.ulp_rng = ulp_rng
        self._scratch = np.zeros((M, N))

        def wrapped(p, x, J, cookie):
            xv, Jv = self.eval(np.ctypeslib.as_array(p, shape=(N,)).copy())
            np.ctypeslib.as_array(x, shape=(M,))[:] = xv
            np.ctypeslib.as_array(J, shape=(M, N))[:] = Jv

        self._keep = CB_DENSE(wrapped)
        self.cb, self.cookie = C.cast(self._keep, C.c_void_p), None

    def p0(self):
        return self.dp.p0()

    def values(self, p):
        x = np.zeros(self.M)
        self.dp.lib.synth_cb_dense(dptr(np.ascontiguousarray(p, dtype=np.float64)), dptr(x), dptr(self._scratch), self.dp.h)
        if self.ulp_rng is not None:
            k = self.ulp_rng.integers(-1, 2, size=self.M)
            x = np.where(k > 0, np.nextafter(x, np.inf), np.where(k < 0, np.nextafter(x, -np.inf), x))
        return x

    def eval(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        pc, d = copies(self.scheme, p[None], self.lo[None], self.hi[None], self.delta_rel, self.delta_abs)
        xc = np.stack([self.values(pc[k, 0]) for k in range(pc.shape[0])])[:, None, :]
        return xc[0, 0].copy(), jacobian(self.scheme, xc, d)[0]


def solve_batch(M, N, seeds, eps, noise, p0_spread, prm, want_margin=True, **numeric):
    """batch_oracle.solve_batch on the numeric host problems"""
    from tests import batch_oracle as bo
    res = []
    for s in seeds:
        hp = NumericHostProblem(M, N, int(s), eps, noise, p0_spread, **numeric)
        res.append(bo.solve_one(hp, prm, want_margin))
        hp.dp.close()
    return res


def find_seed0(M, N, B, eps, noise, p0_spread, prm, floor=1e-6, start=1, tries=200000, **numeric):
    """batch_oracle.find_seed0 on the numeric host problems: (seed0, smallest margin of its window)"""
    from tests import batch_oracle as bo
    marg = {}

    def get(s):
        if s not in marg:
            hp = NumericHostProblem(M, N, s, eps, noise, p0_spread, **numeric)
            marg[s] = bo.solve_one(hp, prm)["margin"]
            hp.dp.close()
        return marg[s]

    s0 = start
    while s0 < start + tries:
        bad = next((s for s in range(s0 + B - 1, s0 - 1, -1) if get(s) <= floor), None)
        if bad is None:
            return s0, min(marg[s] for s in range(s0, s0 + B))
        s0 = bad + 1
    raise RuntimeError("no seed0 found")
