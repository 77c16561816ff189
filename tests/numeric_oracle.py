"""The numeric Jacobians of a single problem (dogleg_amd_numeric_*) restated for the tests: what the adapter's kernels must
produce -- the coloured copies of p and the divisors, and the values of Jt in pattern order from the copies' x -- in numpy, every
operation one rounded float64 operation (the step rule is tests/batch_numeric_oracle.step, bit for bit the header's), and
NumericSparseHostProblem, the model of tests/jacobian_patterns.model as a host callback for the CPU oracle whose J is that
restatement's.  Nothing here calls the library.  Test infrastructure."""
import ctypes as C

import numpy as np

from libdogleg_amd.ctypes_defs import CB_SPARSE, NUMERIC_CENTRAL
from tests import batch_numeric_oracle as bn
from tests import jacobian_patterns as jp


def long_row_pattern(N=120, M=40, R=100, long_row=7, seed=23):
    """1 to 4 entries a row but row `long_row`, which holds R of the N variables: at least R colours.  (Jp, Ji) of Jt"""
    rng = np.random.default_rng(seed)
    Jp, Ji = [0], []
    for r in range(M):
        k = R if r == long_row else int(rng.integers(1, 5))
        Ji.extend(sorted(rng.choice(N, size=k, replace=False).tolist()))
        Jp.append(len(Ji))
    return np.array(Jp, dtype=np.int32), np.array(Ji, dtype=np.int32)


def resized(Jp, Ji, M, seed=31, N=None):
    """the pattern truncated to its first M rows, or extended to M rows with rows of 1 to 5 of the N variables"""
    M0 = len(Jp) - 1
    if M <= M0:
        return Jp[:M + 1].copy(), Ji[:Jp[M]].copy()
    rng = np.random.default_rng(seed)
    N = int(Ji.max()) + 1 if N is None else N
    Jp2, Ji2 = list(Jp), list(Ji)
    for _ in range(M - M0):
        Ji2.extend(sorted(rng.choice(N, size=int(rng.integers(1, 6)), replace=False).tolist()))
        Jp2.append(len(Ji2))
    return np.array(Jp2, dtype=np.int32), np.array(Ji2, dtype=np.int32)


def coefficients(N, nnz, seed, spread=0.5):
    """(a (nnz,) with |a| in [0.1, 1] and either sign, p* (N,), p0 = p* + spread U(-1, 1))"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.1, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)
    pstar = rng.uniform(-1.0, 1.0, N)
    return a, pstar, pstar + spread * rng.uniform(-1.0, 1.0, N)


def n_copies(scheme, ncolours):
    return 2 * ncolours + 1 if scheme == NUMERIC_CENTRAL else ncolours + 1


def device_bytes(scheme, N, M, nnz, ncolours):
    """what dogleg_amd_numeric_plan reports: K (N + M) + N doubles and, for a sparse problem, N + M + 1 + 2 nnz ints"""
    K = n_copies(scheme, ncolours)
    return 8.0 * (K * (N + M) + N) + (4.0 * (N + M + 1 + 2 * nnz) if nnz > 0 else 0.0)


def copies_coloured(scheme, p, lo, hi, delta_rel, delta_abs, colour, ncolours):
    """(p_copies (K, N), divisor (N,)) for p (N,): copy 0 is p, copy 1 + c has every variable of colour c at its plus point, copy
    1 + C + c (central) at its minus point.  lo / hi: (N,) or None"""
    N = len(p)
    lo = np.full(N, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(N, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    tp, tm, d = bn.step(scheme, p, lo, hi, delta_rel, delta_abs)
    K = n_copies(scheme, ncolours)
    pc = np.repeat(np.asarray(p, dtype=np.float64)[None], K, axis=0)
    j = np.arange(N)
    pc[1 + colour, j] = tp
    if scheme == NUMERIC_CENTRAL:
        pc[1 + ncolours + colour, j] = tm
    return pc, d


def jacobian_coloured(scheme, xc, d, Jp, Ji, colour, ncolours):
    """the values of Jt (nnz,) in pattern order from the copies' x (K, M) and the divisors (N,): for entry t in row r with
    variable v of colour c one subtraction and one IEEE division, (x[1 + c][r] - xm[r]) / d[v] with xm copy 1 + C + c (central)
    or copy 0 (forward); exact zeros where the divisor is 0"""
    M = len(Jp) - 1
    row = np.repeat(np.arange(M), np.diff(Jp))
    c = colour[Ji]
    xp = xc[1 + c, row]
    xm = xc[1 + ncolours + c, row] if scheme == NUMERIC_CENTRAL else xc[0, row]
    dd = d[Ji]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (xp - xm) / dd
    return np.where(dd == 0.0, 0.0, q)


def jacobian_dense(scheme, xc, d):
    """J (M, N) of a dense problem: every variable its own colour"""
    N = len(d)
    M = xc.shape[1]
    Jp, Ji = jp.full_pattern(M, N)
    return jacobian_coloured(scheme, xc, d, Jp, Ji, np.arange(N), N).reshape(M, N)


def numeric_jacobian(values, scheme, p, lo, hi, delta_rel, delta_abs, Jp, Ji, colour, ncolours):
    """(x, values of Jt) of the model `values(p) -> x` by the restatement"""
    pc, d = copies_coloured(scheme, p, lo, hi, delta_rel, delta_abs, colour, ncolours)
    xc = np.stack([values(pc[k]) for k in range(pc.shape[0])])
    return xc[0].copy(), jacobian_coloured(scheme, xc, d, Jp, Ji, colour, ncolours)


class NumericSparseHostProblem:
    """x_r = u_r + eps sin(u_r), u_r = sum_t a_t (p[i_t] - p*[i_t]) (jacobian_patterns.model) as the oracle's sparse host
    callback with the NUMERIC Jacobian of the restatement on the first-fit colouring.  ulp_rng: a numpy Generator -- every x the
    model returns is then moved by -1, 0 or +1 ulp at random, to see what last-bit differences of sin between two
    implementations may change."""

    def __init__(self, N, M, Jp, Ji, a, pstar, eps, scheme=NUMERIC_CENTRAL, delta_rel=0.0, delta_abs=0.0, lower=None, upper=None,
                 ulp_rng=None):
        self.N, self.M = N, M
        self.Jp, self.Ji = np.ascontiguousarray(Jp, dtype=np.int32), np.ascontiguousarray(Ji, dtype=np.int32)
        self.nnz = len(self.Ji)
        self.a, self.pstar, self.eps = np.asarray(a, dtype=np.float64), np.asarray(pstar, dtype=np.float64), eps
        self.scheme = scheme
        self.delta_rel, self.delta_abs = bn.deltas(scheme, delta_rel, delta_abs)
        self.lo, self.hi = lower, upper
        self.ulp_rng = ulp_rng
        self.colour = jp.first_fit(N, M, self.Jp, self.Ji)
        self.ncolours = int(self.colour.max()) + 1
        self.nevals = 0

        def wrapped(p, x, Jt, cookie):
            xv, Jv = self.eval(np.ctypeslib.as_array(p, shape=(N,)).copy())
            np.ctypeslib.as_array(x, shape=(M,))[:] = xv
            S = Jt.contents
            np.ctypeslib.as_array(C.cast(S.p, C.POINTER(C.c_int)), shape=(M + 1,))[:] = self.Jp
            np.ctypeslib.as_array(C.cast(S.i, C.POINTER(C.c_int)), shape=(self.nnz,))[:] = self.Ji
            np.ctypeslib.as_array(C.cast(S.x, C.POINTER(C.c_double)), shape=(self.nnz,))[:] = Jv

        self._keep = CB_SPARSE(wrapped)
        self.cb, self.cookie = C.cast(self._keep, C.c_void_p), None

    def values(self, p):
        x = jp.model(self.Jp, self.Ji, self.a, self.pstar, self.eps, p)[0]
        if self.ulp_rng is not None:
            k = self.ulp_rng.integers(-1, 2, size=self.M)
            x = np.where(k > 0, np.nextafter(x, np.inf), np.where(k < 0, np.nextafter(x, -np.inf), x))
        return x

    def eval(self, p):
        self.nevals += 1
        return numeric_jacobian(self.values, self.scheme, np.ascontiguousarray(p, dtype=np.float64), self.lo, self.hi,
                                self.delta_rel, self.delta_abs, self.Jp, self.Ji, self.colour, self.ncolours)
