"""A batch of LINEAR least-squares problems with a prescribed Jacobian (problems/device_batch_linear.hip) behind ctypes:
problem b is x = A[b] p - y[b], J = A[b].  LinearDeviceBatch is the dogleg_callback_device_batch_t with the interface and the
counters of problems/batch.py's DeviceBatch; LinearHostProblem is the same function on the host for the NumPy oracles (.N, .M,
.p0(), .eval(p)).  Since JtJ and Jt x are what the caller chose, a test can place a problem exactly on a branch of the solver's
loop.  exact_bounded_solution is the textbook answer of such a problem under box bounds, by enumeration.  Inputs for tests/
and tools/ only -- nothing of the library computes anything in here."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr
from problems import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_batch_linear.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_batch_linear.so")
_lib = None


def build():
    """hipcc build with the flags problems/batch.py gives its libraries"""
    if batch._stale(_LIB, _SRC):
        subprocess.run([batch.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_batch_linear.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D = C.c_void_p, C.POINTER(C.c_double)
        L.synth_lin_create.restype = V
        L.synth_lin_create.argtypes = [C.c_int, C.c_int, C.c_int, D, D]
        L.synth_lin_free.argtypes = [V]
        L.synth_lin_free.restype = None
        L.synth_lin_ncalls.argtypes = [V]
        L.synth_lin_nevals.argtypes = [V]
        L.synth_lin_nevals.restype = C.c_longlong
        L.synth_lin_reset_counters.argtypes = [V]
        L.synth_lin_reset_counters.restype = None
        L.synth_lin_first_p.argtypes = [V, D]
        _lib = L
    return _lib


class LinearHostProblem:
    """x = A p - y, J = A for A (M, N), y (M,), started at p0 (N,)"""

    def __init__(self, A, y, p0):
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.M, self.N = self.A.shape
        self._p0 = np.array(p0, dtype=np.float64).reshape(self.N)
        assert self.y.shape == (self.M,)

    def p0(self):
        return self._p0.copy()

    def eval(self, p):
        return self.A @ np.asarray(p, dtype=np.float64) - self.y, self.A.copy()

    def close(self):
        pass


class LinearDeviceBatch:
    """B linear problems of one shape on the GPU: A (B, M, N), y (B, M), start points p0 (B, N)"""

    def __init__(self, A, y, p0):
        self.lib = lib()
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.B, self.M, self.N = self.A.shape
        self._p0 = np.array(p0, dtype=np.float64).reshape(self.B, self.N)
        assert self.y.shape == (self.B, self.M)
        self.h = self.lib.synth_lin_create(self.B, self.M, self.N, dptr(self.A), dptr(self.y))
        assert self.h, "device batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch_linear, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def p0(self):
        return self._p0.copy()

    def host(self, b):
        return LinearHostProblem(self.A[b], self.y[b], self._p0[b])

    def ncalls(self):
        """invocations of the batch callback"""
        return self.lib.synth_lin_ncalls(self.h)

    def nevals(self):
        """problem evaluations done (live problems over all invocations)"""
        return self.lib.synth_lin_nevals(self.h)

    def reset_counters(self):
        self.lib.synth_lin_reset_counters(self.h)

    def first_p(self):
        """p_dev (B, N) as the first invocation since reset_counters() got it"""
        out = np.zeros((self.B, self.N))
        assert self.lib.synth_lin_first_p(self.h, dptr(out)) == 0
        return out

    def close(self):
        if self.h:
            self.lib.synth_lin_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def from_normal_equations(H, g0):
    """(A, y) with A' A = H (its upper Cholesky factor) and A' (A 0 - y) = g0: the problem whose JtJ is H and whose Jt x at
    p = 0 is g0"""
    A = np.linalg.cholesky(np.asarray(H, dtype=np.float64)).T
    return A, -np.linalg.solve(A.T, np.asarray(g0, dtype=np.float64))


def exact_bounded_solution(A, y, lo, hi):
    """argmin |A p - y|^2 over lo <= p <= hi by enumeration: every variable free, at lower or at upper (3^N active sets), the
    free ones solved for; of the KKT points (feasible, multipliers of the right sign) the one of smallest cost.  A of full
    column rank."""
    A, y = np.asarray(A, dtype=np.float64), np.asarray(y, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    N = A.shape[1]
    best, best_cost = None, np.inf
    for code in itertools.product((0, 1, 2), repeat=N):
        code = np.array(code)
        if np.any(~np.isfinite(lo[code == 1])) or np.any(~np.isfinite(hi[code == 2])):
            continue
        p = np.where(code == 1, lo, np.where(code == 2, hi, 0.0))
        free = code == 0
        if free.any():
            p[free] = np.linalg.lstsq(A[:, free], y - A[:, ~free] @ p[~free], rcond=None)[0]
        scale = 1e-12 * (1.0 + np.abs(p))
        if np.any(p < lo - scale) or np.any(p > hi + scale):
            continue
        g = A.T @ (A @ p - y)
        tol = 1e-9 * (1.0 + np.abs(g).max())
        if np.any(g[code == 1] < -tol) or np.any(g[code == 2] > tol):
            continue
        cost = float(np.sum((A @ p - y) ** 2))
        if cost < best_cost:
            best, best_cost = p, cost
    assert best is not None
    return best
