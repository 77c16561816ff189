"""A RAGGED batch of LINEAR least-squares problems in the products form (problems/device_batch_linear_products.hip) behind
ctypes: problem b is x = A[b] p - y[b] with A[b] of its own number of rows M[b], and the callback hands back norm2(x), Jt x and
JtJ.  LinearProductsBatch is the dogleg_callback_device_batch_products_t with the layout switch of problems/batch.py's
DeviceProductsBatch and the counters of problems/batch_linear.py's LinearDeviceBatch, whose LinearHostProblem,
from_normal_equations and exact_bounded_solution serve here unchanged.  Inputs for tests/ and tools/ only -- nothing of the
library computes anything in here."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr
from problems import batch
from problems.batch import LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER            # noqa: F401
from problems.batch_linear import LinearHostProblem, exact_bounded_solution, from_normal_equations   # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_batch_linear_products.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_batch_linear_products.so")
_lib = None


def build():
    """hipcc build with the flags problems/batch.py gives its libraries"""
    if batch._stale(_LIB, _SRC):
        subprocess.run([batch.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_batch_linear_products.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D = C.c_void_p, C.POINTER(C.c_double)
        L.synth_linp_create.restype = V
        L.synth_linp_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_longlong), D, D]
        L.synth_linp_free.argtypes = [V]
        L.synth_linp_free.restype = None
        L.synth_linp_set_layout.argtypes = [V, C.c_int]
        L.synth_linp_ncalls.argtypes = [V]
        L.synth_linp_nevals.argtypes = [V]
        L.synth_linp_nevals.restype = C.c_longlong
        L.synth_linp_reset_counters.argtypes = [V]
        L.synth_linp_reset_counters.restype = None
        L.synth_linp_first_p.argtypes = [V, D]
        _lib = L
    return _lib


def random_ragged(N, B, seed, Mmin=None, Mmax=None):
    """(A, y, p0 (B, N), lo (B, N), hi (B, N)) of B random problems: A[b] of M[b] in Mmin .. Mmax (N + 1 .. N + 9 unless given)
    rows of unit normals (full column rank), a box around 0 that cuts the unbounded optimum off in some variables, one side
    open here and there, the start point anywhere (also outside)"""
    rng = np.random.default_rng([seed, N, B])
    Mmin, Mmax = (N + 1 if Mmin is None else Mmin), (N + 9 if Mmax is None else Mmax)
    M = rng.integers(Mmin, Mmax + 1, B)
    A = [rng.standard_normal((m, N)) for m in M]
    y = [rng.standard_normal(m) * 2.0 for m in M]
    lo, hi = -rng.random((B, N)), rng.random((B, N))
    lo[rng.random((B, N)) < 0.25] = -np.inf
    hi[rng.random((B, N)) < 0.25] = np.inf
    return A, y, rng.standard_normal((B, N)) * 1.5, lo, hi


class LinearProductsBatch:
    """B linear problems of N variables on the GPU: A a list of B arrays (M[b], N), y a list of B arrays (M[b],), start points
    p0 (B, N)"""

    def __init__(self, A, y, p0, layout=LAYOUT_PACKED_UPPER):
        self.lib = lib()
        self.A = [np.ascontiguousarray(a, dtype=np.float64) for a in A]
        self.y = [np.ascontiguousarray(v, dtype=np.float64) for v in y]
        self.B, self.N = len(self.A), self.A[0].shape[1]
        self.M = np.array([a.shape[0] for a in self.A], dtype=np.int64)
        assert all(a.shape == (m, self.N) and v.shape == (m,) for a, v, m in zip(self.A, self.y, self.M))
        self._p0 = np.array(p0, dtype=np.float64).reshape(self.B, self.N)
        self.off = np.concatenate(([0], np.cumsum(self.M))).astype(np.int64)
        rows, ys = np.ascontiguousarray(np.concatenate(self.A, axis=0)), np.ascontiguousarray(np.concatenate(self.y))
        self.h = self.lib.synth_linp_create(self.B, self.N, self.off.ctypes.data_as(C.POINTER(C.c_longlong)), dptr(rows), dptr(ys))
        assert self.h, "device batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch_linear_products, C.c_void_p)
        self.cookie = C.c_void_p(self.h)
        self.set_layout(layout)

    def p0(self):
        return self._p0.copy()

    def host(self, b):
        return LinearHostProblem(self.A[b], self.y[b], self._p0[b])

    def set_layout(self, layout):
        """LAYOUT_PACKED_UPPER (the library: JtJ_packed and JtJ_upper), LAYOUT_UNPACKED or LAYOUT_UNPACKED_NAN_LOWER (neither)"""
        assert self.lib.synth_linp_set_layout(self.h, layout) == 0
        self.layout = layout

    def set_params(self, prm):
        """prm with the JtJ_packed / JtJ_upper bits of this batch's layout"""
        prm.JtJ_packed = prm.JtJ_upper = self.layout == LAYOUT_PACKED_UPPER
        return prm

    def ncalls(self):
        """invocations of the batch callback"""
        return self.lib.synth_linp_ncalls(self.h)

    def nevals(self):
        """problem evaluations done (live problems over all invocations)"""
        return self.lib.synth_linp_nevals(self.h)

    def reset_counters(self):
        self.lib.synth_linp_reset_counters(self.h)

    def first_p(self):
        """p_dev (B, N) as the first invocation since reset_counters() got it"""
        out = np.zeros((self.B, self.N))
        assert self.lib.synth_linp_first_p(self.h, dptr(out)) == 0
        return out

    def close(self):
        if self.h:
            self.lib.synth_linp_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
