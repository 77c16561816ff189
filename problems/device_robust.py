"""Device callbacks for the robust device solve (problems/device_robust.hip) and the host side of the same functions.
OffsetDeviceModel wraps a DeviceTwin: the inner dogleg_callback_device_t, then x += off on the callback's stream;
OffsetHostModel is that function on the host for the NumPy oracle (tests/batch_robust_oracle.py's solve_one): eval(p) returns
(x + off, J) with J dense.  TableDeviceModel is a constant model: it copies a given x and given Jacobian values into the
library's buffers, so that any pattern and any values can be put in front of the prelude.  Inputs for tests/ and tools/ only --
nothing here computes what is checked."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr
from problems import BAProblem, batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_robust.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_device_robust.so")
_lib = None


def build():
    """hipcc build with the flags problems/batch.py gives its libraries"""
    if batch._stale(_LIB, _SRC):
        subprocess.run([batch.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_device_robust.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D = C.c_void_p, C.POINTER(C.c_double)
        L.robust_offsets_create.restype = V
        L.robust_offsets_create.argtypes = [V, V, C.c_int, D]
        L.robust_offsets_free.argtypes = [V]
        L.robust_offsets_free.restype = None
        L.robust_table_create.restype = V
        L.robust_table_create.argtypes = [C.c_int, C.c_longlong, D, D]
        L.robust_table_free.argtypes = [V]
        L.robust_table_free.restype = None
        L.robust_table_ncalls.argtypes = [V]
        L.robust_copy_ms.restype = C.c_double
        L.robust_copy_ms.argtypes = [C.c_longlong, C.c_int]
        _lib = L
    return _lib


class OffsetDeviceModel:
    """twin (a DeviceTwin, which it then owns) with off (M,) added to x: cb / cookie of a dogleg_callback_device_t"""

    def __init__(self, twin, off):
        self.lib, self.twin = lib(), twin
        self.off = np.ascontiguousarray(off, dtype=np.float64)
        self.h = self.lib.robust_offsets_create(twin.cb, twin.cookie, len(self.off), dptr(self.off))
        assert self.h, "offset model creation failed"
        self.cb = C.cast(self.lib.robust_cb_offsets, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def neval(self):
        return self.twin.neval()

    def close(self):
        if self.h:
            self.lib.robust_offsets_free(self.h)
            self.h = None
        self.twin.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OffsetHostModel:
    """prob (a BAProblem or a DenseProblem) with off (M,) added to x: p0(), eval(p) -> (x + off, J dense), N, M"""

    def __init__(self, prob, off=None):
        self.prob, self.N, self.M = prob, prob.N, prob.M
        self.off = np.zeros(self.M) if off is None else np.ascontiguousarray(off, dtype=np.float64)
        assert self.off.shape == (self.M,)
        self.pattern = prob.pattern() if isinstance(prob, BAProblem) else None

    def p0(self):
        return self.prob.p0()

    def eval(self, p):
        x, J = self.prob.eval(p)
        if self.pattern is not None:
            J = dense_of(self.pattern[0], self.pattern[1], J, self.N)
        return x + self.off, J


def dense_of(Jp, Ji, Jx, N):
    """the M x N matrix of the values Jx of Jt on the pattern (Jp, Ji)"""
    M = len(Jp) - 1
    J = np.zeros((M, N))
    J[np.repeat(np.arange(M), np.diff(Jp)), Ji] = Jx
    return J


class TableDeviceModel:
    """the constant model x(p) = x_table, J(p) = J_table (the values of Jt in pattern order, or M x N row-major)"""

    def __init__(self, x_table, J_table):
        self.lib = lib()
        self.x = np.ascontiguousarray(x_table, dtype=np.float64)
        self.J = np.ascontiguousarray(J_table, dtype=np.float64).reshape(-1)
        self.h = self.lib.robust_table_create(len(self.x), self.J.size, dptr(self.x), dptr(self.J))
        assert self.h, "table model creation failed"
        self.cb = C.cast(self.lib.robust_cb_table, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def neval(self):
        return self.lib.robust_table_ncalls(self.h)

    def close(self):
        if self.h:
            self.lib.robust_table_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
