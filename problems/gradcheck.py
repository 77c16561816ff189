"""The models for the tests of the Jacobian check on the GPU (problems/device_gradcheck_problems.hip) behind ctypes: a
sparse problem on a caller-supplied pattern and a batch of dense ones, both with the caller's coefficients and with
switches that inject one known fault.  Inputs for tests/ and tools/ only -- nothing here computes what is checked."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr, iptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_gradcheck_problems.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_gradcheck.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
_lib = None


def build():
    """hipcc build with the flags problems/batch.py uses (no contraction: the operation order written in the source)"""
    if not os.path.exists(_LIB) or os.path.getmtime(_SRC) > os.path.getmtime(_LIB):
        subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_gradcheck.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D, I = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.gcp_sparse_create.restype = V
        L.gcp_sparse_create.argtypes = [C.c_int, C.c_int, C.c_int, I, I, D, D, C.c_double]
        L.gcp_sparse_free.argtypes = [V]
        L.gcp_sparse_free.restype = None
        L.gcp_sparse_set_faults.argtypes = [V, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int]
        L.gcp_sparse_ncalls.argtypes = [V]
        L.gcp_sparse_reset.argtypes = [V]
        L.gcp_sparse_reset.restype = None
        L.gcp_batch_create.restype = V
        L.gcp_batch_create.argtypes = [C.c_int, C.c_int, C.c_int, D, D, C.c_double]
        L.gcp_batch_free.argtypes = [V]
        L.gcp_batch_free.restype = None
        L.gcp_batch_set_fault.argtypes = [V, C.c_int, C.c_int, C.c_int, C.c_double]
        L.gcp_batch_ncalls.argtypes = [V]
        L.gcp_batch_notlive.argtypes = [V]
        L.gcp_batch_notlive.restype = C.c_longlong
        _lib = L
    return _lib


class SparseModel:
    """x_r = u_r + eps sin(u_r), u_r = sum_t a_t (p[i_t] - p*[i_t]) on the pattern (Jp, Ji) of Jt; J_t = a_t (1 + eps cos u_r).
    A dense problem is the same with every variable in every row (the values of Jt are then J, row-major)."""

    def __init__(self, N, M, Jp, Ji, a, pstar, eps):
        self.lib = lib()
        self.N, self.M = N, M
        self.Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        self.Ji = np.ascontiguousarray(Ji, dtype=np.int32)
        self.nnz = len(self.Ji)
        a = np.ascontiguousarray(a, dtype=np.float64)
        pstar = np.ascontiguousarray(pstar, dtype=np.float64)
        assert self.Jp.shape == (M + 1,) and a.shape == (self.nnz,) and pstar.shape == (N,)
        self.h = self.lib.gcp_sparse_create(N, M, self.nnz, iptr(self.Jp), iptr(self.Ji), dptr(a), dptr(pstar), eps)
        assert self.h, "device problem creation failed"
        self.cb = C.cast(self.lib.gcp_cb_sparse, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def set_faults(self, t_bad=-1, factor=1.0, r_extra=-1, w=0, c=0.0, r_nan=-1):
        """(a) J of entry t_bad times factor; (b) x[r_extra] += c (p[w] - p*[w]); (c) x[r_nan] = NaN; negative: off"""
        assert self.lib.gcp_sparse_set_faults(self.h, t_bad, factor, r_extra, w, c, r_nan) == 0

    def ncalls(self):
        return self.lib.gcp_sparse_ncalls(self.h)

    def reset(self):
        self.lib.gcp_sparse_reset(self.h)

    def close(self):
        if self.h:
            self.lib.gcp_sparse_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchModel:
    """B dense problems: x[b][r] = u + eps sin(u), u = sum_j c[b][r][j] (p[b][j] - p*[b][j]); J[b][r][j] = c (1 + eps cos u)"""

    def __init__(self, coef, pstar, eps):
        self.lib = lib()
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        pstar = np.ascontiguousarray(pstar, dtype=np.float64)
        self.B, self.M, self.N = coef.shape
        assert pstar.shape == (self.B, self.N)
        self.h = self.lib.gcp_batch_create(self.B, self.M, self.N, dptr(coef), dptr(pstar), eps)
        assert self.h, "device batch creation failed"
        self.cb = C.cast(self.lib.gcp_cb_batch, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def set_fault(self, b=-1, r=0, v=0, factor=1.0):
        """J[b][r][v] times factor; b < 0: off"""
        assert self.lib.gcp_batch_set_fault(self.h, b, r, v, factor) == 0

    def ncalls(self):
        return self.lib.gcp_batch_ncalls(self.h)

    def notlive(self):
        """live bytes that were not 1, over all invocations"""
        return self.lib.gcp_batch_notlive(self.h)

    def close(self):
        if self.h:
            self.lib.gcp_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
