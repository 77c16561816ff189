"""The sparse model of problems/gradcheck.py as a VALUES-ONLY model on the GPU (problems/device_values.hip, a library of its
own) behind ctypes: ValuesModel is evaluated by a dogleg_callback_device_values_t, NaiveNumeric is the naive reference of the
numeric Jacobian over it, a dogleg_callback_device_t: two launches per copy, one thread per entry of Jt.  Inputs for tests/ and
tools/ only -- nothing here computes what is checked."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr, iptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_values.hip")
_HDR = os.path.join(ROOT, "include", "dogleg_numeric_step.h")
_LIB = os.path.join(ROOT, "problems", "libproblems_values.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
_lib = None


def build():
    """hipcc build with the flags of problems/gradcheck.py (no contraction: the operation order written in the source)"""
    stale = not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in (_SRC, _HDR))
    if stale:
        subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_values.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D, I = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
        L.dv_create.restype = V
        L.dv_create.argtypes = [C.c_int, C.c_int, C.c_int, I, I, D, D, C.c_double]
        L.dv_free.argtypes = [V]
        L.dv_free.restype = None
        L.dv_set_box.argtypes = [V, D, D, C.c_int]
        L.dv_set_faults.argtypes = [V, C.c_int, C.c_int, C.c_double, C.c_int]
        for f in ("dv_ncalls", "dv_ncopies", "dv_noutside"):
            getattr(L, f).argtypes = [V]
            getattr(L, f).restype = C.c_longlong
        L.dv_reset.argtypes = [V]
        L.dv_reset.restype = None
        L.dv_naive_create.restype = V
        L.dv_naive_create.argtypes = [V, I, C.c_int, C.c_int, C.c_double, C.c_double, D, D]
        L.dv_naive_free.argtypes = [V]
        L.dv_naive_free.restype = None
        _lib = L
    return _lib


class ValuesModel:
    """x_r = u_r + eps sin(u_r), u_r = sum_t a_t (p[i_t] - p*[i_t]) on the pattern (Jp, Ji) of Jt, values only.  A dense
    problem is the same with every variable in every row (jacobian_patterns.full_pattern)."""

    def __init__(self, N, M, Jp, Ji, a, pstar, eps):
        self.lib = lib()
        self.N, self.M, self.eps = N, M, eps
        self.Jp = np.ascontiguousarray(Jp, dtype=np.int32)
        self.Ji = np.ascontiguousarray(Ji, dtype=np.int32)
        self.nnz = len(self.Ji)
        self.a = np.ascontiguousarray(a, dtype=np.float64)
        self.pstar = np.ascontiguousarray(pstar, dtype=np.float64)
        assert self.Jp.shape == (M + 1,) and self.a.shape == (self.nnz,) and self.pstar.shape == (N,)
        self.h = self.lib.dv_create(N, M, self.nnz, iptr(self.Jp), iptr(self.Ji), dptr(self.a), dptr(self.pstar), eps)
        assert self.h, "device problem creation failed"
        self.cb = C.cast(self.lib.dv_cb_values, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def set_box(self, lower=None, upper=None):
        """every row of a copy with a variable outside [lower, upper] is NaN; None: off"""
        if lower is None:
            assert self.lib.dv_set_box(self.h, None, None, 0) == 0
            return
        lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (lower, upper))
        assert lo.shape == hi.shape == (self.N,)
        assert self.lib.dv_set_box(self.h, dptr(lo), dptr(hi), 1) == 0

    def set_faults(self, r_extra=-1, w=0, c=0.0, r_nan=-1):
        """x[r_extra] += c (p[w] - p*[w]), w not declared in that row; x[r_nan] = NaN; negative: off"""
        assert self.lib.dv_set_faults(self.h, r_extra, w, c, r_nan) == 0

    def ncalls(self):
        """launches of the values kernel (the adapter: one an invocation; the naive reference: one a copy)"""
        return self.lib.dv_ncalls(self.h)

    def ncopies(self):
        """points evaluated"""
        return self.lib.dv_ncopies(self.h)

    def noutside(self):
        """points evaluated with a variable outside the box of set_box (each of them came back all NaN)"""
        return self.lib.dv_noutside(self.h)

    def reset(self):
        self.lib.dv_reset(self.h)

    def close(self):
        if self.h:
            self.lib.dv_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NaiveNumeric:
    """the naive numeric Jacobian over a ValuesModel as a dogleg_callback_device_t (cb, cookie), with the caller's colouring
    (colour[N] in 0 .. C - 1; a dense problem: arange(N)).  The deltas are used as they are: pass the defaults yourself."""

    def __init__(self, model, colour, scheme, delta_rel, delta_abs, lower=None, upper=None):
        self.model = model
        colour = np.ascontiguousarray(colour, dtype=np.int32)
        assert colour.shape == (model.N,)
        self.C = int(colour.max()) + 1
        lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64)
        hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64)
        self.h = model.lib.dv_naive_create(model.h, iptr(colour), self.C, scheme, delta_rel, delta_abs,
                                           None if lo is None else dptr(lo), None if hi is None else dptr(hi))
        assert self.h, "naive reference creation failed"
        self.cb = C.cast(model.lib.dv_cb_naive, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def close(self):
        if self.h:
            self.model.lib.dv_naive_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
