"""The dense synthetic problems of problems/batch.py as a VALUES-ONLY model on the GPU (problems/device_batch_values.hip, a
library of its own) behind ctypes: problem b of a DeviceValuesBatch is DenseProblem(M, N, seed = seeds[b], eps, noise,
p0_spread) of problems.c, evaluated by a dogleg_callback_device_batch_values_t.  NaiveNumeric is the naive reference of the
numeric Jacobian over such a batch, a dogleg_callback_device_batch_t: one launch of the values kernel per copy, one thread per
entry of J.  Inputs for tests/ and tools/ only."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_batch_values.hip")
_HDR = os.path.join(ROOT, "include", "dogleg_numeric_step.h")
_LIB = os.path.join(ROOT, "problems", "libproblems_batch_values.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
_lib = None

MODE_MODEL, MODE_NAN, MODE_ZERO_COLUMN, MODE_BOX_NAN = 0, 1, 2, 3


def _stale(lib, *srcs):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.exists(s) and os.path.getmtime(s) > t for s in srcs)


def build():
    """hipcc build with the flags of problems/batch.py"""
    if _stale(_LIB, _SRC, _HDR):
        subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_batch_values.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D = C.c_void_p, C.POINTER(C.c_double)
        L.synth_vbatch_create.restype = V
        L.synth_vbatch_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_double, C.c_double, C.c_double]
        L.synth_vbatch_free.argtypes = [V]
        L.synth_vbatch_free.restype = None
        for f in ("synth_vbatch_p0", "synth_vbatch_pstar"):
            getattr(L, f).argtypes = [V, D]
            getattr(L, f).restype = None
        L.synth_vbatch_set_mode.argtypes = [V, C.c_char_p, C.c_int]
        L.synth_vbatch_set_box.argtypes = [V, D, D]
        L.synth_vbatch_ncalls.argtypes = [V]
        L.synth_vbatch_ncopies.argtypes = [V]
        L.synth_vbatch_ncopies.restype = C.c_longlong
        L.synth_vbatch_nevals.argtypes = [V]
        L.synth_vbatch_nevals.restype = C.c_longlong
        L.synth_vbatch_reset_counters.argtypes = [V]
        L.synth_vbatch_reset_counters.restype = None
        L.synth_vnaive_create.restype = V
        L.synth_vnaive_create.argtypes = [V, C.c_int, C.c_double, C.c_double, D, D]
        L.synth_vnaive_free.argtypes = [V]
        L.synth_vnaive_free.restype = None
        L.synth_copy_create.restype = V
        L.synth_copy_create.argtypes = [C.c_size_t]
        L.synth_copy_free.argtypes = [V]
        L.synth_copy_free.restype = None
        L.synth_copy_run.restype = C.c_double
        L.synth_copy_run.argtypes = [V]
        _lib = L
    return _lib


class DeviceValuesBatch:
    """B dense problems of one shape on the GPU, values only.  seeds: one per problem (int seed0: seed0 + b)."""

    def __init__(self, B, M, N, seeds=1, eps=0.3, noise=0.01, p0_spread=0.5):
        self.lib = lib()
        self.B, self.M, self.N = B, M, N
        self.eps, self.noise, self.p0_spread = eps, noise, p0_spread
        self.seeds = (np.arange(B, dtype=np.uint64) + np.uint64(seeds)) if np.isscalar(seeds) \
            else np.ascontiguousarray(seeds, dtype=np.uint64)
        assert self.seeds.shape == (B,)
        self.h = self.lib.synth_vbatch_create(B, M, N, self.seeds.ctypes.data_as(C.POINTER(C.c_uint64)), eps, noise, p0_spread)
        assert self.h, "device batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch_values, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def p0(self):
        a = np.zeros((self.B, self.N))
        self.lib.synth_vbatch_p0(self.h, dptr(a))
        return a

    def pstar(self):
        a = np.zeros((self.B, self.N))
        self.lib.synth_vbatch_pstar(self.h, dptr(a))
        return a

    def set_mode(self, mode, zero_col=0):
        """mode[b]: MODE_MODEL, MODE_NAN (x[0] = NaN), MODE_ZERO_COLUMN (no dependence on variable zero_col), MODE_BOX_NAN (every
        x NaN when a variable lies outside the box of set_box)"""
        m = np.ascontiguousarray(mode, dtype=np.uint8)
        assert m.shape == (self.B,) and 0 <= zero_col < self.N
        assert self.lib.synth_vbatch_set_mode(self.h, m.ctypes.data_as(C.c_char_p), zero_col) == 0

    def set_box(self, lower, upper):
        lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (lower, upper))
        assert lo.shape == hi.shape == (self.B, self.N)
        assert self.lib.synth_vbatch_set_box(self.h, dptr(lo), dptr(hi)) == 0

    def ncalls(self):
        """invocations of the values callback"""
        return self.lib.synth_vbatch_ncalls(self.h)

    def ncopies(self):
        """problem-copies requested (copies x B over all invocations)"""
        return self.lib.synth_vbatch_ncopies(self.h)

    def nevals(self):
        """problem-copies evaluated (live problems only; the naive reference's launches count here too)"""
        return self.lib.synth_vbatch_nevals(self.h)

    def reset_counters(self):
        self.lib.synth_vbatch_reset_counters(self.h)

    def close(self):
        if self.h:
            self.lib.synth_vbatch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NaiveNumeric:
    """the naive numeric Jacobian over a DeviceValuesBatch as a dogleg_callback_device_batch_t (cb, cookie).  The deltas are
    used as they are: pass the defaults yourself."""

    def __init__(self, vb, scheme, delta_rel, delta_abs, lower=None, upper=None):
        self.vb = vb
        lo = None if lower is None else np.ascontiguousarray(lower, dtype=np.float64)
        hi = None if upper is None else np.ascontiguousarray(upper, dtype=np.float64)
        self.h = vb.lib.synth_vnaive_create(vb.h, scheme, delta_rel, delta_abs, None if lo is None else dptr(lo),
                                            None if hi is None else dptr(hi))
        assert self.h, "naive reference creation failed"
        self.cb = C.cast(vb.lib.synth_cb_device_batch_naive, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def close(self):
        if self.h:
            self.vb.lib.synth_vnaive_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCopy:
    """a device-to-device copy that moves bytes_moved bytes (half of them read, half written): run() gives one copy's time in ms
    (events).  The yardstick of tools/batch_numeric_bench.py."""

    def __init__(self, bytes_moved):
        self.lib = lib()
        self.h = self.lib.synth_copy_create(int(bytes_moved))
        assert self.h, "copy buffers: allocation failed"

    def run(self):
        ms = self.lib.synth_copy_run(self.h)
        assert ms >= 0.0
        return ms

    def close(self):
        if self.h:
            self.lib.synth_copy_free(self.h)
            self.h = None
