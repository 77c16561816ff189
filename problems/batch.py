"""A batch of dense synthetic problems on the GPU (problems/device_batch_problems.hip) behind ctypes: problem b of a
DeviceBatch is DenseProblem(M, N, seed = seeds[b], eps, noise, p0_spread) of problems.c, evaluated by a
dogleg_callback_device_batch_t.  DeviceProductsBatch (problems/device_batch_products.hip, a library of its own) is the same
problems behind a dogleg_callback_device_batch_products_t, every problem with its own M.  Inputs for tests/ and tools/ only
-- nothing here computes what is checked."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_batch_problems.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_batch.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
_SRC_PRODUCTS = os.path.join(ROOT, "problems", "device_batch_products.hip")
_LIB_PRODUCTS = os.path.join(ROOT, "problems", "libproblems_batch_products.so")
_lib = None
_lib_products = None

MODE_MODEL, MODE_NAN, MODE_ZERO_COLUMN = 0, 1, 2
MODE_NAN_OFFDIAGONAL = 3                 # DeviceProductsBatch only: JtJ[0][1] = NaN and nothing else
LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER = 0, 1, 2


def _stale(lib, *srcs):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.exists(s) and os.path.getmtime(s) > t for s in srcs)


def build():
    """hipcc build with the flags oracle/Makefile gives libproblems_dev.so (same operation order and rounding as gcc
    gives problems.c on x86-64)"""
    for so, src in ((_LIB, _SRC), (_LIB_PRODUCTS, _SRC_PRODUCTS)):
        if _stale(so, src):
            subprocess.run([HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                            "-o", so, src], check=True)
    return _LIB


def lib():
    """problems/libproblems_batch.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V, D = C.c_void_p, C.POINTER(C.c_double)
        L.synth_batch_create.restype = V
        L.synth_batch_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_double, C.c_double, C.c_double]
        L.synth_batch_free.argtypes = [V]
        L.synth_batch_free.restype = None
        L.synth_batch_p0.argtypes = [V, D]
        L.synth_batch_p0.restype = None
        L.synth_batch_set_mode.argtypes = [V, C.c_char_p, C.c_int]
        L.synth_batch_ncalls.argtypes = [V]
        L.synth_batch_nevals.argtypes = [V]
        L.synth_batch_nevals.restype = C.c_longlong
        L.synth_batch_reset_counters.argtypes = [V]
        L.synth_batch_reset_counters.restype = None
        _lib = L
    return _lib


class DeviceBatch:
    """B dense problems of one shape on the GPU.  seeds: one per problem (int seed0: seed0 + b)."""

    def __init__(self, B, M, N, seeds=1, eps=0.3, noise=0.01, p0_spread=0.5):
        self.lib = lib()
        self.B, self.M, self.N = B, M, N
        self.eps, self.noise, self.p0_spread = eps, noise, p0_spread
        self.seeds = (np.arange(B, dtype=np.uint64) + np.uint64(seeds)) if np.isscalar(seeds) \
            else np.ascontiguousarray(seeds, dtype=np.uint64)
        assert self.seeds.shape == (B,)
        self.h = self.lib.synth_batch_create(B, M, N, self.seeds.ctypes.data_as(C.POINTER(C.c_uint64)), eps, noise, p0_spread)
        assert self.h, "device batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def p0(self):
        a = np.zeros((self.B, self.N))
        self.lib.synth_batch_p0(self.h, dptr(a))
        return a

    def set_mode(self, mode, zero_col=0):
        """mode[b]: MODE_MODEL, MODE_NAN (x[0] = NaN), MODE_ZERO_COLUMN (column zero_col of J exactly zero)"""
        m = np.ascontiguousarray(mode, dtype=np.uint8)
        assert m.shape == (self.B,) and 0 <= zero_col < self.N
        assert self.lib.synth_batch_set_mode(self.h, m.ctypes.data_as(C.c_char_p), zero_col) == 0

    def ncalls(self):
        """invocations of the batch callback"""
        return self.lib.synth_batch_ncalls(self.h)

    def nevals(self):
        """problem evaluations done (live problems over all invocations)"""
        return self.lib.synth_batch_nevals(self.h)

    def reset_counters(self):
        self.lib.synth_batch_reset_counters(self.h)

    def close(self):
        if self.h:
            self.lib.synth_batch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lib_products():
    """problems/libproblems_batch_products.so; needs a HIP device at call time, not at load time"""
    global _lib_products
    if _lib_products is None:
        build()
        L = C.CDLL(_LIB_PRODUCTS)
        V, D = C.c_void_p, C.POINTER(C.c_double)
        L.synth_pbatch_create.restype = V
        L.synth_pbatch_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.c_double, C.c_double,
                                          C.c_double]
        L.synth_pbatch_free.argtypes = [V]
        L.synth_pbatch_free.restype = None
        L.synth_pbatch_p0.argtypes = [V, D]
        L.synth_pbatch_p0.restype = None
        L.synth_pbatch_set_mode.argtypes = [V, C.c_char_p, C.c_int]
        L.synth_pbatch_set_layout.argtypes = [V, C.c_int]
        L.synth_pbatch_ncalls.argtypes = [V]
        L.synth_pbatch_nevals.argtypes = [V]
        L.synth_pbatch_nevals.restype = C.c_longlong
        L.synth_pbatch_reset_counters.argtypes = [V]
        L.synth_pbatch_reset_counters.restype = None
        _lib_products = L
    return _lib_products


class DeviceProductsBatch:
    """B dense problems of N variables on the GPU behind a dogleg_callback_device_batch_products_t.  M: one number of
    measurements for all, or one per problem; seeds: one per problem (int seed0: seed0 + b)."""

    def __init__(self, B, M, N, seeds=1, eps=0.3, noise=0.01, p0_spread=0.5, layout=LAYOUT_PACKED_UPPER):
        self.lib = lib_products()
        self.B, self.N = B, N
        self.M = np.ascontiguousarray(np.broadcast_to(M, (B,)), dtype=np.int32)
        self.eps, self.noise, self.p0_spread = eps, noise, p0_spread
        self.seeds = (np.arange(B, dtype=np.uint64) + np.uint64(seeds)) if np.isscalar(seeds) \
            else np.ascontiguousarray(seeds, dtype=np.uint64)
        assert self.seeds.shape == (B,)
        self.h = self.lib.synth_pbatch_create(B, N, self.M.ctypes.data_as(C.POINTER(C.c_int)),
                                              self.seeds.ctypes.data_as(C.POINTER(C.c_uint64)), eps, noise, p0_spread)
        assert self.h, "device batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch_products, C.c_void_p)
        self.cookie = C.c_void_p(self.h)
        self.set_layout(layout)

    def p0(self):
        a = np.zeros((self.B, self.N))
        self.lib.synth_pbatch_p0(self.h, dptr(a))
        return a

    def set_layout(self, layout):
        """LAYOUT_PACKED_UPPER (the library: JtJ_packed and JtJ_upper), LAYOUT_UNPACKED or LAYOUT_UNPACKED_NAN_LOWER (neither)"""
        assert self.lib.synth_pbatch_set_layout(self.h, layout) == 0
        self.layout = layout

    def set_params(self, prm):
        """prm with the JtJ_packed / JtJ_upper bits of this batch's layout"""
        prm.JtJ_packed = prm.JtJ_upper = self.layout == LAYOUT_PACKED_UPPER
        return prm

    def set_mode(self, mode, zero_col=0):
        """mode[b]: MODE_MODEL, MODE_NAN (x[0] = NaN), MODE_ZERO_COLUMN (column zero_col of J exactly zero),
        MODE_NAN_OFFDIAGONAL"""
        m = np.ascontiguousarray(mode, dtype=np.uint8)
        assert m.shape == (self.B,) and 0 <= zero_col < self.N
        assert self.lib.synth_pbatch_set_mode(self.h, m.ctypes.data_as(C.c_char_p), zero_col) == 0

    def ncalls(self):
        """invocations of the batch callback"""
        return self.lib.synth_pbatch_ncalls(self.h)

    def nevals(self):
        """problem evaluations done (live problems over all invocations)"""
        return self.lib.synth_pbatch_nevals(self.h)

    def reset_counters(self):
        self.lib.synth_pbatch_reset_counters(self.h)

    def close(self):
        if self.h:
            self.lib.synth_pbatch_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
