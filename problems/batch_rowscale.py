"""A batch callback (a DeviceBatch of problems/batch.py, or anything with its interface, an OffsetDeviceBatch say) with row r of
x and J of every live problem multiplied by sqrt(w[b][r // fs]): RowScaleDeviceBatch is the batch callback of
problems/device_batch_rowscale.hip (the inner model, then one kernel over all of x and J on the callback's stream),
RowScaleHostProblem the same function for the host oracles.  This is the way to the uncertainty of a robust batch fit without
the ..._fit entry points: a test input (the fit forms are compared with it) and the benchmark's opponent.  Inputs for tests/
and tools/ only -- nothing here computes what is checked."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr
from problems import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_batch_rowscale.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_batch_rowscale.so")
_lib = None


def build():
    """hipcc build with the flags problems/batch.py gives its libraries"""
    if batch._stale(_LIB, _SRC):
        subprocess.run([batch.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_batch_rowscale.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V = C.c_void_p
        L.synth_rowscale_create.restype = V
        L.synth_rowscale_create.argtypes = [V, V, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.synth_rowscale_free.argtypes = [V]
        L.synth_rowscale_free.restype = None
        _lib = L
    return _lib


class RowScaleDeviceBatch:
    """db (an object with the interface of DeviceBatch, which stays the caller's) with the rows of x and J scaled by the square
    roots of w (B, M // fs); cb and cookie are the batch callback"""

    def __init__(self, db, w, fs):
        self.lib, self.db = lib(), db
        self.B, self.M, self.N, self.fs = db.B, db.M, db.N, fs
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        assert self.M % fs == 0 and self.w.shape == (self.B, self.M // fs)
        self.h = self.lib.synth_rowscale_create(db.cb, db.cookie, self.B, self.M, self.N, fs, dptr(self.w))
        assert self.h, "row-scaling batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch_rowscale, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def close(self):
        if self.h:
            self.lib.synth_rowscale_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowScaleHostProblem:
    """hp (an object with eval(p), N, M) with the rows of x and J scaled by the square roots of w (M // fs,)"""

    def __init__(self, hp, w, fs):
        self.hp, self.N, self.M = hp, hp.N, hp.M
        self.sw = np.repeat(np.sqrt(np.ascontiguousarray(w, dtype=np.float64)), fs)
        assert self.sw.shape == (self.M,)

    def eval(self, p):
        x, J = self.hp.eval(p)
        return self.sw * x, self.sw[:, None] * J
