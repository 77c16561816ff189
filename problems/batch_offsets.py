"""A DeviceBatch (problems/batch.py) with a per-problem offset array added to x: OffsetDeviceBatch is the batch callback of
problems/device_batch_offsets.hip (the inner model, then x[b] += off[b] on the callback's stream, live problems only),
OffsetHostProblem the same function for the host oracles, HostProblem.eval(p)[0] + off.  The offsets plant gross outliers
for the robust batch solve.  Inputs for tests/ and tools/ only -- nothing here computes what is checked."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd.ctypes_defs import dptr
from problems import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "problems", "device_batch_offsets.hip")
_LIB = os.path.join(ROOT, "problems", "libproblems_batch_offsets.so")
_lib = None


def build():
    """hipcc build with the flags problems/batch.py gives its libraries"""
    if batch._stale(_LIB, _SRC):
        subprocess.run([batch.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-o", _LIB, _SRC], check=True)
    return _LIB


def lib():
    """problems/libproblems_batch_offsets.so; needs a HIP device at call time, not at load time"""
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        V = C.c_void_p
        L.synth_offsets_create.restype = V
        L.synth_offsets_create.argtypes = [V, V, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.synth_offsets_free.argtypes = [V]
        L.synth_offsets_free.restype = None
        _lib = L
    return _lib


def planted_offsets(B, M, fs, fraction, size, seed):
    """(off (B, M), planted (B, M // fs) bool): round(fraction * M / fs) features per problem, chosen by a seeded generator,
    have every one of their rows displaced by +-size"""
    rng = np.random.default_rng(seed)
    NF = M // fs
    k = int(round(fraction * NF))
    off = np.zeros((B, M))
    planted = np.zeros((B, NF), dtype=bool)
    for b in range(B):
        f = rng.choice(NF, size=k, replace=False)
        planted[b, f] = True
        sign = rng.choice([-1.0, 1.0], size=(k, fs))
        off[b].reshape(NF, fs)[f] = size * sign
    return off, planted


class OffsetDeviceBatch:
    """db (a DeviceBatch, which it then owns) with off (B, M) added to x; the interface of DeviceBatch"""

    def __init__(self, db, off):
        self.lib, self.db = lib(), db
        self.B, self.M, self.N = db.B, db.M, db.N
        self.off = np.ascontiguousarray(off, dtype=np.float64)
        assert self.off.shape == (self.B, self.M)
        self.h = self.lib.synth_offsets_create(db.cb, db.cookie, self.B, self.M, dptr(self.off))
        assert self.h, "offset batch creation failed"
        self.cb = C.cast(self.lib.synth_cb_device_batch_offsets, C.c_void_p)
        self.cookie = C.c_void_p(self.h)

    def p0(self):
        return self.db.p0()

    def set_mode(self, mode, zero_col=0):
        self.db.set_mode(mode, zero_col)

    def ncalls(self):
        return self.db.ncalls()

    def nevals(self):
        return self.db.nevals()

    def reset_counters(self):
        self.db.reset_counters()

    def close(self):
        if self.h:
            self.lib.synth_offsets_free(self.h)
            self.h = None
        self.db.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OffsetHostProblem:
    """hp (an object with p0(), eval(p), N, M: tests/batch_oracle.py's HostProblem) with off (M,) added to x"""

    def __init__(self, hp, off):
        self.hp, self.N, self.M = hp, hp.N, hp.M
        self.off = np.ascontiguousarray(off, dtype=np.float64)
        assert self.off.shape == (self.M,)

    def p0(self):
        return self.hp.p0()

    def eval(self, p):
        x, J = self.hp.eval(p)
        return x + self.off, J

    def close(self):
        self.hp.dp.close()
