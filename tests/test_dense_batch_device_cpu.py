"""The device-resident batch entry points without a GPU: their export, the ABI a C user compiles against (tests/c/
batch_device_abi.c) and the refusals that are decided before any pointer is looked at -- each returns -1, invokes nothing and
writes nothing.  The arrays handed over here are host arrays: a call that got past these checks would be refused by the
pointer check that follows them, never launched."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd import capi
from libdogleg_amd import ctypes_defs as d
from libdogleg_amd.ctypes_defs import CB_DEVICE_BATCH, BATCH_MAX_NSTATE, BatchResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_batch_device", "dogleg_amd_optimize_dense_products_batch_device",
         "dogleg_amd_dense_batch_uncertainty_device", "dogleg_amd_dense_products_batch_uncertainty_device",
         "dlg_batch_device_span_ok")


def test_symbols_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n
        assert hasattr(capi.lib(), n)


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_device_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_device_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [int(v) for v in r.stdout.split()] == [40, d.BATCH_NOT_RUN, d.BATCH_UNC_SKIPPED] == [40, 0, 2]
    assert C.sizeof(BatchResult) == 40
    assert [getattr(BatchResult, n).offset for n, _ in BatchResult._fields_] == [0, 8, 16, 24, 28, 32]


def test_refusals_that_need_no_device():
    calls = []
    cb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, M, B = 3, 12, 4
    SENT = -7.5
    buf = dict(p=np.arange(1.0, 1.0 + B * N), res=np.full(B * 5, SENT), lam=np.full(B, SENT), cov=np.full(B * N * N, SENT),
               var=np.full(B * N, SENT), fac=np.full(B * M, SENT), scale=np.full(B, 1.0), status=np.full(B, 42, dtype=np.int32),
               big=np.ones(BATCH_MAX_NSTATE + 1))
    keep = {k: v.copy() for k, v in buf.items()}
    a = lambda k: None if k is None else buf[k].ctypes.data
    prm = capi.default_parameters()

    def unchanged(rc):
        for k in buf:
            assert np.array_equal(buf[k], keep[k]), k
        return rc

    def solve(p="p", b=B, n=N, m=M, fn=f, res="res"):
        return unchanged(capi.optimize_dense_batch_device(a(p), b, n, m, fn, None, prm, a(res), a("lam")))

    def solve_p(p="p", b=B, n=N, fn=f, res="res"):
        return unchanged(capi.optimize_dense_products_batch_device(a(p), b, n, fn, None, prm, a(res), a("lam")))

    def unc(p="p", b=B, n=N, m=M, fn=f, status="status", scale="scale", fs=1):
        return unchanged(capi.dense_batch_uncertainty_device(a(p), b, n, m, fn, None, a(status), a("lam"), a("cov"), a("var"),
                                                             a("fac"), a(scale), fs))

    def unc_p(p="p", b=B, n=N, fn=f, status="status"):
        return unchanged(capi.dense_products_batch_uncertainty_device(a(p), b, n, fn, None, prm, a(status), a("lam"), a("cov"),
                                                                      a("var")))

    assert solve(p=None) == -1 and solve(fn=None) == -1 and solve(res=None) == -1
    assert solve_p(p=None) == -1 and solve_p(fn=None) == -1 and solve_p(res=None) == -1
    assert unc(p=None) == -1 and unc(fn=None) == -1 and unc(status=None) == -1
    assert unc_p(p=None) == -1 and unc_p(fn=None) == -1 and unc_p(status=None) == -1
    assert solve(b=0) == -1 and solve_p(b=0) == -1 and unc(b=0) == -1 and unc_p(b=0) == -1
    n65 = BATCH_MAX_NSTATE + 1
    assert solve(p="big", b=1, n=n65) == -1 and solve_p(p="big", b=1, n=n65) == -1
    assert unc(p="big", b=1, n=n65, m=200) == -1 and unc_p(p="big", b=1, n=n65) == -1
    assert unc(fs=3) == -1                                      # feature sizes above 2
    assert unc(scale=None) == -1                                # factors without scale
    assert not calls
