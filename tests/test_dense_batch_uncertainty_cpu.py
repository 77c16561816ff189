"""dogleg_amd_dense_batch_uncertainty as a C user compiles against it, its export, and its refusals that need no device:
each returns -1 and leaves every output as it was."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd import ctypes_defs as d
from libdogleg_amd.ctypes_defs import CB_DEVICE_BATCH, BATCH_MAX_NSTATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <stdio.h>
#include "dogleg.h"

typedef int (*unc_fn)(const double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                      double*, double*, double*, double*, double*, int, int*);
typedef int (*stats_fn)(double*, int);

int main(void)
{
  unc_fn f = &dogleg_amd_dense_batch_uncertainty;
  stats_fn s = &dogleg_amd_batch_uncertainty_last_stats;
  double p[2] = {1.0, 2.0}, var[2] = {7.0, 7.0};
  int status[1] = {42};
  printf("%d %d\n", DOGLEG_AMD_BATCH_UNC_OK, DOGLEG_AMD_BATCH_UNC_FAILED);
  /* no callback: -1, never an exit, the outputs as they were */
  printf("%d %g %g %d\n", f(p, 1, 2, 4, NULL, NULL, NULL, NULL, var, NULL, NULL, 1, status), var[0], var[1], status[0]);
  return (f && s) ? 0 : 1;
}
'''


def test_symbol_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ("dogleg_amd_dense_batch_uncertainty", "dogleg_amd_batch_uncertainty_last_stats"):
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n


def test_prototype_compiles_and_constants(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", libdir, "-ldogleg_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [int(v) for v in lines[0].split()] == [d.BATCH_UNC_OK, d.BATCH_UNC_FAILED] == [0, 1]
    assert lines[1].split() == ["-1", "7", "7", "42"]


def test_refusals_leave_the_outputs_alone(capfd):
    L = capi.lib()
    calls = []
    cb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, M, B = 3, 12, 4
    SENT = -7.5
    p = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    buf = dict(lam=np.zeros(B), cov=np.full((B, N, N), SENT), var=np.full((B, N), SENT), fac=np.full((B, M), SENT),
               scale=np.full(B, 1.0), status=np.full(B, 42, dtype=np.int32))
    keep = {k: v.copy() for k, v in buf.items()}

    def call(p=p, b=B, n=N, m=M, fn=f, lam="lam", cov="cov", var="var", fac="fac", scale="scale", fs=1, status="status"):
        a = lambda k: None if k is None else (capi.iptr(buf[k]) if k == "status" else capi.dptr(buf[k]))
        rc = L.dogleg_amd_dense_batch_uncertainty(None if p is None else capi.dptr(p), b, n, m, fn, None, a(lam), a(cov), a(var),
                                                  a(fac), a(scale), fs, a(status))
        for k in buf:
            assert np.array_equal(buf[k], keep[k]), k
        return rc

    assert call(p=None) == -1                                   # no p
    assert call(fn=None) == -1                                  # no callback
    assert call(status=None) == -1                              # no status
    assert call(b=0) == -1 and call(n=0) == -1 and call(m=0) == -1
    big = np.ones((1, BATCH_MAX_NSTATE + 1))
    assert call(p=big, b=1, n=BATCH_MAX_NSTATE + 1) == -1       # above the cap
    assert call(fs=3) == -1                                     # feature sizes above 2
    assert call(scale=None) == -1                               # factors without scale
    assert call(cov=None, var=None, fac=None) == -1             # nothing asked for
    # a scale to be computed while Nmeas <= Nstate + 1
    buf["scale"][2] = keep["scale"][2] = 0.0
    assert call(m=N + 1) == -1 and call(m=N) == -1
    buf["scale"][2] = keep["scale"][2] = 1.0
    # device memory that cannot fit: refused from the sizes alone (p is not read), the message names the size
    capfd.readouterr()
    bmax, mmax = 0x7fffffff // 4, 0x7fffffff // (N + 1)
    assert call(b=bmax, m=mmax) == -1
    err = capfd.readouterr().err
    want = 8.0 * bmax * (mmax * (N + 1.0) + N + 3.0 + N + N * N + mmax)
    assert want > 1e15 and "bytes of device memory" in err and f"{want:.3g}" in err, err
    fn = capi.ALLREDUCE_FN(lambda b_, n_, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call() == -1                                     # a communicator is set: one rank only
    finally:
        L.dogleg_amd_clear_communicator()
    assert not calls


def test_valid_call_without_a_device_fails_cleanly():
    L = capi.lib()
    if L.dlg_device_count() > 0:
        pytest.skip("a GPU is present: the valid call is tests/test_dense_batch_uncertainty_gpu.py's")
    cb = CB_DEVICE_BATCH(lambda *a: None)
    p = np.arange(1.0, 13.0).reshape(4, 3)
    out = capi.dense_batch_uncertainty(p, 3, 12, C.cast(cb, C.c_void_p), None)
    assert out["rc"] == -1 and not out["cov"].any() and not out["var"].any() and not out["factors"].any()
    assert np.all(out["status"] == -1) and np.all(out["scale"] == -1.0)
    L.dogleg_amd_release_cache()
