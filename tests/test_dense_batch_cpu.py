"""dogleg_amd_optimize_dense_batch as a C user compiles against it, the layout of its result struct, and its refusals
that need no device (none of them touches p); on a machine without a GPU a valid call returns -1 cleanly, as
dogleg_optimize* returns -1.0 there."""
import ctypes as C
import os
import subprocess

import numpy as np

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchResult, CB_DEVICE_BATCH, BATCH_MAX_NSTATE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "dogleg.h"

typedef int (*batch_fn)(double*, unsigned int, unsigned int, unsigned int, dogleg_callback_device_batch_t*, void*,
                        const dogleg_parameters2_t*, dogleg_amd_batch_result_t*);
static void cb(const double* p_dev, double* x_dev, double* J_dev, const unsigned char* live_dev, unsigned int B,
               void* hip_stream, void* cookie)
{ (void)p_dev; (void)x_dev; (void)J_dev; (void)live_dev; (void)B; (void)hip_stream; (void)cookie; }

int main(void)
{
  batch_fn f = &dogleg_amd_optimize_dense_batch;
  dogleg_callback_device_batch_t* c = &cb;
  dogleg_amd_batch_result_t r;
  double p[2] = {1.0, 2.0};
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(dogleg_amd_batch_result_t), offsetof(dogleg_amd_batch_result_t, norm2_x),
         offsetof(dogleg_amd_batch_result_t, trustregion), offsetof(dogleg_amd_batch_result_t, lambda),
         offsetof(dogleg_amd_batch_result_t, iterations), offsetof(dogleg_amd_batch_result_t, evaluations),
         offsetof(dogleg_amd_batch_result_t, status));
  printf("%d %d %d %d %d %d\n", DOGLEG_AMD_BATCH_MAX_NSTATE, DOGLEG_AMD_BATCH_JTX, DOGLEG_AMD_BATCH_SMALL_STEP,
         DOGLEG_AMD_BATCH_TRUSTREGION, DOGLEG_AMD_BATCH_MAX_ITERATIONS, DOGLEG_AMD_BATCH_FAILED);
  /* no callback: -1, never an exit, p as it was */
  printf("%d %g %g\n", f(p, 1, 2, 4, NULL, NULL, NULL, &r), p[0], p[1]);
  return (f && c) ? 0 : 1;
}
'''


def test_symbol_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in ("dogleg_amd_optimize_dense_batch", "dogleg_amd_batch_last_stats"):
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n


def test_prototype_and_result_struct_layout(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", libdir, "-ldogleg_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    want = [C.sizeof(BatchResult)] + [getattr(BatchResult, n).offset for n in
                                      ("norm2_x", "trustregion", "lambda_", "iterations", "evaluations", "status")]
    assert [int(v) for v in lines[0].split()] == want
    from libdogleg_amd import ctypes_defs as d
    assert [int(v) for v in lines[1].split()] == [BATCH_MAX_NSTATE, d.BATCH_JTX, d.BATCH_SMALL_STEP, d.BATCH_TRUSTREGION,
                                                  d.BATCH_MAX_ITERATIONS, d.BATCH_FAILED]
    assert BATCH_MAX_NSTATE >= 32
    assert lines[2].split() == ["-1", "1", "2"]


def test_refusals_leave_p_alone():
    L = capi.lib()
    calls = []
    cb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, M, B = 3, 12, 4
    p0 = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    res = (BatchResult * B)()

    def call(p, b, n, m, fn, r):
        return L.dogleg_amd_optimize_dense_batch(None if p is None else capi.dptr(p), b, n, m, fn, None, None, r)

    p = p0.copy()
    assert call(p, 0, N, M, f, res) == -1                       # B == 0
    assert call(p, B, 0, M, f, res) == -1                       # Nstate == 0
    assert call(p, B, N, 0, f, res) == -1                       # Nmeas == 0
    assert call(p, B, N, M, None, res) == -1                    # no callback
    assert call(None, B, N, M, f, res) == -1                    # no p
    assert call(p, B, N, M, f, None) == -1                      # no results
    big = np.ones((1, BATCH_MAX_NSTATE + 1))
    assert call(big, 1, BATCH_MAX_NSTATE + 1, M, f, res) == -1  # above the cap
    assert np.all(big == 1.0)
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call(p, B, N, M, f, res) == -1                   # a communicator is set: one rank only
    finally:
        L.dogleg_amd_clear_communicator()
    assert np.array_equal(p, p0) and not calls


def test_valid_call_without_a_device_fails_cleanly():
    L = capi.lib()
    if L.dlg_device_count() > 0:
        return                                                   # (with a GPU: tests/test_dense_batch_gpu.py)
    cb = CB_DEVICE_BATCH(lambda *a: None)
    p0 = np.arange(1.0, 13.0).reshape(4, 3)
    rc, p, res = capi.optimize_dense_batch(p0, 3, 12, C.cast(cb, C.c_void_p), None)
    assert rc == -1 and np.array_equal(p, p0)
    L.dogleg_amd_release_cache()
