"""dogleg_amd_optimize_dense_products_batch and dogleg_amd_dense_products_batch_uncertainty as a C user compiles against
them, their refusals that need no device (none of them touches p or an output, none calls the callback), a valid call on
a machine without a GPU, and the CPU half of tests/test_dense_products_batch_gpu.py: the decision margins recorded in
tests/batch_products_oracle.py, reproduced with the products oracle alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchResult, CB_DEVICE_BATCH_PRODUCTS, BATCH_MAX_NSTATE, Parameters2
from tests import batch_products_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_products_batch", "dogleg_amd_dense_products_batch_uncertainty")

PROBE = r'''
#include <stdio.h>
#include "dogleg.h"

typedef int (*solve_fn)(double*, unsigned int, unsigned int, dogleg_callback_device_batch_products_t*, void*,
                        const dogleg_parameters2_t*, dogleg_amd_batch_result_t*);
typedef int (*unc_fn)(const double*, unsigned int, unsigned int, dogleg_callback_device_batch_products_t*, void*,
                      const dogleg_parameters2_t*, double*, double*, double*, int*);
static void cb(const double* p_dev, double* norm2x_dev, double* xtJ_dev, double* JtJ_dev, const unsigned char* live_dev,
               unsigned int B, void* hip_stream, void* cookie)
{ (void)p_dev; (void)norm2x_dev; (void)xtJ_dev; (void)JtJ_dev; (void)live_dev; (void)B; (void)hip_stream; (void)cookie; }

int main(void)
{
  solve_fn f = &dogleg_amd_optimize_dense_products_batch;
  unc_fn u = &dogleg_amd_dense_products_batch_uncertainty;
  dogleg_callback_device_batch_products_t* c = &cb;
  dogleg_amd_batch_result_t r;
  double p[2] = {1.0, 2.0}, var[2] = {7.0, 8.0};
  int status = 9;
  /* no callback: -1, never an exit, p and the outputs as they were */
  printf("%d %g %g\n", f(p, 1, 2, NULL, NULL, NULL, &r), p[0], p[1]);
  printf("%d %g %g %d\n", u(p, 1, 2, NULL, NULL, NULL, NULL, NULL, var, &status), var[0], var[1], status);
  return (f && u && c) ? 0 : 1;
}
'''


def test_symbols_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n


def test_prototypes_compile_as_c(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", libdir, "-ldogleg_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split() == ["-1", "1", "2"] and lines[1].split() == ["-1", "7", "8", "9"]


def _layout(packed, upper):
    prm = Parameters2()
    capi.lib().dogleg_getDefaultParameters(C.byref(prm))
    prm.JtJ_packed, prm.JtJ_upper = packed, upper
    return prm


def test_solve_refusals_leave_p_alone():
    L = capi.lib()
    calls = []
    cb = CB_DEVICE_BATCH_PRODUCTS(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, B = 3, 4
    p0 = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    res = (BatchResult * B)()

    def call(p, b, n, fn, r, prm=None):
        return L.dogleg_amd_optimize_dense_products_batch(None if p is None else capi.dptr(p), b, n, fn, None,
                                                          None if prm is None else C.byref(prm), r)

    p = p0.copy()
    assert call(p, 0, N, f, res) == -1                       # B == 0
    assert call(p, B, 0, f, res) == -1                       # Nstate == 0
    assert call(p, B, N, None, res) == -1                    # no callback
    assert call(None, B, N, f, res) == -1                    # no p
    assert call(p, B, N, f, None) == -1                      # no results
    big = np.ones((1, BATCH_MAX_NSTATE + 1))
    assert call(big, 1, BATCH_MAX_NSTATE + 1, f, res) == -1  # above the cap
    assert np.all(big == 1.0)
    assert call(p, B, N, f, res, _layout(True, False)) == -1  # packed lower
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call(p, B, N, f, res) == -1                   # a communicator is set: one rank only
        assert call(p, B, N, f, res, _layout(True, True)) == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert np.array_equal(p, p0) and not calls


def test_uncertainty_refusals_leave_the_outputs_alone():
    L = capi.lib()
    calls = []
    cb = CB_DEVICE_BATCH_PRODUCTS(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, B = 3, 4
    p = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    out = dict(lam=np.full(B, 0.5), cov=np.full((B, N, N), 7.0), var=np.full((B, N), 8.0), status=np.full(B, 9, dtype=np.int32))
    keep = {k: v.copy() for k, v in out.items()}

    def call(p_, b, n, fn, prm=None, cov=True, var=True, status=True):
        return L.dogleg_amd_dense_products_batch_uncertainty(
            None if p_ is None else capi.dptr(p_), b, n, fn, None, None if prm is None else C.byref(prm), capi.dptr(out["lam"]),
            capi.dptr(out["cov"]) if cov else None, capi.dptr(out["var"]) if var else None,
            capi.iptr(out["status"]) if status else None)

    assert call(p, 0, N, f) == -1
    assert call(p, B, 0, f) == -1
    assert call(p, B, N, None) == -1
    assert call(None, B, N, f) == -1
    assert call(p, B, N, f, status=False) == -1
    assert call(p, B, BATCH_MAX_NSTATE + 1, f) == -1
    assert call(p, B, N, f, _layout(True, False)) == -1       # packed lower
    assert call(p, B, N, f, cov=False, var=False) == -1       # nothing asked for
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call(p, B, N, f) == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert all(np.array_equal(out[k], keep[k]) for k in out) and not calls


def test_valid_calls_without_a_device_fail_cleanly():
    L = capi.lib()
    if L.dlg_device_count() > 0:
        return                                                   # (with a GPU: tests/test_dense_products_batch_gpu.py)
    calls = []
    cb = CB_DEVICE_BATCH_PRODUCTS(lambda *a: calls.append(a))
    p0 = np.arange(1.0, 13.0).reshape(4, 3)
    for prm in (None, _layout(True, True), _layout(False, False)):
        rc, p, res = capi.optimize_dense_products_batch(p0, 3, C.cast(cb, C.c_void_p), None, prm)
        assert rc == -1 and np.array_equal(p, p0)
        out = capi.dense_products_batch_uncertainty(p0, 3, C.cast(cb, C.c_void_p), None, prm, lam=np.zeros(4))
        assert out["rc"] == -1 and not out["cov"].any() and not out["var"].any() and np.all(out["status"] == -1)
    assert not calls
    L.dogleg_amd_release_cache()


# ---------------------------------------------------------------- the CPU half of the GPU tests: the recorded margins
@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(po.PARITY))
def test_parity_margins(shape, setname):
    N, M = shape
    B, want = po.PARITY[shape]
    orc = po.oracle_batch(N, M, 1, B, setname)
    po.assert_margin(orc, f"{shape} {setname}", want[setname])
    if setname == "diverse":
        types = set().union(*[o["step_types"] for o in orc])
        assert types == ({0, 1, 2} if N >= 2 else {0, 1})


@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("N", sorted(po.RAGGED))
def test_ragged_margins(N, setname):
    (Mmin, Mmax), want = po.RAGGED[N]
    Ms = po.ragged_M(po.B, Mmin, Mmax)
    # (7 and 96 - 20 + 1 = 77 share a factor: the N 16 set has 11 different M, up to 90)
    assert Ms.min() == Mmin and Mmin < Ms.max() <= Mmax and len(set(Ms[:4])) == 4    # one workgroup holds four different M
    orc = po.oracle_batch(N, 0, 1, po.B, setname, ragged=(Mmin, Mmax))
    po.assert_margin(orc, f"ragged N {N} {setname}", want[setname])


def test_hard_set_margin_and_rejections():
    N, M = po.HARD_SHAPE
    orc = po.oracle_batch(N, M, po.HARD_SEED0, po.HARD_B, "hard")
    po.assert_margin(orc, "hard set", po.HARD_MARGIN)
    assert sum(o["rejected"] for o in orc) == po.HARD_REJECTED
    ev = [o["evaluations"] for o in orc]
    assert (min(ev), max(ev)) == po.HARD_EVALS


@pytest.mark.parametrize("shape", sorted(po.ZERO_COLUMN))
def test_zero_column_margins_and_lambdas(shape):
    N, M = shape
    col, want = po.ZERO_COLUMN[shape]
    orc = po.oracle_batch(N, M, 1, po.ZERO_B, "default", zero=(po.ZERO_CHOSEN, col))
    po.assert_margin(orc, f"zero column {shape}", want)
    assert [o["lambda_"] for o in orc] == [1e-10 if b in po.ZERO_CHOSEN else 0.0 for b in range(po.ZERO_B)]


def test_the_table_reaches_every_size_class_and_both_kinds_of_triangle_load():
    Ns = {N for N, _ in po.PARITY}
    assert {1, 8, 9, 16, 17, 24, 25, 32} <= Ns
    assert any(N * (N + 1) // 2 <= 64 for N in Ns) and any(N * (N + 1) // 2 > 64 for N in Ns if N <= 16)
    assert po.B % 4 == 1 and po.B_SMALL % 4 == 1            # a last wavefront alone in its workgroup
