"""The bounded products batch solve without a GPU: of the library what needs no device -- the exports, the header as C and the
refusals, each of which returns -1, invokes nothing and writes nothing --; the batches of tests/batch_products_bounds_cases.py
against the margins recorded for them; and the NumPy oracle of the bounded loop (tests/batch_bounds_oracle.py) on the host twin
of the ragged linear model (problems/batch_linear_products.py) against the exact bounded least-squares solution."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (CB_DEVICE_BATCH_PRODUCTS, BatchResult, BatchBounds, BATCH_JTX, BATCH_SMALL_STEP,
                                       LOSS_TRIVIAL, dptr)
from problems.batch_linear_products import LinearHostProblem, exact_bounded_solution, random_ragged
from tests import batch_bounds_oracle as bb
from tests import batch_products_bounds_cases as pc
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_gpu as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_products_batch_bounded", "dogleg_amd_optimize_dense_products_batch_bounded_device")
KKT_TOL = 1e-9


# ---------------------------------------------------------------- 1. the library without a device
def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "dogleg.h")) as f:
        header = f.read()
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n
        assert hasattr(capi.lib(), n)
        assert f"int {n}(double* p" in header, n


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_products_bounds_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_products_bounds_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1", "-1", "1", "2", "9", "9", "-3"]
    for n in NAMES:
        assert n + ": bounds must be given" in r.stderr, r.stderr


def test_refusals_that_need_no_device():
    """both entry points; the device twin is handed host arrays: a call that got past the checks under test would be refused
    by the pointer check that follows them, never launched"""
    L = capi.lib()
    calls = []
    cb = CB_DEVICE_BATCH_PRODUCTS(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, B = 3, 4
    p0 = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    p = p0.copy()
    res = (BatchResult * B)()
    C.memset(res, 0xA5, C.sizeof(res))
    res0 = bytes(res)
    lam = np.full(B, -7.5)
    lo, hi, held = np.zeros((B, N)), np.ones((B, N)), np.full((B, N), 9, dtype=np.uint8)
    good = BatchBounds(lo.ctypes.data, hi.ctypes.data, held.ctypes.data)
    packed_upper, packed_lower = capi.default_parameters(), capi.default_parameters()
    packed_upper.JtJ_packed = packed_upper.JtJ_upper = True
    packed_lower.JtJ_packed, packed_lower.JtJ_upper = True, False

    def host_call(pp=p, b=B, n=N, fn=f, prm=packed_upper, bounds=good, r=res):
        return L.dogleg_amd_optimize_dense_products_batch_bounded(None if pp is None else dptr(pp), b, n, fn, None, C.byref(prm),
                                                                  None if bounds is None else C.byref(bounds), r)

    def dev_call(pp=p, b=B, n=N, fn=f, prm=packed_upper, bounds=good, r=res):
        return L.dogleg_amd_optimize_dense_products_batch_bounded_device(None if pp is None else pp.ctypes.data, b, n, fn, None,
                                                                         C.byref(prm), None if bounds is None else C.byref(bounds),
                                                                         None if r is None else C.addressof(r), lam.ctypes.data,
                                                                         None, None)

    for call in (host_call, dev_call):
        # the feature's own
        assert call(bounds=None) == -1
        # what the plain products twin refuses
        assert call(b=0) == -1 and call(n=0) == -1 and call(n=65) == -1
        assert call(fn=None) == -1 and call(pp=None) == -1 and call(r=None) == -1
        assert call(prm=packed_lower) == -1
        fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
        assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
        try:
            assert call() == -1
        finally:
            L.dogleg_amd_clear_communicator()
    assert np.array_equal(p, p0) and not calls and bytes(res) == res0 and np.all(lam == -7.5)
    assert np.all(held == 9) and not lo.any() and np.all(hi == 1.0)


def test_valid_call_without_a_device_fails_cleanly():
    L = capi.lib()
    if L.dlg_device_count() > 0:
        return                                                   # (with a GPU: tests/test_dense_products_batch_bounds_gpu.py)
    cb = CB_DEVICE_BATCH_PRODUCTS(lambda *a: None)
    p0 = np.arange(1.0, 13.0).reshape(4, 3)
    prm = capi.default_parameters()
    prm.JtJ_packed = prm.JtJ_upper = True
    rc, p, res, held = capi.optimize_dense_products_batch_bounded(p0, 3, C.cast(cb, C.c_void_p), None, None, np.full((4, 3), 20.0),
                                                                  prm)
    assert rc == -1 and np.array_equal(p, p0) and np.all(held == 255)
    L.dogleg_amd_release_cache()


# ---------------------------------------------------------------- 2. the batches are what the cases file records
@pytest.mark.parametrize("batch", pc.all_batches(), ids=lambda t: f"N{t[0]}-M{t[1][0]}..{t[1][1]}-B{t[2]}")
def test_the_recorded_margins(batch):
    N, ragged, B, every, recorded, nheld = batch
    orc, lo, hi, Ms = pc.oracle_batch(N, ragged, B, every)
    assert len(orc) == B and len(set(Ms.tolist())) > 1 and Ms.min() >= ragged[0] and Ms.max() <= ragged[1]
    pc.assert_margin(orc, recorded, f"N = {N}, M {ragged}, B = {B}")
    print(f"{pc.held_problems(orc)} of {B} problems end with a held variable (recorded {nheld})")
    assert pc.held_problems(orc) == nheld
    if every:
        assert N == 64 and any(o["held"][N - 1] for o in orc), "no problem holds the last variable: bit 63 is not exercised"
    for b, o in enumerate(orc):
        assert np.all(o["p"] >= lo[b]) and np.all(o["p"] <= hi[b])


# ---------------------------------------------------------------- 3. the ragged linear model: the exact bounded solution
@pytest.mark.parametrize("N,B", [(2, 40), (3, 40), (6, 12)])
def test_ragged_linear_problems_reach_the_exact_bounded_solution(N, B):
    prm = tb.params("default")
    A, y, p0, lo, hi = random_ragged(N, B, seed=1)
    assert len({a.shape[0] for a in A}) > 1 and all(np.linalg.matrix_rank(a) == N for a in A)
    worst, nheld, nclipped = 0.0, 0, 0
    for b in range(B):
        r = bb.solve_one(LinearHostProblem(A[b], y[b], p0[b]), prm, ro.Loss(LOSS_TRIVIAL), lo[b], hi[b])
        exact = exact_bounded_solution(A[b], y[b], lo[b], hi[b])
        assert r["status"] in (BATCH_JTX, BATCH_SMALL_STEP), (b, r["status"])
        assert np.all(r["p"] >= lo[b]) and np.all(r["p"] <= hi[b])
        assert np.all(r["first_p"] >= lo[b]) and np.all(r["first_p"] <= hi[b])
        err = float(np.max(np.abs(r["p"] - exact)))
        worst = max(worst, err)
        assert err <= KKT_TOL, (b, err, r["p"], exact)
        at_lo, at_hi = r["held"] == bb.AT_LOWER, r["held"] == bb.AT_UPPER
        assert np.all(r["p"][at_lo] == lo[b][at_lo]) and np.all(r["p"][at_hi] == hi[b][at_hi])
        nheld += bool(r["held"].any())
        nclipped += r["clipped"] > 0
    print(f"N = {N}: {B} problems of {sorted({a.shape[0] for a in A})} rows, {nheld} end with a held variable, {nclipped} clipped "
          f"a step, worst |p - exact| {worst:.3g}")
    assert 2 * nheld >= B and 4 * nclipped >= B
