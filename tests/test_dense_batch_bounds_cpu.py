"""The bounded batch solve without a GPU: the NumPy oracle of its loop (tests/batch_bounds_oracle.py) held against the robust
oracle where the bounds clamp nothing, against the exact bounded least-squares solution on linear problems, and on the example
that takes the fallback; of the library what needs no device: the exports, the header as C and the refusals -- each returns
-1, invokes nothing and writes nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (CB_DEVICE_BATCH, BatchResult, BatchLoss, BatchBounds, BATCH_JTX, BATCH_SMALL_STEP,
                                       BATCH_FAILED, LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY, dptr)
from problems.batch_linear import LinearHostProblem, exact_bounded_solution, from_normal_equations
from tests import batch_oracle as bo
from tests import batch_bounds_oracle as bb
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_gpu as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_batch_bounded", "dogleg_amd_optimize_dense_batch_bounded_device")
KINDS = {"trivial": LOSS_TRIVIAL, "huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}
KKT_TOL = 1e-9


def fallback_example():
    """(hp, lo, hi, prm): H = [[1, .95], [.95, 1]], g(0) = (-.14, -.25), upper = (inf, 0.1), trustregion0 = 10.  The first step
    is the Gauss-Newton step (-1, 1.2); clipped it is (-1, 0.1), whose expected improvement is -1.05"""
    A, y = from_normal_equations([[1.0, 0.95], [0.95, 1.0]], [-0.14, -0.25])
    prm = tb.params("default")
    prm.trustregion0 = 10.0
    return LinearHostProblem(A, y, np.zeros(2)), np.full(2, -np.inf), np.array([np.inf, 0.1]), prm


def random_linear(N, seed):
    """(A, y, p0, lo, hi): M = N + 3 rows of unit normals, a box around 0 that cuts the unbounded optimum off in some
    variables, one side open here and there, the start point anywhere (also outside)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N + 3, N))
    y = rng.standard_normal(N + 3) * 2.0
    lo, hi = -rng.random(N), rng.random(N)
    lo[rng.random(N) < 0.25] = -np.inf
    hi[rng.random(N) < 0.25] = np.inf
    return A, y, rng.standard_normal(N) * 1.5, lo, hi


# ---------------------------------------------------------------- 1. bounds that clamp nothing: the robust oracle, exactly
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("setname,seed0,nb", [("diverse", 1, 64), ("hard", tb.HARD_SEED0, tb.HARD_B)])
def test_infinite_bounds_reproduce_the_robust_oracle(setname, seed0, nb, kind):
    N, M, fs = 6, 40, 2
    eps, noise, spread, _ = tb.SETS[setname]
    prm = tb.params(setname)
    loss = ro.Loss(KINDS[kind], 0.5 * noise * np.sqrt(fs), fs)
    for b in range(nb):
        hp = bo.HostProblem(M, N, seed0 + b, eps, noise, spread)
        want = ro.solve_one(hp, prm, loss)
        for lo, hi in ((None, None), (np.full(N, -np.inf), np.full(N, np.inf))):
            got = bb.solve_one(hp, prm, loss, lo, hi)
            for k, v in want.items():
                if isinstance(v, np.ndarray):
                    assert got[k].tobytes() == v.tobytes(), (b, k)
                else:
                    assert got[k] == v, (b, k, got[k], v)
            assert not got["held"].any() and got["clipped"] == got["fallbacks"] == got["held_steps"] == 0
        hp.dp.close()


# ---------------------------------------------------------------- 2. linear problems: the exact bounded solution
@pytest.mark.parametrize("N", [2, 3])
def test_linear_problems_reach_the_exact_bounded_solution(N):
    prm = tb.params("default")
    worst, nheld, nclipped = 0.0, 0, 0
    for seed in range(1, 41):
        A, y, p0, lo, hi = random_linear(N, seed)
        r = bb.solve_one(LinearHostProblem(A, y, p0), prm, ro.Loss(LOSS_TRIVIAL), lo, hi)
        exact = exact_bounded_solution(A, y, lo, hi)
        assert r["status"] in (BATCH_JTX, BATCH_SMALL_STEP), (seed, r["status"])
        assert np.all(r["p"] >= lo) and np.all(r["p"] <= hi) and np.all(r["first_p"] >= lo) and np.all(r["first_p"] <= hi)
        err = float(np.max(np.abs(r["p"] - exact)))
        worst = max(worst, err)
        assert err <= KKT_TOL, (seed, err, r["p"], exact)
        # a held variable sits on its bound, bit for bit; none is held where the exact solution lies inside
        at_lo, at_hi = r["held"] == bb.AT_LOWER, r["held"] == bb.AT_UPPER
        assert np.all(r["p"][at_lo] == lo[at_lo]) and np.all(r["p"][at_hi] == hi[at_hi])
        assert not r["held"][(exact > lo + 1e-6) & (exact < hi - 1e-6)].any()
        nheld += bool(r["held"].any())
        nclipped += r["clipped"] > 0
    print(f"N = {N}: 40 problems, {nheld} end with a held variable, {nclipped} clipped a step, worst |p - exact| {worst:.3g}")
    assert nheld >= 20 and nclipped >= 10


# ---------------------------------------------------------------- 3. the fallback
def test_the_fallback_example_takes_exactly_one_fallback():
    hp, lo, hi, prm = fallback_example()
    x, J = hp.eval(hp.p0())
    H, g = J.T @ J, J.T @ x
    assert np.allclose(H, [[1.0, 0.95], [0.95, 1.0]], rtol=0, atol=1e-15) and np.allclose(g, [-0.14, -0.25], rtol=0, atol=1e-15)
    gn = -np.linalg.solve(H, g)
    assert np.allclose(gn, [-1.0, 1.2], rtol=0, atol=1e-12)
    _, s, clamped = bb.clip(hp.p0(), gn, lo, hi)
    assert clamped.tolist() == [False, True] and abs(bb.expected_improvement(g, H, s) + 1.05) < 1e-12
    r = bb.solve_one(hp, prm, ro.Loss(LOSS_TRIVIAL), lo, hi)
    assert r["fallbacks"] == 1 and r["clipped"] >= 1 and r["status"] in (BATCH_JTX, BATCH_SMALL_STEP)
    assert r["held"].tolist() == [bb.FREE, bb.AT_UPPER]
    assert float(np.max(np.abs(r["p"] - exact_bounded_solution(hp.A, hp.y, lo, hi)))) <= KKT_TOL


def test_bad_bounds_fail_alone_and_a_held_start_stops_at_once():
    hp, _, _, prm = fallback_example()
    for lo, hi in (([0.0, 1.0], [1.0, 0.5]), ([np.nan, 0.0], [1.0, 1.0]), ([0.0, 0.0], [1.0, np.nan])):
        r = bb.solve_one(hp, prm, ro.Loss(LOSS_TRIVIAL), lo, hi)
        assert (r["status"], r["evaluations"], r["iterations"], r["norm2_x"]) == (BATCH_FAILED, 0, 0, -1.0)
        assert r["p"].tobytes() == hp.p0().tobytes() and not r["held"].any()
    # g(0) < 0 in both variables: with upper = 0 both are held at the start
    r = bb.solve_one(hp, prm, ro.Loss(LOSS_TRIVIAL), [-1.0, -1.0], [0.0, 0.0])
    assert (r["status"], r["evaluations"], r["iterations"]) == (BATCH_JTX, 1, 0) and r["held"].tolist() == [2, 2]
    assert r["p"].tobytes() == hp.p0().tobytes()


# ---------------------------------------------------------------- 4. the library without a device
def test_symbols_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n
        assert hasattr(capi.lib(), n)


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_bounds_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_bounds_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    ptr = C.sizeof(C.c_void_p)
    assert [int(v) for v in lines[0].split()] == [C.sizeof(BatchBounds), BatchBounds.lower.offset, BatchBounds.upper.offset,
                                                  BatchBounds.held.offset, ptr] == [3 * ptr, 0, ptr, 2 * ptr, ptr]
    assert lines[1].split() == ["-1", "-1", "1", "2", "9", "9", "-3"]


def test_refusals_that_need_no_device():
    """both entry points; the device twin is handed host arrays: a call that got past the checks under test would be refused
    by the pointer check that follows them, never launched"""
    L = capi.lib()
    calls = []
    cb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, M, B = 3, 12, 4
    p0 = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    p = p0.copy()
    res = (BatchResult * B)()
    C.memset(res, 0xA5, C.sizeof(res))
    res0 = bytes(res)
    w = np.full((B, M), -7.5)
    lam = np.full(B, -7.5)
    lo, hi, held = np.zeros((B, N)), np.ones((B, N)), np.full((B, N), 9, dtype=np.uint8)
    good = BatchBounds(lo.ctypes.data, hi.ctypes.data, held.ctypes.data)
    huber = BatchLoss(LOSS_HUBER, 0.5, 2)

    def host_call(pp=p, b=B, n=N, m=M, fn=f, loss=None, bounds=good, r=res, wts=None):
        return L.dogleg_amd_optimize_dense_batch_bounded(None if pp is None else dptr(pp), b, n, m, fn, None, None,
                                                         None if loss is None else C.byref(loss),
                                                         None if bounds is None else C.byref(bounds), r,
                                                         None if wts is None else dptr(wts))

    def dev_call(pp=p, b=B, n=N, m=M, fn=f, loss=None, bounds=good, r=res, wts=None):
        return L.dogleg_amd_optimize_dense_batch_bounded_device(None if pp is None else pp.ctypes.data, b, n, m, fn, None, None,
                                                                None if loss is None else C.byref(loss),
                                                                None if bounds is None else C.byref(bounds),
                                                                None if r is None else C.addressof(r), lam.ctypes.data,
                                                                None if wts is None else wts.ctypes.data, None, None)

    for call in (host_call, dev_call):
        # the feature's own
        assert call(bounds=None) == -1
        assert call(wts=w) == -1                                 # weights without a loss
        # what the plain twin refuses
        assert call(b=0) == -1 and call(n=0) == -1 and call(m=0) == -1
        assert call(fn=None) == -1 and call(pp=None) == -1 and call(r=None) == -1
        # what the robust twin refuses
        assert call(loss=BatchLoss(4, 0.5, 1)) == -1 and call(loss=BatchLoss(LOSS_CAUCHY, 0.0, 1), wts=w) == -1
        assert call(loss=BatchLoss(LOSS_CAUCHY, 0.5, 5)) == -1 and call(loss=huber, m=13) == -1
        fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
        assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
        try:
            assert call() == -1 and call(loss=huber, wts=w) == -1
        finally:
            L.dogleg_amd_clear_communicator()
    assert np.array_equal(p, p0) and not calls and bytes(res) == res0 and np.all(w == -7.5) and np.all(lam == -7.5)
    assert np.all(held == 9) and not lo.any() and np.all(hi == 1.0)


def test_valid_call_without_a_device_fails_cleanly():
    L = capi.lib()
    if L.dlg_device_count() > 0:
        return                                                   # (with a GPU: tests/test_dense_batch_bounds_gpu.py)
    cb = CB_DEVICE_BATCH(lambda *a: None)
    p0 = np.arange(1.0, 13.0).reshape(4, 3)
    rc, p, res, held, w = capi.optimize_dense_batch_bounded(p0, 3, 12, C.cast(cb, C.c_void_p), None, None, np.full((4, 3), 20.0))
    assert rc == -1 and np.array_equal(p, p0) and np.all(held == 255) and w is None
    L.dogleg_amd_release_cache()
