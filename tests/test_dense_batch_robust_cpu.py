"""The robust batch solve without a GPU: the NumPy oracle of its loop (tests/batch_robust_oracle.py) held against the C oracle
under LOSS_TRIVIAL, its gradient against central differences for every loss, the point of the feature on the oracle alone
(planted outliers lose their pull), and of the library what needs no device: the exports, the header as C, and every refusal
-- each returns -1, invokes nothing and writes nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd import ctypes_defs as d
from libdogleg_amd.ctypes_defs import (CB_DEVICE_BATCH, BATCH_MAX_NSTATE, BatchResult, BatchLoss, LOSS_TRIVIAL, LOSS_HUBER,
                                       LOSS_SOFT_L1, LOSS_CAUCHY, dptr)
from problems.batch_offsets import OffsetHostProblem, planted_offsets
from tests import batch_oracle as bo
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_gpu as tb
from tests.parity import STEP_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_batch_robust", "dogleg_amd_optimize_dense_batch_robust_device")
KINDS = {"trivial": LOSS_TRIVIAL, "huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}


def host(N, M, seed, setname, off=None):
    eps, noise, spread, _ = tb.SETS[setname]
    hp = bo.HostProblem(M, N, int(seed), eps, noise, spread)
    return hp if off is None else OffsetHostProblem(hp, off)


# ---------------------------------------------------------------- 1. TRIVIAL is the plain loop
@pytest.mark.parametrize("setname,seed0,nb,fs", [("diverse", 1, 64, 1), ("hard", tb.HARD_SEED0, tb.HARD_B, 2)])
def test_trivial_reproduces_the_c_oracle(setname, seed0, nb, fs):
    N, M = 6, 40
    prm = tb.params(setname)
    orc = tb.oracle_batch(N, M, seed0, nb, setname)
    worst = dict(p=0.0, n2=0.0, tr=0.0, margin=0.0)
    rejected = 0
    for b in range(nb):
        hp = host(N, M, seed0 + b, setname)
        r, o = ro.solve_one(hp, prm, ro.Loss(LOSS_TRIVIAL, 1.0, fs)), orc[b]
        hp.dp.close()
        assert (r["iterations"], r["evaluations"], r["status"], r["lambda_"], r["rejected"], r["step_types"]) == \
               (o["iterations"], o["evaluations"], o["status"], o["lambda_"], o["rejected"], o["step_types"]), b
        worst["p"] = max(worst["p"], float(np.max(np.abs(r["p"] - o["p"]))))
        worst["n2"] = max(worst["n2"], abs(r["norm2_x"] - o["norm2_x"]) / max(abs(o["norm2_x"]), 1e-300))
        worst["tr"] = max(worst["tr"], abs(r["trustregion"] - o["trustregion"]) / abs(o["trustregion"]))
        worst["margin"] = max(worst["margin"], abs(r["margin"] - o["margin"]) / o["margin"])
        assert np.all(r["weights"] == 1.0) and r["weights"].shape == (M // fs,)
        rejected += r["rejected"]
    print(f"{setname}: {nb} problems, {rejected} rejected trials, worst differences {worst}")
    assert worst["p"] <= STEP_TOL and worst["n2"] <= tb.REL_SCALAR_TOL and worst["tr"] <= tb.REL_SCALAR_TOL
    # the same decisions measured the same way: the two differ by the rounding of rho near a solve's end, where F_before - F is
    # a difference of nearly equal sums (what rho_err allows for), so the margins agree to a few digits, not to rounding
    assert worst["margin"] <= 1e-2
    if setname == "hard":
        assert rejected >= 1


# ---------------------------------------------------------------- 2. g is half the gradient of F
@pytest.mark.parametrize("fs", [1, 2, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_gradient_by_central_differences(kind, fs):
    """at the oracle's end point (where g is small) and at the start point (where it is not), on problems with planted
    outliers.  h = 1e-6: the truncation error h^2 F''' / 6 and the rounding error eps F / h are both below 1e-9 (1 + F) here,
    the tolerance is two decades above that"""
    N, M, nb = 6, 40, 4
    prm = tb.params("default")
    noise = tb.SETS["default"][1]
    off, _ = planted_offsets(nb, M, fs, 0.1, 50 * noise, seed=3)
    loss = ro.Loss(KINDS[kind], 2.0 * noise * np.sqrt(fs), fs)
    h = 1e-6
    worst = 0.0
    for b in range(nb):
        hp = host(N, M, 1 + b, "default", off[b])
        r = ro.solve_one(hp, prm, loss)
        for p in (r["p"], hp.p0()):
            x, J = hp.eval(p)
            F, g, H, w, s = ro.products(x, J, loss)
            fd = np.zeros(N)
            for i in range(N):
                e = np.zeros(N)
                e[i] = h
                fd[i] = (loss.cost(hp.eval(p + e)[0]) - loss.cost(hp.eval(p - e)[0])) / (2 * h)
            err = float(np.max(np.abs(fd - 2.0 * g)))
            worst = max(worst, err / (1.0 + F))
            assert err <= 1e-7 * (1.0 + F), (kind, fs, b, err, F)
        hp.close()
    print(f"{kind} fs {fs}: worst |fd - 2 g| / (1 + F) {worst:.3g}")


# ---------------------------------------------------------------- 3. the point of the feature
OUTLIER_SEED = 11               # (of the generator that plants the outliers; chosen here, on the oracle alone)


def test_planted_outliers_lose_their_pull():
    """10 % of the features displaced by 50 x the noise: the Cauchy and the Huber solutions lie closer to p* than the least-
    squares solution, in the median over 64 problems; the planted features are those with the smallest weights"""
    N, M, nb, fs = 6, 40, 64, 1
    prm = tb.params("default")
    eps, noise, spread, _ = tb.SETS["default"]
    off, planted = planted_offsets(nb, M, fs, 0.1, 50 * noise, seed=OUTLIER_SEED)
    dist = {k: [] for k in ("trivial", "huber", "cauchy")}
    named = 0
    for b in range(nb):
        hp = host(N, M, 1 + b, "default", off[b])
        pstar = np.zeros(N)
        hp.hp.dp.lib.synth_pstar(hp.hp.dp.h, dptr(pstar))
        for k in dist:
            r = ro.solve_one(hp, prm, ro.Loss(KINDS[k], 2.0 * noise, fs))
            assert r["status"] in (d.BATCH_JTX, d.BATCH_SMALL_STEP)
            dist[k].append(float(np.linalg.norm(r["p"] - pstar)))
            if k == "cauchy":
                named += set(np.argsort(r["weights"])[:planted[b].sum()]) == set(np.flatnonzero(planted[b]))
        hp.close()
    med = {k: float(np.median(v)) for k, v in dist.items()}
    print(f"median |p - p*|: {med}; problems whose {planted[0].sum()} smallest Cauchy weights are the planted features: {named}")
    assert med["cauchy"] < med["trivial"] and med["huber"] < med["trivial"]
    assert named == nb


# ---------------------------------------------------------------- 4. the library without a device
def test_symbols_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n
        assert hasattr(capi.lib(), n)


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_robust_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_robust_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [int(v) for v in lines[0].split()] == [C.sizeof(BatchLoss), BatchLoss.kind.offset, BatchLoss.scale.offset,
                                                  BatchLoss.featureSize.offset] == [24, 0, 8, 16]
    assert lines[1].split() == ["-1", "1", "2", "-3", "-3"]
    assert (d.LOSS_TRIVIAL, d.LOSS_HUBER, d.LOSS_SOFT_L1, d.LOSS_CAUCHY, d.BATCH_LOSS_MAX_FEATURESIZE) == (0, 1, 2, 3, 4)


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
    good = BatchLoss(LOSS_HUBER, 0.5, 2)

    def host_call(pp=p, b=B, n=N, m=M, fn=f, loss=good, r=res):
        return L.dogleg_amd_optimize_dense_batch_robust(None if pp is None else dptr(pp), b, n, m, fn, None, None,
                                                        None if loss is None else C.byref(loss), r, dptr(w))

    def dev_call(pp=p, b=B, n=N, m=M, fn=f, loss=good, r=res):
        return L.dogleg_amd_optimize_dense_batch_robust_device(None if pp is None else pp.ctypes.data, b, n, m, fn, None, None,
                                                               None if loss is None else C.byref(loss),
                                                               None if r is None else C.addressof(r), lam.ctypes.data,
                                                               w.ctypes.data, None, None)

    big = np.ones((1, BATCH_MAX_NSTATE + 1))
    for call in (host_call, dev_call):
        # what the plain twin refuses
        assert call(b=0) == -1 and call(n=0) == -1 and call(m=0) == -1
        assert call(fn=None) == -1 and call(pp=None) == -1 and call(r=None) == -1
        assert call(pp=big, b=1, n=BATCH_MAX_NSTATE + 1) == -1
        # the loss
        assert call(loss=None) == -1
        assert call(loss=BatchLoss(4, 0.5, 1)) == -1 and call(loss=BatchLoss(-1, 0.5, 1)) == -1
        for kind in (LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY):
            for scale in (0.0, -1.0, np.inf, np.nan):
                assert call(loss=BatchLoss(kind, scale, 1)) == -1, (kind, scale)
        assert call(loss=BatchLoss(LOSS_CAUCHY, 0.5, 5)) == -1
        assert call(loss=BatchLoss(LOSS_CAUCHY, 0.5, 3), m=13) == -1 and call(loss=BatchLoss(LOSS_TRIVIAL, 0.0, 4), m=14) == -1
        fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
        assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
        try:
            assert call() == -1                                  # a communicator is set: one rank only
        finally:
            L.dogleg_amd_clear_communicator()
    assert np.all(big == 1.0)
    assert np.array_equal(p, p0) and not calls and bytes(res) == res0 and np.all(w == -7.5) and np.all(lam == -7.5)


def test_valid_call_without_a_device_fails_cleanly():
    L = capi.lib()
    if L.dlg_device_count() > 0:
        return                                                   # (with a GPU: tests/test_dense_batch_robust_gpu.py)
    cb = CB_DEVICE_BATCH(lambda *a: None)
    p0 = np.arange(1.0, 13.0).reshape(4, 3)
    # (TRIVIAL ignores its scale; featureSize 0 means 1)
    rc, p, res, w = capi.optimize_dense_batch_robust(p0, 3, 12, C.cast(cb, C.c_void_p), None, BatchLoss(LOSS_TRIVIAL, 0.0, 0))
    assert rc == -1 and np.array_equal(p, p0) and np.all(w == -1.0)
    L.dogleg_amd_release_cache()
