"""dogleg_amd_optimize_device2_bounded without a GPU: the symbol as a C user compiles against it, every refusal (all are made on
the host, before any device work), the cases of tests/test_device_bounds_gpu.py against the floor on the oracle's decision
margins (tests/device_bounds_cases.py), and the bounded oracle with infinite bounds against the robust oracle on these problems."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_TRIVIAL, LOSS_HUBER, LOSS_CAUCHY
from problems.device_robust import OffsetHostModel
from tests import batch_bounds_oracle as bb
from tests import batch_robust_oracle as ro
from tests import device_bounds_cases as bc
from tests import device_robust_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dogleg_amd_optimize_device2_bounded"


def test_symbol_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    for n in (NAME, "dogleg_amd_bounded_last_stats"):
        assert n in exported and n in capi.DOGLEG_SYMBOLS and re.search(r"\b%s\(" % n, header), n
    backend = open(os.path.join(ROOT, "include", "dlg_backend.h")).read()
    assert "dlg_point_bind_held" in exported and "dlg_point_bind_held" in capi.BACKEND_SYMBOLS and "dlg_point_bind_held(" in backend
    assert capi.lib().dogleg_amd_optimize_device2_bounded.restype is C.c_double
    assert len(capi.lib().dogleg_amd_optimize_device2_bounded.argtypes) == 13
    # the header says what a returned context holds
    block = header[header.index("box bounds in dogleg_optimize_device2"):header.index(NAME + "(")]
    for phrase in ("A returned context holds the MASKED point", "Jt_x is g_F", "exact zeros in the held columns",
                   "the matrix of step 4", "1.0 on the diagonal, 0 elsewhere", "Not provided"):
        assert phrase in block, phrase


def test_a_c_translation_unit_compiles_and_calls_it(tmp_path):
    exe = str(tmp_path / "device_bounds_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "device_bounds_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1", "-1", "-1", "1", "6"], r.stdout + r.stderr


CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def test_every_refusal_returns_minus_one_and_writes_nothing(monkeypatch):
    """no GPU is touched: the callback is never invoked, p, weights and held keep their bits"""
    N, M, fs = 6, 12, 2
    Jp = np.arange(0, 2 * (M + 1), 2, dtype=np.int32)
    Ji = np.tile(np.array([0, 3], dtype=np.int32), M)
    nnz = int(Jp[-1])
    ncalls = []
    cb = CALLBACK(lambda *a: ncalls.append(1))
    cbp = C.cast(cb, C.c_void_p)
    p0 = np.linspace(-1.0, 2.0, N)
    lo0, hi0 = p0 - 1.0, p0 + 1.0
    good = BatchLoss(LOSS_CAUCHY, 0.5, fs)
    L = capi.lib()

    def call(loss=None, n=N, m=M, z=nnz, jp=Jp, ji=Ji, f=cbp, lo=lo0, hi=hi0, **kw):
        r, p, tr, w, held = capi.optimize_device_bounded(p0, n, m, z, jp, ji, f, None, lo, hi, loss, dc.params(), trace=False, **kw)
        assert p.tobytes() == p0.tobytes() and np.all(held == 255) and (w is None or np.all(w == -1.0))
        return r

    # the bounds
    assert call(null_bounds=True) == -1.0 and call(loss=good, null_bounds=True) == -1.0
    assert call(want_weights=True) == -1.0                                                           # weights without a loss
    for k in (0, N - 1):
        bad = lo0.copy()
        bad[k] = np.nan
        assert call(lo=bad) == -1.0 and call(hi=bad) == -1.0 and call(lo=bad, hi=None) == -1.0       # a NaN bound
        above = lo0.copy()
        above[k] = hi0[k] + 1e-3
        assert call(lo=above) == -1.0                                                                # lower > upper
    assert call(lo=np.full(N, np.inf), hi=np.full(N, -np.inf)) == -1.0
    # with a loss: what _robust refuses
    for kind in (-1, 4, 17):
        assert call(loss=BatchLoss(kind, 0.5, fs)) == -1.0, kind
    for kind in (LOSS_HUBER, LOSS_CAUCHY):
        for scale in (0.0, -2.0, np.inf, np.nan):
            assert call(loss=BatchLoss(kind, scale, fs)) == -1.0, (kind, scale)
    assert call(loss=BatchLoss(LOSS_TRIVIAL, 0.5, 5)) == -1.0                                        # featureSize > 4
    assert call(loss=BatchLoss(LOSS_HUBER, 0.5, 4), m=M - 2, z=int(Jp[M - 2])) == -1.0               # 10 rows, features of 4
    down = Jp.copy()
    down[3] = down[2] - 1
    assert call(loss=good, jp=down) == -1.0                                                          # a colptr that decreases
    # what dogleg_optimize_device2 refuses: no callback, a sparse solve without its pattern, a pattern that disagrees with NJnnz
    assert call(f=None) == -1.0
    bounds = capi.BatchBounds(lo0.ctypes.data, hi0.ctypes.data, None)
    assert L.dogleg_amd_optimize_device2_bounded(capi.dptr(p0.copy()), N, M, nnz, None, None, cbp, None, None, None, C.byref(bounds),
                                                 None, None) == -1.0
    assert call(z=nnz - 1) == -1.0
    assert L.dogleg_amd_optimize_device2_bounded(None, N, M, nnz, capi.iptr(Jp), capi.iptr(Ji), cbp, None, None, None, C.byref(bounds),
                                                 None, None) == -1.0                                 # a NULL p
    # more than one rank, all three ways
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call() == -1.0 and call(z=0) == -1.0 and call(loss=good) == -1.0
    finally:
        L.dogleg_amd_clear_communicator()
    ident = (C.c_ubyte * 128)()
    assert L.dogleg_amd_set_communicator(1, 2, -1, C.cast(ident, C.c_void_p)) == 0
    try:
        assert call() == -1.0
    finally:
        L.dogleg_amd_clear_communicator()
    monkeypatch.setenv("DOGLEG_AMD_WORLD_SIZE", "2")
    assert call() == -1.0 and call(z=0) == -1.0
    monkeypatch.delenv("DOGLEG_AMD_WORLD_SIZE")
    assert not ncalls


@pytest.mark.parametrize("name", sorted(bc.MARGINS), ids=str)
def test_the_cases_keep_the_oracle_off_the_rounding_edges(name):
    o = bc.assert_margin(name)
    rec = bc.RECORDED[name]
    assert o["status"] > 0 and o["norm2_x"] >= 0
    assert (int(np.count_nonzero(o["held"])), o["clipped"], o["fallbacks"], o["held_resteps"]) == \
           (rec["held"], rec["clipped"], rec["fallbacks"], rec["held_resteps"])
    lo, hi = bc.oracle(name)[1:3]
    assert np.all((o["p"] >= lo) & (o["p"] <= hi)) and np.all(o["p"][o["held"] == 1] == lo[o["held"] == 1]) and \
        np.all(o["p"][o["held"] == 2] == hi[o["held"] == 2])


def test_the_cases_are_the_ones_asked_for():
    assert set(bc.MARGINS) == set(bc.CASES) == set(bc.RECORDED)
    assert set(bc.SPARSE) == {"ba_small", "ba_small_huber", "ba_medium3", "branch1", "branch2", "branch4"}
    assert set(bc.DENSE) == {"dense_small", "dense_medium"}
    # every branch: fallbacks, rejected trials stepped again with held variables, all three kinds of step
    for name in ("branch2", "branch4"):
        o = bc.oracle(name)[0]
        assert o["fallbacks"] > 0 and o["held_resteps"] > 0 and o["step_types"] == {0, 1, 2}, name
    assert bc.oracle("branch1")[0]["fallbacks"] > 0 and bc.oracle("branch1")[0]["held_resteps"] > 0
    # the mild cases end on their bounds: a third of the variables is bounded, most of those are held
    for name in ("ba_small", "ba_medium3", "dense_medium"):
        o, lo, hi, free = bc.oracle(name)
        bounded = np.isfinite(lo) | np.isfinite(hi)
        assert bounded.sum() == (len(lo) + 2) // 3 and np.count_nonzero(o["held"]) >= 0.8 * bounded.sum()
        assert not np.all((free["p"] >= lo) & (free["p"] <= hi))          # (the unbounded optimum is outside the box)
    a, b = bc.problem("parked_a"), bc.problem("parked_b")
    assert (a.N, a.M, a.nnz) == (b.N, b.M, b.nnz) and not np.array_equal(a.pattern()[1], b.pattern()[1])
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["ba_small", "ba_small_huber", "dense_small", "dense_medium", "branch2"], ids=str)
def test_infinite_bounds_are_the_robust_oracle(name):
    """the bounded oracle with bounds that clamp nothing (none, infinite entries, a box that is never met) returns what
    batch_robust_oracle.solve_one returns on these problems, bit for bit"""
    prob = bc.problem(name)
    hm = OffsetHostModel(prob, bc.offsets(name))
    loss = bc.loss_pair(name)[0]
    want = ro.solve_one(hm, bc.params(name), loss)
    N = prob.N
    far = 1e6 * (1.0 + np.abs(hm.p0()))
    for lo, hi in ((None, None), (np.full(N, -np.inf), np.full(N, np.inf)), (hm.p0() - far, hm.p0() + far)):
        got = bb.solve_one(hm, bc.params(name), loss, lo, hi)
        assert got["p"].tobytes() == want["p"].tobytes() and got["norm2_x"] == want["norm2_x"]
        assert (got["iterations"], got["evaluations"], got["status"], got["lambda_"]) == \
               (want["iterations"], want["evaluations"], want["status"], want["lambda_"])
        assert got["weights"].tobytes() == want["weights"].tobytes()
        assert not got["held"].any() and got["clipped"] == got["fallbacks"] == got["held_steps"] == 0
    prob.close()
