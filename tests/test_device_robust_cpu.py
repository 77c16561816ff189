"""dogleg_amd_optimize_device2_robust without a GPU: the symbol as a C user compiles against it, every refusal (all are made on
the host, before any device work), and the seeds of tests/test_device_robust_gpu.py against the floor on the oracle's decision
margins (tests/device_robust_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY
from tests import device_robust_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dogleg_amd_optimize_device2_robust"


def test_symbol_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    for n in (NAME, "dogleg_amd_robust_last_stats"):
        assert n in exported and n in capi.DOGLEG_SYMBOLS and re.search(r"\b%s\(" % n, header), n
    assert capi.lib().dogleg_amd_optimize_device2_robust.restype is C.c_double
    assert len(capi.lib().dogleg_amd_optimize_device2_robust.argtypes) == 12
    # the header says what a returned context holds
    block = header[header.index("robust loss functions in dogleg_optimize_device2"):header.index(NAME + "(")]
    for phrase in ("beforeStep->norm2_x is F", "times sqrt(w_f)", "H + lambda I", "reweighted problem", "Not provided"):
        assert phrase in block, phrase


def test_a_c_translation_unit_compiles_and_calls_it(tmp_path):
    exe = str(tmp_path / "device_robust_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-DDEVICE_ROBUST_ABI_MAIN", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "device_robust_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1", "-1", "1"], r.stdout + r.stderr


CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def test_every_refusal_returns_minus_one_and_writes_nothing(monkeypatch):
    """no GPU is touched: the callback is never invoked, p and weights keep their bits"""
    N, M, fs = 6, 12, 2
    Jp = np.arange(0, 2 * (M + 1), 2, dtype=np.int32)
    Ji = np.tile(np.array([0, 3], dtype=np.int32), M)
    nnz = int(Jp[-1])
    ncalls = []
    cb = CALLBACK(lambda *a: ncalls.append(1))
    cbp = C.cast(cb, C.c_void_p)
    p0 = np.linspace(-1.0, 2.0, N)
    good = BatchLoss(LOSS_CAUCHY, 0.5, fs)
    L = capi.lib()

    def call(loss=good, n=N, m=M, z=nnz, jp=Jp, ji=Ji, f=cbp):
        r, p, tr, w = capi.optimize_device_robust(p0, n, m, z, jp, ji, f, None, loss, dc.params(), trace=False)
        assert p.tobytes() == p0.tobytes() and np.all(w == -1.0)
        return r

    # the loss
    assert call(loss=None) == -1.0
    for kind in (-1, 4, 17):
        assert call(loss=BatchLoss(kind, 0.5, fs)) == -1.0, kind
    for kind in (LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY):
        for scale in (0.0, -2.0, np.inf, -np.inf, np.nan):
            assert call(loss=BatchLoss(kind, scale, fs)) == -1.0, (kind, scale)
    assert call(loss=BatchLoss(LOSS_TRIVIAL, 0.5, 5)) == -1.0 and call(loss=BatchLoss(LOSS_HUBER, 0.5, 5)) == -1.0      # featureSize > 4
    assert call(loss=BatchLoss(LOSS_HUBER, 0.5, 4), m=M - 2, z=int(Jp[M - 2])) == -1.0          # 10 rows, features of 4
    assert call(loss=BatchLoss(LOSS_HUBER, 0.5, 3), z=0, m=M - 2) == -1.0                            # dense, 10 rows, features of 3
    # what dogleg_optimize_device2 refuses: no callback, a sparse solve without its pattern, a pattern that disagrees with NJnnz
    assert call(f=None) == -1.0
    assert L.dogleg_amd_optimize_device2_robust(capi.dptr(p0.copy()), N, M, nnz, None, None, cbp, None, C.byref(good), None, None,
                                                None) == -1.0
    assert call(z=nnz - 1) == -1.0
    down = Jp.copy()
    down[3] = down[2] - 1
    assert call(jp=down) == -1.0                                                                     # a colptr that decreases
    # more than one rank, all three ways
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call() == -1.0 and call(z=0) == -1.0
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


@pytest.mark.parametrize("case", sorted(dc.MARGINS), ids=str)
def test_the_seeds_keep_the_oracle_off_the_rounding_edges(case):
    o = dc.assert_margin(case)
    assert o["status"] > 0 and o["norm2_x"] >= 0 and np.all((o["weights"] > 0) & (o["weights"] <= 1))


def test_the_cases_are_the_ones_asked_for():
    names = {c[0] for c in dc.MARGINS}
    assert names == set(dc.PROBLEMS)
    for name in ("ba_small", "ba_medium", "dense_small", "dense_medium"):
        assert {k for n, fs, k in dc.MARGINS if n == name and fs == 2} == set(dc.KINDS), name
    assert {fs for n, fs, k in dc.MARGINS if n == "ba_small"} == {1, 2, 3, 4}
    a, b = dc.problem("parked_a"), dc.problem("parked_b")
    assert (a.N, a.M, a.nnz) == (b.N, b.M, b.nnz) and not np.array_equal(a.pattern()[1], b.pattern()[1])
    small, medium = dc.problem("ba_small"), dc.problem("ba_medium")
    assert (small.N, small.M, small.nnz) == (96, 120, 1800) and (medium.N, medium.M, medium.nnz) == (438, 1440, 21600)
    # under Cauchy the planted features end with the smallest weights (the GPU test asks the library for the same)
    for name in ("ba_small", "ba_medium"):
        o, planted = dc.oracle(name, 2, "cauchy"), dc.offsets(name, 2)[1]
        assert planted.sum() == round(dc.FRACTION * len(planted)) and o["weights"][planted].max() < o["weights"][~planted].min()
    for p in (a, b, small, medium):
        p.close()
