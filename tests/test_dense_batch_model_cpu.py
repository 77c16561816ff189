"""The built-in fit models of the batch solver without a GPU: include/dogleg_batch_models.h compiled for the host against the
NumPy restatement of tests/batch_models_np.py; the restatement's J against its own central differences; the exports and the
header as C; the refusals of the fused solve, each of which returns -1 with its message before any device work and writes
nothing; and the case tables the GPU tests compare against: what they must contain is asserted here, so that no GPU comparison
is vacuous.

Tolerances.  The host header and NumPy evaluate the same formulas in double precision in their own order (z = (t - mu) / sigma
against (t - mu)^2 / (2 sigma^2), libm's exp against NumPy's).  An entry of J is a product of a few factors and e = exp(u): each
rounding adds eps relative to the entry, and the 2 to 3 roundings of u are amplified by |u|, where |u|^k e^u <= 1 for the powers
that occur, so the error stays below about 10 eps of the column's largest magnitude.  x = s (f - y) cancels: f carries about 6 eps
of |A| + |c|, which is the size of the data, not of x.  So asserted (HOST_TOL) are 64 eps relative to the largest |s y| of the
problem for x, and 64 eps relative to the largest magnitude in that column for J; the figure measured is printed.  Central
differences with h = 1e-6 (1 + |p_j|) carry an error of about h^2 |f'''| + eps |f| / h ~ 1e-9 on these O(1 .. 10) models: 1e-6
relative to the column's largest magnitude is asserted (FD_TOL)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BatchBounds, BatchModel, BatchResult, BATCH_JTX, BATCH_SMALL_STEP, MODEL_EXPDECAY,
                                       MODEL_GAUSS1D, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC, MODEL_NSTATE, dptr)
from tests import batch_models_np as mz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_batch_model", "dogleg_amd_optimize_dense_batch_model_device")
HOST_TOL = 64 * np.finfo(float).eps
FD_TOL = 1e-6
VARIANTS = [(None, False), (None, True), ("shared", False), ("each", True)]


def scaled_error(got, want, axis):
    """max |got - want| relative to the largest |want| along `axis` (of the whole array where that is 0)"""
    ref = np.max(np.abs(want), axis=axis, keepdims=True)
    ref = np.where(ref > 0.0, ref, 1.0)
    return float(np.max(np.abs(got - want) / ref))


# ---------------------------------------------------------------- 1. the header on the host
@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("batch_model_rows") / "libbatch_model_rows.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "batch_model_rows.c"), "-o", so, "-lm"],
                   check=True)
    L = C.CDLL(so)
    D = C.POINTER(C.c_double)
    L.model_rows.argtypes = [C.c_int, D, C.c_int, C.c_int, D, D, D, D, D]
    L.model_rows.restype = None
    return L


def header_eval(L, kind, p, y, t, scale, width):
    M, N = len(y), MODEL_NSTATE[kind]
    x, J = np.full(M, np.nan), np.full((M, N), np.nan)
    p = np.ascontiguousarray(p, dtype=np.float64)
    opt = lambda a: None if a is None else dptr(np.ascontiguousarray(a, dtype=np.float64))
    L.model_rows(kind, dptr(p), M, width, opt(t), dptr(np.ascontiguousarray(y)), opt(scale), dptr(x), dptr(J))
    return x, J


@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_host_header_against_numpy(host_rows, case):
    kind, _ = case
    assert host_rows.model_nstate(kind) == MODEL_NSTATE[kind] and host_rows.model_nstate(4) == -1
    worst = 0.0
    for t_mode, with_scale in VARIANTS:
        if t_mode is not None and mz.is_2d(kind):
            continue
        bt = mz.batch(case, nb=5, t_mode=t_mode, with_scale=with_scale)
        for b in range(5):
            hp = mz.host_model(bt, b)
            for p in (bt["p0"][b], bt["truth"][b]):
                x, J = header_eval(host_rows, kind, p, hp.y, hp.t, hp.scale, hp.width)
                xn, Jn = hp.eval(p)
                sy = hp.y if hp.scale is None else hp.scale * hp.y
                worst = max(worst, float(np.max(np.abs(x - xn))) / float(np.max(np.abs(sy))), scaled_error(J, Jn, 0))
    print(f"{mz.case_id(case)}: largest scaled deviation of the host header from NumPy {worst:.3g} (asserted {HOST_TOL:.3g})")
    assert worst <= HOST_TOL


@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_numpy_jacobian_against_central_differences(case):
    kind, _ = case
    worst = 0.0
    for t_mode, with_scale in VARIANTS:
        if t_mode is not None and mz.is_2d(kind):
            continue
        bt = mz.batch(case, nb=3, t_mode=t_mode, with_scale=with_scale)
        for b in range(3):
            hp = mz.host_model(bt, b)
            p = bt["p0"][b]
            _, J = hp.eval(p)
            fd = np.zeros_like(J)
            for j in range(hp.N):
                h = 1e-6 * (1.0 + abs(p[j]))
                pp, pm = p.copy(), p.copy()
                pp[j] += h
                pm[j] -= h
                fd[:, j] = (hp.eval(pp)[0] - hp.eval(pm)[0]) / (pp[j] - pm[j])
            worst = max(worst, scaled_error(J, fd, 0))
    print(f"{mz.case_id(case)}: largest scaled deviation of J from central differences {worst:.3g}")
    assert worst <= FD_TOL


def test_non_finite_rows(host_rows):
    """a sigma of exactly 0 and a NaN datum give non-finite rows in the header, as dogleg.h says"""
    y = np.linspace(1.0, 2.0, 9)
    for kind, p, width in ((MODEL_GAUSS1D, [5.0, 4.0, 0.0, 1.0], 0), (MODEL_GAUSS2D, [5.0, 1.0, 1.0, 0.0, 1.0], 3),
                           (MODEL_GAUSS2D_ELLIPTIC, [5.0, 1.0, 1.0, 1.0, 0.0, 1.0], 3)):
        x, J = header_eval(host_rows, kind, p, y, None, None, width)
        assert not np.all(np.isfinite(J)), kind
    yn = y.copy()
    yn[4] = np.nan
    x, J = header_eval(host_rows, MODEL_EXPDECAY, [5.0, 0.3, 1.0], yn, None, None, 0)
    assert np.isnan(x[4]) and np.all(np.isfinite(np.delete(x, 4)))


# ---------------------------------------------------------------- 2. the library without a device
def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "dogleg.h")) as f:
        header = f.read()
    for n in NAMES + ("dogleg_amd_batch_model_callback", "dogleg_amd_batch_model_nstate",
                      "dogleg_amd_batch_model_callback_invocations"):
        assert n in exported and n in capi.DOGLEG_SYMBOLS and hasattr(capi.lib(), n) and n + "(" in header, n
    L = capi.lib()
    assert [L.dogleg_amd_batch_model_nstate(k) for k in (0, 1, 2, 3, 4, -1)] == [3, 4, 5, 6, -1, -1]


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_model_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_model_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1", "-1", "1", "5", "-3", "3", "4", "5", "6", "-1", "0"]
    for n in NAMES:
        assert n + ": model must be given" in r.stderr, r.stderr
    assert "a window of model->width x model->height = 2 x 3 pixels, and model->Nmeas = 4" in r.stderr


def test_ctypes_record_matches_the_header():
    assert C.sizeof(BatchModel) == 48
    assert [getattr(BatchModel, f).offset for f, _ in BatchModel._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]


def test_refusals_that_need_no_device(capfd):
    """both entry points; the record's arrays and the device twin's arrays are host memory here: a call that got past the checks
    under test would be refused by the pointer checks that follow them, never launched.  Every refusal is told by its message"""
    L = capi.lib()
    B, M = 4, 12
    y, t = np.ones((B, M)), np.arange(float(M))
    before = capi.batch_model_callback_invocations()

    def model(kind=MODEL_EXPDECAY, nmeas=M, width=0, height=0, yy=y, tt=None):
        return BatchModel(kind, nmeas, width, height, None if yy is None else yy.ctypes.data, None if tt is None else tt.ctypes.data,
                          None, 0)

    p0 = np.arange(1.0, 1.0 + B * 6).reshape(B, 6)
    p = p0.copy()
    res = (BatchResult * B)()
    C.memset(res, 0xA5, C.sizeof(res))
    res0 = bytes(res)
    lam = np.full(B, -7.5)
    lo, hi, held = np.zeros((B, 6)), np.ones((B, 6)), np.full((B, 6), 9, dtype=np.uint8)
    bounds = BatchBounds(lo.ctypes.data, hi.ctypes.data, held.ctypes.data)

    def host_call(m, pp=p, b=B, r=res, bd=None):
        return L.dogleg_amd_optimize_dense_batch_model(None if pp is None else dptr(pp), b, None if m is None else C.byref(m), None,
                                                       None if bd is None else C.byref(bd), r)

    def dev_call(m, pp=p, b=B, r=res, bd=None):
        return L.dogleg_amd_optimize_dense_batch_model_device(None if pp is None else pp.ctypes.data, b,
                                                              None if m is None else C.byref(m), None,
                                                              None if bd is None else C.byref(bd),
                                                              None if r is None else C.addressof(r), lam.ctypes.data, None, None)

    refusals = [
        (dict(m=None), "model must be given"),
        (dict(m=model(yy=None)), "model->y must be given"),
        (dict(m=model(kind=4)), "model->kind = 4 is none of"),
        (dict(m=model(kind=-1)), "model->kind = -1 is none of"),
        (dict(m=model(nmeas=0)), "model->Nmeas = 0"),
        (dict(m=model(kind=MODEL_GAUSS2D, width=3, height=5)), "3 x 5 pixels, and model->Nmeas = 12"),
        (dict(m=model(kind=MODEL_GAUSS2D_ELLIPTIC, width=0, height=0)), "0 x 0 pixels, and model->Nmeas = 12"),
        (dict(m=model(kind=MODEL_GAUSS2D, width=3, height=4, tt=t)), "model->t must be NULL for the 2D kinds"),
        (dict(m=model(kind=MODEL_GAUSS1D, width=3, height=4)), "both are 0 for the 1D kinds"),
        # what the plain and the bounded twin refuse
        (dict(m=model(), b=0), "none may be 0"),
        (dict(m=model(), pp=None), "must be given"),
        (dict(m=model(), r=None), "must be given"),
    ]
    for call in (host_call, dev_call):
        for kw, msg in refusals:
            capfd.readouterr()
            assert call(**kw) == -1, (call.__name__, msg)
            err = capfd.readouterr().err
            assert msg in err and NAMES[call is dev_call] + ":" in err, (call.__name__, msg, err)
        for bd in (None, bounds):
            fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
            assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
            try:
                capfd.readouterr()
                assert call(model(), bd=bd) == -1
                assert "rank" in capfd.readouterr().err
            finally:
                L.dogleg_amd_clear_communicator()
    # the record's arrays are checked as the _device twins check theirs: host memory is refused by name, on either route
    if L.dlg_device_count() == 0:
        for call in (host_call, dev_call):
            capfd.readouterr()
            assert call(model(), bd=bounds) == -1
    assert np.array_equal(p, p0) and bytes(res) == res0 and np.all(lam == -7.5)
    assert np.all(held == 9) and not lo.any() and np.all(hi == 1.0)
    assert capi.batch_model_callback_invocations() == before


# ---------------------------------------------------------------- 3. the case tables
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_case_tables(case):
    plain, bounded = mz.oracle_table(case, False), mz.oracle_table(case, True)
    assert len(plain) == len(bounded) == mz.B
    for what, orc in (("plain", plain), ("bounded", bounded)):
        assert all(o["status"] in (BATCH_JTX, BATCH_SMALL_STEP) for o in orc), what
    m = min(o["margin"] for o in plain + bounded)
    nheld, nclipped = sum(bool(o["held"].any()) for o in bounded), sum(o["clipped"] for o in bounded)
    print(f"{mz.case_id(case)}: smallest decision margin {m:.3g} (recorded {mz.MARGINS[case]:.3g}), {nheld} of {mz.B} bounded "
          f"problems end with a held variable, {nclipped} clipped steps, evaluations "
          f"{sorted({o['evaluations'] for o in plain + bounded})}")
    assert m > mz.MARGIN_FLOOR
    assert abs(m - mz.MARGINS[case]) <= 0.05 * mz.MARGINS[case], "the generator or the oracle changed: choose the seeds again"
    assert 4 * nheld >= mz.B and nclipped >= 1
    assert not any(o["held"].any() for o in plain)
    assert len({o["evaluations"] for o in plain + bounded}) > 1
    # the bounded optimum differs from the plain one where a variable is held: the bounds do something
    assert any(np.max(np.abs(a["p"] - b["p"])) > 1e-3 for a, b in zip(plain, bounded))
