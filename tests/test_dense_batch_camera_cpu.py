"""Raw camera frames in the fused calls of the built-in models, without a device (the GPU part: test_dense_batch_camera_gpu.py).

1. The header's arithmetic on the host (tests/c/batch_camera_rows.c): dogleg_batch_camera_datum against NumPy float64 arithmetic, bit
   for bit, for the three dtypes (uint16 0 and 65535 among them); dogleg_batch_model_row_poisson_v with v = 0 against
   dogleg_batch_model_row_poisson, bit for bit, over every kind, rows with y = 0, y = NaN and an infeasible f among them; with
   v > 0 against a NumPy restatement of the definition (ROWS_TOL of the Poisson GPU test, 1e-13, scaled as there); the clamp:
   y + v < 0 gives d = 2 f', and a NaN stays NaN.
2. The layout of dogleg_amd_batch_camera_t in C against the ctypes definition.
4. The oracle of the read-noise fit (tests/batch_camera_oracle.py): with v = 0 and data >= 0 it reproduces batch_poisson_oracle
   exactly; every problem of its tables lies above MARGIN_FLOOR and below COST_TOL and ends in JTX or SMALL_STEP; the recorded
   seeds and margins are what the tables give; the low tables hold readings under their offset and pixels the clamp acts on.
3. Every refusal of the camera entry points returns -1 with a message and leaves the outputs untouched; every solve entry point
   refuses dogleg_amd_batch_camera_fisher_callback."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BatchBounds, BatchCamera, BatchLoss, BatchModel, BatchResult, LOSS_TRIVIAL, MODEL_EXPDECAY,
                                       MODEL_GAUSS1D, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC, MODEL_NSTATE, LIKELIHOOD_GAUSS,
                                       LIKELIHOOD_POISSON, DATA_F64, DATA_F32, DATA_U16, DATA_NUMPY, BATCH_JTX, BATCH_SMALL_STEP)
from tests import batch_camera_oracle as co
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests.test_dense_batch_poisson_cpu import scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_TOL = 1e-13           # = ROWS_TOL of tests/test_dense_batch_poisson_gpu.py (importing that module needs nothing of a GPU, but
                           # it is a GPU test file: the figure is restated)
dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
NAMES = ("dogleg_amd_optimize_dense_batch_camera", "dogleg_amd_optimize_dense_batch_camera_device",
         "dogleg_amd_dense_batch_camera_uncertainty", "dogleg_amd_dense_batch_camera_uncertainty_device",
         "dogleg_amd_dense_batch_camera_query_covariance", "dogleg_amd_dense_batch_camera_query_covariance_device",
         "dogleg_amd_batch_camera_callback", "dogleg_amd_batch_camera_fisher_callback")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("batch_camera_rows") / "libbatch_camera_rows.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "batch_camera_rows.c"), "-o", so, "-lm"], check=True)
    L = C.CDLL(so)
    D, V = C.POINTER(C.c_double), C.c_void_p
    L.camera_data.argtypes = [C.c_int, V, C.c_int, V, V, V, D, D]
    L.camera_data.restype = None
    L.camera_rows_poisson.argtypes = [C.c_int, C.c_int, D, C.c_int, C.c_int, D, D, D, D, D, D, C.POINTER(C.c_int)]
    L.camera_rows_poisson.restype = None
    L.camera_layout.argtypes = [C.POINTER(C.c_size_t)]
    return L


def rows(L, with_v, kind, p, y, v, width):
    M, N = len(y), MODEL_NSTATE[kind]
    x, J, d, ok = np.full(M, 7.0), np.full((M, N), 7.0), np.full(M, 7.0), np.full(M, -1, dtype=np.int32)
    p, y, v = (np.ascontiguousarray(a, dtype=np.float64) for a in (p, y, v))
    L.camera_rows_poisson(with_v, kind, dptr(p), M, width, None, dptr(y), dptr(v), dptr(x), dptr(J), dptr(d),
                          ok.ctypes.data_as(C.POINTER(C.c_int)))
    return x, J, d, ok != 0


# ---------------------------------------------------------------- 1. the header on the host
@pytest.mark.parametrize("dtype", [DATA_F64, DATA_F32, DATA_U16], ids=["f64", "f32", "u16"])
def test_datum_against_numpy_bit_for_bit(host, dtype):
    rng = np.random.default_rng([5, dtype])
    n = 4096
    if dtype == DATA_U16:
        raw = rng.integers(0, 65536, size=n).astype(np.uint16)
        raw[:4] = [0, 65535, 1, 100]
    else:
        raw = (rng.uniform(-50.0, 4000.0, size=n)).astype(DATA_NUMPY[dtype])
        raw[:3] = [0.0, -0.0, 65535.0]
    off = (100.0 + 5.0 * rng.uniform(-1.0, 1.0, size=n)).astype(np.float32)
    gi = rng.uniform(0.4, 2.5, size=n).astype(np.float32)
    rv = rng.uniform(0.0, 4.0, size=n).astype(np.float32)
    y, v = np.full(n, 7.0), np.full(n, 7.0)
    host.camera_data(dtype, raw.ctypes.data, n, off.ctypes.data, gi.ctypes.data, rv.ctypes.data, dptr(y), dptr(v))
    want = (raw.astype(np.float64) - off.astype(np.float64)) * gi.astype(np.float64)
    assert y.tobytes() == want.tobytes() and v.tobytes() == rv.astype(np.float64).tobytes()
    # no calibration: offset 0, gain 1, readvar 0 leave the reading as it is (a -0.0 aside, which becomes +0.0)
    one, zero = np.ones(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    host.camera_data(dtype, raw.ctypes.data, n, zero.ctypes.data, one.ctypes.data, zero.ctypes.data, dptr(y), dptr(v))
    assert np.array_equal(y, raw.astype(np.float64)) and not v.any()


def special_rows(bt, b):
    """the problem's data with a zero and a NaN, and parameters that make the rows infeasible: the truth with an offset far under zero"""
    y = bt["y"][b].copy()
    y[1], y[2] = 0.0, np.nan
    p = bt["truth"][b].copy()
    p[-1] = -2.0 * abs(p[0]) - 1.0           # under minus the amplitude: no row is feasible
    return y, p


@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_v_zero_has_the_bits_of_the_poisson_row(host, case):
    kind = case[0]
    _, w, _ = mz.case_shape(case)
    for level in ("low", "high"):
        bt = po.batch((case, level), nb=3)
        for b in range(3):
            y, bad = special_rows(bt, b)
            for p in (bt["p0"][b], bt["truth"][b], bad):
                a = rows(host, 0, kind, p, y, np.zeros(len(y)), w)
                c = rows(host, 1, kind, p, y, np.zeros(len(y)), w)
                for u, t in zip(a, c):
                    assert u.tobytes() == t.tobytes(), (mz.case_id(case), level, b)
                if p is not bad:
                    # a feasible point: the NaN datum alone makes its row's x~ and d NaN, the zero count gives d = 2 f
                    assert c[3].all() and np.isnan(c[0][2]) and np.isnan(c[2][2]) and np.all(np.isfinite(c[1][2]))
                    rest = np.arange(len(y)) != 2
                    assert np.all(np.isfinite(c[0][rest])) and np.all(np.isfinite(c[2][rest]))
            assert not rows(host, 1, kind, bad, y, np.zeros(len(y)), w)[3].any(), "infeasible rows among them"
            assert (y == 0.0).sum() >= 1


def rows_v_np(kind, p, y, v, width):
    """the definition: f' = f + v, y' = max(y + v, 0); x~ = (f' - y') / sqrt(f'), J~ = grad f / sqrt(f'), d = 2 (f' - y' - y' log(f' / y'))"""
    f, G = mz.model_eval(kind, p, np.zeros(len(y)), None, None, width)
    fv, ys = f + v, y + v
    yv = np.where(ys < 0.0, 0.0, ys)
    with np.errstate(all="ignore"):
        ok = fv > 0.0
        q = np.where(ok, 1.0 / np.sqrt(fv), np.nan)
        d = np.where(yv == 0.0, 2.0 * fv, 2.0 * ((fv - yv) - yv * np.log(fv / np.where(yv == 0.0, 1.0, yv))))
    return (fv - yv) * q, G * q[:, None], np.where(ok, d, np.nan), ok


@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_v_positive_against_numpy(host, case):
    kind = case[0]
    _, w, _ = mz.case_shape(case)
    worst = 0.0
    for level in ("low", "high"):
        bt = po.batch((case, level), nb=4)
        for b in range(4):
            y = bt["y"][b] - 0.8 * (np.arange(len(bt["y"][b])) % 3 == 0)        # some data under zero, as readings under their offset give
            v = np.random.default_rng([7, b]).uniform(0.05, 4.0, size=len(y))
            for p in (bt["p0"][b], bt["truth"][b]):
                x, J, d, ok = rows(host, 1, kind, p, y, v, w)
                xn, Jn, dn, okn = rows_v_np(kind, p, y, v, w)
                assert ok.all() and okn.all()
                worst = max(worst, scaled(x, xn, 0), scaled(J, Jn, 0), scaled(d, dn, 0))
    print(f"{mz.case_id(case)}: largest scaled deviation of the host header from NumPy {worst:.3g} (asserted {ROWS_TOL:.3g})")
    assert worst <= ROWS_TOL


def test_the_clamp(host):
    """y + v < 0 counts as no photon: d = 2 f', x~ = sqrt(f'); a NaN datum stays NaN (the clamp is a comparison, not fmax); a model
    value that only v lifts above zero is feasible"""
    case = (MODEL_GAUSS2D, (7, 7))
    bt = po.batch((case, "low"), nb=1)
    p = bt["truth"][0]
    y = bt["y"][0].copy()
    v = np.full(len(y), 0.75)
    y[0], y[5], y[9] = -3.0, np.nan, -0.75
    x, J, d, ok = rows(host, 1, case[0], p, y, v, 7)
    f, _ = mz.model_eval(case[0], p, np.zeros(len(y)), None, None, 7)
    fv = f + v
    assert ok.all()
    for i in (0, 9):
        assert d[i] == 2.0 * fv[i] and x[i] == fv[i] * (1.0 / np.sqrt(fv[i]))
    assert np.isnan(x[5]) and np.isnan(d[5]) and np.all(np.isfinite(J[5]))
    q = p.copy()
    q[4] = -0.5
    f, _ = mz.model_eval(case[0], q, np.zeros(len(y)), None, None, 7)
    assert (f <= 0.0).any() and ((f + v) > 0.0).all()
    assert rows(host, 1, case[0], q, y, v, 7)[3].all() and not rows(host, 0, case[0], q, y, v, 7)[3].all()


# ---------------------------------------------------------------- 4. the oracle with read noise
@pytest.mark.parametrize("table", [((MODEL_GAUSS2D, (7, 7)), "low"), ((MODEL_GAUSS2D_ELLIPTIC, (9, 5)), "low"), ((MODEL_GAUSS2D, (8, 8)), "high"),
                                   ((MODEL_EXPDECAY, 65), "low"), ((MODEL_GAUSS1D, 5), "low")], ids=po.table_id)
def test_oracle_with_v_zero_is_the_poisson_oracle(table):
    """the hook with v = 0 on the Poisson tables' data (counts, >= 0): every entry of the result equal, plain and bounded"""
    bt = po.batch(table)
    prm = po.params()
    for bounded in (False, True):
        ref = po.oracle_table(table, bounded)
        for b in range(po.B):
            hp = mz.host_model(bt, b)
            got = co.solve_one(hp, np.zeros(hp.M), prm, bt["lo"][b] if bounded else None, bt["hi"][b] if bounded else None)
            assert got.keys() == ref[b].keys()
            for k, want in ref[b].items():
                same = np.array_equal(got[k], want) if isinstance(want, np.ndarray) else got[k] == want
                assert same, (po.table_id(table), bounded, b, k)


@pytest.mark.parametrize("table", co.TABLES, ids=co.table_id)
def test_oracle_tables(table):
    """no problem of a table is left out of a comparison: each one meets the conditions the seeds were chosen for"""
    assert co.SEED0[table] >= 1
    bt = co.batch(table)
    _, w, h = mz.case_shape(table[0])
    for k, bounded in enumerate((False, True)):
        orc = co.oracle_table(table, bounded)
        assert len(orc) == co.B
        margin = min(o["margin"] for o in orc)
        assert margin > co.MARGIN_FLOOR and max(o["cost_error"] for o in orc) <= co.COST_TOL
        assert all(o["status"] in (BATCH_JTX, BATCH_SMALL_STEP) for o in orc)
        assert abs(margin - co.MARGINS[table][k]) <= 0.005 * co.MARGINS[table][k], "the recorded margin (3 digits)"
        if bounded:
            assert any(o["held"].any() for o in orc)
    off = np.stack([co.window(bt["maps"]["offset"], bt["origin"][b], w, h) for b in range(co.B)])
    assert bt["raw"].dtype == np.uint16 and bt["v"].min() >= 0.5
    y, v = zip(*[co.calibrate(bt["raw"][b], table[0], bt["origin"][b]) for b in range(co.B)])
    assert np.array_equal(np.array(y), bt["y"]) and np.array_equal(np.array(v), bt["v"])
    if table[1] == "low":
        assert (bt["raw"] < off).sum() >= 100 and ((bt["y"] + bt["v"]) < 0.0).sum() >= 10


# ---------------------------------------------------------------- 2. the layout
def test_struct_layout(host):
    out = (C.c_size_t * 16)()
    n = host.camera_layout(out)
    fields = ("model", "dtype", "raw", "sensor_width", "sensor_height", "offset", "gain_inv", "readvar", "origin")
    want = [C.sizeof(BatchCamera)] + [getattr(BatchCamera, f).offset for f in fields] + [C.sizeof(BatchModel)]
    assert n == len(want) and list(out[:n]) == want
    assert [f for f, _ in BatchCamera._fields_] == list(fields)


def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "dogleg.h")) as f:
        header = f.read()
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS and hasattr(capi.lib(), n) and n + "(" in header, n
    for k, name in ((DATA_F64, "F64"), (DATA_F32, "F32"), (DATA_U16, "U16")):
        assert f"#define DOGLEG_AMD_DATA_{name} {k}" in header
    for phrase in ("5. Raw camera frames", "calibration for the 1D kinds", "uint8 / int32 data", "EMCCD excess-noise models"):
        assert phrase in header, phrase


# ---------------------------------------------------------------- 3. refusals, no device needed
def test_refusals_that_need_no_device(capfd):
    """the arrays are host memory here: a call that got past the checks under test would be refused by the pointer checks that
    follow them, never launched"""
    L = capi.lib()
    B, W, H = 4, 7, 7
    M = W * H
    raw = np.ones((B, M), dtype=np.uint16)
    rawb = np.ones(B * M * 2 + 8, dtype=np.uint8)
    maps = np.ones((48, 64), dtype=np.float32)
    org = np.zeros((B, 2), dtype=np.int32)
    s = np.ones((B, M))

    def camera(kind=MODEL_GAUSS2D, nmeas=M, width=W, height=H, y=None, scale=None, dtype=DATA_U16, raw_=raw.ctypes.data, sensor=(0, 0),
               offset=None, gain_inv=None, readvar=None, origin=None):
        m = BatchModel(kind, nmeas, width, height, y, None, None if scale is None else scale.ctypes.data, 0)
        return BatchCamera(m, dtype, raw_, sensor[0], sensor[1], offset, gain_inv, readvar, origin)

    mp, og = maps.ctypes.data, org.ctypes.data
    full = dict(sensor=(64, 48), offset=mp, gain_inv=mp, origin=og)
    p0 = np.arange(1.0, 1.0 + B * 5).reshape(B, 5)
    p = p0.copy()
    res = (BatchResult * B)()
    C.memset(res, 0xA5, C.sizeof(res))
    res0 = bytes(res)
    lam, status = np.full(B, -7.5), np.full(B, 42, dtype=np.int32)
    cov, Jq, out = np.full((B, 5, 5), 3.25), np.ones((B, 1, 2, 5)), np.full((B, 1, 2, 2), 3.25)
    I = C.POINTER(C.c_int)

    def solve(c, lk=LIKELIHOOD_POISSON):
        return L.dogleg_amd_optimize_dense_batch_camera(dptr(p), B, None if c is None else C.byref(c), lk, None, None, res)

    def solve_dev(c, lk=LIKELIHOOD_POISSON):
        return L.dogleg_amd_optimize_dense_batch_camera_device(p.ctypes.data, B, None if c is None else C.byref(c), lk, None, None,
                                                               C.addressof(res), lam.ctypes.data, None, None)

    def unc(c, lk=LIKELIHOOD_POISSON):
        return L.dogleg_amd_dense_batch_camera_uncertainty(dptr(p), B, None if c is None else C.byref(c), lk, dptr(lam), dptr(cov), None,
                                                           None, None, 1, status.ctypes.data_as(I), None)

    def unc_dev(c, lk=LIKELIHOOD_POISSON):
        return L.dogleg_amd_dense_batch_camera_uncertainty_device(p.ctypes.data, B, None if c is None else C.byref(c), lk, lam.ctypes.data,
                                                                  cov.ctypes.data, None, None, None, 1, status.ctypes.data, None, None,
                                                                  None)

    def query(c, lk=LIKELIHOOD_POISSON):
        return L.dogleg_amd_dense_batch_camera_query_covariance(dptr(p), B, None if c is None else C.byref(c), lk, dptr(lam), dptr(Jq), 1,
                                                                2, -1, dptr(out), status.ctypes.data_as(I), None)

    def query_dev(c, lk=LIKELIHOOD_POISSON):
        return L.dogleg_amd_dense_batch_camera_query_covariance_device(p.ctypes.data, B, None if c is None else C.byref(c), lk,
                                                                       lam.ctypes.data, Jq.ctypes.data, 1, 2, -1, out.ctypes.data,
                                                                       status.ctypes.data, None, None, None)

    calls = (solve, solve_dev, unc, unc_dev, query, query_dev)
    refusals = [
        (dict(c=None), "camera must be given"),
        (dict(c=camera(y=s.ctypes.data)), "camera->model.y must be NULL"),
        (dict(c=camera(raw_=None)), "camera->raw must be given"),
        (dict(c=camera(raw_=rawb.ctypes.data + 1)), "is not aligned to its element of 2 bytes"),
        (dict(c=camera(dtype=DATA_F32, raw_=rawb.ctypes.data + 2)), "is not aligned to its element of 4 bytes"),
        (dict(c=camera(dtype=DATA_F64, raw_=rawb.ctypes.data + 4)), "is not aligned to its element of 8 bytes"),
        (dict(c=camera(dtype=3)), "camera->dtype = 3 is none of"),
        (dict(c=camera(dtype=-1)), "camera->dtype = -1 is none of"),
        # calibration in part
        (dict(c=camera(**dict(full, offset=None))), "calibration is given in part"),
        (dict(c=camera(**dict(full, gain_inv=None))), "calibration is given in part"),
        (dict(c=camera(**dict(full, origin=None))), "calibration is given in part"),
        (dict(c=camera(**dict(full, sensor=(0, 48)))), "calibration is given in part"),
        (dict(c=camera(**dict(full, sensor=(64, 0)))), "calibration is given in part"),
        (dict(c=camera(readvar=mp)), "calibration is given in part"),
        (dict(c=camera(sensor=(64, 48))), "calibration is given in part"),
        (dict(c=camera(kind=MODEL_GAUSS1D, width=0, height=0, **full)), "calibration maps go with the 2D kinds only"),
        (dict(c=camera(kind=MODEL_EXPDECAY, width=0, height=0, **full)), "calibration maps go with the 2D kinds only"),
        (dict(c=camera(**dict(full, sensor=(6, 48)))), "a sensor of 6 x 48 pixels is smaller than the window of 7 x 7"),
        (dict(c=camera(**dict(full, sensor=(64, 5)))), "a sensor of 64 x 5 pixels is smaller than the window of 7 x 7"),
        (dict(c=camera(scale=s)), "model->scale must be NULL with DOGLEG_AMD_LIKELIHOOD_POISSON"),
        (dict(c=camera(scale=s, **full)), "model->scale must be NULL with DOGLEG_AMD_LIKELIHOOD_POISSON"),
        # what the mirrored call refuses of the model
        (dict(c=camera(), lk=2), "likelihood = 2 is neither"),
        (dict(c=camera(kind=4)), "model->kind = 4 is none of"),
        (dict(c=camera(nmeas=0)), "model->Nmeas = 0"),
        (dict(c=camera(width=3, height=5)), "3 x 5 pixels, and model->Nmeas = 49"),
        (dict(c=camera(kind=MODEL_EXPDECAY)), "both are 0 for the 1D kinds"),
    ]
    for call, name in zip(calls, NAMES):
        for kw, msg in refusals:
            capfd.readouterr()
            assert call(**kw) == -1, (name, msg)
            err = capfd.readouterr().err
            assert msg in err and name + ":" in err, (name, msg, err)
    # host memory is no device-accessible span: refused by name, after every check above
    if L.dlg_device_count() == 0:
        for call, name in zip(calls, NAMES):
            for c in (camera(), camera(readvar=mp, **full)):
                capfd.readouterr()
                assert call(c, LIKELIHOOD_GAUSS) == -1
                err = capfd.readouterr().err
                # (the host-pointer forms reach the record's arrays first, the _device twins their own p_dev)
                first = "p_dev" if name.endswith("_device") else "camera->raw"
                assert name + ": " + first + " = " in err and "is not device-accessible" in err, err

    # the camera Fisher callback is refused by every solve entry point, by name
    rec = camera()
    cb, cookie, N, Mm = capi.batch_camera_callback(rec, fisher=True)
    assert (N, Mm) == (5, M)
    pf, trivial = p0.copy(), BatchLoss(LOSS_TRIVIAL, 1.0, 1)
    for name, call in (
            ("dogleg_amd_optimize_dense_batch", lambda: capi.optimize_dense_batch(pf, N, M, cb, cookie, None)[0]),
            ("dogleg_amd_optimize_dense_batch_robust", lambda: capi.optimize_dense_batch_robust(pf, N, M, cb, cookie, trivial, None)[0]),
            ("dogleg_amd_optimize_dense_batch_bounded",
             lambda: capi.optimize_dense_batch_bounded(pf, N, M, cb, cookie, None, None, None, None)[0]),
            ("dogleg_amd_optimize_dense_batch_device",
             lambda: capi.optimize_dense_batch_device(pf.ctypes.data, B, N, M, cb, cookie, None, C.addressof(res))),
            ("dogleg_amd_optimize_dense_batch_robust_device",
             lambda: capi.optimize_dense_batch_robust_device(pf.ctypes.data, B, N, M, cb, cookie, None, trivial, C.addressof(res))),
            ("dogleg_amd_optimize_dense_batch_bounded_device",
             lambda: capi.optimize_dense_batch_bounded_device(pf.ctypes.data, B, N, M, cb, cookie, None, None, None, None, None,
                                                              C.addressof(res)))):
        capfd.readouterr()
        assert call() == -1, name
        err = capfd.readouterr().err
        assert name + ": dogleg_amd_batch_camera_fisher_callback is no callback of a solve" in err, (name, err)
    assert np.array_equal(pf, p0) and np.array_equal(p, p0) and bytes(res) == res0 and np.all(lam == -7.5)
    assert np.all(status == 42) and np.all(cov == 3.25) and np.all(out == 3.25)
