"""Raw camera frames in the fused calls of the built-in models (dogleg.h, item 5): dogleg_amd_optimize_dense_batch_camera, the
camera uncertainty and query calls, their _device twins and the two adapter callbacks.  B = 65; the shapes are
batch_models_np.CASES (Nmeas below, at and above the 64-row tile, 150 rows, 7 x 7, 8 x 8 and 9 x 5 windows).

1. Uncalibrated data, the solve: dtype x likelihood x plain / bounded; every output (p, the six result fields, lambda, held) has
   the bits of dogleg_amd_optimize_dense_batch_model_mle on y = float64(raw).
2. Uncalibrated data, the uncertainty and query calls: the bits of the _model_ calls, with held, featureSize 1 and 2,
   Nobservations < Nmeas and a scale to be computed.
3. Calibration, GAUSS, the 2D cases: random maps on a 64 x 48 sensor, origins flush with each of the four edges among them; the
   bits of the fused solve on the y NumPy computes, model.scale passed through.
4. Calibration, POISSON, readvar NULL or all zero, no negative y: the bits of the _mle solve and of the _model_uncertainty call on
   the y NumPy computes.
6. The adapter route: the rows of the two camera callbacks against NumPy (ROWS_TOL of the Poisson test); the fused GAUSS solve
   has the bits of the plain and bounded solve through dogleg_amd_batch_camera_callback; the fused camera uncertainty and query
   calls have the bits of the _fit calls through the matching camera callback, POISSON with readvar > 0 included; every solve
   entry point refuses the camera Fisher callback.
   With readvar > 0 the fused solve is also held against the definition: the returned cost is the deviance NumPy sums at the
   returned point (REL_TOL) and not above that of the start, and at a point returned with DOGLEG_AMD_BATCH_JTX the gradient NumPy
   forms from the definition lies under the threshold (to GRAD_SLACK).
7. An origin out of the sensor on each of the four sides, one of them by a single pixel: FAILED / UNC_FAILED, alone; every other
   problem has the bits it has when those problems are masked out.  The maps are allocated exactly sensor-sized.
8. The device twin has the host twin's bits, with a mask and on a stream, for u16 uncalibrated and u16 calibrated with read noise.
9. Two problems with the same origin and the same readings return the same bits; a batch whose windows all overlap one sensor
   region has the bits of the batch solved one problem at a time.
5. Calibration, POISSON, readvar > 0: against the tables of tests/batch_camera_oracle.py, the six 2D shapes at the low and the high
   count level, plain and bounded, no problem left out: status, iterations, evaluations, lambda and held equal; F and the trust
   region to REL_TOL; |p - p_oracle| <= STEP_TOL max(1, |p_oracle|): the comparisons of test_against_the_oracle in
   tests/test_dense_batch_poisson_gpu.py.  The low tables hold readings under their offset, and pixels where the clamp runs.
   MEASURED on an MI355X over the 24 tables: |p - p_oracle| / max(1, |p_oracle|) at most 2.4e-15, F relative at most 8.6e-15, the
   trust region relative at most 5.7e-12; no status, count, lambda or held differed."""
import ctypes as C

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BATCH_JTX, BATCH_UNC_FAILED, BATCH_UNC_OK, BATCH_UNC_SKIPPED, BatchLoss, LOSS_TRIVIAL, MODEL_GAUSS2D,
                                       MODEL_GAUSS2D_ELLIPTIC, MODEL_NSTATE, LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON, DATA_F64,
                                       DATA_F32, DATA_U16, DATA_NUMPY)
from tests import batch_camera_oracle as co
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_model_gpu as tm
from tests import test_dense_batch_model_uncertainty_gpu as tu
from tests import test_dense_batch_poisson_gpu as tp
from tests.parity import STEP_TOL
from tests.test_dense_batch_poisson_cpu import scaled

pytestmark = pytest.mark.gpu

B = mz.B
ROWS_TOL = tp.ROWS_TOL
REL_TOL = tp.REL_TOL
GRAD_SLACK = 1e-9          # |g| of the definition at a JTX point against the threshold 1e-4: rounding of a sum of <= 150 terms of size <= 1e2
GUARD, PAD, RSIZE = td.GUARD, td.PAD, td.RSIZE
OFF = (0, 32, 64)
SENSOR = (64, 48)          # width, height
CASES_2D = [c for c in mz.CASES if mz.is_2d(c[0])]
DTYPES = [DATA_F64, DATA_F32, DATA_U16]
DT_NAMES = {DATA_F64: "f64", DATA_F32: "f32", DATA_U16: "u16"}
LK_NAMES = {LIKELIHOOD_GAUSS: "gauss", LIKELIHOOD_POISSON: "poisson"}
LK = pytest.mark.parametrize("lk", [LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON], ids=lambda k: LK_NAMES[k])
DT = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: DT_NAMES[d])


def prm_of(lk):
    return mz.params() if lk == LIKELIHOOD_GAUSS else po.params()


class DevCamera:
    """a batch's readings (and maps) in device memory and its dogleg_amd_batch_camera_t.  cal: dict(offset, gain_inv, readvar or
    None: (H, W) float32; origin (nb, 2) int32) or None"""

    def __init__(self, bt, raw, dtype, cal=None, scale=None):
        assert raw.dtype == np.dtype(DATA_NUMPY[dtype])
        self.raw = capi.DeviceArray(raw)
        self.t = None if bt["t"] is None else capi.DeviceArray(bt["t"])
        self.scale = None if scale is None else capi.DeviceArray(scale)
        self.model = capi.batch_model(bt["kind"], None, bt["M"], bt["width"], bt["height"], self.t, bt["t_mode"] == "each", self.scale)
        self.maps = {}
        if cal is not None:
            for k in ("offset", "gain_inv", "readvar"):
                if cal.get(k) is not None:
                    assert cal[k].dtype == np.float32 and cal[k].shape == (SENSOR[1], SENSOR[0])
                    self.maps[k] = capi.DeviceArray(cal[k])       # exactly sensor-sized: nothing lies behind the last pixel
            self.maps["origin"] = capi.DeviceArray(np.ascontiguousarray(cal["origin"], dtype=np.int32))
        self.rec = capi.batch_camera(self.model, dtype, self.raw, SENSOR if cal is not None else (0, 0), self.maps.get("offset"),
                                     self.maps.get("gain_inv"), self.maps.get("readvar"), self.maps.get("origin"))
        self.N, self.M = MODEL_NSTATE[bt["kind"]], bt["M"]


def cam_solve(dc, p0, lk, lo=None, hi=None, bounded=False):
    """the camera solve, host pointers: (p, results, held or None); checks the constant cost"""
    before = capi.batch_model_callback_invocations()
    rc, p, res, held = capi.optimize_dense_batch_camera(p0, dc.rec, lk, lo, hi, prm_of(lk), bounded=bounded)
    assert rc == 0
    stats = capi.batch_last_stats()
    assert capi.batch_model_callback_invocations() == before
    assert stats["rounds"] == int(res["evaluations"].max()) and stats["ms_callback"] == 0.0
    return p, res, held


def ref_solve(bt, y, lk, bounded, scale=None):
    """the existing fused solve on doubles y"""
    bt = dict(bt, scale=scale)
    return tp.mle(tm.DevModel(bt, y=y), bt["p0"], bt["lo"], bt["hi"], bounded, lk, prm_of(lk))


def raw_of(case, lk, dtype):
    """(bt, raw) of the uncalibrated tests: Poisson draws for u16 (either likelihood), the likelihood's own table rounded to float
    for f32 and as it is for f64"""
    if dtype == DATA_U16 or lk == LIKELIHOOD_POISSON:
        bt = po.batch((case, "high"))
    else:
        bt = mz.batch(case)
    raw = np.ascontiguousarray(bt["y"].astype(DATA_NUMPY[dtype]))
    if dtype == DATA_U16:
        assert np.array_equal(raw.astype(np.float64), bt["y"])
    return bt, raw


# ---------------------------------------------------------------- 1. uncalibrated data, the solve
@DT
@LK
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_uncalibrated_solve_has_the_model_solves_bits(case, lk, dtype):
    bt, raw = raw_of(case, lk, dtype)
    dc = DevCamera(bt, raw, dtype)
    y = raw.astype(np.float64)
    for bounded in (False, True):
        tm.same_bits(ref_solve(bt, y, lk, bounded), cam_solve(dc, bt["p0"], lk, bt["lo"], bt["hi"], bounded),
                     f"{mz.case_id(case)}, {LK_NAMES[lk]}, {DT_NAMES[dtype]}, bounded {bounded}")


# ---------------------------------------------------------------- 2. uncalibrated data, the uncertainty and query calls
def cam_unc(dc, lk, p, lam, held, **kw):
    before = capi.batch_model_callback_invocations()
    out = capi.dense_batch_camera_uncertainty(p, dc.rec, lk, lam=lam, held=held, **kw)
    stats = capi.batch_uncertainty_last_stats()
    assert capi.batch_model_callback_invocations() == before
    if out["rc"] == 0:
        assert stats["ms_callback"] == 0.0 and stats["launches"] == 1 and stats["syncs"] == 1
    return out


def cam_query(dc, lk, p, lam, held, Jq, nobs):
    return capi.dense_batch_camera_query_covariance(p, dc.rec, lk, Jq, lam=lam, nobs=nobs, held=held)


def queries(N, seed):
    return np.random.default_rng([29, N, seed]).uniform(-1.0, 1.0, size=(B, 2, 3, N))


def compare_unc_and_query(dm, dc, lk, p, lam, held, what, M):
    """every uncertainty and query output of the camera calls against the _model_ calls on the record dm"""
    N = dc.N
    for fs in (1, 2):
        for scale in (2.5, None):
            kw = dict(want=("cov", "var", "factors"), fs=fs, scale=scale)
            r, f = tu.unc_fused(dm, lk, p, lam, held, **kw), cam_unc(dc, lk, p, lam, held, **kw)
            tu.same(r, f, tu.UNC_KEYS, f"{what}, fs {fs}, scale {scale}", nan_equal=True)
            # (a scale to be computed needs Nmeas > Nstate + 1: where the _model_ call refuses, so does the camera call)
            assert r["rc"] == (0 if scale or M > N + 1 else -1) and (r["rc"] == -1 or np.all(f["status"] == BATCH_UNC_OK)), what
    tu.same(tu.unc_fused(dm, lk, p, None, held, want=("var",)), cam_unc(dc, lk, p, None, held, want=("var",)), tu.UNC_KEYS, what)
    Jq = queries(N, M)
    for nobs in (-1, M, M - M // 3):
        r, f = tu.query_fused(dm, lk, p, lam, held, Jq, nobs), cam_query(dc, lk, p, lam, held, Jq, nobs)
        assert r["rc"] == 0
        tu.same(r, f, tu.QUERY_KEYS, f"{what}, Nobservations {nobs}", nan_equal=True)


@DT
@LK
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_uncalibrated_uncertainty_and_query_have_the_model_calls_bits(case, lk, dtype):
    bt, raw = raw_of(case, lk, dtype)
    dc = DevCamera(bt, raw, dtype)
    y = raw.astype(np.float64)
    dm = tm.DevModel(bt, y=y)
    for bounded in (False, True):
        p, res, held = ref_solve(bt, y, lk, bounded)
        compare_unc_and_query(dm, dc, lk, p, np.ascontiguousarray(res["lambda_"]), held,
                              f"{mz.case_id(case)}, {LK_NAMES[lk]}, {DT_NAMES[dtype]}, bounded {bounded}", bt["M"])


# ---------------------------------------------------------------- calibration: the maps, the origins, the readings
def calibration(w, h, seed, nb=B, readvar=None):
    """random maps on the sensor and origins, the first four flush with the left, top, right and bottom edge (the first two in a
    corner each); readvar: None, "zero" or "noise" (0.05 .. 1.5 photoelectrons^2: under what a reading rounded below its offset lacks)"""
    rng = np.random.default_rng([31, w, h, seed])
    W, H = SENSOR
    cal = dict(offset=(100.0 + 5.0 * rng.uniform(-1.0, 1.0, size=(H, W))).astype(np.float32),
               gain_inv=rng.uniform(0.4, 2.5, size=(H, W)).astype(np.float32), readvar=None)
    if readvar == "zero":
        cal["readvar"] = np.zeros((H, W), dtype=np.float32)
    elif readvar == "noise":
        cal["readvar"] = rng.uniform(0.05, 1.5, size=(H, W)).astype(np.float32)
    org = np.stack([rng.integers(0, W - w + 1, size=nb), rng.integers(0, H - h + 1, size=nb)], axis=1).astype(np.int32)
    org[:4] = [[0, 0], [W - w, 0], [W - w, H - h], [0, H - h]]
    org[4:8] = [[0, 7], [5, 0], [W - w, 9], [11, H - h]]
    cal["origin"] = org[:nb]
    return cal


def window(m, org, w, h):
    """(nb, h w) values of a map under every problem's window"""
    return np.stack([m[oy:oy + h, ox:ox + w].reshape(-1) for ox, oy in org])


def calibrated_y(raw, cal, w, h):
    """y and v as the definition forms them, in float64"""
    off, gi = (window(cal[k], cal["origin"], w, h).astype(np.float64) for k in ("offset", "gain_inv"))
    v = np.zeros(raw.shape) if cal["readvar"] is None else window(cal["readvar"], cal["origin"], w, h).astype(np.float64)
    return (raw.astype(np.float64) - off) * gi, v


def readings(y, cal, w, h, dtype, below=False):
    """readings of dtype whose calibrated value is close to the photoelectrons y; below: rounded to the nearest (a reading may lie
    under its offset), otherwise rounded up so that no calibrated value is negative"""
    off, gi = (window(cal[k], cal["origin"], w, h).astype(np.float64) for k in ("offset", "gain_inv"))
    adu = y / gi + off
    if dtype == DATA_U16:
        adu = np.rint(adu) if below else np.ceil(adu)
        assert adu.min() >= 0 and adu.max() <= 65535
    return np.ascontiguousarray(adu.astype(DATA_NUMPY[dtype]))


# ---------------------------------------------------------------- 3. calibration, GAUSS
@DT
@pytest.mark.parametrize("case", CASES_2D, ids=mz.case_id)
def test_calibrated_gauss_has_the_fused_solves_bits(case, dtype):
    _, w, h = mz.case_shape(case)
    for with_scale, readvar in ((False, None), (True, "noise")):
        bt = mz.batch(case, with_scale=with_scale)
        cal = calibration(w, h, 1, readvar=readvar)
        raw = readings(bt["y"], cal, w, h, dtype, below=True)
        y, _ = calibrated_y(raw, cal, w, h)
        dc = DevCamera(bt, raw, dtype, cal, bt["scale"])
        for bounded in (False, True):
            tm.same_bits(ref_solve(bt, y, LIKELIHOOD_GAUSS, bounded, bt["scale"]),
                         cam_solve(dc, bt["p0"], LIKELIHOOD_GAUSS, bt["lo"], bt["hi"], bounded),
                         f"{mz.case_id(case)}, {DT_NAMES[dtype]}, scale {with_scale}, bounded {bounded}")


# ---------------------------------------------------------------- 4. calibration, POISSON, no read noise
@pytest.mark.parametrize("readvar", [None, "zero"], ids=["readvar-null", "readvar-zero"])
@DT
@pytest.mark.parametrize("case", CASES_2D, ids=mz.case_id)
def test_calibrated_poisson_without_read_noise_has_the_mle_calls_bits(case, dtype, readvar):
    _, w, h = mz.case_shape(case)
    bt = po.batch((case, "high"))
    cal = calibration(w, h, 2, readvar=readvar)
    raw = readings(bt["y"], cal, w, h, dtype)
    y, v = calibrated_y(raw, cal, w, h)
    assert y.min() >= 0.0 and not v.any()
    dc = DevCamera(bt, raw, dtype, cal)
    dm = tm.DevModel(bt, y=y)
    for bounded in (False, True):
        what = f"{mz.case_id(case)}, {DT_NAMES[dtype]}, bounded {bounded}"
        ref = ref_solve(bt, y, LIKELIHOOD_POISSON, bounded)
        tm.same_bits(ref, cam_solve(dc, bt["p0"], LIKELIHOOD_POISSON, bt["lo"], bt["hi"], bounded), what)
        compare_unc_and_query(dm, dc, LIKELIHOOD_POISSON, ref[0], np.ascontiguousarray(ref[1]["lambda_"]), ref[2], what, bt["M"])


# ---------------------------------------------------------------- 5. calibration, POISSON, read noise: the oracle's tables
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
@pytest.mark.parametrize("table", co.TABLES, ids=co.table_id)
def test_read_noise_solve_against_the_oracle(table, bounded):
    orc = co.oracle_table(table, bounded)
    assert min(o["margin"] for o in orc) > co.MARGIN_FLOOR and max(o["cost_error"] for o in orc) <= co.COST_TOL
    bt = co.batch(table)
    _, w, h = mz.case_shape(table[0])
    if table[1] == "low":
        off = np.stack([co.window(bt["maps"]["offset"], bt["origin"][b], w, h) for b in range(B)])
        assert (bt["raw"] < off).any() and ((bt["y"] + bt["v"]) < 0.0).any(), "readings under their offset: the clamp runs"
    dc = DevCamera(bt, bt["raw"], DATA_U16, dict(bt["maps"], origin=bt["origin"]))
    p, res, held = cam_solve(dc, bt["p0"], LIKELIHOOD_POISSON, bt["lo"], bt["hi"], bounded)
    dp = max(float(np.max(np.abs(p[b] - orc[b]["p"]) / np.maximum(1.0, np.abs(orc[b]["p"])))) for b in range(B))
    dn = max(abs(res["norm2_x"][b] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for b in range(B))
    dt = max(abs(res["trustregion"][b] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for b in range(B))
    print(f"{co.table_id(table)}, bounded {bounded}: max |p - p_oracle| / max(1, |p_oracle|) {dp:.3g}, F rel {dn:.3g}, trust region "
          f"rel {dt:.3g}, infeasible trials {sum(o['infeasible'] for o in orc)}")
    for b in range(B):
        o = orc[b]
        got = (int(res["status"][b]), int(res["iterations"][b]), int(res["evaluations"][b]), float(res["lambda_"][b]))
        assert got == (o["status"], o["iterations"], o["evaluations"], o["lambda_"]), (b, got)
        if bounded:
            assert held[b].tolist() == o["held"].tolist(), b
    assert dp <= STEP_TOL and dn <= REL_TOL and dt <= REL_TOL


# ---------------------------------------------------------------- 6. the adapter route
def camera_rows(dc, p, fisher):
    nb, N, M = p.shape[0], dc.N, dc.M
    P, X, J = capi.DeviceArray(p), td.Buf(np.full((nb, M), GUARD)), td.Buf(np.full((nb, M, N), GUARD))
    live = capi.DeviceArray(np.ones(nb, dtype=np.uint8))
    L = capi.lib()
    (L.dogleg_amd_batch_camera_fisher_callback if fisher else L.dogleg_amd_batch_camera_callback)(
        P.ptr, X.ptr, J.ptr, live.ptr, nb, None, C.c_void_p(C.addressof(dc.rec)))
    return X.get(), J.get()


def rows_np(bt, b, p, y, v, fisher):
    """x, J of the GAUSS definition, or x~, J~, d of the Poisson definition with read noise, of problem b"""
    f, G = mz.model_eval(bt["kind"], p, np.zeros(bt["M"]), None if bt["t"] is None else (bt["t"] if bt["t"].ndim == 1 else bt["t"][b]),
                         None, bt["width"])
    if not fisher:
        s = 1.0 if bt["scale"] is None else bt["scale"][b]
        return s * (f - y), G * np.reshape(s, (-1, 1)) if bt["scale"] is not None else G, None
    fv, yv = f + v, np.maximum(y + v, 0.0)
    q = 1.0 / np.sqrt(fv)
    with np.errstate(all="ignore"):
        d = np.where(yv == 0.0, 2.0 * fv, 2.0 * ((fv - yv) - yv * np.log(fv / np.where(yv == 0.0, 1.0, yv))))
    return (fv - yv) * q, G * q[:, None], d


def low_count_camera(case, dtype=DATA_U16, readvar="noise", seed=3):
    """the low-count table of a 2D case behind maps with read noise: (bt, cal, raw, y, v, the camera)"""
    _, w, h = mz.case_shape(case)
    bt = po.batch((case, "low"))
    cal = calibration(w, h, seed, readvar=readvar)
    raw = readings(bt["y"], cal, w, h, dtype, below=True)
    y, v = calibrated_y(raw, cal, w, h)
    return bt, cal, raw, y, v, DevCamera(bt, raw, dtype, cal)


@pytest.mark.parametrize("case", CASES_2D, ids=mz.case_id)
def test_camera_callbacks_rows_against_numpy(case):
    bt, cal, raw, y, v, dc = low_count_camera(case)
    assert (y < 0.0).any() and ((y + v) < 0.0).any(), "readings under their offset, so that the clamp runs"
    worst = 0.0
    for fisher in (False, True):
        x, J = camera_rows(dc, bt["truth"], fisher)
        for b in range(B):
            xn, Jn, _ = rows_np(bt, b, bt["truth"][b], y[b], v[b], fisher)
            worst = max(worst, scaled(x[b], xn, 0), scaled(J[b], Jn, 0))
    print(f"{mz.case_id(case)}: largest scaled deviation of the camera callbacks' rows from NumPy {worst:.3g} (asserted {ROWS_TOL:.3g})")
    assert worst <= ROWS_TOL


@pytest.mark.parametrize("case", [(MODEL_GAUSS2D, (7, 7)), (MODEL_GAUSS2D_ELLIPTIC, (9, 5))], ids=mz.case_id)
def test_fused_gauss_solve_has_the_camera_callbacks_bits(case):
    _, w, h = mz.case_shape(case)
    bt = mz.batch(case, with_scale=True)
    cal = calibration(w, h, 4, readvar="noise")
    raw = readings(bt["y"], cal, w, h, DATA_U16, below=True)
    dc = DevCamera(bt, raw, DATA_U16, cal, bt["scale"])
    cb, cookie, N, M = capi.batch_camera_callback(dc.rec)
    prm = mz.params()
    for bounded in (False, True):
        if bounded:
            rc, p, res, held, _ = capi.optimize_dense_batch_bounded(bt["p0"], N, M, cb, cookie, bt["lo"], bt["hi"], None, prm)
        else:
            (rc, p, res), held = capi.optimize_dense_batch(bt["p0"], N, M, cb, cookie, prm), None
        assert rc == 0
        tm.same_bits((p, res, held), cam_solve(dc, bt["p0"], LIKELIHOOD_GAUSS, bt["lo"], bt["hi"], bounded), f"bounded {bounded}")


@LK
@pytest.mark.parametrize("case", CASES_2D, ids=mz.case_id)
def test_fused_camera_uncertainty_has_the_camera_callbacks_bits(case, lk):
    """the fused camera uncertainty and query calls against the _fit calls through the matching camera callback, read noise > 0"""
    bt, cal, raw, y, v, dc = low_count_camera(case)
    cb, cookie, N, M = capi.batch_camera_callback(dc.rec, fisher=lk == LIKELIHOOD_POISSON)
    Jq = queries(N, M)
    for bounded in (False, True):
        p, res, held = cam_solve(dc, bt["p0"], lk, bt["lo"], bt["hi"], bounded)
        lam = np.ascontiguousarray(res["lambda_"])
        fit = tu.fit_of(held)
        for fs in (1, 2):
            for scale in (2.5, None):
                kw = dict(want=("cov", "var", "factors"), fs=fs, scale=scale)
                r = capi.dense_batch_uncertainty(p, N, M, cb, cookie, lam=lam, fit=fit, **kw)
                f = cam_unc(dc, lk, p, lam, held, **kw)
                assert r["rc"] == 0
                tu.same(r, f, tu.UNC_KEYS, f"{mz.case_id(case)}, bounded {bounded}, fs {fs}, scale {scale}", nan_equal=True)
        for nobs in (-1, M - M // 3):
            r = capi.dense_batch_query_covariance(p, N, M, cb, cookie, Jq, lam=lam, nobs=nobs, fit=fit)
            f = cam_query(dc, lk, p, lam, held, Jq, nobs)
            assert r["rc"] == 0
            tu.same(r, f, tu.QUERY_KEYS, f"{mz.case_id(case)}, bounded {bounded}, Nobservations {nobs}", nan_equal=True)


@pytest.mark.parametrize("level", ["low", "high"])
@pytest.mark.parametrize("case", CASES_2D, ids=mz.case_id)
def test_read_noise_solve_against_the_definition(case, level):
    """readvar > 0, plain: no problem fails; the cost a problem returns is the deviance the definition has at the point it returns,
    which is not above that of its start (only improving steps are taken); where the solve stops with JTX the gradient of the
    definition is under the threshold"""
    _, w, h = mz.case_shape(case)
    bt = po.batch((case, level))
    cal = calibration(w, h, 5, readvar="noise")
    raw = readings(bt["y"], cal, w, h, DATA_U16, below=True)
    y, v = calibrated_y(raw, cal, w, h)
    if level == "low":
        assert ((y + v) < 0.0).any()
    p, res, _ = cam_solve(DevCamera(bt, raw, DATA_U16, cal), bt["p0"], LIKELIHOOD_POISSON)
    thr = po.params().Jt_x_threshold
    jtx = [b for b in range(B) if res["status"][b] == BATCH_JTX]
    assert np.all(res["status"] != BATCH_FAILED)
    worst_g = worst_F = 0.0
    for b in range(B):
        xn, Jn, d = rows_np(bt, b, p[b], y[b], v[b], True)
        if b in jtx:
            worst_g = max(worst_g, float(np.max(np.abs(Jn.T @ xn))))
        worst_F = max(worst_F, abs(res["norm2_x"][b] - d.sum()) / abs(d.sum()))
        assert d.sum() <= rows_np(bt, b, bt["p0"][b], y[b], v[b], True)[2].sum(), b
    print(f"{mz.case_id(case)}-{level}: {len(jtx)} JTX; largest |g| of the definition {worst_g:.3g} (threshold {thr:.3g}), cost rel {worst_F:.3g}")
    assert worst_g <= thr + GRAD_SLACK and worst_F <= REL_TOL


def test_every_solve_entry_point_refuses_the_camera_fisher_callback(capfd):
    bt, cal, raw, y, v, dc = low_count_camera((MODEL_GAUSS2D, (7, 7)))
    nb = 4
    cb, cookie, N, M = capi.batch_camera_callback(dc.rec, fisher=True)
    p0 = bt["p0"][:nb]
    P, R = td.Buf(p0), td.Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8))
    Hd = td.Buf(np.full((nb, N), 0x5A, dtype=np.uint8))
    trivial = BatchLoss(LOSS_TRIVIAL, 1.0, 1)
    prm = po.params()
    for name, call in (
            ("dogleg_amd_optimize_dense_batch", lambda: capi.optimize_dense_batch(p0, N, M, cb, cookie, prm)[0]),
            ("dogleg_amd_optimize_dense_batch_robust", lambda: capi.optimize_dense_batch_robust(p0, N, M, cb, cookie, trivial, prm)[0]),
            ("dogleg_amd_optimize_dense_batch_bounded",
             lambda: capi.optimize_dense_batch_bounded(p0, N, M, cb, cookie, bt["lo"][:nb], bt["hi"][:nb], None, prm)[0]),
            ("dogleg_amd_optimize_dense_batch_device", lambda: capi.optimize_dense_batch_device(P.ptr, nb, N, M, cb, cookie, prm, R.ptr)),
            ("dogleg_amd_optimize_dense_batch_robust_device",
             lambda: capi.optimize_dense_batch_robust_device(P.ptr, nb, N, M, cb, cookie, prm, trivial, R.ptr)),
            ("dogleg_amd_optimize_dense_batch_bounded_device",
             lambda: capi.optimize_dense_batch_bounded_device(P.ptr, nb, N, M, cb, cookie, prm, None, None, None, Hd.ptr, R.ptr))):
        capfd.readouterr()
        assert call() == -1, name
        assert name + ": dogleg_amd_batch_camera_fisher_callback is no callback of a solve" in capfd.readouterr().err, name
    assert P.get().tobytes() == p0.tobytes() and np.all(R.get() == PAD) and np.all(Hd.get() == 0x5A)


# ---------------------------------------------------------------- 7. an origin out of the sensor
@LK
def test_origin_out_of_the_sensor_fails_alone(lk):
    """the kernel's test, ox >= 0, oy >= 0, ox <= W - w, oy <= H - h, is what keeps the gather inside the maps, which are exactly
    sensor-sized here: a problem that fails it loads nothing from them and its data are NaN"""
    case = (MODEL_GAUSS2D, (7, 7))
    _, w, h = mz.case_shape(case)
    W, H = SENSOR
    bt = po.batch((case, "high"))
    cal = calibration(w, h, 6, readvar="noise")
    raw = readings(bt["y"], cal, w, h, DATA_U16)
    out = {9: (-1, 5), 20: (3, -2), 33: (W - w + 1, 4), 47: (10, H - h + 3), 58: (-2000000000, 2000000000)}
    org = cal["origin"].copy()
    for b, o in out.items():
        org[b] = o
    bad = sorted(out)
    good = [b for b in range(B) if b not in out]
    mask = np.ones(B, dtype=np.uint8)
    mask[bad] = 0
    dc = DevCamera(bt, raw, DATA_U16, dict(cal, origin=org))
    for bounded in (False, True):
        p, res, held = cam_solve(dc, bt["p0"], lk, bt["lo"], bt["hi"], bounded)
        assert np.all(res["status"][bad] == BATCH_FAILED) and p[bad].tobytes() == bt["p0"][bad].tobytes()
        assert np.all(res["status"][good] != BATCH_FAILED)
        m = cam_solve_device(dc, bt["p0"], lk, bt["lo"], bt["hi"], bounded, mask=mask)
        assert p[good].tobytes() == m[0][good].tobytes() and tb.bitwise_equal(res[good], m[1][good])
        if bounded:
            assert held[good].tobytes() == m[2][good].tobytes()
        lam = np.ascontiguousarray(res["lambda_"])
        lam[bad] = 0.0
        u = cam_unc(dc, lk, p, lam, held, want=("cov", "var", "factors"), scale=None)
        assert u["rc"] == 0 and np.all(u["status"][bad] == BATCH_UNC_FAILED) and np.all(u["status"][good] == BATCH_UNC_OK)
        assert np.all(np.isnan(u["cov"][bad])) and np.all(np.isfinite(u["cov"][good]))
        um = cam_unc_device(dc, lk, p, lam, held, mask)
        for k in ("cov", "var", "factors", "scale", "lam"):
            assert np.ascontiguousarray(u[k][good]).tobytes() == np.ascontiguousarray(um[k][good]).tobytes(), k
        Jq = queries(dc.N, 7)
        q = cam_query(dc, lk, p, lam, held, Jq, -1)
        assert q["rc"] == 0 and np.all(q["status"][bad] == BATCH_UNC_FAILED) and np.all(q["status"][good] == BATCH_UNC_OK)


def test_an_undersized_map_or_origin_array_is_refused_by_name(capfd):
    """the spans: a map of one float less than sensor_width sensor_height, origins of one int less than 2 B, readings of one less
    than B Nmeas: -1 with the array's name, outputs untouched"""
    case = (MODEL_GAUSS2D, (7, 7))
    bt, cal, raw, y, v, dc = low_count_camera(case)
    W, H = SENSOR
    short_map = capi.DeviceArray(np.ones(W * H - 1, dtype=np.float32))
    short_org = capi.DeviceArray(np.zeros(2 * B - 1, dtype=np.int32))
    short_raw = capi.DeviceArray(np.ones(B * dc.M - 1, dtype=np.uint16))
    mp = dc.maps
    for name, rec in (
            ("camera->offset", capi.batch_camera(dc.model, DATA_U16, dc.raw, SENSOR, short_map, mp["gain_inv"], mp["readvar"], mp["origin"])),
            ("camera->gain_inv", capi.batch_camera(dc.model, DATA_U16, dc.raw, SENSOR, mp["offset"], short_map, mp["readvar"], mp["origin"])),
            ("camera->readvar", capi.batch_camera(dc.model, DATA_U16, dc.raw, SENSOR, mp["offset"], mp["gain_inv"], short_map, mp["origin"])),
            ("camera->origin", capi.batch_camera(dc.model, DATA_U16, dc.raw, SENSOR, mp["offset"], mp["gain_inv"], mp["readvar"], short_org)),
            ("camera->raw", capi.batch_camera(dc.model, DATA_U16, short_raw, SENSOR, mp["offset"], mp["gain_inv"], mp["readvar"], mp["origin"]))):
        for lk in (LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON):
            capfd.readouterr()
            rc, p, res, _ = capi.optimize_dense_batch_camera(bt["p0"], rec, lk, None, None, prm_of(lk))
            err = capfd.readouterr().err
            assert rc == -1 and f"dogleg_amd_optimize_dense_batch_camera: {name} = " in err and "is not device-accessible" in err, (name, err)
            assert p.tobytes() == bt["p0"].tobytes()
            capfd.readouterr()
            u = capi.dense_batch_camera_uncertainty(bt["p0"], rec, lk, want=("var",))
            err = capfd.readouterr().err
            assert u["rc"] == -1 and f"dogleg_amd_dense_batch_camera_uncertainty: {name} = " in err, (name, err)
            assert np.all(u["status"] == -1) and not u["var"].any()


# ---------------------------------------------------------------- 8. the device twin
@pytest.fixture(scope="module")
def stream():
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    yield s.value
    assert hip.hipStreamDestroy(s) == 0


def cam_solve_device(dc, p0, lk, lo, hi, bounded, mask=None, stream=None):
    """the _device twin: (p, results, held or None, lambda)"""
    nb, N = p0.shape
    P, R, Lm = td.Buf(p0), td.Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8)), td.Buf(np.full(nb, GUARD))
    A = td.mask_dev(mask)
    Lo, Hi = (td.Buf(a) if bounded and a is not None else None for a in (lo, hi))
    Hd = td.Buf(np.full((nb, N), 0x5A, dtype=np.uint8)) if bounded else None
    ptr = lambda b: None if b is None else b.ptr
    rc = capi.optimize_dense_batch_camera_device(P.ptr, nb, dc.rec, lk, prm_of(lk), R.ptr, ptr(Lo), ptr(Hi), ptr(Hd), Lm.ptr, ptr(A),
                                                 stream, bounded=bounded)
    assert rc == 0
    return P.get(), td.results_of(R, nb), None if Hd is None else Hd.get(), Lm.get()


def cam_unc_device(dc, lk, p, lam, held, mask=None, stream=None):
    """the uncertainty call's _device twin, a scale to be computed: dict(cov, var, factors, scale, lam, status)"""
    nb, N, M = p.shape[0], dc.N, dc.M
    P, Lm, St = td.Buf(p), td.Buf(lam), td.Buf(np.full(nb, -7, dtype=np.int32))
    Cv, Vr, Fc, Sc = td.Buf(np.full((nb, N, N), GUARD)), td.Buf(np.full((nb, N), GUARD)), td.Buf(np.full((nb, M), GUARD)), td.Buf(np.full(nb, -1.0))
    Hd = None if held is None else td.Buf(held)
    A = td.mask_dev(mask)
    ptr = lambda b: None if b is None else b.ptr
    rc = capi.dense_batch_camera_uncertainty_device(P.ptr, nb, dc.rec, lk, St.ptr, Lm.ptr, Cv.ptr, Vr.ptr, Fc.ptr, Sc.ptr, 1, ptr(Hd),
                                                    ptr(A), stream)
    assert rc == 0
    return dict(cov=Cv.get(), var=Vr.get(), factors=Fc.get(), scale=Sc.get(), lam=Lm.get(), status=St.get())


@pytest.mark.parametrize("calibrated", [False, True], ids=["u16", "u16-maps-readnoise"])
def test_device_twin_has_the_host_twins_bits(calibrated, stream):
    case = (MODEL_GAUSS2D, (8, 8))
    if calibrated:
        bt, cal, raw, y, v, dc = low_count_camera(case)
    else:
        bt, raw = raw_of(case, LIKELIHOOD_POISSON, DATA_U16)
        dc = DevCamera(bt, raw, DATA_U16)
    mask = np.ones(B, dtype=np.uint8)
    mask[list(OFF)] = 0
    on, off = np.flatnonzero(mask), list(OFF)
    p0, lo, hi = bt["p0"], bt["lo"], bt["hi"]
    lk = LIKELIHOOD_POISSON
    for bounded in (False, True):
        hs = cam_solve(dc, p0, lk, lo, hi, bounded)
        for st in (None, stream):
            d = cam_solve_device(dc, p0, lk, lo, hi, bounded, stream=st)
            tm.same_bits(hs, d[:3], f"bounded {bounded}, stream {st is not None}")
            assert d[3].tobytes() == np.ascontiguousarray(d[1]["lambda_"]).tobytes()
            m = cam_solve_device(dc, p0, lk, lo, hi, bounded, mask=mask, stream=st)
            assert m[0][off].tobytes() == p0[off].tobytes() and np.all(m[3][off] == 0.0)
            assert m[0][on].tobytes() == hs[0][on].tobytes() and tb.bitwise_equal(m[1][on], hs[1][on])
            if bounded:
                assert np.all(m[2][off] == 0x5A) and m[2][on].tobytes() == hs[2][on].tobytes()
            lam = np.ascontiguousarray(hs[1]["lambda_"])
            u = cam_unc(dc, lk, hs[0], lam, hs[2], want=("cov", "var", "factors"), scale=None)
            um = cam_unc_device(dc, lk, hs[0], lam, hs[2], mask, st)
            assert u["rc"] == 0 and np.all(um["status"][off] == BATCH_UNC_SKIPPED) and np.all(um["cov"][off] == GUARD)
            for k in ("cov", "var", "factors", "scale", "lam", "status"):
                assert np.ascontiguousarray(u[k][on]).tobytes() == np.ascontiguousarray(um[k][on]).tobytes(), k


# ---------------------------------------------------------------- 9. shared pixels
@LK
def test_shared_pixels(lk):
    case = (MODEL_GAUSS2D_ELLIPTIC, (7, 7))
    _, w, h = mz.case_shape(case)
    bt = po.batch((case, "high"))
    cal = calibration(w, h, 7, readvar="noise")
    # every window inside one 10 x 10 region of the sensor, and problems 1 and 2 the same problem
    rng = np.random.default_rng(41)
    cal["origin"] = np.stack([20 + rng.integers(0, 4, size=B), 30 + rng.integers(0, 4, size=B)], axis=1).astype(np.int32)
    cal["origin"][2] = cal["origin"][1]
    raw = readings(bt["y"], cal, w, h, DATA_U16)
    raw[2] = raw[1]
    p0, lo, hi = bt["p0"].copy(), bt["lo"].copy(), bt["hi"].copy()
    p0[2], lo[2], hi[2] = p0[1], lo[1], hi[1]
    dc = DevCamera(bt, raw, DATA_U16, cal)
    for bounded in (False, True):
        p, res, held = cam_solve(dc, p0, lk, lo, hi, bounded)
        assert p[1].tobytes() == p[2].tobytes() and tb.bitwise_equal(res[1:2], res[2:3])
        for b in range(B):
            one = DevCamera(bt, raw[b:b + 1], DATA_U16, dict(cal, origin=cal["origin"][b:b + 1]))
            q, rs, hd = cam_solve(one, p0[b:b + 1], lk, lo[b:b + 1], hi[b:b + 1], bounded)
            assert q.tobytes() == p[b:b + 1].tobytes() and tb.bitwise_equal(rs, res[b:b + 1]), (b, bounded)
            if bounded:
                assert hd.tobytes() == held[b:b + 1].tobytes()
