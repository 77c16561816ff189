"""The built-in fit models of the batch solver on the GPU: dogleg_amd_batch_model_callback (the adapter) and the fused solve
dogleg_amd_optimize_dense_batch_model[_device].  The batches, their bounds and their seeds: tests/batch_models_np.py; what the
oracle's tables contain is asserted in tests/test_dense_batch_model_cpu.py.

1. The adapter's rows against the NumPy restatement.  The device's exp and NumPy's differ in the last place, so this is a
   tolerance: the largest deviation over all cases and variants, relative to the largest magnitude in that problem's x and in that
   column of J, MEASURED on an MI355X, is ROWS_MEASURED = 5.0e-14 below; asserted is 16 times that, ROWS_TOL = 8.0e-13.  The
   figure of a run is printed before it is asserted.  dogleg_amd_check_jacobian_device_batch passes on the adapter for every kind
   at rtol = 1e-6, atol = 1e-7: its central differences over delta = 1e-6 carry eps |f| / delta = 2e-9 of rounding on data of
   size 10 and about delta^2 / 24 times the third derivative, 1e-11, of truncation.
2. The defining property: every output of the fused solve has the bits of the same solve through the adapter.  No tolerance.
3. Against the NumPy oracle (tests/batch_bounds_oracle.py on the restatement): status, iterations, evaluations, lambda and held
   equal, |p - p_oracle|_inf <= 1e-10 (tests/parity.py STEP_TOL), norm2_x and the trust region to 1e-8 relative.
4. to 7.: constant cost, failures stay alone, position independence, composition with the _fit uncertainty call: bit for bit."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BATCH_NOT_RUN, MODEL_EXPDECAY, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC,
                                       MODEL_NSTATE)
from tests import batch_models_np as mz
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu

ROWS_MEASURED = 5.0e-14        # x, J of the adapter against NumPy, scaled as above: the largest figure of a run on an MI355X (gauss1d-5;
                               # the other cases 2.1e-14 .. 4.8e-14: x = s (f - y) cancels, its error is that of f, about 10 times x)
ROWS_TOL = 16 * ROWS_MEASURED
REL_TOL = tb.REL_SCALAR_TOL
GUARD, PAD, RSIZE = td.GUARD, td.PAD, td.RSIZE
OFF = (0, 32, 64)              # the problems an active mask leaves out
# (t_mode, with_scale) of a case's data
VARIANTS_1D = [(None, False), (None, True), ("shared", False), ("each", True)]
VARIANTS_2D = [(None, False), (None, True)]


def variants(case):
    return VARIANTS_2D if mz.is_2d(case[0]) else VARIANTS_1D


class DevModel:
    """a batch's data in device memory and its dogleg_amd_batch_model_t; cb, cookie, N, M: the adapter on it"""

    def __init__(self, bt, y=None):
        self.bt = bt
        self.y = capi.DeviceArray(bt["y"] if y is None else y)
        self.t = None if bt["t"] is None else capi.DeviceArray(bt["t"])
        self.scale = None if bt["scale"] is None else capi.DeviceArray(bt["scale"])
        self.rec = capi.batch_model(bt["kind"], self.y, bt["M"], bt["width"], bt["height"], self.t, bt["t_mode"] == "each", self.scale)
        self.cb, self.cookie, self.N, self.M = capi.batch_model_callback(self.rec)


def adapter(dm, p0, lo=None, hi=None, bounded=False):
    """the solve through the adapter callback, host pointers: (p, results, held or None)"""
    if bounded:
        rc, p, res, held, _ = capi.optimize_dense_batch_bounded(p0, dm.N, dm.M, dm.cb, dm.cookie, lo, hi, None, mz.params())
    else:
        (rc, p, res), held = capi.optimize_dense_batch(p0, dm.N, dm.M, dm.cb, dm.cookie, mz.params()), None
    assert rc == 0
    return p, res, held


def fused(dm, p0, lo=None, hi=None, bounded=False):
    """the fused solve, host pointers; checks the constant cost: no invocation of the adapter, rounds = the most evaluations"""
    before = capi.batch_model_callback_invocations()
    rc, p, res, held = capi.optimize_dense_batch_model(p0, dm.rec, lo, hi, mz.params(), bounded=bounded)
    assert rc == 0
    stats = capi.batch_last_stats()
    assert capi.batch_model_callback_invocations() == before
    assert stats["rounds"] == int(res["evaluations"].max()) and stats["ms_callback"] == 0.0
    return p, res, held


def device_route(dm, p0, lo, hi, bounded, mask, use_fused):
    """either solve through its _device entry point: (p, results, lambda, held or None)"""
    nb, N = p0.shape
    P, R, Lm = td.Buf(p0), td.Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8)), td.Buf(np.full(nb, GUARD))
    A = td.mask_dev(mask)
    Lo, Hi = (td.Buf(a) if bounded and a is not None else None for a in (lo, hi))
    H = td.Buf(np.full((nb, N), 0x5A, dtype=np.uint8)) if bounded else None
    ptr = lambda b: None if b is None else b.ptr
    if use_fused:
        before = capi.batch_model_callback_invocations()
        rc = capi.optimize_dense_batch_model_device(P.ptr, nb, dm.rec, mz.params(), R.ptr, ptr(Lo), ptr(Hi), ptr(H), Lm.ptr, ptr(A),
                                                    bounded=bounded)
        assert capi.batch_model_callback_invocations() == before
    elif bounded:
        rc = capi.optimize_dense_batch_bounded_device(P.ptr, nb, dm.N, dm.M, dm.cb, dm.cookie, mz.params(), None, ptr(Lo), ptr(Hi),
                                                      ptr(H), R.ptr, Lm.ptr, None, ptr(A))
    else:
        rc = capi.optimize_dense_batch_device(P.ptr, nb, dm.N, dm.M, dm.cb, dm.cookie, mz.params(), R.ptr, Lm.ptr, ptr(A))
    assert rc == 0
    return P.get(), td.results_of(R, nb), Lm.get(), None if H is None else H.get()


def same_bits(a, b, what):
    """(p, results, [lambda,] held) of two solves"""
    assert a[0].tobytes() == b[0].tobytes(), f"{what}: p"
    assert tb.bitwise_equal(a[1], b[1]), f"{what}: the results"
    for k in range(2, len(a)):
        assert (a[k] is None) == (b[k] is None), what
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes(), f"{what}: output {k}"


# ---------------------------------------------------------------- 1. the adapter's rows
def adapter_rows(dm, p):
    nb, N, M = p.shape[0], dm.N, dm.M
    P, X, J = capi.DeviceArray(p), td.Buf(np.full((nb, M), GUARD)), td.Buf(np.full((nb, M, N), GUARD))
    live = capi.DeviceArray(np.ones(nb, dtype=np.uint8))
    capi.lib().dogleg_amd_batch_model_callback(P.ptr, X.ptr, J.ptr, live.ptr, nb, None, dm.cookie)
    return X.get(), J.get()


@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_adapter_rows_against_numpy(case):
    worst = 0.0
    for t_mode, with_scale in variants(case):
        bt = mz.batch(case, t_mode=t_mode, with_scale=with_scale)
        dm = DevModel(bt)
        for p in (bt["p0"], bt["truth"]):
            x, J = adapter_rows(dm, p)
            for b in range(mz.B):
                xn, Jn = mz.host_model(bt, b).eval(p[b])
                dx = float(np.max(np.abs(x[b] - xn))) / float(np.max(np.abs(xn)))
                dJ = float(np.max(np.max(np.abs(J[b] - Jn), axis=0) / np.max(np.abs(Jn), axis=0)))
                worst = max(worst, dx, dJ)
    print(f"{mz.case_id(case)}: largest scaled deviation of the adapter's x and J from NumPy {worst:.3g} (asserted {ROWS_TOL:.3g})")
    assert worst <= ROWS_TOL


@pytest.mark.parametrize("kind", sorted(MODEL_NSTATE), ids=lambda k: mz.KIND_NAMES[k])
def test_check_jacobian_passes_on_the_adapter(kind):
    case = next(c for c in mz.CASES if c[0] == kind and mz.case_shape(c)[0] > 40)
    for t_mode, with_scale in variants(case):
        bt = mz.batch(case, t_mode=t_mode, with_scale=with_scale)
        dm = DevModel(bt)
        out = capi.check_jacobian_device_batch(bt["p0"], dm.N, dm.M, dm.cb, dm.cookie, rtol=1e-6, atol=1e-7)
        assert out["rc"] == 0 and not out["bad"], (mz.case_id(case), t_mode, with_scale, out["bad"][:3])


# ---------------------------------------------------------------- 2. the defining property
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_fused_solve_has_the_adapter_routes_bits(case):
    mask = np.ones(mz.B, dtype=np.uint8)
    mask[list(OFF)] = 0
    for t_mode, with_scale in variants(case):
        bt = mz.batch(case, t_mode=t_mode, with_scale=with_scale)
        dm = DevModel(bt)
        p0, lo, hi = bt["p0"], bt["lo"], bt["hi"]
        for bounded in (False, True):
            what = f"{mz.case_id(case)}, t {t_mode}, scale {with_scale}, bounded {bounded}"
            a, f = adapter(dm, p0, lo, hi, bounded), fused(dm, p0, lo, hi, bounded)
            same_bits(a, f, what + ", host pointers")
            assert np.all(f[1]["status"] != BATCH_FAILED), what
            if bounded:
                assert np.all(f[0] >= lo) and np.all(f[0] <= hi) and f[2].max() <= 2
            for m in (None, mask):
                da, df = (device_route(dm, p0, lo, hi, bounded, m, use_fused) for use_fused in (False, True))
                same_bits(da, df, what + f", device, mask {m is not None}")
                if m is None:
                    # the two entry points of the fused solve agree, and lambda_dev is the results' lambda
                    same_bits((f[0], f[1], f[2]), (df[0], df[1], df[3]), what + ", device against host pointers")
                    assert df[2].tobytes() == np.ascontiguousarray(df[1]["lambda_"]).tobytes()
                else:
                    on, off = np.flatnonzero(m), list(OFF)
                    # a problem that is not run keeps p and held and gets the NOT_RUN record; the others: the full batch's bits
                    assert df[0][off].tobytes() == p0[off].tobytes() and np.all(df[2][off] == 0.0)
                    r = df[1][off]
                    assert np.all(r["status"] == BATCH_NOT_RUN) and np.all(r["norm2_x"] == -1.0) and not r["evaluations"].any()
                    assert not r["iterations"].any() and not r["trustregion"].any() and not r["lambda_"].any()
                    assert df[0][on].tobytes() == f[0][on].tobytes() and tb.bitwise_equal(df[1][on], f[1][on])
                    if bounded:
                        assert np.all(df[3][off] == 0x5A) and df[3][on].tobytes() == f[2][on].tobytes()


# ---------------------------------------------------------------- 3. against the NumPy oracle
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_against_the_oracle(case, bounded):
    orc = mz.oracle_table(case, bounded)
    assert min(o["margin"] for o in orc) > mz.MARGIN_FLOOR
    bt = mz.batch(case)
    p, res, held = fused(DevModel(bt), bt["p0"], bt["lo"], bt["hi"], bounded)
    nb = mz.B
    dp = max(float(np.max(np.abs(p[b] - orc[b]["p"]))) for b in range(nb))
    dn = max(abs(res["norm2_x"][b] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for b in range(nb))
    dt = max(abs(res["trustregion"][b] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for b in range(nb))
    print(f"{mz.case_id(case)}, bounded {bounded}: max |p - p_oracle| {dp:.3g}, norm2_x rel {dn:.3g}, trust region rel {dt:.3g}")
    for b in range(nb):
        o = orc[b]
        got = (int(res["status"][b]), int(res["iterations"][b]), int(res["evaluations"][b]), float(res["lambda_"][b]))
        assert got == (o["status"], o["iterations"], o["evaluations"], o["lambda_"]), (b, got)
        if bounded:
            assert held[b].tolist() == o["held"].tolist(), b
    assert dp <= STEP_TOL and dn <= REL_TOL and dt <= REL_TOL


# ---------------------------------------------------------------- 4. constant cost
def test_constant_cost(monkeypatch):
    """one launch and one read-back a round whatever B is: the rounds are the most evaluations of a problem, the adapter never
    runs, and with the timing on the callback's share is exactly 0 while the library's is not"""
    monkeypatch.setenv("DOGLEG_AMD_BATCH_TIMING", "1")
    case = (MODEL_GAUSS2D, (7, 7))
    for nb in (1, mz.B):
        bt = mz.batch(case, nb=nb)
        p, res, _ = fused(DevModel(bt), bt["p0"])
        stats = capi.batch_last_stats()
        assert stats["rounds"] == int(res["evaluations"].max()) and stats["ms_callback"] == 0.0 and stats["ms_library"] > 0.0


# ---------------------------------------------------------------- 5. failures stay alone
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_failures_stay_alone(bounded):
    case = (MODEL_GAUSS2D_ELLIPTIC, (7, 7))
    bt = mz.batch(case)
    clean = fused(DevModel(bt), bt["p0"], bt["lo"], bt["hi"], bounded)
    p0, y = bt["p0"].copy(), bt["y"].copy()
    p0[5, 3] = 0.0                  # sigma_x = 0 at the start (problem 5 has no bounds)
    y[40, 17] = np.nan              # a NaN datum
    dm = DevModel(bt, y=y)
    p, res, held = fused(dm, p0, bt["lo"], bt["hi"], bounded)
    same_bits(adapter(dm, p0, bt["lo"], bt["hi"], bounded), (p, res, held), "with the two failures")
    bad, good = [5, 40], [b for b in range(mz.B) if b not in (5, 40)]
    assert np.all(res["status"][bad] == BATCH_FAILED) and np.all(res["norm2_x"][bad] == -1.0)
    assert np.all(res["evaluations"][bad] == 1)
    assert p[bad].tobytes() == p0[bad].tobytes()
    assert p[good].tobytes() == clean[0][good].tobytes() and tb.bitwise_equal(res[good], clean[1][good])
    if bounded:
        assert not held[bad].any() and held[good].tobytes() == clean[2][good].tobytes()


# ---------------------------------------------------------------- 6. position independence
@pytest.mark.parametrize("case", [(MODEL_EXPDECAY, 65), (MODEL_GAUSS2D, (8, 8))], ids=mz.case_id)
def test_position_independence(case):
    bt = mz.batch(case, with_scale=True)
    for bounded in (False, True):
        full = fused(DevModel(bt), bt["p0"], bt["lo"], bt["hi"], bounded)
        rev = {k: (v[::-1].copy() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == mz.B else v) for k, v in bt.items()}
        r = fused(DevModel(rev), rev["p0"], rev["lo"], rev["hi"], bounded)
        same_bits(full, tuple(None if a is None else a[::-1].copy() for a in r), f"reversed, bounded {bounded}")
        for b in (0, 3, 64):
            one = {k: (v[b:b + 1].copy() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == mz.B else v) for k, v in bt.items()}
            s = fused(DevModel(one), one["p0"], one["lo"], one["hi"], bounded)
            same_bits(tuple(None if a is None else a[b:b + 1] for a in full), s, f"problem {b} alone, bounded {bounded}")


# ---------------------------------------------------------------- 7. composition
def test_composition_with_the_fit_uncertainty():
    """held and lambda of a fused bounded solve in the fit record of dogleg_amd_dense_batch_uncertainty_fit through the adapter:
    the bits of the same call behind the adapter-route solve"""
    case = (MODEL_GAUSS2D, (7, 7))
    bt = mz.batch(case)
    dm = DevModel(bt)
    outs = []
    for solve in (adapter, fused):
        p, res, held = solve(dm, bt["p0"], bt["lo"], bt["hi"], True)
        assert held.any()
        out = capi.dense_batch_uncertainty(p, dm.N, dm.M, dm.cb, dm.cookie, lam=res["lambda_"], want=("cov", "var", "factors"),
                                           fit=capi.batch_fit(held=held))
        assert out["rc"] == 0 and not out["status"].any()
        outs.append(out)
    for k in ("cov", "var", "factors", "scale", "lam", "status"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
    h = outs[1]["var"][held != 0]
    assert h.size and not h.any()                  # a held variable has variance 0 in the fit
