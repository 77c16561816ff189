"""The Poisson maximum-likelihood fit of the built-in models on the GPU: dogleg_amd_optimize_dense_batch_model_mle[_device] and
dogleg_amd_batch_model_fisher_callback.  The tables, their bounds and their seeds: tests/batch_poisson_oracle.py; what the
oracle's tables contain is asserted in tests/test_dense_batch_poisson_cpu.py.

1. Against the NumPy oracle over every table, plain and bounded: status, iterations, evaluations, lambda and held equal; F and the
   trust region to REL_SCALAR_TOL = 1e-8 relative; |p - p_oracle| <= STEP_TOL max(1, |p_oracle|) per component with STEP_TOL =
   1e-10 (tests/parity.py; relative because the amplitudes here reach 400).  The figures of a run are printed before they are
   asserted.
   MEASURED on an MI355X over the 56 tables: |p - p_oracle| / max(1, |p_oracle|) at most 3.2e-13 (gauss1d-5-low, plain), F
   relative at most 4.9e-10 (gauss1d-5-high: one degree of freedom, a small F summed from terms that cancel), the trust region
   relative at most 2.1e-10; no status, count, lambda or held differed.  The Fisher callback's rows: at most 9.2e-15; the
   inverse Fisher information: at most 9.7e-14.
2. The device twin has the bits of the host twin, with an active mask and on a caller's stream.
3. likelihood = GAUSS has the bits of dogleg_amd_optimize_dense_batch_model, plain and bounded, both twins.
4. An infeasible start, a NaN datum and a negative datum each end FAILED alone; a problem infeasible only at trial points ends
   as the oracle says.
5. The Fisher callback: its rows against NumPy (ROWS_TOL = 1e-13, scaled as in the CPU test; the device's exp, log and the
   rounding of f differ from NumPy's in the last places as the CPU test's header does), (H + lambda I)^-1 through the
   uncertainty call, exact zeros for held variables, and the refusal by every solve entry point.
6. The estimator differs from least squares on the same data, and its deviance is the smaller."""
import ctypes as C

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BATCH_JTX, BATCH_NOT_RUN, BATCH_SMALL_STEP, BatchLoss, LOSS_TRIVIAL,
                                       MODEL_GAUSS1D, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC, MODEL_EXPDECAY, LIKELIHOOD_GAUSS,
                                       LIKELIHOOD_POISSON)
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_model_gpu as tm
from tests.parity import STEP_TOL
from tests.test_dense_batch_poisson_cpu import poisson_rows_np, scaled

pytestmark = pytest.mark.gpu

REL_TOL = tb.REL_SCALAR_TOL
ROWS_TOL = 1e-13
GUARD, PAD, RSIZE = td.GUARD, td.PAD, td.RSIZE
OFF = (0, 32, 64)
# one low-count table a kind for the bit-for-bit tests, each with infeasible trials in its plain table, and a high-count one
TWIN_TABLES = [((MODEL_EXPDECAY, 5), "low"), ((MODEL_GAUSS1D, 65), "low"), ((MODEL_GAUSS2D, (7, 7)), "low"),
               ((MODEL_GAUSS2D_ELLIPTIC, (7, 7)), "low"), ((MODEL_GAUSS2D, (8, 8)), "high")]


def mle(dm, p0, lo=None, hi=None, bounded=False, likelihood=LIKELIHOOD_POISSON, prm=None):
    """the fused solve with a likelihood, host pointers: (p, results, held or None); checks the constant cost"""
    before = capi.batch_model_callback_invocations()
    rc, p, res, held = capi.optimize_dense_batch_model_mle(p0, dm.rec, likelihood, lo, hi, po.params() if prm is None else prm,
                                                           bounded=bounded)
    assert rc == 0
    stats = capi.batch_last_stats()
    assert capi.batch_model_callback_invocations() == before
    assert stats["rounds"] == int(res["evaluations"].max()) and stats["ms_callback"] == 0.0
    return p, res, held


def mle_device(dm, p0, lo, hi, bounded, mask=None, likelihood=LIKELIHOOD_POISSON, prm=None, stream=None):
    """the _device twin: (p, results, held or None, lambda)"""
    nb, N = p0.shape
    P, R, Lm = td.Buf(p0), td.Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8)), td.Buf(np.full(nb, GUARD))
    A = td.mask_dev(mask)
    Lo, Hi = (td.Buf(a) if bounded and a is not None else None for a in (lo, hi))
    H = td.Buf(np.full((nb, N), 0x5A, dtype=np.uint8)) if bounded else None
    ptr = lambda b: None if b is None else b.ptr
    rc = capi.optimize_dense_batch_model_mle_device(P.ptr, nb, dm.rec, likelihood, po.params() if prm is None else prm, R.ptr,
                                                    ptr(Lo), ptr(Hi), ptr(H), Lm.ptr, ptr(A), stream, bounded=bounded)
    assert rc == 0
    return P.get(), td.results_of(R, nb), None if H is None else H.get(), Lm.get()


# ---------------------------------------------------------------- 1. against the NumPy oracle
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
@pytest.mark.parametrize("table", po.TABLES, ids=po.table_id)
def test_against_the_oracle(table, bounded):
    orc = po.oracle_table(table, bounded)
    assert min(o["margin"] for o in orc) > po.MARGIN_FLOOR
    bt = po.batch(table)
    p, res, held = mle(tm.DevModel(bt), bt["p0"], bt["lo"], bt["hi"], bounded)
    nb = po.B
    dp = max(float(np.max(np.abs(p[b] - orc[b]["p"]) / np.maximum(1.0, np.abs(orc[b]["p"])))) for b in range(nb))
    dn = max(abs(res["norm2_x"][b] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for b in range(nb))
    dt = max(abs(res["trustregion"][b] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for b in range(nb))
    print(f"{po.table_id(table)}, bounded {bounded}: max |p - p_oracle| / max(1, |p_oracle|) {dp:.3g}, F rel {dn:.3g}, trust region "
          f"rel {dt:.3g}, infeasible trials {sum(o['infeasible'] for o in orc)}")
    for b in range(nb):
        o = orc[b]
        got = (int(res["status"][b]), int(res["iterations"][b]), int(res["evaluations"][b]), float(res["lambda_"][b]))
        assert got == (o["status"], o["iterations"], o["evaluations"], o["lambda_"]), (b, got)
        if bounded:
            assert held[b].tolist() == o["held"].tolist(), b
    assert dp <= STEP_TOL and dn <= REL_TOL and dt <= REL_TOL


# ---------------------------------------------------------------- 2. the device twin
@pytest.fixture(scope="module")
def stream():
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0 and s.value
    yield s.value
    assert hip.hipStreamDestroy(s) == 0


@pytest.mark.parametrize("table", TWIN_TABLES, ids=po.table_id)
def test_device_twin_has_the_host_twins_bits(table, stream):
    mask = np.ones(po.B, dtype=np.uint8)
    mask[list(OFF)] = 0
    on, off = np.flatnonzero(mask), list(OFF)
    bt = po.batch(table)
    dm = tm.DevModel(bt)
    p0, lo, hi = bt["p0"], bt["lo"], bt["hi"]
    for bounded in (False, True):
        what = f"{po.table_id(table)}, bounded {bounded}"
        h = mle(dm, p0, lo, hi, bounded)
        for st in (None, stream):
            d = mle_device(dm, p0, lo, hi, bounded, stream=st)
            tm.same_bits(h, d[:3], what + f", stream {st is not None}")
            assert d[3].tobytes() == np.ascontiguousarray(d[1]["lambda_"]).tobytes()
            m = mle_device(dm, p0, lo, hi, bounded, mask=mask, stream=st)
            assert m[0][off].tobytes() == p0[off].tobytes() and np.all(m[3][off] == 0.0)
            r = m[1][off]
            assert np.all(r["status"] == BATCH_NOT_RUN) and np.all(r["norm2_x"] == -1.0) and not r["evaluations"].any()
            assert m[0][on].tobytes() == h[0][on].tobytes() and tb.bitwise_equal(m[1][on], h[1][on]), what
            if bounded:
                assert np.all(m[2][off] == 0x5A) and m[2][on].tobytes() == h[2][on].tobytes()


# ---------------------------------------------------------------- 3. GAUSS is the fused solve
@pytest.mark.parametrize("case", [(MODEL_EXPDECAY, 65), (MODEL_GAUSS1D, 150), (MODEL_GAUSS2D, (7, 7)), (MODEL_GAUSS2D_ELLIPTIC, (9, 5))],
                         ids=mz.case_id)
def test_gauss_is_the_fused_solve(case):
    for with_scale in (False, True):
        bt = mz.batch(case, with_scale=with_scale)
        dm = tm.DevModel(bt)
        p0, lo, hi = bt["p0"], bt["lo"], bt["hi"]
        for bounded in (False, True):
            what = f"{mz.case_id(case)}, scale {with_scale}, bounded {bounded}"
            tm.same_bits(tm.fused(dm, p0, lo, hi, bounded), mle(dm, p0, lo, hi, bounded, LIKELIHOOD_GAUSS, mz.params()), what)
            a = tm.device_route(dm, p0, lo, hi, bounded, None, True)
            b = mle_device(dm, p0, lo, hi, bounded, likelihood=LIKELIHOOD_GAUSS, prm=mz.params())
            tm.same_bits((a[0], a[1], a[3], a[2]), b, what + ", device")


# ---------------------------------------------------------------- 4. failures, and infeasible trial points
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_failures_stay_alone(bounded):
    table = ((MODEL_GAUSS2D_ELLIPTIC, (7, 7)), "high")
    bt = po.batch(table)
    clean = mle(tm.DevModel(bt), bt["p0"], bt["lo"], bt["hi"], bounded)
    assert np.all(clean[1]["status"] != BATCH_FAILED)
    p0, y = bt["p0"].copy(), bt["y"].copy()
    p0[5, 5] = -20.0                # an infeasible start: the offset below minus the peak's flanks (problem 5 has no bounds)
    y[40, 17] = np.nan              # a NaN datum
    y[22, 3] = -1.0                 # a negative datum
    p, res, held = mle(tm.DevModel(bt, y=y), p0, bt["lo"], bt["hi"], bounded)
    bad = [5, 22, 40]
    good = [b for b in range(po.B) if b not in bad]
    assert np.all(res["status"][bad] == BATCH_FAILED) and np.all(res["norm2_x"][bad] == -1.0)
    assert np.all(res["evaluations"][bad] == 1) and not res["iterations"][bad].any()
    assert p[bad].tobytes() == p0[bad].tobytes()
    assert p[good].tobytes() == clean[0][good].tobytes() and tb.bitwise_equal(res[good], clean[1][good])
    if bounded:
        assert not held[bad].any() and held[good].tobytes() == clean[2][good].tobytes()


def test_infeasible_only_at_trial_points():
    """the problems of the table with the most infeasible trials that meet one, as a batch of their own: none starts infeasible,
    each ends as the oracle says"""
    table = ((MODEL_GAUSS1D, 5), "low")
    orc = po.oracle_table(table, False)
    idx = [b for b in range(po.B) if orc[b]["infeasible"] > 0]
    assert len(idx) >= 5 and sum(orc[b]["infeasible"] for b in idx) >= 50
    bt = po.batch(table)
    sub = {k: (v[idx].copy() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == po.B else v) for k, v in bt.items()}
    for b in range(len(idx)):
        assert po.poisson_products(mz.host_model(sub, b))(sub["p0"][b])[5], "feasible at the start"
    p, res, _ = mle(tm.DevModel(sub), sub["p0"])
    for k, b in enumerate(idx):
        o = orc[b]
        got = (int(res["status"][k]), int(res["iterations"][k]), int(res["evaluations"][k]), float(res["lambda_"][k]))
        assert got == (o["status"], o["iterations"], o["evaluations"], o["lambda_"]), (b, got)
        assert o["status"] in (BATCH_JTX, BATCH_SMALL_STEP) and o["evaluations"] > o["iterations"] + 1
        assert np.max(np.abs(p[k] - o["p"]) / np.maximum(1.0, np.abs(o["p"]))) <= STEP_TOL
        assert abs(res["norm2_x"][k] - o["norm2_x"]) <= REL_TOL * abs(o["norm2_x"])


# ---------------------------------------------------------------- 5. the Fisher callback
def fisher_rows(dm, p):
    nb, N, M = p.shape[0], dm.N, dm.M
    P, X, J = capi.DeviceArray(p), td.Buf(np.full((nb, M), GUARD)), td.Buf(np.full((nb, M, N), GUARD))
    live = capi.DeviceArray(np.ones(nb, dtype=np.uint8))
    capi.lib().dogleg_amd_batch_model_fisher_callback(P.ptr, X.ptr, J.ptr, live.ptr, nb, None, C.c_void_p(C.addressof(dm.rec)))
    return X.get(), J.get()


@pytest.mark.parametrize("table", po.TABLES, ids=po.table_id)
def test_fisher_rows_against_numpy(table):
    bt = po.batch(table)
    dm = tm.DevModel(bt)
    worst = 0.0
    for p in (bt["p0"], bt["truth"]):
        x, J = fisher_rows(dm, p)
        for b in range(po.B):
            xn, Jn, _, ok = poisson_rows_np(mz.host_model(bt, b), p[b])
            assert ok.all()
            worst = max(worst, scaled(x[b], xn, 0), scaled(J[b], Jn, 0))
    print(f"{po.table_id(table)}: largest scaled deviation of the Fisher callback's rows from NumPy {worst:.3g} (asserted {ROWS_TOL:.3g})")
    assert worst <= ROWS_TOL


def test_fisher_rows_of_an_infeasible_point_are_nan():
    table = ((MODEL_GAUSS2D, (7, 7)), "low")
    bt = po.batch(table, nb=3)
    p = bt["truth"].copy()
    p[1, 4] = -0.5
    x, J = fisher_rows(tm.DevModel(bt), p)
    _, _, _, ok = poisson_rows_np(mz.host_model(bt, 1), p[1])
    assert 0 < ok.sum() < ok.size
    assert np.all(np.isnan(x[1][~ok])) and np.all(np.isnan(J[1][~ok])) and np.all(np.isfinite(x[1][ok])) and np.all(np.isfinite(J[1][ok]))
    assert np.all(np.isfinite(x[[0, 2]])) and np.all(np.isfinite(J[[0, 2]]))


@pytest.mark.parametrize("table", [((MODEL_GAUSS2D, (7, 7)), "low"), ((MODEL_EXPDECAY, 65), "high")], ids=po.table_id)
def test_uncertainty_through_the_fisher_callback(table):
    """(H + lambda I)^-1 at the fused optimum, plain; with held of the bounded solve in the fit record, the inverse on the free set
    and exact zeros in the held rows and columns"""
    bt = po.batch(table)
    dm = tm.DevModel(bt)
    cb, cookie, N, M = capi.batch_model_fisher_callback(dm.rec)
    for bounded in (False, True):
        p, res, held = mle(dm, bt["p0"], bt["lo"], bt["hi"], bounded)
        assert not bounded or held.any()
        out = capi.dense_batch_uncertainty(p, N, M, cb, cookie, lam=res["lambda_"].copy(), want=("cov", "var"),
                                           fit=capi.batch_fit(held=held) if bounded else None)
        assert out["rc"] == 0 and not out["status"].any()
        worst = 0.0
        for b in range(po.B):
            _, _, H, _, _, ok = po.poisson_products(mz.host_model(bt, b))(p[b])
            assert ok
            free = np.ones(N, dtype=bool) if not bounded else held[b] == 0
            want = np.zeros((N, N))
            want[np.ix_(free, free)] = np.linalg.inv((H + out["lam"][b] * np.eye(N))[np.ix_(free, free)])
            cov = out["cov"][b]
            if bounded:
                assert not cov[~free, :].any() and not cov[:, ~free].any() and not out["var"][b][~free].any()
            sd = np.sqrt(np.diag(want)[free])
            worst = max(worst, float(np.max(np.abs(cov - want)[np.ix_(free, free)] / np.outer(sd, sd))))
            assert out["var"][b].tobytes() == np.ascontiguousarray(np.diag(cov)).tobytes()
        print(f"{po.table_id(table)}, bounded {bounded}: (H + lambda I)^-1 against NumPy, relative to sqrt(S_ii S_jj): {worst:.3g} "
              f"(asserted {REL_TOL:.3g})")
        assert worst <= REL_TOL


def test_jacobian_check_reports_the_fisher_callback():
    """its J~ is not the derivative of its x~, and the check says so"""
    bt = po.batch(((MODEL_GAUSS2D, (7, 7)), "high"), nb=3)
    dm = tm.DevModel(bt)
    cb, cookie, N, M = capi.batch_model_fisher_callback(dm.rec)
    out = capi.check_jacobian_device_batch(bt["p0"], N, M, cb, cookie, rtol=1e-6, atol=1e-7)
    assert out["bad"]


def test_every_solve_entry_point_refuses_the_fisher_callback(capfd):
    bt = po.batch(((MODEL_EXPDECAY, 64), "high"), nb=4)
    dm = tm.DevModel(bt)
    cb, cookie, N, M = capi.batch_model_fisher_callback(dm.rec)
    nb = 4
    p0 = bt["p0"]
    P, R = td.Buf(p0), td.Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8))
    Hd = td.Buf(np.full((nb, N), 0x5A, dtype=np.uint8))
    trivial = BatchLoss(LOSS_TRIVIAL, 1.0, 1)
    prm = po.params()
    before = capi.batch_model_callback_invocations()
    for name, call in (
            ("dogleg_amd_optimize_dense_batch", lambda: capi.optimize_dense_batch(p0, N, M, cb, cookie, prm)[0]),
            ("dogleg_amd_optimize_dense_batch_robust", lambda: capi.optimize_dense_batch_robust(p0, N, M, cb, cookie, trivial, prm)[0]),
            ("dogleg_amd_optimize_dense_batch_bounded",
             lambda: capi.optimize_dense_batch_bounded(p0, N, M, cb, cookie, bt["lo"], bt["hi"], None, prm)[0]),
            ("dogleg_amd_optimize_dense_batch_device", lambda: capi.optimize_dense_batch_device(P.ptr, nb, N, M, cb, cookie, prm, R.ptr)),
            ("dogleg_amd_optimize_dense_batch_robust_device",
             lambda: capi.optimize_dense_batch_robust_device(P.ptr, nb, N, M, cb, cookie, prm, trivial, R.ptr)),
            ("dogleg_amd_optimize_dense_batch_bounded_device",
             lambda: capi.optimize_dense_batch_bounded_device(P.ptr, nb, N, M, cb, cookie, prm, None, None, None, Hd.ptr, R.ptr))):
        capfd.readouterr()
        assert call() == -1, name
        assert name + ": dogleg_amd_batch_model_fisher_callback is no callback of a solve" in capfd.readouterr().err, name
    assert P.get().tobytes() == p0.tobytes() and np.all(R.get() == PAD) and np.all(Hd.get() == 0x5A)
    assert capi.batch_model_callback_invocations() == before


# ---------------------------------------------------------------- 6. another estimator
def test_the_estimator_differs_from_least_squares():
    """the low-count GAUSS2D 7 x 7 table: the Poisson optimum lies far from the least-squares optimum of the same data, by much more
    than any tolerance above, and its deviance is the smaller"""
    table = ((MODEL_GAUSS2D, (7, 7)), "low")
    bt = po.batch(table)
    dm = tm.DevModel(bt)
    pm, rm, _ = mle(dm, bt["p0"])
    pl, rl, _ = mle(dm, bt["p0"], likelihood=LIKELIHOOD_GAUSS)
    both = [b for b in range(po.B) if rm["status"][b] in (BATCH_JTX, BATCH_SMALL_STEP) and rl["status"][b] in (BATCH_JTX, BATCH_SMALL_STEP)]
    assert len(both) >= po.B // 2
    gap = np.array([np.max(np.abs(pm[b] - pl[b])) for b in both])
    dev_ls = np.array([po.poisson_products(mz.host_model(bt, b))(pl[b])[0] for b in both])
    gain = dev_ls - rm["norm2_x"][both]
    print(f"gap in p between the two estimators: median {np.median(gap):.3g}, smallest {gap.min():.3g}; deviance of the least-squares "
          f"point above that of the Poisson point: median {np.median(gain):.3g}, smallest {gain.min():.3g}")
    assert np.median(gap) > 1e-2 and gap.min() > 1e3 * STEP_TOL
    assert np.all(gain > 0.0) and np.median(gain) > 0.1
