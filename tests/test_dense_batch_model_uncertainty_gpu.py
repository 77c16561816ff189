"""The fused uncertainty and query calls of the built-in models on the GPU: dogleg_amd_dense_batch_model_uncertainty[_device] and
dogleg_amd_dense_batch_model_query_covariance[_device].  The batches, their data variants and the NumPy rows:
tests/batch_model_uncertainty_np.py; what the tables contain is asserted in tests/test_dense_batch_model_uncertainty_cpu.py.

The defining property is that every output has the bits of the call it replaces: dogleg_amd_dense_batch_uncertainty_fit /
_query_covariance_fit (held == NULL: the calls without _fit) through dogleg_amd_batch_model_callback with GAUSS, through
dogleg_amd_batch_model_fisher_callback with POISSON.  No tolerance in 1. to 6.  B = 65; the cases are batch_models_np.CASES, whose
Nmeas lie below, on and above the tile heights 64, 64, 51, 42 of N = 3, 4, 5, 6 (with featureSize 2: 64, 64, 50, 42).

3. (failures stay alone): a problem that fails gets status FAILED and NaN outputs.  A computed scale[b] is NaN where the rows' x is
   not finite (the NaN datum, the infeasible point); sigma = 0 makes J non-finite and leaves x finite (e = exp(-inf) = 0, f = c),
   and a negative lambda fails before the factorisation with finite rows: there the computed scale is the finite number the
   callback route computes, and its bits are asserted equal to that route's like every other output.
7. (against NumPy): the tolerances are imported: COV_TOL and VAR_TOL of tests/test_dense_batch_uncertainty_gpu.py for the
   least-squares tables, REL_TOL of tests/test_dense_batch_poisson_gpu.py for the inverse Fisher information; the largest
   deviation of a run is printed before it is asserted.  MEASURED on an MI355X: at most 1.1e-13 for least squares (gauss1d-5: four
   variables on five rows) against 1e-9, at most 7.4e-11 for the inverse Fisher information (gauss1d-5, low counts) against 1e-8;
   every other table stays below 1e-12."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_UNC_FAILED, BATCH_UNC_OK, BATCH_UNC_SKIPPED, LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON,
                                       MODEL_EXPDECAY, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC, MODEL_NSTATE)
from tests import batch_model_uncertainty_np as mu
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_model_gpu as tm
from tests import test_dense_batch_poisson_gpu as tp
from tests import test_dense_batch_uncertainty_gpu as tu
from tests.test_dense_batch_poisson_gpu import stream          # noqa: F401  (the fixture: a stream that is not the default one)

pytestmark = pytest.mark.gpu

B = mz.B
GUARD = td.GUARD
OFF = (0, 32, 64)              # the problems an active mask leaves out
TILE = {3: 64, 4: 64, 5: 51, 6: 42}
UNC_KEYS = ("cov", "var", "factors", "scale", "lam", "status")
QUERY_KEYS = ("out", "lam", "status")
LK = pytest.mark.parametrize("lk", mu.LIKELIHOODS, ids=lambda k: mu.LK_NAMES[k])


def callback_of(dm, lk):
    """(cb, cookie, N, M) of the callback the fused call replaces"""
    return capi.batch_model_callback(dm.rec) if lk == LIKELIHOOD_GAUSS else capi.batch_model_fisher_callback(dm.rec)


def solve(dm, bt, lk, bounded):
    """(p, lambda, held or None) of the fused solve of the batch"""
    if lk == LIKELIHOOD_GAUSS:
        p, res, held = tm.fused(dm, bt["p0"], bt["lo"], bt["hi"], bounded)
    else:
        p, res, held = tp.mle(dm, bt["p0"], bt["lo"], bt["hi"], bounded)
    return p, np.ascontiguousarray(res["lambda_"]), held


def fit_of(held):
    return None if held is None else capi.batch_fit(held=held)


def unc_replaced(dm, lk, p, lam, held, **kw):
    cb, cookie, N, M = callback_of(dm, lk)
    return capi.dense_batch_uncertainty(p, N, M, cb, cookie, lam=lam, fit=fit_of(held), **kw)


def unc_fused(dm, lk, p, lam, held, **kw):
    """the fused call; checks that no callback ran: the adapter's counter, and 0 ms of callback"""
    before = capi.batch_model_callback_invocations()
    out = capi.dense_batch_model_uncertainty(p, dm.rec, lk, lam=lam, held=held, **kw)
    out["stats"] = capi.batch_uncertainty_last_stats()
    assert capi.batch_model_callback_invocations() == before
    if out["rc"] == 0:
        assert out["stats"]["ms_callback"] == 0.0 and out["stats"]["launches"] == 1 and out["stats"]["syncs"] == 1
    return out


def query_replaced(dm, lk, p, lam, held, Jq, nobs):
    cb, cookie, N, M = callback_of(dm, lk)
    return capi.dense_batch_query_covariance(p, N, M, cb, cookie, Jq, lam=lam, nobs=nobs, fit=fit_of(held))


def query_fused(dm, lk, p, lam, held, Jq, nobs):
    before = capi.batch_model_callback_invocations()
    out = capi.dense_batch_model_query_covariance(p, dm.rec, lk, Jq, lam=lam, nobs=nobs, held=held)
    out["stats"] = capi.batch_uncertainty_last_stats()
    assert capi.batch_model_callback_invocations() == before
    if out["rc"] == 0:
        assert out["stats"]["ms_callback"] == 0.0 and out["stats"]["launches"] == 1 and out["stats"]["syncs"] == 1
    return out


def same(a, b, keys, what, idx=None, nan_equal=False):
    """the outputs `keys` of two calls, bytewise (nan_equal: a NaN equals a NaN, every other value bytewise)"""
    assert a["rc"] == b["rc"], f"{what}: rc {a['rc']}, {b['rc']}"
    for k in keys:
        if a.get(k) is None and b.get(k) is None:
            continue
        x, y = (a[k], b[k]) if idx is None else (a[k][idx], b[k][idx])
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if nan_equal and x.dtype == np.float64:
            nx, ny = np.isnan(x), np.isnan(y)
            assert np.array_equal(nx, ny), f"{what}: the NaNs of {k}"
            x, y = np.where(nx, 0.0, x), np.where(ny, 0.0, y)
        assert x.tobytes() == y.tobytes(), f"{what}: {k}"


# ---------------------------------------------------------------- 1. the bits of the callback route
@LK
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_fused_uncertainty_has_the_callback_routes_bits(case, lk):
    N = MODEL_NSTATE[case[0]]
    M = mz.case_shape(case)[0]
    for t_mode, with_scale in mu.variants(case, lk):
        bt = mu.batch_of(case, lk, t_mode, with_scale)
        dm = tm.DevModel(bt)
        for bounded in (False, True):
            p, lam, held = solve(dm, bt, lk, bounded)
            # (the base variant's tables are the oracle's: that they hold held variables is asserted without a GPU)
            assert not bounded or t_mode is not None or with_scale or held.any()
            for fs in (1, 2):
                for scale in (2.5, None):
                    what = f"{mz.case_id(case)}, {mu.LK_NAMES[lk]}, t {t_mode}, scale {with_scale}, bounded {bounded}, fs {fs}, " \
                           f"scale {'given' if scale else 'computed'}"
                    kw = dict(want=("cov", "var", "factors"), fs=fs, scale=scale)
                    r, f = unc_replaced(dm, lk, p, lam, held, **kw), unc_fused(dm, lk, p, lam, held, **kw)
                    # (a scale to be computed needs Nmeas > Nstate + 1: where the replaced call refuses, so does the fused one)
                    assert r["rc"] == (0 if scale or M > N + 1 else -1), what
                    same(r, f, UNC_KEYS, what)
                    if r["rc"] == 0:
                        assert np.all(f["status"] == BATCH_UNC_OK) and np.all(f["scale"] > 0.0), what
                        if bounded:
                            assert not f["var"][held != 0].any(), what
            # fewer outputs, and no lambda
            for kw in (dict(want=("var",)), dict(want=("cov",)), dict(want=("factors",), scale=1.5)):
                same(unc_replaced(dm, lk, p, lam, held, **kw), unc_fused(dm, lk, p, lam, held, **kw), UNC_KEYS, f"{kw}")
            same(unc_replaced(dm, lk, p, None, held, want=("cov", "var")), unc_fused(dm, lk, p, None, held, want=("cov", "var")),
                 UNC_KEYS, "lambda NULL")


@LK
def test_constant_cost(lk, monkeypatch):
    """one launch, one synchronisation and the same copies whatever B is; with the timing on the callback's share is exactly 0 while
    the library's is not"""
    monkeypatch.setenv("DOGLEG_AMD_BATCH_TIMING", "1")
    case = (MODEL_GAUSS2D, (7, 7))
    counts = {}
    for nb in (5, B):
        bt = mu.batch_of(case, lk, nb=nb)
        dm = tm.DevModel(bt)
        p, lam, held = solve(dm, bt, lk, True)
        out = unc_fused(dm, lk, p, lam, held, fs=2)
        assert out["rc"] == 0
        s = out["stats"]
        assert s["ms_callback"] == 0.0 and s["ms_library"] > 0.0
        counts[nb] = (s["launches"], s["syncs"], s["copies"])
        q = query_fused(dm, lk, p, lam, held, np.ones((nb, 3, 4, MODEL_NSTATE[case[0]])), 10)
        assert q["rc"] == 0 and q["stats"]["ms_callback"] == 0.0 and q["stats"]["ms_library"] > 0.0
        counts[(nb, "q")] = (q["stats"]["launches"], q["stats"]["syncs"], q["stats"]["copies"])
    print(counts)
    assert counts[5] == counts[B] and counts[(5, "q")] == counts[(B, "q")] and counts[B][:2] == (1, 1)


# ---------------------------------------------------------------- 2. the lambda loop
@LK
def test_lambda_loop(lk):
    bt, p = mu.singular_batch(lk, nb=3)
    dm = tm.DevModel(bt)
    lam = np.array([0.0, -1.0, np.nan])
    for held in (None, np.zeros(p.shape, dtype=np.uint8)):
        kw = dict(want=("cov", "var", "factors"), fs=1)
        r, f = unc_replaced(dm, lk, p, lam, held, **kw), unc_fused(dm, lk, p, lam, held, **kw)
        assert f["rc"] == 0
        same(r, f, UNC_KEYS, "the singular problem", nan_equal=True)
        assert f["status"].tolist() == [BATCH_UNC_OK, BATCH_UNC_FAILED, BATCH_UNC_FAILED]
        # lambda moved from 0 to LAMBDA_INITIAL times a power of ten, by the loop's own multiplications
        ladder, v = [], mu.LAMBDA_INITIAL
        for _ in range(40):
            ladder.append(v)
            v *= 10.0
        assert f["lam"][0] in ladder, f["lam"][0]
        assert f["lam"][1] == -1.0 and f["lam"].view(np.uint64)[2] == lam.view(np.uint64)[2]
        assert np.all(np.isfinite(f["cov"][0])) and np.all(np.isnan(f["cov"][1:])) and np.all(np.isnan(f["factors"][1:]))
        Jq = np.random.default_rng(5).standard_normal((3, 3, 4, 5))
        for nobs in (-1, 20):
            rq, fq = query_replaced(dm, lk, p, lam, held, Jq, nobs), query_fused(dm, lk, p, lam, held, Jq, nobs)
            assert fq["rc"] == 0
            same(rq, fq, QUERY_KEYS, f"the singular problem, query, nobs {nobs}", nan_equal=True)
            assert fq["lam"][0] == f["lam"][0] and np.all(np.isnan(fq["out"][1:])) and np.all(np.isfinite(fq["out"][0]))


# ---------------------------------------------------------------- 3. failures stay alone
@LK
@pytest.mark.parametrize("bounded", [False, True], ids=["plain", "bounded"])
def test_failures_stay_alone(lk, bounded):
    case = (MODEL_GAUSS2D_ELLIPTIC, (7, 7))
    bt = mu.batch_of(case, lk)
    dm = tm.DevModel(bt)
    p, lam, held = solve(dm, bt, lk, bounded)
    kw = dict(want=("cov", "var", "factors"), fs=1)
    clean = unc_fused(dm, lk, p, lam, held, **kw)
    assert clean["rc"] == 0 and np.all(clean["status"] == BATCH_UNC_OK)
    p2, lam2, y = p.copy(), lam.copy(), bt["y"].copy()
    y[40, 17] = np.nan              # a NaN datum
    p2[5, 3] = 0.0                  # sigma_x = 0
    lam2[22] = -1.0                 # a negative lambda
    bad, nonfinite_x = [5, 22, 40], [40]
    if lk == LIKELIHOOD_POISSON:
        p2[11, 5] = -20.0           # the offset below minus the peak's flanks: some f_i <= 0
        bad, nonfinite_x = [5, 11, 22, 40], [11, 40]
    good = [b for b in range(B) if b not in bad]
    dm2 = tm.DevModel(bt, y=y)
    for scale in (None, 2.5):
        r = unc_replaced(dm2, lk, p2, lam2, held, scale=scale, **kw)
        f = unc_fused(dm2, lk, p2, lam2, held, scale=scale, **kw)
        assert f["rc"] == 0
        same(r, f, UNC_KEYS, f"with the failures, scale {scale}", nan_equal=True)
        assert np.all(f["status"][bad] == BATCH_UNC_FAILED) and np.all(f["status"][good] == BATCH_UNC_OK)
        for k in ("cov", "var", "factors"):
            assert np.all(np.isnan(f[k][bad])), k
        assert f["lam"][22] == -1.0
        if scale is None:
            assert np.all(np.isnan(f["scale"][nonfinite_x]))
            same(f, clean, UNC_KEYS, "the other problems", idx=good)
        else:
            assert np.all(f["scale"] == 2.5)
            same(f, clean, ("cov", "var", "lam", "status"), "the other problems", idx=good)
    Jq = np.random.default_rng(6).standard_normal((B, 3, 4, 6))
    for nobs in (-1, 42):
        rq, fq = query_replaced(dm2, lk, p2, lam2, held, Jq, nobs), query_fused(dm2, lk, p2, lam2, held, Jq, nobs)
        same(rq, fq, QUERY_KEYS, f"query with the failures, nobs {nobs}", nan_equal=True)
        cq = query_fused(dm, lk, p, lam, held, Jq, nobs)
        assert np.all(fq["status"][bad] == BATCH_UNC_FAILED) and np.all(np.isnan(fq["out"][bad]))
        same(fq, cq, QUERY_KEYS, "query, the other problems", idx=good)


# ---------------------------------------------------------------- 4. position independence
@LK
@pytest.mark.parametrize("case", [(MODEL_EXPDECAY, 65), (MODEL_GAUSS2D, (8, 8))], ids=mz.case_id)
def test_position_independence(case, lk):
    bt = mu.batch_of(case, lk, with_scale=lk == LIKELIHOOD_GAUSS)
    dm = tm.DevModel(bt)
    N = MODEL_NSTATE[case[0]]
    Jq = np.random.default_rng(7).standard_normal((B, 3, 4, N))
    for bounded in (False, True):
        p, lam, held = solve(dm, bt, lk, bounded)
        full = unc_fused(dm, lk, p, lam, held, fs=2)
        fullq = query_fused(dm, lk, p, lam, held, Jq, TILE[N] + 1)
        assert full["rc"] == 0 and fullq["rc"] == 0
        for b in (0, 3, 64):
            one = {k: (v[b:b + 1].copy() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B else v) for k, v in bt.items()}
            dm1 = tm.DevModel(one)
            h1 = None if held is None else held[b:b + 1].copy()
            s = unc_fused(dm1, lk, p[b:b + 1], lam[b:b + 1], h1, fs=2)
            q = query_fused(dm1, lk, p[b:b + 1], lam[b:b + 1], h1, Jq[b:b + 1], TILE[N] + 1)
            for k in UNC_KEYS:
                assert s[k].tobytes() == np.ascontiguousarray(full[k][b:b + 1]).tobytes(), (b, bounded, k)
            for k in QUERY_KEYS:
                assert q[k].tobytes() == np.ascontiguousarray(fullq[k][b:b + 1]).tobytes(), (b, bounded, k)


# ---------------------------------------------------------------- 5. the device twins
def unc_device(dm, lk, p, lam, held, mask, st, fs=1, scale=None):
    nb, N = p.shape
    M = dm.M
    P, Lm, S = td.Buf(p), td.Buf(lam.copy()), td.Buf(np.full(nb, 42, dtype=np.int32))
    O = dict(cov=td.Buf(np.full((nb, N, N), GUARD)), var=td.Buf(np.full((nb, N), GUARD)),
             factors=td.Buf(np.full((nb, M // fs), GUARD)),
             scale=td.Buf(np.full(nb, -1.0) if scale is None else np.full(nb, float(scale))))
    H, A = (None if held is None else td.Buf(held)), td.mask_dev(mask)
    before = capi.batch_model_callback_invocations()
    rc = capi.dense_batch_model_uncertainty_device(P.ptr, nb, dm.rec, lk, S.ptr, Lm.ptr, O["cov"].ptr, O["var"].ptr, O["factors"].ptr,
                                                   O["scale"].ptr, fs, None if H is None else H.ptr, None if A is None else A.ptr, st)
    assert capi.batch_model_callback_invocations() == before
    out = dict(rc=rc, status=S.get(), lam=Lm.get(), stats=capi.batch_uncertainty_last_stats())
    out.update({k: b.get() for k, b in O.items()})
    assert P.get().tobytes() == p.tobytes() and (H is None or H.get().tobytes() == held.tobytes())
    return out


def query_device(dm, lk, p, lam, held, Jq, nobs, mask, st):
    nb = p.shape[0]
    P, Lm, S, Q = td.Buf(p), td.Buf(lam.copy()), td.Buf(np.full(nb, 42, dtype=np.int32)), td.Buf(Jq)
    Out = td.Buf(np.full((nb, Jq.shape[1], Jq.shape[2], Jq.shape[2]), GUARD))
    H, A = (None if held is None else td.Buf(held)), td.mask_dev(mask)
    before = capi.batch_model_callback_invocations()
    rc = capi.dense_batch_model_query_covariance_device(P.ptr, nb, dm.rec, lk, Q.ptr, Jq.shape[1], Jq.shape[2], Out.ptr, S.ptr, nobs,
                                                        Lm.ptr, None if H is None else H.ptr, None if A is None else A.ptr, st)
    assert capi.batch_model_callback_invocations() == before
    assert Q.get().tobytes() == Jq.tobytes()
    return dict(rc=rc, status=S.get(), lam=Lm.get(), out=Out.get(), stats=capi.batch_uncertainty_last_stats())


@LK
@pytest.mark.parametrize("case", [(MODEL_EXPDECAY, 150), (MODEL_GAUSS2D, (7, 7)), (MODEL_GAUSS2D_ELLIPTIC, (9, 5))], ids=mz.case_id)
def test_device_twins(case, lk, stream):
    mask = np.ones(B, dtype=np.uint8)
    mask[list(OFF)] = 0
    on, off = np.flatnonzero(mask), list(OFF)
    bt = mu.batch_of(case, lk)
    dm = tm.DevModel(bt)
    N = MODEL_NSTATE[case[0]]
    Jq = np.random.default_rng(8).standard_normal((B, 3, 4, N))
    for bounded in (False, True):
        p, lam, held = solve(dm, bt, lk, bounded)
        for fs, scale in ((1, None), (2, 2.5)):
            host = unc_fused(dm, lk, p, lam, held, fs=fs, scale=scale)
            assert host["rc"] == 0
            for st in (None, stream):
                dev = unc_device(dm, lk, p, lam, held, None, st, fs, scale)
                same(host, dev, UNC_KEYS, f"device twin, stream {st is not None}")
                assert dev["stats"]["ms_callback"] == 0.0 and dev["stats"]["launches"] == 1
            dev = unc_device(dm, lk, p, lam, held, mask, stream, fs, scale)
            assert dev["rc"] == 0 and np.all(dev["status"][off] == BATCH_UNC_SKIPPED)
            for k in ("cov", "var", "factors"):
                assert np.all(dev[k][off] == GUARD), k
            assert dev["lam"][off].tobytes() == lam[off].tobytes()
            assert np.all(dev["scale"][off] == (-1.0 if scale is None else scale))
            same(host, dev, UNC_KEYS, "device twin with the mask", idx=on)
        for nobs in (-1, min(TILE[N], dm.M - 1)):
            hostq = query_fused(dm, lk, p, lam, held, Jq, nobs)
            assert hostq["rc"] == 0
            same(hostq, query_device(dm, lk, p, lam, held, Jq, nobs, None, None), QUERY_KEYS, "query device twin")
            devq = query_device(dm, lk, p, lam, held, Jq, nobs, mask, stream)
            assert devq["rc"] == 0 and np.all(devq["status"][off] == BATCH_UNC_SKIPPED) and np.all(devq["out"][off] == GUARD)
            same(hostq, devq, QUERY_KEYS, "query device twin with the mask", idx=on)


# ---------------------------------------------------------------- 6. the query covariance
@LK
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_query_covariance_has_the_callback_routes_bits(case, lk, stream):
    N = MODEL_NSTATE[case[0]]
    M = mz.case_shape(case)[0]
    T = TILE[N]
    bt = mu.batch_of(case, lk)
    dm = tm.DevModel(bt)
    rng = np.random.default_rng(9)
    for bounded in (False, True):
        p, lam, held = solve(dm, bt, lk, bounded)
        for Q in (1, 4, 16):
            Jq = rng.standard_normal((B, 3, Q, N))
            for nobs in [-1] + sorted({n for n in (0, T, T + 1, M) if n <= M}):
                what = f"{mz.case_id(case)}, {mu.LK_NAMES[lk]}, bounded {bounded}, Qrows {Q}, Nobservations {nobs}"
                r, f = query_replaced(dm, lk, p, lam, held, Jq, nobs), query_fused(dm, lk, p, lam, held, Jq, nobs)
                assert f["rc"] == 0 and np.all(f["status"] == BATCH_UNC_OK), what
                same(r, f, QUERY_KEYS, what)
                if nobs == 0:
                    assert not f["out"].any(), what
                if Q == 4:
                    same(f, query_device(dm, lk, p, lam, held, Jq, nobs, None, stream), QUERY_KEYS, what + ", device twin")


# ---------------------------------------------------------------- 7. against NumPy
@LK
@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_against_numpy(case, lk):
    tol = tu.COV_TOL if lk == LIKELIHOOD_GAUSS else tp.REL_TOL
    vtol = tu.VAR_TOL if lk == LIKELIHOOD_GAUSS else tp.REL_TOL
    levels = (None,) if lk == LIKELIHOOD_GAUSS else ("high", "low")
    for level in levels:
        bt = mz.batch(case) if level is None else po.batch((case, level))
        dm = tm.DevModel(bt)
        for bounded in (False, True):
            p, lam, held = solve(dm, bt, lk, bounded)
            out = unc_fused(dm, lk, p, lam, held, want=("cov", "var"))
            assert out["rc"] == 0 and np.all(out["status"] == BATCH_UNC_OK)
            worst = vworst = 0.0
            for b in range(B):
                want, free = mu.sigma_np(bt, b, p[b], out["lam"][b], None if held is None else held[b], lk)
                cov, var = out["cov"][b], out["var"][b]
                assert not cov[~free, :].any() and not cov[:, ~free].any() and not var[~free].any(), b
                sd = np.sqrt(np.diag(want)[free])
                worst = max(worst, float(np.max(np.abs(cov - want)[np.ix_(free, free)] / np.outer(sd, sd))))
                vworst = max(vworst, float(np.max(np.abs(var - np.diag(want))[free] / np.diag(want)[free])))
                assert var.tobytes() == np.ascontiguousarray(np.diag(cov)).tobytes()
            print(f"{mz.case_id(case)}, {mu.LK_NAMES[lk]} {level or ''}, bounded {bounded}: covariance against NumPy, relative to "
                  f"sqrt(S_ii S_jj): {worst:.3g} (asserted {tol:.3g}), variances relative {vworst:.3g} (asserted {vtol:.3g})")
            assert worst <= tol and vworst <= vtol
