"""The Poisson maximum-likelihood fit of the built-in models without a GPU: dogleg_batch_model_row_poisson of
include/dogleg_batch_models.h compiled for the host against the NumPy restatement of tests/batch_poisson_oracle.py; the
restatement's g and H against central differences of its F and against the Fisher information formed row by row; the oracle's loop
under the least-squares hook against tests/batch_bounds_oracle.py, field by field and exactly; the exports and the header as C;
the refusals that need no device, each told by its message; and the case tables the GPU tests compare against: what they must
contain is asserted here, so that no GPU comparison is vacuous.

Tolerances.  ROW_TOL = 1e-13 on x~, J~ and d of the host header against NumPy, relative to the largest magnitude of the problem's
x~ and d and of the column of J~: f carries about 6 eps of |A e| + |c| in either evaluation, x~ = r / sqrt(f) and d (whose
derivative with respect to f is 2 r / f) inherit it scaled by sqrt(f) and r, so about 6 eps f / sqrt(f) = 1.3e-14 at f = 400
against an x~ of size 1 and 12 eps |r| = 5e-14 against a d of size 1 and more; the figure measured is printed.  FD_TOL = 1e-6 on
g against half the central-difference gradient of F with h = 1e-6 (1 + |p_j|), relative to the largest |g_j|: truncation h^2 F'''
and rounding eps F / h are both about 1e-9 of F's scale."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BatchBounds, BatchLoss, BatchModel, BatchResult, BATCH_FAILED, BATCH_JTX, BATCH_SMALL_STEP, LOSS_TRIVIAL,
                                       MODEL_EXPDECAY, MODEL_GAUSS2D, MODEL_NSTATE, LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON, dptr)
from tests import batch_bounds_oracle as bb
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests import batch_robust_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_optimize_dense_batch_model_mle", "dogleg_amd_optimize_dense_batch_model_mle_device")
ROW_TOL = 1e-13
FD_TOL = 1e-6


def poisson_rows_np(hp, p):
    """(x~ (M,), J~ (M, N), d (M,), feasible (M,)) of the definition; NaN in an infeasible row"""
    f, G = po.model_values(hp, p)
    y = hp.y
    with np.errstate(all="ignore"):
        ok = f > 0.0
        q = np.where(ok, 1.0 / np.sqrt(f), np.nan)
        r = f - y
        d = np.where(y == 0.0, 2.0 * f, 2.0 * (r - y * np.log(f / np.where(y == 0.0, 1.0, y))))
    return r * q, G * q[:, None], np.where(ok, d, np.nan), ok


def scaled(got, want, axis):
    ref = np.max(np.abs(want), axis=axis, keepdims=True)
    ref = np.where(ref > 0.0, ref, 1.0)
    return float(np.max(np.abs(got - want) / ref))


# ---------------------------------------------------------------- 1. the header on the host
@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("batch_poisson_rows") / "libbatch_poisson_rows.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "batch_model_rows_poisson.c"), "-o", so, "-lm"],
                   check=True)
    L = C.CDLL(so)
    D = C.POINTER(C.c_double)
    L.model_rows_poisson.argtypes = [C.c_int, D, C.c_int, C.c_int, D, D, D, D, D, C.POINTER(C.c_int)]
    L.model_rows_poisson.restype = None
    return L


def header_eval(L, kind, p, y, width):
    M, N = len(y), MODEL_NSTATE[kind]
    x, J, d, ok = np.full(M, 7.0), np.full((M, N), 7.0), np.full(M, 7.0), np.full(M, -1, dtype=np.int32)
    p = np.ascontiguousarray(p, dtype=np.float64)
    L.model_rows_poisson(kind, dptr(p), M, width, None, dptr(np.ascontiguousarray(y, dtype=np.float64)), dptr(x), dptr(J), dptr(d),
                         ok.ctypes.data_as(C.POINTER(C.c_int)))
    return x, J, d, ok != 0


@pytest.mark.parametrize("table", po.TABLES, ids=po.table_id)
def test_host_header_against_numpy(host_rows, table):
    bt = po.batch(table, nb=5)
    worst, zeros = 0.0, 0
    for b in range(5):
        hp = mz.host_model(bt, b)
        zeros += int(np.sum(hp.y == 0.0))
        for p in (bt["p0"][b], bt["truth"][b]):
            x, J, d, ok = header_eval(host_rows, hp.kind, p, hp.y, hp.width)
            xn, Jn, dn, okn = poisson_rows_np(hp, p)
            assert ok.all() and okn.all()
            worst = max(worst, scaled(x, xn, 0), scaled(J, Jn, 0), scaled(d, dn, 0))
    print(f"{po.table_id(table)}: largest scaled deviation of the host header from NumPy {worst:.3g} (asserted {ROW_TOL:.3g}), "
          f"{zeros} zero counts")
    assert worst <= ROW_TOL
    assert zeros > 0 if table[1] == "low" else zeros == 0


def test_infeasible_row_negative_and_nan_datum(host_rows):
    """an offset below zero makes the rows far from the peak infeasible: the flag is clear and the row NaN, the others keep their
    values; a negative datum gives a NaN d beside a finite x~ and J~; a NaN datum a NaN x~ and d"""
    table = ((MODEL_GAUSS2D, (7, 7)), "low")
    bt = po.batch(table, nb=1)
    hp = mz.host_model(bt, 0)
    p = bt["truth"][0].copy()
    p[4] = -0.5
    x, J, d, ok = header_eval(host_rows, hp.kind, p, hp.y, hp.width)
    xn, Jn, dn, okn = poisson_rows_np(hp, p)
    assert ok.tolist() == okn.tolist() and 0 < ok.sum() < hp.M
    assert np.all(np.isnan(x[~ok])) and np.all(np.isnan(d[~ok])) and np.all(np.isnan(J[~ok]))
    assert max(scaled(x[ok], xn[ok], 0), scaled(J[ok], Jn[ok], 0), scaled(d[ok], dn[ok], 0)) <= ROW_TOL
    y = hp.y.copy()
    y[3], y[10] = -2.0, np.nan
    hq = mz.HostModel(hp.kind, y, bt["p0"][0], None, None, hp.width)
    x, J, d, ok = header_eval(host_rows, hp.kind, bt["truth"][0], y, hp.width)
    xn, Jn, dn, _ = poisson_rows_np(hq, bt["truth"][0])
    assert ok.all() and np.isnan(d[3]) and np.isfinite(x[3]) and np.all(np.isfinite(J[3]))
    assert np.isnan(d[10]) and np.isnan(x[10]) and np.all(np.isfinite(J[10]))
    rest = np.ones(hp.M, dtype=bool)
    rest[[3, 10]] = False
    assert np.all(np.isfinite(d[rest])) and scaled(d[rest], dn[rest], 0) <= ROW_TOL
    # the oracle's products say the same: a NaN cost or gradient
    F, g, *_ = po.poisson_products(hq)(bt["truth"][0])
    assert np.isnan(F) or np.any(np.isnan(g))


# ---------------------------------------------------------------- 2. the restatement against itself
@pytest.mark.parametrize("table", po.TABLES, ids=po.table_id)
def test_oracle_products(table):
    """g = 1/2 grad F by central differences; H = sum grad f grad f' / f row by row; g = J~' x~ and H = J~' J~ of the rows"""
    bt = po.batch(table, nb=3)
    worst_g = worst_h = 0.0
    for b in range(3):
        hp = mz.host_model(bt, b)
        hook = po.poisson_products(hp)
        rng = np.random.default_rng([31, b])
        p = bt["truth"][b] * (1.0 + 0.02 * rng.uniform(-1.0, 1.0, hp.N))
        F, g, H, Ferr, fm, ok = hook(p)
        assert ok and fm > 0.0 and np.isfinite(F) and Ferr > 0.0
        fd = np.zeros(hp.N)
        for j in range(hp.N):
            h = 1e-6 * (1.0 + abs(p[j]))
            pp, pm = p.copy(), p.copy()
            pp[j] += h
            pm[j] -= h
            fd[j] = 0.5 * (hook(pp)[0] - hook(pm)[0]) / (pp[j] - pm[j])
        worst_g = max(worst_g, float(np.max(np.abs(g - fd))) / float(np.max(np.abs(fd))))
        f, G = po.model_values(hp, p)
        Hd = np.zeros((hp.N, hp.N))
        for i in range(hp.M):
            Hd += np.outer(G[i], G[i]) / f[i]
        worst_h = max(worst_h, float(np.max(np.abs(H - Hd))) / float(np.max(np.abs(Hd))))
        xt, Jt, d, _ = poisson_rows_np(hp, p)
        assert np.allclose(Jt.T @ xt, g, rtol=1e-11, atol=1e-11 * np.max(np.abs(g)))
        assert np.allclose(Jt.T @ Jt, H, rtol=1e-11, atol=1e-11 * np.max(np.abs(H)))
        assert abs(d.sum() - F) <= 1e-12 * abs(F)
    print(f"{po.table_id(table)}: g against central differences {worst_g:.3g} (asserted {FD_TOL:.3g}), H against the sum of outer "
          f"products {worst_h:.3g}")
    assert worst_g <= FD_TOL and worst_h <= 1e-13


@pytest.mark.parametrize("case", mz.CASES, ids=mz.case_id)
def test_gauss_hook_reproduces_the_bounds_oracle(case):
    """the restated loop under the least-squares hook: every field of batch_bounds_oracle.solve_one, exactly"""
    nb = 13
    bt = mz.batch(case, nb=nb)
    prm, loss = mz.params(), ro.Loss(LOSS_TRIVIAL, 1.0, 1)
    for bounded in (False, True):
        for b in range(nb):
            lo, hi = (bt["lo"][b], bt["hi"][b]) if bounded else (None, None)
            want = bb.solve_one(mz.host_model(bt, b), prm, loss, lo, hi)
            got = po.solve_one(mz.host_model(bt, b), prm, LIKELIHOOD_GAUSS, lo, hi)
            assert got["infeasible"] == 0
            for k in ("norm2_x", "trustregion", "lambda_", "iterations", "evaluations", "status", "step_types", "rejected",
                      "clipped", "fallbacks", "held_steps", "held_resteps", "landings", "margin"):
                assert got[k] == want[k], (b, bounded, k)
            for k in ("p", "held", "first_p"):
                assert got[k].tobytes() == want[k].tobytes(), (b, bounded, k)


# ---------------------------------------------------------------- 3. the library without a device
def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "dogleg.h")) as f:
        header = f.read()
    for n in NAMES + ("dogleg_amd_batch_model_fisher_callback",):
        assert n in exported and n in capi.DOGLEG_SYMBOLS and hasattr(capi.lib(), n) and n + "(" in header, n
    assert "#define DOGLEG_AMD_LIKELIHOOD_GAUSS   0" in header and "#define DOGLEG_AMD_LIKELIHOOD_POISSON 1" in header
    assert (LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON) == (0, 1)
    for n in ("optimize_dense_batch_model_mle", "optimize_dense_batch_model_mle_device", "batch_model_fisher_callback"):
        assert callable(getattr(capi, n))


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_poisson_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_poisson_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1", "-1", "1", "3", "-3"]
    assert NAMES[0] + ": likelihood = 2 is neither" in r.stderr and NAMES[1] + ": likelihood = -1 is neither" in r.stderr
    assert NAMES[0] + ": model->scale must be NULL with DOGLEG_AMD_LIKELIHOOD_POISSON" in r.stderr


def test_refusals_that_need_no_device(capfd):
    """both entry points and every solve entry point given the Fisher callback; the arrays are host memory here: a call that got
    past the checks under test would be refused by the pointer checks that follow them, never launched"""
    L = capi.lib()
    B, M = 4, 12
    y, s = np.ones((B, M)), np.ones((B, M))
    before = capi.batch_model_callback_invocations()

    def model(kind=MODEL_EXPDECAY, nmeas=M, width=0, height=0, yy=y, scale=None):
        return BatchModel(kind, nmeas, width, height, None if yy is None else yy.ctypes.data, None,
                          None if scale is None else scale.ctypes.data, 0)

    p0 = np.arange(1.0, 1.0 + B * 6).reshape(B, 6)
    p = p0.copy()
    res = (BatchResult * B)()
    C.memset(res, 0xA5, C.sizeof(res))
    res0 = bytes(res)
    lam = np.full(B, -7.5)
    lo, hi, held = np.zeros((B, 6)), np.ones((B, 6)), np.full((B, 6), 9, dtype=np.uint8)
    bounds = BatchBounds(lo.ctypes.data, hi.ctypes.data, held.ctypes.data)

    def host_call(m, lk=LIKELIHOOD_POISSON, pp=p, b=B, r=res, bd=None):
        return L.dogleg_amd_optimize_dense_batch_model_mle(None if pp is None else dptr(pp), b, None if m is None else C.byref(m), lk,
                                                           None, None if bd is None else C.byref(bd), r)

    def dev_call(m, lk=LIKELIHOOD_POISSON, pp=p, b=B, r=res, bd=None):
        return L.dogleg_amd_optimize_dense_batch_model_mle_device(None if pp is None else pp.ctypes.data, b,
                                                                  None if m is None else C.byref(m), lk, None,
                                                                  None if bd is None else C.byref(bd),
                                                                  None if r is None else C.addressof(r), lam.ctypes.data, None, None)

    refusals = [
        (dict(m=model(), lk=2), "likelihood = 2 is neither DOGLEG_AMD_LIKELIHOOD_GAUSS nor DOGLEG_AMD_LIKELIHOOD_POISSON"),
        (dict(m=model(), lk=-1), "likelihood = -1 is neither"),
        (dict(m=model(scale=s)), "model->scale must be NULL with DOGLEG_AMD_LIKELIHOOD_POISSON: counts carry their own variance"),
        # everything the fused entry points refuse, with either likelihood
        (dict(m=None), "model must be given"),
        (dict(m=model(yy=None)), "model->y must be given"),
        (dict(m=model(kind=4)), "model->kind = 4 is none of"),
        (dict(m=model(nmeas=0), lk=LIKELIHOOD_GAUSS), "model->Nmeas = 0"),
        (dict(m=model(kind=MODEL_GAUSS2D, width=3, height=5)), "3 x 5 pixels, and model->Nmeas = 12"),
        (dict(m=model(width=3, height=4)), "both are 0 for the 1D kinds"),
        (dict(m=model(), b=0), "none may be 0"),
        (dict(m=model(), pp=None), "must be given"),
        (dict(m=model(), r=None, lk=LIKELIHOOD_GAUSS), "must be given"),
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
    # a scale is still taken with GAUSS: that call gets as far as the pointer checks (or, with a device, further: not made here)
    if L.dlg_device_count() == 0:
        for call in (host_call, dev_call):
            capfd.readouterr()
            assert call(model(scale=s), lk=LIKELIHOOD_GAUSS, bd=bounds) == -1
            assert "model->scale must be NULL" not in capfd.readouterr().err

    # the Fisher callback is refused by every solve entry point, by name
    rec = model()
    cb, cookie, N, Mm = capi.batch_model_fisher_callback(rec)
    assert (N, Mm) == (3, M)
    pf = p0[:, :3].copy()
    pf0 = pf.copy()
    trivial = BatchLoss(LOSS_TRIVIAL, 1.0, 1)
    for name, call in (
            ("dogleg_amd_optimize_dense_batch", lambda: capi.optimize_dense_batch(pf, N, M, cb, cookie, None)[0]),
            ("dogleg_amd_optimize_dense_batch_robust",
             lambda: capi.optimize_dense_batch_robust(pf, N, M, cb, cookie, trivial, None)[0]),
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
        assert name + ": dogleg_amd_batch_model_fisher_callback is no callback of a solve" in err, (name, err)
    assert np.array_equal(pf, pf0)
    assert np.array_equal(p, p0) and bytes(res) == res0 and np.all(lam == -7.5)
    assert np.all(held == 9) and not lo.any() and np.all(hi == 1.0)
    assert capi.batch_model_callback_invocations() == before


# ---------------------------------------------------------------- 4. the case tables
@pytest.mark.parametrize("table", po.TABLES, ids=po.table_id)
def test_case_tables(table):
    plain, bounded = po.oracle_table(table, False), po.oracle_table(table, True)
    assert len(plain) == len(bounded) == po.B
    bt = po.batch(table)
    zeros = float(np.mean(bt["y"] == 0.0))
    for what, orc in (("plain", plain), ("bounded", bounded)):
        assert all(o["status"] in (BATCH_JTX, BATCH_SMALL_STEP) for o in orc), what
    mp, mb = min(o["margin"] for o in plain), min(o["margin"] for o in bounded)
    nheld, nclipped = sum(bool(o["held"].any()) for o in bounded), sum(o["clipped"] for o in bounded)
    print(f"{po.table_id(table)}: smallest decision margin plain {mp:.3g}, bounded {mb:.3g} (recorded {po.MARGINS[table]}), zero "
          f"counts {100 * zeros:.0f} %, infeasible trials {sum(o['infeasible'] for o in plain)} / "
          f"{sum(o['infeasible'] for o in bounded)}, rejected {sum(o['rejected'] for o in plain)}, {nheld} bounded problems end "
          f"with a held variable, {nclipped} clipped steps, {sum(o['fallbacks'] for o in bounded)} fallbacks")
    assert mp > po.MARGIN_FLOOR and mb > po.MARGIN_FLOOR
    # the returned cost of every problem is known well enough for the 1e-8 the GPU tests ask of it (batch_poisson_oracle.COST_TOL)
    assert max(o["cost_error"] for o in plain + bounded) <= po.COST_TOL
    for m, rec in zip((mp, mb), po.MARGINS[table]):
        assert abs(m - rec) <= 0.05 * rec, "the generator or the oracle changed: choose the seeds again"
    if table[1] == "low":
        # (7 % to 30 % of a low table's data are zero: the decays and the peaks' flanks stay above the offset of 0.3 over most rows)
        assert zeros >= 0.05
    else:
        assert zeros == 0.0
    assert not any(o["held"].any() for o in plain)
    assert nheld >= 1 and nclipped >= 1
    assert len({o["evaluations"] for o in plain + bounded}) > 1
    assert any(np.max(np.abs(a["p"] - b["p"])) > 1e-3 for a, b in zip(plain, bounded))


def test_tables_are_not_vacuous():
    """together: the low-count plain tables contain infeasible trials and rejected steps, the bounded tables held variables, clips
    and fallbacks"""
    low_plain = [o for t in po.TABLES if t[1] == "low" for o in po.oracle_table(t, False)]
    bounded = [o for t in po.TABLES for o in po.oracle_table(t, True)]
    ninf, nrej = sum(o["infeasible"] for o in low_plain), sum(o["rejected"] for o in low_plain)
    nheld, nclip, nfall = sum(bool(o["held"].any()) for o in bounded), sum(o["clipped"] for o in bounded), sum(o["fallbacks"] for o in bounded)
    tables_inf = sum(any(o["infeasible"] for o in po.oracle_table(t, False)) for t in po.TABLES if t[1] == "low")
    print(f"low-count plain tables: {ninf} infeasible trials in {tables_inf} of 14 tables, {nrej} rejected steps; bounded tables: "
          f"{nheld} problems end with a held variable, {nclip} clipped steps, {nfall} fallbacks")
    assert ninf > 0 and nrej >= ninf and nheld > 0 and nclip > 0 and nfall > 0
    # an infeasible start fails in the oracle too
    t = ((MODEL_EXPDECAY, 64), "low")
    bt = po.batch(t, nb=1)
    p0 = bt["p0"][0].copy()
    p0[2] = -5.0
    o = po.solve_one(mz.host_model(bt, 0, p0), po.params(), LIKELIHOOD_POISSON)
    assert o["status"] == BATCH_FAILED and o["evaluations"] == 1 and o["norm2_x"] == -1.0
