"""The ..._fit uncertainty and query entry points without a GPU: their export, declaration and binding, the refusals that are
decided before any device work -- each returns -1, invokes nothing and writes nothing; the arrays handed over are host arrays,
so a call that got past these checks would be refused by the pointer check (device twins) or for want of a device, never
launched -- and the agreement of the two host routes of tests/batch_fit_oracle.py on every case of the GPU tests.

Observed agreement of the two routes (the C oracle's packed Cholesky of the masked matrix against LAPACK's inverse of the
compacted free block), scaled as the GPU tests scale their error: 2.3e-15 at most on Sigma, 6.8e-14 on the query blocks (the
largest at the observations-only form over one weight feature, a block of low rank), 4.0e-14 on the factors (relative, with the
floor of the GPU tests' atol / rtol); the largest cond(H_FF + lambda I) of the cases is 49.9, at (64, 134) with no variable held
under soft-L1 weights (the planted batch of the robust tests: 5.4, under Cauchy weights).  The bound asserted here, 1e-12, is a
thousandth of the GPU tests' 1e-9; no case is left out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd import ctypes_defs as d
from libdogleg_amd.ctypes_defs import CB_DEVICE_BATCH, CB_DEVICE_BATCH_PRODUCTS, BatchLoss, LOSS_HUBER, LOSS_TRIVIAL
from tests import batch_fit_oracle as fo
from tests import batch_query_oracle as qo
from tests import test_dense_batch_robust_gpu as rt
from tests import test_dense_batch_uncertainty_gpu as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = ("dogleg_amd_dense_batch_uncertainty", "dogleg_amd_dense_products_batch_uncertainty",
         "dogleg_amd_dense_batch_uncertainty_device", "dogleg_amd_dense_products_batch_uncertainty_device",
         "dogleg_amd_dense_batch_query_covariance", "dogleg_amd_dense_products_batch_query_covariance",
         "dogleg_amd_dense_batch_query_covariance_device", "dogleg_amd_dense_products_batch_query_covariance_device")
NAMES = tuple(n[:-len("_device")] + "_fit_device" if n.endswith("_device") else n + "_fit" for n in TWINS)
ROUTES_TOL = 1e-12
COND_MAX = 100.0                # (recorded: 49.9; a batch that passes this by far is no longer the one the docstring describes)


def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n
        assert hasattr(capi.lib(), n)
        assert re.search(r"^int %s\(" % n, header, re.M), n


def test_bindings_agree_with_the_header():
    header = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    L = capi.lib()
    protos = {}
    for n in NAMES + TWINS:
        proto = re.search(r"^int %s\((.*?)\);" % n, header, re.M | re.S).group(1)
        protos[n] = [" ".join(a.split()) for a in proto.split(",")]
        kinds = ["ptr" if "*" in a else "uint" if a.startswith("unsigned") else "int" for a in protos[n]]
        got = ["uint" if t is C.c_uint else "int" if t is C.c_int else "ptr" for t in getattr(L, n).argtypes]
        assert got == kinds, n
    # the argument list of the twin, then the fit
    for n, t in zip(NAMES, TWINS):
        assert protos[n] == protos[t] + ["const dogleg_amd_batch_fit_t* fit"], n
        assert getattr(L, n).argtypes[-1] is C.POINTER(d.BatchFit)
    # the record: three pointers in the header's order
    body = re.search(r"typedef struct\s*\{([^}]*)\}\s*dogleg_amd_batch_fit_t;", header).group(1)
    members = re.findall(r"\*\s*(\w+)\s*;", body)
    assert members == [f for f, _ in d.BatchFit._fields_] == ["loss", "weights", "held"]
    assert C.sizeof(d.BatchFit) == 3 * C.sizeof(C.c_void_p)


def test_refusals_that_need_no_device():
    calls = []
    cb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    cbp = CB_DEVICE_BATCH_PRODUCTS(lambda *a: calls.append(a))
    f, fp = C.cast(cb, C.c_void_p), C.cast(cbp, C.c_void_p)
    N, M, B = 3, 12, 4
    p = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    Jq = np.ones((B, 2, 2, N))
    w4, w12 = np.ones((B, M // 4)), np.ones((B, M))
    held = np.zeros((B, N), dtype=np.uint8)
    SENT = -7.5
    dev = dict(lam=np.full(B, SENT), cov=np.full((B, N, N), SENT), var=np.full((B, N), SENT), fac=np.full((B, M), SENT),
               scale=np.full(B, 1.0), out=np.full((B, 2, 2, 2), SENT), status=np.full(B, 42, dtype=np.int32))
    keep = {k: v.copy() for k, v in dev.items()}
    a = lambda k: dev[k].ctypes.data
    prm = capi.default_parameters()

    def untouched(o):
        """a host wrapper's outputs as it prefilled them"""
        assert np.all(o["status"] == -1)
        for k in ("cov", "var", "factors", "out"):
            assert k not in o or not o[k].any(), k
        return o["rc"]

    def unc(fit, **kw):
        return untouched(capi.dense_batch_uncertainty(p, N, kw.get("M", M), f, None, lam=np.zeros(B), scale=1.0, fit=fit))

    def unc_p(fit):
        return untouched(capi.dense_products_batch_uncertainty(p, N, fp, None, prm, lam=np.zeros(B), fit=fit))

    def qry(fit, nobs=-1):
        return untouched(capi.dense_batch_query_covariance(p, N, M, f, None, Jq, lam=np.zeros(B), nobs=nobs, fit=fit))

    def qry_p(fit):
        return untouched(capi.dense_products_batch_query_covariance(p, N, fp, None, Jq, prm, lam=np.zeros(B), fit=fit))

    def unc_d(fit):
        return capi.dense_batch_uncertainty_device(p.ctypes.data, B, N, M, f, None, a("status"), a("lam"), a("cov"), a("var"),
                                                   a("fac"), a("scale"), 1, fit=fit)

    def unc_pd(fit):
        return capi.dense_products_batch_uncertainty_device(p.ctypes.data, B, N, fp, None, prm, a("status"), a("lam"), a("cov"),
                                                            a("var"), fit=fit)

    def qry_d(fit, nobs=-1):
        return capi.dense_batch_query_covariance_device(p.ctypes.data, B, N, M, f, None, Jq.ctypes.data, 2, 2, a("out"),
                                                        a("status"), nobs, a("lam"), fit=fit)

    def qry_pd(fit):
        return capi.dense_products_batch_query_covariance_device(p.ctypes.data, B, N, fp, None, prm, Jq.ctypes.data, 2, 2,
                                                                 a("out"), a("status"), a("lam"), fit=fit)

    fit = capi.batch_fit
    huber = lambda fs=1, scale=0.5, kind=LOSS_HUBER: BatchLoss(kind, scale, fs)
    J_FORM, P_FORM = (unc, qry, unc_d, qry_d), (unc_p, qry_p, unc_pd, qry_pd)
    for call in J_FORM:
        # weights without a loss
        assert call(fit(weights=w12)) == -1, call.__name__
        # an unknown kind, a bad scale -- while weights is NULL
        for bad in (huber(kind=7), huber(kind=-1), huber(scale=0.0), huber(scale=-1.0), huber(scale=np.nan), huber(scale=np.inf)):
            assert call(fit(loss=bad)) == -1, call.__name__
            assert call(fit(loss=bad, held=held)) == -1, call.__name__
        # a featureSize above 4 or one that does not divide Nmeas, with and without weights
        for bad in (huber(fs=5), huber(fs=8), BatchLoss(LOSS_TRIVIAL, 0.0, 5)):
            assert call(fit(loss=bad)) == -1 and call(fit(loss=bad, weights=w12)) == -1, call.__name__
    assert unc(fit(loss=huber(fs=4)), M=10) == -1 and unc(fit(loss=huber(fs=4), weights=w4), M=10) == -1
    # Nobservations that cuts a weight feature
    for call in (qry, qry_d):
        for nobs in (1, 2, 3, 5, 11):
            assert call(fit(loss=huber(fs=4)), nobs=nobs) == -1 and call(fit(loss=huber(fs=4), weights=w4), nobs=nobs) == -1
    # the products form takes held only
    for call in P_FORM:
        assert call(fit(loss=huber())) == -1 and call(fit(loss=huber(), weights=w12)) == -1, call.__name__
        assert call(fit(weights=w12, held=held)) == -1, call.__name__
    # what the twin refuses is refused with a fit too: a NULL p, B = 0, too many variables, nothing asked for
    L = capi.lib()
    rec = d.BatchFit(None, None, held.ctypes.data)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int)
    dp = lambda k: C.cast(a(k), D)
    st = C.cast(a("status"), I)
    assert L.dogleg_amd_dense_batch_uncertainty_fit(None, B, N, M, f, None, dp("lam"), dp("cov"), None, None, None, 1, st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_batch_uncertainty_fit(d.dptr(p), 0, N, M, f, None, dp("lam"), dp("cov"), None, None, None, 1, st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_batch_uncertainty_fit(d.dptr(p), 1, 65, M, f, None, dp("lam"), dp("cov"), None, None, None, 1, st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_batch_uncertainty_fit(d.dptr(p), B, N, M, f, None, dp("lam"), None, None, None, None, 1, st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_batch_uncertainty_fit(d.dptr(p), B, N, M, f, None, dp("lam"), dp("cov"), None, None, None, 3, st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_batch_query_covariance_fit(d.dptr(p), B, N, M, f, None, dp("lam"), d.dptr(Jq), 2, 17, -1, dp("out"), st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_batch_query_covariance_fit(d.dptr(p), B, N, M, f, None, dp("lam"), d.dptr(Jq), 2, 2, M + 1, dp("out"), st, C.byref(rec)) == -1
    assert L.dogleg_amd_dense_products_batch_query_covariance_fit(d.dptr(p), B, N, None, None, C.byref(prm), dp("lam"), d.dptr(Jq), 2, 2, dp("out"), st, C.byref(rec)) == -1
    # a set communicator: one rank only
    fn = capi.ALLREDUCE_FN(lambda b_, n_, c_: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        for call in J_FORM + P_FORM:
            assert call(fit(held=held)) == -1, call.__name__
    finally:
        L.dogleg_amd_clear_communicator()
    for k in dev:
        assert np.array_equal(dev[k], keep[k]), k
    assert not calls


# ---------------------------------------------------------------- the two host routes
WORST = dict(cond=0.0)


def routes(N, M, fs, lfs, kind, pattern, nb, what):
    """both routes of the reference on one batch: the loss and the held pattern together, every output"""
    seeds, p, lam, w = fo.points(N, M, lfs, kind, nb)
    held = fo.held_pattern(pattern, nb, N)
    Jq = fo.queries(nb, N)
    ecov = efac = eblk = cond = 0.0
    for b, (x, J) in enumerate(fo.evaluated(N, M, lfs, kind, nb)):
        for nobs in (-1, 0, lfs, M):
            kw = dict(lfs=lfs, loss=fo.loss_of(kind, lfs)[0], fs=fs, Jq=Jq[b], nobs=nobs)
            r1, r2 = fo.reference(x, J, lam[b], held[b], **kw), fo.reference(x, J, lam[b], held[b], route="inv", **kw)
            # the loss route gives the weights the robust oracle returned at that point
            assert np.allclose(r1["w"], w[b], rtol=1e-12, atol=0)
            ecov = max(ecov, fo.cov_error(r2["S"], r1["S"], held[b]))
            eblk = max(eblk, qo.scaled_error(r2["blocks"], r1["blocks"]))
            big = r1["factors"] == fo.DBL_MAX
            assert np.array_equal(big, r2["factors"] == fo.DBL_MAX)
            if np.any(~big):
                # (the measure of the GPU tests' rtol 1e-9 / atol 1e-12)
                den = np.maximum(np.abs(r1["factors"][~big]), tu.FAC_ATOL / tu.FAC_RTOL)
                efac = max(efac, float(np.max(np.abs(r2["factors"] - r1["factors"])[~big] / den)))
            cond = max(cond, r1["cond"])
            if pattern == "all":
                assert not r1["S"].any() and not r1["blocks"].any() and not r2["S"].any()
            if nobs == 0:
                assert not r1["blocks"].any()
    WORST["cond"] = max(WORST["cond"], cond)
    print(f"{what}: the two host routes differ by {ecov:.3g} scaled on Sigma, {eblk:.3g} on the query blocks, {efac:.3g} relative "
          f"on the factors; cond(H_FF + lambda I) <= {cond:.3g} (the largest so far {WORST['cond']:.3g})")
    assert ecov <= ROUTES_TOL and eblk <= ROUTES_TOL and efac <= ROUTES_TOL and cond <= COND_MAX


@pytest.mark.parametrize("pattern", fo.HELD_PATTERNS)
@pytest.mark.parametrize("case", fo.CASES, ids=str)
def test_the_two_host_routes_agree(case, pattern):
    N, M, fs, lfs, kind = case
    routes(N, M, fs, lfs, kind, pattern, fo.B, f"{case} {pattern}")


@pytest.mark.parametrize("kind", sorted(rt.KINDS))
def test_the_two_host_routes_agree_on_the_planted_batch(kind):
    (N, M), lfs = fo.PLANTED_SHAPE, fo.PLANTED_LFS
    for fs in (1, 2):
        routes(N, M, fs, lfs, kind, "none", fo.PLANTED_B, f"planted {kind} fs {fs}")


def test_the_case_table_is_what_it_says():
    from tests import dense_batch_wide_shapes as ws
    assert sorted({ws.size_class(c[0]) for c in fo.CASES}) == [8, 16, 24, 32, 48, 64]
    assert {c[2] for c in fo.CASES} == {1, 2} and {c[3] for c in fo.CASES} == {1, 2, 4}
    for N, M, fs, lfs, _ in fo.CASES:
        assert M % lfs == 0 and M % fs == 0 and M > N + 1
    for N, M, fs, lfs, _ in fo.RAGGED:
        assert M % rt.tile_rows(N, lfs) != 0, (N, M, lfs)
    assert rt.tile_rows(48, 4) == 4 and rt.tile_rows(64, 4) == 4         # (no ragged tile at lfs 4 above 32)
    both = [ws.size_class(c[0]) for c in fo.CASES if c[2] == 2 and c[3] == 4]
    assert min(both) <= 32 and max(both) > 32
    # the weights matter: planted features are all but dropped, and a good share of the others is below 1
    for N, M, fs, lfs, kind in fo.CASES:
        w = fo.points(N, M, lfs, kind)[3]
        assert w.min() < 0.1 and np.all((w > 0) & (w <= 1))
