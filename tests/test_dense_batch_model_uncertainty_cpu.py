"""The fused uncertainty and query calls of the built-in models without a GPU (dogleg_amd_dense_batch_model_uncertainty[_device],
dogleg_amd_dense_batch_model_query_covariance[_device]): the exports and the header as C; every refusal on the four entry points,
each of which returns -1 with a message that names the entry point, before any device work and with every output untouched; and
what the tables of the GPU tests must contain, so that no comparison there is vacuous."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BatchModel, LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON, MODEL_EXPDECAY, MODEL_GAUSS1D,
                                       MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC, BATCH_QUERY_MAX_ROWS)
from tests import batch_model_uncertainty_np as mu
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = mu.NAMES
GUARD = -7.5


# ---------------------------------------------------------------- 1. the library without a device
def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    with open(os.path.join(ROOT, "include", "dogleg.h")) as f:
        header = f.read()
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS and hasattr(capi.lib(), n) and n + "(" in header, n
        assert getattr(capi.lib(), n).argtypes is not None, n
    for n in ("dense_batch_model_uncertainty", "dense_batch_model_uncertainty_device", "dense_batch_model_query_covariance",
              "dense_batch_model_query_covariance_device"):
        assert callable(getattr(capi, n))


def test_abi_as_c(tmp_path):
    exe = str(tmp_path / "batch_model_uncertainty_abi")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "batch_model_uncertainty_abi.c"), "-o", exe, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1", "-1", "-1", "-3", "-5", "-4", "7"]
    for n in NAMES:
        assert n + ": model must be given" in r.stderr, r.stderr


class Arrays:
    """guard-filled outputs of the four calls in host memory, and what they held at first"""

    def __init__(self, B, N, M, Nq, Q):
        self.lam, self.scale = np.full(B, GUARD), np.full(B, GUARD)
        self.cov, self.var, self.fac = np.full((B, N, N), GUARD), np.full((B, N), GUARD), np.full((B, M), GUARD)
        self.status = np.full(B, 77, dtype=np.int32)
        self.out = np.full((B, Nq, Q, Q), GUARD)
        self.first = self.snapshot()

    def snapshot(self):
        return tuple(a.tobytes() for a in (self.lam, self.scale, self.cov, self.var, self.fac, self.status, self.out))


def test_refusals_that_need_no_device(capfd):
    """the four entry points; every array is host memory here, the record's too: a call that got past the checks under test would be
    refused by the pointer checks that follow them, never launched.  Every refusal is told by its message"""
    L = capi.lib()
    B, M, N, Nq, Q = 4, 12, 3, 2, 3
    y, s, t = np.ones((B, M)), np.ones((B, M)), np.arange(float(M))
    before = capi.batch_model_callback_invocations()
    p = np.arange(1.0, 1.0 + B * 6).reshape(B, 6)
    p0 = p.copy()
    Jq = np.ones((B, Nq, BATCH_QUERY_MAX_ROWS + 1, 6))
    held = np.zeros((B, 6), dtype=np.uint8)
    A = Arrays(B, 6, M, Nq, BATCH_QUERY_MAX_ROWS + 1)
    adr = lambda a: None if a is None else a.ctypes.data

    def model(kind=MODEL_EXPDECAY, nmeas=M, width=0, height=0, yy=y, tt=None, scale=None):
        return BatchModel(kind, nmeas, width, height, adr(yy), adr(tt), adr(scale), 0)

    # the arguments every call below starts from; a refusal overrides some
    base = dict(m=model(), lk=LIKELIHOOD_GAUSS, pp=p, b=B, lam=A.lam, cov=A.cov, var=A.var, fac=None, scale=None, fs=1, st=A.status,
                jq=Jq, nq=Nq, q=Q, nobs=-1, out=A.out)

    def unc(device):
        def call(**over):
            k = dict(base, **over)
            mref = None if k["m"] is None else C.byref(k["m"])
            args = [adr(k["pp"]), k["b"], mref, k["lk"], adr(k["lam"]), adr(k["cov"]), adr(k["var"]), adr(k["fac"]), adr(k["scale"]),
                    k["fs"], adr(k["st"]), adr(held)]
            if device:
                return L.dogleg_amd_dense_batch_model_uncertainty_device(*args, None, None)
            cast = lambda a, T: None if a is None else C.cast(a, C.POINTER(T))
            args = [cast(args[0], C.c_double), args[1], args[2], args[3]] + [cast(a, C.c_double) for a in args[4:9]] + \
                   [args[9], cast(args[10], C.c_int), args[11]]
            return L.dogleg_amd_dense_batch_model_uncertainty(*args)
        return call

    def query(device):
        def call(**over):
            k = dict(base, **over)
            mref = None if k["m"] is None else C.byref(k["m"])
            args = [adr(k["pp"]), k["b"], mref, k["lk"], adr(k["lam"]), adr(k["jq"]), k["nq"], k["q"], k["nobs"], adr(k["out"]),
                    adr(k["st"]), adr(held)]
            if device:
                return L.dogleg_amd_dense_batch_model_query_covariance_device(*args, None, None)
            cast = lambda a, T: None if a is None else C.cast(a, C.POINTER(T))
            args = [cast(args[0], C.c_double), args[1], args[2], args[3], cast(args[4], C.c_double), cast(args[5], C.c_double)] + \
                   args[6:9] + [cast(args[9], C.c_double), cast(args[10], C.c_int), args[11]]
            return L.dogleg_amd_dense_batch_model_query_covariance(*args)
        return call

    calls = [(NAMES[0], unc(False), "unc"), (NAMES[1], unc(True), "unc"), (NAMES[2], query(False), "query"),
             (NAMES[3], query(True), "query")]
    # what batch_model_ok refuses, an unknown likelihood, a scale with POISSON, and what both replaced twins refuse
    common = [
        (dict(m=None), "model must be given"),
        (dict(m=model(yy=None)), "model->y must be given"),
        (dict(m=model(kind=4)), "model->kind = 4 is none of"),
        (dict(m=model(kind=-1), lk=LIKELIHOOD_POISSON), "model->kind = -1 is none of"),
        (dict(m=model(nmeas=0)), "model->Nmeas = 0"),
        (dict(m=model(kind=MODEL_GAUSS2D, width=3, height=5)), "3 x 5 pixels, and model->Nmeas = 12"),
        (dict(m=model(kind=MODEL_GAUSS2D_ELLIPTIC), lk=LIKELIHOOD_POISSON), "0 x 0 pixels, and model->Nmeas = 12"),
        (dict(m=model(kind=MODEL_GAUSS2D, width=3, height=4, tt=t)), "model->t must be NULL for the 2D kinds"),
        (dict(m=model(kind=MODEL_GAUSS1D, width=3, height=4)), "both are 0 for the 1D kinds"),
        (dict(lk=2), "likelihood = 2 is neither DOGLEG_AMD_LIKELIHOOD_GAUSS nor DOGLEG_AMD_LIKELIHOOD_POISSON"),
        (dict(lk=-1), "likelihood = -1 is neither"),
        (dict(m=model(scale=s), lk=LIKELIHOOD_POISSON), "model->scale must be NULL with DOGLEG_AMD_LIKELIHOOD_POISSON"),
        (dict(b=0), "none may be 0"),
        (dict(pp=None), "must be given"),
        (dict(st=None), "must be given"),
    ]
    only = dict(
        unc=[
            (dict(cov=None, var=None), "is asked for"),
            (dict(fac=A.fac), "need"),                                 # factors without scale
            (dict(fac=A.fac, scale=A.scale, fs=3), "featureSize = 3: only 1 and 2 are supported"),
            # a scale <= 0 is to be computed, which needs Nmeas > Nstate + 1
            (dict(m=model(nmeas=4, yy=y), fac=A.fac, scale=A.scale), "Nmeas"),
        ],
        query=[
            (dict(jq=None), "must be given"),
            (dict(out=None), "must be given"),
            (dict(nq=0), "neither may be 0"),
            (dict(q=0), "neither may be 0"),
            (dict(q=BATCH_QUERY_MAX_ROWS + 1), f"a query has at most {BATCH_QUERY_MAX_ROWS} rows"),
            (dict(nobs=M + 1), f"Nobservations = {M + 1} exceeds Nmeas = {M}"),
        ])
    for name, call, kind in calls:
        for kw, msg in common + only[kind]:
            capfd.readouterr()
            assert call(**kw) == -1, (name, msg)
            err = capfd.readouterr().err
            assert msg in err and name + ":" in err, (name, msg, err)
        # a set communicator
        fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
        assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
        try:
            capfd.readouterr()
            assert call() == -1
            err = capfd.readouterr().err
            assert "rank" in err and name + ":" in err, (name, err)
        finally:
            L.dogleg_amd_clear_communicator()
        # host memory where device memory is required: the _device twins' own arrays (p_dev first), and the record's arrays on
        # either route, as in the fused solve
        capfd.readouterr()
        assert call() == -1
        err = capfd.readouterr().err
        assert name + ":" in err and "is not device-accessible memory" in err, (name, err)
        assert ("p_dev = " if name.endswith("_device") else "model->y = ") in err, (name, err)
    assert A.snapshot() == A.first and np.array_equal(p, p0) and not held.any()
    assert capi.batch_model_callback_invocations() == before


# ---------------------------------------------------------------- 2. the tables are not vacuous
def tables():
    """(what, likelihood, batch, the oracle's results) of every table the GPU tests use, plain and bounded"""
    for case in mz.CASES:
        for bounded in (False, True):
            yield f"{mz.case_id(case)}, gauss, bounded {bounded}", LIKELIHOOD_GAUSS, mz.batch(case), mz.oracle_table(case, bounded), bounded
    for table in po.TABLES:
        for bounded in (False, True):
            yield f"{po.table_id(table)}, bounded {bounded}", LIKELIHOOD_POISSON, po.batch(table), po.oracle_table(table, bounded), bounded


def test_tables_are_not_vacuous():
    """every J'J + lambda I of the tables is invertible on its free variables with a finite inverse; at least a quarter of the
    bounded problems end with a held variable; and a lambda > 0 comes from a table or, failing that, from the constructed singular
    problem, whose J'J is shown to be singular here"""
    nbounded = nheld = npos = 0
    worst = 0.0
    for what, lk, bt, orc, bounded in tables():
        for b, o in enumerate(orc):
            held = o["held"] if bounded else None
            N = o["p"].shape[0]
            _, J = mu.rows_np(bt, b, o["p"], lk)
            free = np.ones(N, dtype=bool) if held is None else np.asarray(held) == 0
            A = (J.T @ J + o["lambda_"] * np.eye(N))[np.ix_(free, free)]
            assert free.any() and np.all(np.isfinite(A)), (what, b)
            assert np.linalg.matrix_rank(A) == A.shape[0], (what, b)
            S, _ = mu.sigma_np(bt, b, o["p"], o["lambda_"], held, lk)
            assert np.all(np.isfinite(S)), (what, b)
            worst = max(worst, float(np.linalg.cond(A)))
            npos += o["lambda_"] > 0.0
            if bounded:
                nbounded += 1
                nheld += bool(np.asarray(held).any())
    print(f"{nheld} of {nbounded} bounded problems end with a held variable; {npos} problems end with lambda > 0; the largest "
          f"condition number of a free block {worst:.3g}")
    assert 4 * nheld >= nbounded
    # the lambda loop: a table problem, or else the constructed one
    for lk in mu.LIKELIHOODS:
        bt, p = mu.singular_batch(lk)
        for b in range(p.shape[0]):
            x, J = mu.rows_np(bt, b, p[b], lk)
            assert np.all(np.isfinite(x)) and np.all(np.isfinite(J))
            assert not J[:, 1:4].any() and np.linalg.matrix_rank(J.T @ J) == 2, "the constructed problem is singular"
            if lk == LIKELIHOOD_POISSON:
                assert p[b, 4] > 0.0, "f = c > 0: feasible"
    # (no table problem needs to end with lambda > 0: the constructed problem, singular as shown, starts the loop on the GPU)
