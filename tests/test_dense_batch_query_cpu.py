"""The batch query-covariance entry points without a GPU: their export and declaration, the refusals that are decided before
any device work -- each returns -1, invokes nothing and writes nothing; the arrays handed over are host arrays, so a call that
got past these checks would be refused by the pointer check (device twins) or for want of a device, never launched -- and the
agreement of the two host routes of tests/batch_query_oracle.py on the parity cases of the GPU tests.

Observed agreement of the two routes (the oracle's packed Cholesky against LAPACK's general inverse), scaled as the GPU
tests scale their error: 2.0e-15 at most over the plain cases, 2.2e-14 over the observations-only cases (the largest at
Nobservations = 1, a block of rank 1); the largest cond(JtJ) of the cases is 34.  The bound asserted here, 1e-12, is a
thousandth of the GPU tests' 1e-9."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd import ctypes_defs as d
from libdogleg_amd.ctypes_defs import CB_DEVICE_BATCH, BATCH_MAX_NSTATE, BATCH_QUERY_MAX_ROWS
from tests import batch_query_oracle as qo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dogleg_amd_dense_batch_query_covariance", "dogleg_amd_dense_products_batch_query_covariance",
         "dogleg_amd_dense_batch_query_covariance_device", "dogleg_amd_dense_products_batch_query_covariance_device")
ROUTES_TOL = 1e-12


def test_symbols_exported_declared_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    header = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    for n in NAMES:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n
        assert hasattr(capi.lib(), n)
        assert re.search(r"^int %s\(" % n, header, re.M), n


def test_ctypes_defs_agree_with_the_header():
    header = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    macro = lambda name: int(re.search(r"^#define %s\s+(\d+)" % name, header, re.M).group(1))
    assert macro("DOGLEG_AMD_BATCH_QUERY_MAX_ROWS") == d.BATCH_QUERY_MAX_ROWS == 16
    assert macro("DOGLEG_AMD_BATCH_MAX_NSTATE") == d.BATCH_MAX_NSTATE
    assert (macro("DOGLEG_AMD_BATCH_UNC_OK"), macro("DOGLEG_AMD_BATCH_UNC_FAILED"), macro("DOGLEG_AMD_BATCH_UNC_SKIPPED")) == \
        (d.BATCH_UNC_OK, d.BATCH_UNC_FAILED, d.BATCH_UNC_SKIPPED)
    # the argument lists of the bindings against the prototypes: as many arguments, unsigned / int / pointer in the same places
    L = capi.lib()
    for n in NAMES:
        proto = re.search(r"^int %s\((.*?)\);" % n, header, re.M | re.S).group(1)
        kinds = []
        for a in proto.split(","):
            a = " ".join(a.split())
            kinds.append("ptr" if "*" in a else "uint" if a.startswith("unsigned") else "int")
        got = ["uint" if t is C.c_uint else "int" if t is C.c_int else "ptr" for t in getattr(L, n).argtypes]
        assert got == kinds, n


def test_refusals_that_need_no_device():
    calls = []
    cb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    f = C.cast(cb, C.c_void_p)
    N, M, B, NQ, Q = 3, 12, 4, 2, 2
    SENT = -7.5
    buf = dict(p=np.arange(1.0, 1.0 + B * N), lam=np.full(B, SENT), Jq=np.ones(B * NQ * BATCH_QUERY_MAX_ROWS * N),
               out=np.full(B * NQ * (BATCH_QUERY_MAX_ROWS + 1) ** 2, SENT), status=np.full(B, 42, dtype=np.int32),
               big=np.ones((BATCH_MAX_NSTATE + 1) * NQ * Q))
    keep = {k: v.copy() for k, v in buf.items()}
    a = lambda k: None if k is None else buf[k].ctypes.data
    prm = capi.default_parameters()
    L = capi.lib()

    def unchanged(rc):
        for k in buf:
            assert np.array_equal(buf[k], keep[k]), k
        return rc

    def host(p="p", b=B, n=N, m=M, fn=f, Jq="Jq", nq=NQ, q=Q, nobs=-1, out="out", status="status"):
        return unchanged(L.dogleg_amd_dense_batch_query_covariance(
            C.cast(a(p), C.POINTER(C.c_double)), b, n, m, fn, None, C.cast(a("lam"), C.POINTER(C.c_double)),
            C.cast(a(Jq), C.POINTER(C.c_double)), nq, q, nobs, C.cast(a(out), C.POINTER(C.c_double)),
            C.cast(a(status), C.POINTER(C.c_int))))

    def host_p(p="p", b=B, n=N, fn=f, Jq="Jq", nq=NQ, q=Q, out="out", status="status", prm=prm):
        return unchanged(L.dogleg_amd_dense_products_batch_query_covariance(
            C.cast(a(p), C.POINTER(C.c_double)), b, n, fn, None, C.byref(prm), C.cast(a("lam"), C.POINTER(C.c_double)),
            C.cast(a(Jq), C.POINTER(C.c_double)), nq, q, C.cast(a(out), C.POINTER(C.c_double)),
            C.cast(a(status), C.POINTER(C.c_int))))

    def dev(p="p", b=B, n=N, m=M, fn=f, Jq="Jq", nq=NQ, q=Q, nobs=-1, out="out", status="status"):
        return unchanged(capi.dense_batch_query_covariance_device(a(p), b, n, m, fn, None, a(Jq), nq, q, a(out), a(status), nobs,
                                                                  a("lam")))

    def dev_p(p="p", b=B, n=N, fn=f, Jq="Jq", nq=NQ, q=Q, out="out", status="status", prm=prm):
        return unchanged(capi.dense_products_batch_query_covariance_device(a(p), b, n, fn, None, prm, a(Jq), nq, q, a(out),
                                                                           a(status), a("lam")))

    n65 = BATCH_MAX_NSTATE + 1
    for call in (host, host_p, dev, dev_p):
        for k in ("p", "fn", "Jq", "out", "status"):
            assert call(**{k: None}) == -1, (call.__name__, k)
        assert call(b=0) == -1 and call(n=0) == -1 and call(nq=0) == -1 and call(q=0) == -1, call.__name__
        assert call(q=BATCH_QUERY_MAX_ROWS + 1) == -1, call.__name__
        assert call(p="big", b=1, n=n65) == -1, call.__name__
    for call in (host, dev):
        assert call(m=0) == -1
        assert call(nobs=M + 1) == -1
    lower = capi.default_parameters()
    lower.JtJ_packed, lower.JtJ_upper = True, False
    assert host_p(prm=lower) == -1 and dev_p(prm=lower) == -1
    # a set communicator: one rank only
    fn = capi.ALLREDUCE_FN(lambda b_, n_, c_: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert host() == -1 and host_p() == -1 and dev() == -1 and dev_p() == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert not calls


@pytest.mark.parametrize("shape", qo.PLAIN_SHAPES, ids=str)
def test_the_two_host_routes_agree_plain(shape):
    N, M = shape
    _, _, Js = qo.solved(N, M)
    cond = max(np.linalg.cond(J.T @ J) for J in Js)
    worst = max(qo.scaled_error(qo.expected(N, M, Q, route="inv"), qo.expected(N, M, Q)) for Q in qo.QROWS)
    print(f"{shape}: the two host routes differ by {worst:.3g} scaled; cond(JtJ) <= {cond:.3g}")
    assert worst <= ROUTES_TOL and cond <= 51


@pytest.mark.parametrize("case", qo.SANDWICH_CASES, ids=str)
def test_the_two_host_routes_agree_sandwich(case):
    (N, M), nobs = case
    worst = qo.scaled_error(qo.expected(N, M, 2, nobs, route="inv"), qo.expected(N, M, 2, nobs))
    print(f"{case}: the two host routes differ by {worst:.3g} scaled")
    assert worst <= ROUTES_TOL
    if nobs == 0:
        assert not qo.expected(N, M, 2, nobs).any()
