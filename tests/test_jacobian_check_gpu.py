"""dogleg_amd_check_jacobian_device{,_batch} and dogleg_amd_testGradient_device on the GPU, against models whose every
value the test restates in numpy from the pattern, coefficients, p*, eps and p0 it generated itself
(problems/device_gradcheck_problems.hip evaluates them; tests/jacobian_patterns.py restates them).

delta = 1e-6, rtol = 0, atol = 1e-7 unless stated: the rounding floor of the central difference is about
2 eps |x| / delta ~ 1e-9 for |x| of a few, so atol sits about 100 times above it; an injected factor of 1.01 on an entry
a (1 + eps cos u) with |a| >= 0.1 and eps <= 0.4 is an error of at least 6e-4."""
import ctypes as C

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import JACOBIAN_ONE_AT_A_TIME, dptr, iptr
from problems import gradcheck as gp
from tests import oracle_api as oa
from tests import jacobian_patterns as jp

pytestmark = pytest.mark.gpu

DELTA, ATOL = 1e-6, 1e-7
FACTOR = 1.01
COUNTS = ("nchecked", "nbad", "nnonfinite", "noutside")


def _coefs(rng, n):
    """|a| in [0.1, 1], either sign"""
    return rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)


def _sparse(N, M, Jp, Ji, seed, eps, spread=0.5):
    rng = np.random.default_rng(seed)
    a, pstar = _coefs(rng, len(Ji)), rng.uniform(-1.0, 1.0, N)
    p0 = pstar + spread * rng.uniform(-1.0, 1.0, N)
    return gp.SparseModel(N, M, Jp, Ji, a, pstar, eps), a, pstar, p0


def _ba(shape, seed=3, eps=0.3):
    prob = oa.BAProblem(*shape)
    Jp, Ji = prob.pattern()
    return (prob.N, prob.M, Jp, Ji) + _sparse(prob.N, prob.M, Jp, Ji, seed, eps)


def _check(model, p0, nnz=None, **kw):
    nnz = model.nnz if nnz is None else nnz
    kw.setdefault("delta", DELTA)
    kw.setdefault("atol", ATOL)
    return capi.check_jacobian_device(p0, model.N, model.M, nnz, model.Jp, model.Ji, model.cb, model.cookie, **kw)


def _assert_clean(rep, nchecked, ncolours):
    assert (rep["nbad"], rep["noutside"], rep["nnonfinite"]) == (0, 0, 0), rep
    assert rep["nchecked"] == nchecked and rep["ncolours"] == ncolours and rep["evaluations"] == 2 * ncolours, rep
    assert 0.0 < rep["max_error"] <= ATOL, rep


def test_honest_sparse_model(gpu):
    stats = []
    for shape in [(3, 8, 24), (7, 50, 400)]:
        N, M, Jp, Ji, model, a, pstar, p0 = _ba(shape)
        assert np.all(np.diff(Jp) == 15)
        out = _check(model, p0)
        print(shape, out["report"])
        assert out["rc"] == 0 and not out["bad"]
        _assert_clean(out["report"], len(Ji), 15)
        assert model.ncalls() == 30
        assert np.all(out["var_error"] <= ATOL) and out["var_error"].max() == out["report"]["max_error"]
        stats.append(capi.check_jacobian_last_stats())
    # the second shape has 800 entries a colour, more than one workgroup: the counts do not depend on the size
    assert stats[0] == stats[1] and stats[0]["callbacks"] == 30 and stats[0]["syncs"] == 1, stats


def test_coloured_equals_one_at_a_time(gpu):
    N, M, Jp, Ji, model, a, pstar, p0 = _ba((3, 8, 24))
    col = _check(model, p0)
    assert model.ncalls() == 30
    model.reset()
    one = _check(model, p0, flags=JACOBIAN_ONE_AT_A_TIME)
    assert model.ncalls() == 2 * N == 96
    assert col["rc"] == one["rc"] == 0
    rc, ro = col["report"], one["report"]
    assert (rc["ncolours"], ro["ncolours"]) == (15, N)
    for k in COUNTS + ("max_error", "max_error_relative", "worst_var", "worst_meas", "worst_reported", "worst_observed"):
        assert rc[k] == ro[k], (k, rc[k], ro[k])                 # bitwise: a row's x and J depend on its own variables only
    assert np.array_equal(col["var_error"], one["var_error"])
    assert rc["worst_var"] >= 0 and col["var_error"][rc["worst_var"]] == rc["max_error"]


def test_fault_in_one_reported_entry(gpu):
    N, M, Jp, Ji, model, a, pstar, p0 = _ba((3, 8, 24))
    t_bad = 15 * 17 + 6
    meas, var = 17, int(Ji[t_bad])
    model.set_faults(t_bad=t_bad, factor=FACTOR)
    out = _check(model, p0)
    rep = out["report"]
    print(rep, out["bad"])
    assert out["rc"] == 1 and rep["nbad"] == 1 and rep["noutside"] == 0 and rep["nnonfinite"] == 0 and rep["nchecked"] == len(Ji)
    problem, bvar, bmeas, reported, observed = out["bad"][0]
    assert (problem, bvar, bmeas) == (0, var, meas)
    x, u, J = jp.model(Jp, Ji, a, pstar, 0.3, p0)
    want = (FACTOR - 1.0) * a[t_bad] * (1.0 + 0.3 * np.cos(u[meas]))
    assert abs(want) >= 6e-4 and abs((reported - observed) - want) <= 1e-7
    assert (rep["worst_var"], rep["worst_meas"]) == (var, meas)
    assert (rep["worst_reported"], rep["worst_observed"]) == (reported, observed)
    assert rep["max_error"] == abs(reported - observed)
    assert np.array_equal(np.nonzero(out["var_error"] > ATOL)[0], [var])


def test_fault_in_a_row_outside_the_pattern(gpu):
    N, M = 40, 70
    Jp, Ji = jp.ragged_pattern(N, M)
    colour = jp.first_fit(N, M, Jp, Ji)
    model, a, pstar, p0 = _sparse(N, M, Jp, Ji, seed=5, eps=0.4)
    out = _check(model, p0)
    _assert_clean(out["report"], len(Ji), int(colour.max()) + 1)
    r_extra = 40
    row = Ji[Jp[r_extra]:Jp[r_extra + 1]]
    assert len(row) >= 1
    # a variable whose colour the row does not hold: the row must not move with that colour
    w = next(v for v in range(N) if colour[v] not in colour[row])
    c = 0.5
    model.set_faults(r_extra=r_extra, w=w, c=c)
    out = _check(model, p0)
    rep = out["report"]
    print(rep, out["bad"])
    assert rep["noutside"] == 1 and rep["nbad"] == 0 and out["rc"] == 1
    problem, bvar, bmeas, reported, observed = out["bad"][0]
    assert (problem, bvar, bmeas, reported) == (0, -1 - int(colour[w]), r_extra, 0.0) and abs(observed - c) <= 1e-7
    # a variable outside the row whose colour the row does hold: that entry of the row turns bad instead
    w2 = next(v for v in range(N) if v not in row and colour[v] in colour[row] and any(Ji == v))
    v_hit = int(row[list(colour[row]).index(colour[w2])])
    model.set_faults(r_extra=r_extra, w=w2, c=c)
    out = _check(model, p0)
    rep = out["report"]
    print(rep, out["bad"])
    assert rep["noutside"] == 0 and rep["nbad"] == 1 and out["rc"] == 1
    assert out["bad"][0][:3] == (0, v_hit, r_extra)
    assert abs((out["bad"][0][3] - out["bad"][0][4]) + c) <= 1e-7


def test_fault_nan_measurement(gpu):
    N, M, Jp, Ji, model, a, pstar, p0 = _ba((3, 8, 24))
    r_nan = 5
    model.set_faults(r_nan=r_nan)
    out = _check(model, p0)
    rep = out["report"]
    print(rep)
    assert rep["nnonfinite"] == 15 == rep["nbad"] and rep["noutside"] == 0 and rep["nchecked"] == len(Ji)
    assert np.isfinite(rep["max_error"]) and 0.0 < rep["max_error"] <= ATOL
    assert out["rc"] == 15 and all(b[2] == r_nan and np.isnan(b[4]) for b in out["bad"])
    assert sorted(b[1] for b in out["bad"]) == sorted(Ji[Jp[r_nan]:Jp[r_nan + 1]].tolist())
    assert np.all(np.isfinite(out["var_error"])) and np.all(out["var_error"] <= ATOL)


@pytest.mark.parametrize("M,N", [(40, 6), (70, 33)])
def test_dense_single_problem(gpu, M, N):
    Jp, Ji = jp.full_pattern(M, N)
    model, a, pstar, p0 = _sparse(N, M, Jp, Ji, seed=7, eps=0.3, spread=0.3)
    out = _check(model, p0, nnz=0, delta=0.0)                    # NJnnz = 0: the dense path; delta <= 0: the reference's
    print(out["report"])
    assert out["rc"] == 0
    _assert_clean(out["report"], M * N, N)
    assert model.ncalls() == 2 * N
    assert np.all(out["var_error"] <= ATOL) and out["var_error"].max() == out["report"]["max_error"]
    # the same problem as a sparse one with a full pattern: the other compare kernel, the same numbers
    model.reset()
    sp = _check(model, p0)
    assert sp["report"] == out["report"] and np.array_equal(sp["var_error"], out["var_error"])
    meas, var = M - 3, N - 2
    model.set_faults(t_bad=meas * N + var, factor=FACTOR)
    out = _check(model, p0, nnz=0)
    rep = out["report"]
    assert out["rc"] == 1 and rep["nbad"] == 1 and out["bad"][0][:3] == (0, var, meas)
    x, u, J = jp.model(Jp, Ji, a, pstar, 0.3, p0)
    want = (FACTOR - 1.0) * a[meas * N + var] * (1.0 + 0.3 * np.cos(u[meas]))
    assert abs((out["bad"][0][3] - out["bad"][0][4]) - want) <= 1e-7
    assert (rep["worst_var"], rep["worst_meas"]) == (var, meas)
    assert np.array_equal(np.nonzero(out["var_error"] > ATOL)[0], [var])


@pytest.mark.parametrize("B,N,M", [(5, 6, 40), (37, 16, 96), (3, 32, 70), (4, 1, 3)])
def test_batch(gpu, B, N, M):
    rng = np.random.default_rng(100 + B)
    eps = 0.3
    coef = _coefs(rng, B * M * N).reshape(B, M, N)
    pstar = rng.uniform(-1.0, 1.0, (B, N))
    p0 = pstar + 0.3 * rng.uniform(-1.0, 1.0, (B, N))
    model = gp.BatchModel(coef, pstar, eps)
    out = capi.check_jacobian_device_batch(p0, N, M, model.cb, model.cookie, delta=DELTA, atol=ATOL)
    assert out["rc"] == 0 and not out["bad"]
    assert model.ncalls() == 2 * N and model.notlive() == 0      # whatever B is; every live byte 1
    for b in range(B):
        _assert_clean(out["reports"][b], M * N, N)
    stats = capi.check_jacobian_last_stats()
    assert stats["callbacks"] == 2 * N and stats["syncs"] == 1
    honest = out["reports"]

    bs, r, v = B // 2, M - 1, N // 2
    model.set_fault(bs, r, v, FACTOR)
    out = capi.check_jacobian_device_batch(p0, N, M, model.cb, model.cookie, delta=DELTA, atol=ATOL)
    assert out["rc"] == 0 and len(out["bad"]) == 1
    for b in range(B):
        if b != bs:
            assert out["reports"][b] == honest[b]                # untouched by the neighbour's fault, bit for bit
    rep = out["reports"][bs]
    assert rep["nbad"] == 1 and rep["nnonfinite"] == 0 and (rep["worst_var"], rep["worst_meas"]) == (v, r)
    problem, bvar, bmeas, reported, observed = out["bad"][0]
    assert (problem, bvar, bmeas) == (bs, v, r)
    u = np.sum(coef[bs, r] * (p0[bs] - pstar[bs]))
    want = (FACTOR - 1.0) * coef[bs, r, v] * (1.0 + eps * np.cos(u))
    assert abs(want) >= 6e-4 and abs((reported - observed) - want) <= 1e-7

    # a problem alone (B = 1) gives the report it has inside the batch, bit for bit: the faulty one and an honest one
    for b in {bs, 0}:
        alone = gp.BatchModel(coef[b:b + 1], pstar[b:b + 1], eps)
        if b == bs:
            alone.set_fault(0, r, v, FACTOR)
        one = capi.check_jacobian_device_batch(p0[b:b + 1], N, M, alone.cb, alone.cookie, delta=DELTA, atol=ATOL)
        assert one["rc"] == 0 and one["reports"][0] == out["reports"][b], b
        assert [e[1:] for e in one["bad"]] == [e[1:] for e in out["bad"] if e[0] == b]
        alone.close()
    model.close()


def _table(text):
    lines = text.strip().splitlines()
    return lines[0], np.array([[float(t) for t in ln.split()] for ln in lines[1:]])


def test_testGradient_device_prints_the_reference_table(gpu, capfd):
    prob = oa.BAProblem(3, 8, 24)
    twin = oa.DeviceTwin(prob)
    Jp, Ji = prob.pattern()
    p0 = prob.p0()
    var = 7
    libc = C.CDLL(None)
    capfd.readouterr()
    gpu.dogleg_amd_testGradient_device(var, dptr(p0), prob.N, prob.M, prob.nnz, iptr(Jp), iptr(Ji), twin.cb, twin.cookie)
    libc.fflush(None)
    dev = capfd.readouterr().out
    gpu.dogleg_testGradient.argtypes = [C.c_uint, C.POINTER(C.c_double), C.c_uint, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    gpu.dogleg_testGradient.restype = None
    gpu.dogleg_testGradient(var, dptr(p0), prob.N, prob.M, prob.nnz, prob.cb, prob.cookie)
    libc.fflush(None)
    host = capfd.readouterr().out
    assert twin.neval() == 2
    hd, td = _table(dev)
    hh, th = _table(host)
    assert hd == hh == "# ivar imeasurement gradient_reported gradient_observed error error_relative"
    assert td.shape == th.shape == (prob.M, 6)
    assert np.array_equal(td[:, :2], th[:, :2]) and np.all(td[:, 0] == var) and np.array_equal(td[:, 1], np.arange(prob.M))
    declared = np.array([var in Ji[Jp[r]:Jp[r + 1]] for r in range(prob.M)])
    assert declared.any() and np.all(td[~declared, 2] == 0.0) and np.all(td[declared, 2] != 0.0)
    # printed at 6 digits; the device's sin / cos differ from the host's in the last bits
    assert np.all(np.abs(td[:, 2] - th[:, 2]) <= 2e-6 * np.abs(th[:, 2]))
    assert np.all(np.abs(td[:, 3] - th[:, 3]) <= 1e-7)
    stats = capi.check_jacobian_last_stats()
    assert (stats["callbacks"], stats["launches"], stats["syncs"]) == (2, 2, 1)
    twin.close()
