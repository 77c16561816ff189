"""The numeric-Jacobian adapter of a single problem (dogleg_amd_numeric_*), what needs no GPU: the host plan against the numpy
first-fit colouring with K and the bytes by formula, the restatement (tests/numeric_oracle.py) -- coloured equals one variable at
a time bit for bit, and an invalid colouring breaks that --, every refusal of dogleg_amd_numeric_create and _plan with its
message (all decided from the arguments before a device is touched), and the exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (CB_DEVICE_VALUES, NUMERIC_FORWARD, NUMERIC_CENTRAL, NUMERIC_DEVICE_TILE_ROWS,
                                       NUMERIC_DEVICE_LDS_SLOTS, NUMERIC_DEVICE_THREADS, NUMERIC_DEVICE_DENSE_TILE, iptr)
from tests import batch_numeric_oracle as bn
from tests import jacobian_patterns as jp
from tests import numeric_oracle as no
from tests import oracle_api as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = [NUMERIC_FORWARD, NUMERIC_CENTRAL]
NAMES = ["dogleg_amd_numeric_plan", "dogleg_amd_numeric_create", "dogleg_amd_numeric_destroy", "dogleg_amd_numeric_callback",
         "dogleg_amd_numeric_stats", "dogleg_amd_numeric_buffers"]


def arrowhead_pattern():
    """3 cameras x 8 points, 24 observations: 15 entries a row"""
    prob = oa.BAProblem(3, 8, 24)
    Jp, Ji = prob.pattern()
    N, M = prob.N, prob.M
    prob.close()
    return N, M, Jp, Ji


def sparse_patterns():
    Jp, Ji = jp.ragged_pattern()
    yield "ragged", 40, 70, Jp, Ji
    yield ("arrowhead",) + arrowhead_pattern()
    Jp, Ji = jp.full_pattern(5, 7)
    yield "full", 7, 5, Jp, Ji
    Jp, Ji = no.long_row_pattern()
    yield "long row", 120, 40, Jp, Ji


# ---- the plan ----
@pytest.mark.parametrize("scheme", SCHEMES)
def test_plan_equals_first_fit(scheme):
    for name, N, M, Jp, Ji in sparse_patterns():
        want = jp.first_fit(N, M, Jp, Ji)
        ncol = int(want.max()) + 1
        got_c, colour, K, nbytes = capi.numeric_plan(N, M, len(Ji), Jp, Ji, scheme)
        assert got_c == ncol and np.array_equal(colour, want), name
        assert K == no.n_copies(scheme, ncol) and nbytes == no.device_bytes(scheme, N, M, len(Ji), ncol), name
        # the Jacobian check's own colouring: the adapter and the check agree on the groups
        chk_c, chk = capi.jacobian_colouring(N, M, Jp, Ji)
        assert chk_c == got_c and np.array_equal(chk, colour), name
        if name == "ragged":
            assert Jp[14] == Jp[13] and colour[29] == 0 and not np.any(Ji == 29)       # an empty row, a variable in no row
        if name == "arrowhead":
            assert ncol == 15 and np.all(np.diff(Jp) == 15)
        if name == "full":
            assert np.array_equal(colour, np.arange(7))
        if name == "long row":
            assert ncol >= 100 and np.diff(Jp).max() == 100
    # the output arguments are optional
    _, N, M, Jp, Ji = next(sparse_patterns())
    assert capi.lib().dogleg_amd_numeric_plan(N, M, len(Ji), iptr(Jp), iptr(Ji), scheme, None, None, None) == int(jp.first_fit(N, M, Jp, Ji).max()) + 1


@pytest.mark.parametrize("scheme", SCHEMES)
def test_plan_of_a_dense_problem(scheme):
    """NJnnz == 0 with NULL pointers: every variable its own colour, no index arrays"""
    for N, M in ((1, 1), (7, 5), (130, 67)):
        ncol, colour, K, nbytes = capi.numeric_plan(N, M, 0, None, None, scheme)
        assert ncol == N and np.array_equal(colour, np.arange(N))
        assert K == no.n_copies(scheme, N) and nbytes == no.device_bytes(scheme, N, M, 0, N) == 8.0 * (K * (N + M) + N)


# ---- the restatement ----
def _bounds(rng, p, N):
    """a third of the variables bounded: a narrow box around p, p on either bound, and variable 3 with lo == hi"""
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    kind = rng.integers(0, 9, size=N)
    lo[kind == 0] = p[kind == 0] - 1e-9
    hi[kind == 0] = p[kind == 0] + 1e-10
    hi[kind == 1] = p[kind == 1]
    lo[kind == 2] = p[kind == 2]
    lo[3] = hi[3] = p[3]
    return lo, hi


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_coloured_equals_one_variable_at_a_time(scheme, bounded):
    """on the numpy model a row reads only its own variables, so perturbing a whole colour at once moves a row exactly as
    perturbing its one variable of that colour does: the two Jacobians are the same bits"""
    dr, da = bn.deltas(scheme)
    for name, N, M, Jp, Ji in sparse_patterns():
        a, pstar, p = no.coefficients(N, len(Ji), seed=5)
        lo, hi = _bounds(np.random.default_rng(9), p, N) if bounded else (None, None)
        values = lambda q: jp.model(Jp, Ji, a, pstar, 0.4, q)[0]
        colour = jp.first_fit(N, M, Jp, Ji)
        ncol = int(colour.max()) + 1
        x1, J1 = no.numeric_jacobian(values, scheme, p, lo, hi, dr, da, Jp, Ji, colour, ncol)
        x2, J2 = no.numeric_jacobian(values, scheme, p, lo, hi, dr, da, Jp, Ji, np.arange(N), N)
        assert x1.tobytes() == x2.tobytes() and J1.tobytes() == J2.tobytes(), name
        assert np.all(np.isfinite(J1)) and np.any(J1 != 0.0)
        if bounded:
            assert np.all(J1[Ji == 3] == 0.0) and not np.any(np.signbit(J1[Ji == 3]))
            pc, d = no.copies_coloured(scheme, p, lo, hi, dr, da, colour, ncol)
            assert d[3] == 0.0 and np.all(pc >= lo[None]) and np.all(pc <= hi[None])
        # close to the analytic Jacobian: a sanity bound only (|d2x/dp2| <= eps a^2 <= 0.4, steps below 2e-5)
        Jtrue = jp.model(Jp, Ji, a, pstar, 0.4, p)[2]
        free = np.ones(len(Ji), dtype=bool) if not bounded else (Ji != 3)
        assert np.max(np.abs(J1[free] - Jtrue[free])) <= 1e-5, name
        # the contract of the copies
        pc, d = no.copies_coloured(scheme, p, lo, hi, dr, da, colour, ncol)
        assert pc.shape == (no.n_copies(scheme, ncol), N) and pc[0].tobytes() == p.tobytes()
        for k in range(1, pc.shape[0]):
            moved = pc[k] != p
            assert np.all(colour[moved] == (k - 1) % ncol), name


@pytest.mark.parametrize("scheme", SCHEMES)
def test_an_invalid_colouring_breaks_the_equality(scheme):
    """two variables of one row given one colour: that row's quotient holds both derivatives, and the test above would fail"""
    dr, da = bn.deltas(scheme)
    N, M = 40, 70
    Jp, Ji = jp.ragged_pattern()
    a, pstar, p = no.coefficients(N, len(Ji), seed=5)
    values = lambda q: jp.model(Jp, Ji, a, pstar, 0.4, q)[0]
    colour = jp.first_fit(N, M, Jp, Ji)
    ncol = int(colour.max()) + 1
    r = next(r for r in range(M) if Jp[r + 1] - Jp[r] >= 2)
    u, v = Ji[Jp[r]], Ji[Jp[r] + 1]
    bad = colour.copy()
    bad[v] = bad[u]
    _, J_bad = no.numeric_jacobian(values, scheme, p, None, None, dr, da, Jp, Ji, bad, ncol)
    _, J_one = no.numeric_jacobian(values, scheme, p, None, None, dr, da, Jp, Ji, np.arange(N), N)
    assert J_bad.tobytes() != J_one.tobytes()
    assert abs(J_bad[Jp[r]] - J_one[Jp[r]]) > 0.05          # off by about the other entry, |a| >= 0.1 times 1 + eps cos u >= 0.6


# ---- refusals ----
def _values_cb():
    return CB_DEVICE_VALUES(lambda *a: None)


def _ptr(a):
    return None if a is None else iptr(np.ascontiguousarray(a, dtype=np.int32))


def _pattern_faults(N, M, Jp, Ji):
    """(what, Jp, Ji, nnz, a word of the message)"""
    nnz = len(Ji)
    bad = Jp.copy()
    bad[0] = 1
    yield "colptr[0]", bad, Ji, nnz, "Jt_colptr[0]"
    bad = Jp.copy()
    bad[5] = bad[4] - 1
    yield "colptr decreases", bad, Ji, nnz, "decreases"
    yield "NJnnz disagrees", Jp, Ji, nnz + 1, "disagrees with NJnnz"
    bad = Ji.copy()
    bad[2] = N
    yield "row index outside", Jp, bad, nnz, "is outside"
    r = next(r for r in range(M) if Jp[r + 1] - Jp[r] >= 2)
    bad = Ji.copy()
    bad[Jp[r]], bad[Jp[r] + 1] = bad[Jp[r] + 1], bad[Jp[r]]
    yield "not ascending", Jp, bad, nnz, "not ascending"
    yield "NULL colptr", None, Ji, nnz, "Jt_colptr"
    yield "NULL rowidx", Jp, None, nnz, "Jt_rowidx is NULL"


def test_create_and_plan_refusals(capfd):
    """every refusal, each with NULL / -1 and its message, none of which is the complaint about a missing device: they come
    first"""
    L = capi.lib()
    keep = _values_cb()
    f = C.cast(keep, C.c_void_p)
    N, M = 40, 70
    Jp, Ji = jp.ragged_pattern()
    nnz = len(Ji)

    def opts(**kw):
        return capi.numeric_options(**kw)

    def create(n, m, z, p, i, fn, opt):
        o = opt[0] if isinstance(opt, tuple) else opt
        return L.dogleg_amd_numeric_create(n, m, z, _ptr(p), _ptr(i), fn, None, C.byref(o) if o is not None else None)

    cases = [("Nstate 0", (0, M, nnz, Jp, Ji, f, None), "must not be 0"), ("Nmeas 0", (N, 0, nnz, Jp, Ji, f, None), "must not be 0"),
             ("Nstate 0 dense", (0, M, 0, None, None, f, None), "must not be 0"),
             ("NULL f", (N, M, nnz, Jp, Ji, None, None), "f is NULL"), ("NULL f dense", (N, M, 0, None, None, None, None), "f is NULL")]
    for what, p, i, z, msg in _pattern_faults(N, M, Jp, Ji):
        cases.append((what, (N, M, z, p, i, f, None), msg))
    for scheme in (2, -1):
        cases.append((f"scheme {scheme}", (N, M, nnz, Jp, Ji, f, opts(scheme=scheme)), "unknown scheme"))
    for dr, da in ((-1e-8, 0.0), (0.0, -1e-8), (float("nan"), 1e-8), (1e-8, float("nan"))):
        cases.append((f"deltas {dr} {da}", (N, M, nnz, Jp, Ji, f, opts(scheme=NUMERIC_FORWARD, delta_rel=dr, delta_abs=da)),
                      "negative or NaN"))
    lo, hi = np.full(N, -1.0), np.full(N, 1.0)
    lo[17] = 1.5
    cases.append(("lower > upper", (N, M, nnz, Jp, Ji, f, opts(scheme=NUMERIC_CENTRAL, lower=lo, upper=hi)), "variable 17"))
    nan_hi = np.full(N, 1.0)
    nan_hi[4] = np.nan
    cases.append(("a NaN bound", (N, M, 0, None, None, f, opts(scheme=NUMERIC_FORWARD, upper=nan_hi)), "variable 4"))
    # a size that does not fit: a dense problem whose Nstate + 1 copies of Nmeas doubles no device holds
    big = (2 ** 20, 2 ** 31 - 3, 0, None, None, f, None)
    cases.append(("too large", big, "too large"))
    for what, args, msg in cases:
        capfd.readouterr()
        h = create(*args)
        err = capfd.readouterr().err
        assert not h, what
        assert msg in err and "dogleg_amd_numeric_create" in err and "no HIP device" not in err, f"{what}: {err!r}"
        assert b"dogleg_amd_numeric_create" in L.dlg_last_error(), what
    for word in ("C = 1048576", "K = 1048577", "bytes", "longest row holds 1048576"):       # (the last case)
        assert word in err, err

    # the plan: the same checks of sizes, pattern, scheme and size, -1 and a message
    def plan(n, m, z, p, i, scheme):
        return L.dogleg_amd_numeric_plan(n, m, z, _ptr(p), _ptr(i), scheme, None, None, None)

    pcases = [("Nstate 0", (0, M, nnz, Jp, Ji, 0), "must not be 0"), ("Nmeas 0", (N, 0, 0, None, None, 1), "must not be 0"),
              ("scheme", (N, M, nnz, Jp, Ji, 7), "unknown scheme"), ("too large", big[:5] + (NUMERIC_CENTRAL,), "K = 2097153")]
    for what, p, i, z, msg in _pattern_faults(N, M, Jp, Ji):
        pcases.append((what, (N, M, z, p, i, 0), msg))
    for what, args, msg in pcases:
        capfd.readouterr()
        rc = plan(*args)
        err = capfd.readouterr().err
        assert rc == -1 and msg in err and "dogleg_amd_numeric_plan" in err, f"{what}: {err!r}"
        assert b"dogleg_amd_numeric_plan" in L.dlg_last_error(), what

    # valid arguments -- +-inf bounds, lower == upper, a sparse and a dense problem -- are NOT refused: without a device creation
    # reaches the device check, with one it succeeds
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    lo[3] = hi[3] = 0.25
    for args in ((N, M, nnz, Jp, Ji, f, opts(scheme=NUMERIC_CENTRAL, lower=lo, upper=hi)), (N, M, 0, None, None, f, None)):
        capfd.readouterr()
        h = create(*args)
        err = capfd.readouterr().err
        if h:
            L.dogleg_amd_numeric_destroy(h)
        else:
            assert "no HIP device" in err and b"no HIP device" in L.dlg_last_error()


def test_destroy_stats_and_buffers_take_null():
    L = capi.lib()
    L.dogleg_amd_numeric_destroy(None)
    out = (C.c_double * 6)()
    assert L.dogleg_amd_numeric_stats(None, out, 6) == 0
    assert L.dogleg_amd_numeric_buffers(None, None, None, None) == -1


# ---- exports ----
def test_exports():
    L = capi.lib()
    for name in NAMES:
        assert name in capi.DOGLEG_SYMBOLS and getattr(L, name)
    hdr = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    for name in NAMES + ["dogleg_callback_device_values_t"]:
        assert name in hdr
    src = open(os.path.join(ROOT, "libdogleg_amd", "csrc", "numeric_device.hip")).read()
    const = lambda n: int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1))
    assert (const("ND_TR"), const("ND_SLOTS"), const("ND_THREADS"), const("ND_DTR"), const("ND_DTV")) == \
        (NUMERIC_DEVICE_TILE_ROWS, NUMERIC_DEVICE_LDS_SLOTS, NUMERIC_DEVICE_THREADS, NUMERIC_DEVICE_DENSE_TILE,
         NUMERIC_DEVICE_DENSE_TILE)
    bld = open(os.path.join(ROOT, "libdogleg_amd", "build.py")).read()
    assert re.search(r'"numeric_device\.hip": \["-ffp-contract=off"\]', bld)
