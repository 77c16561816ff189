"""The numeric-Jacobian adapter of a single problem (dogleg_amd_numeric_*) on the GPU, over the values-only model of
problems/device_values.hip.

1. the adapter's kernels alone against the numpy restatement (tests/numeric_oracle.py), bit for bit: the copies, the divisors,
   and J recomputed from the downloaded x copies;
2. whole solves through the adapter against the same solves through the naive reference callback (two launches a copy, one
   thread per entry of Jt, the colouring restated in numpy), bit for bit;
3. central differences against the CPU oracle on the numeric host problem;
4. bounds: a model that is NaN outside the box solves under the bounded entry point;
5. the adapter under dogleg_amd_check_jacobian_device, healthy and with an undeclared dependence;
6. the costs per invocation do not depend on the problem;
7. a failing model fails the solve as an analytic callback's NaN does; a handle dies on whatever device is current.

The problem of 3.  Device and host sin differ in last bits and a difference quotient divides that by the step, so the problem
was chosen on the CPU: the block-arrowhead pattern of 7 cameras x 50 points x 400 observations (N 198, M 800, 15 entries a row),
eps 0.4, spread 0.5, coefficient seed 5, trustregion0 0.3 -- six trials, two Cauchy, two interpolated and two Gauss-Newton steps.
The oracle run again with every x of the host model moved by -1, 0 or +1 ulp at random (ulp seed 7) makes the same decisions on
every trial and its steps differ from the unmoved run's by at most 3.59e-11 (ulp seed 8: 1.41e-11), recorded as ULP_SPREAD.  The
step tolerance of the comparison with the device is max(STEP_TOL, 10 x that spread) = 3.6e-10: one random draw samples the
bound and does not attain it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BatchLoss, LOSS_CAUCHY, NUMERIC_FORWARD, NUMERIC_CENTRAL, NUMERIC_DEVICE_TILE_ROWS,
                                       NUMERIC_DEVICE_LDS_SLOTS, NUMERIC_DEVICE_THREADS, Trial, dptr, iptr)
from tests import batch_numeric_oracle as bn
from tests import jacobian_patterns as jp
from tests import numeric_oracle as no
from tests import oracle_api as oa
from tests.parity import STEP_TOL, compare_traces

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = [NUMERIC_FORWARD, NUMERIC_CENTRAL]
SENTINEL = 0xA5
PAD = 16                             # sentinel doubles behind x and J: a store past the end shows
EPS = 0.4
# the problem of 3.: (shape of the block-arrowhead pattern, eps, spread, coefficient seed, trustregion0, ulp seed, the largest step
# difference between the oracle and the oracle with x moved by an ulp that the CPU search recorded)
ORACLE_CASE = ((7, 50, 400), 0.4, 0.5, 5, 0.3, 7)
ULP_SPREAD = 3.59e-11


def sentinel(n):
    return np.frombuffer(bytes([SENTINEL]) * (8 * n), dtype=np.float64).copy()


def arrowhead(shape):
    prob = oa.BAProblem(*shape)
    Jp, Ji = prob.pattern()
    N, M = prob.N, prob.M
    prob.close()
    return N, M, Jp, Ji


def values_model(N, M, Jp, Ji, seed=5, eps=EPS, spread=0.5):
    from problems.values import ValuesModel
    a, pstar, p0 = no.coefficients(N, len(Ji), seed, spread)
    return ValuesModel(N, M, Jp, Ji, a, pstar, eps), p0


def adapter(model, nnz, scheme=None, **kw):
    return capi.DeviceNumeric(model.N, model.M, nnz, model.Jp, model.Ji, model.cb, model.cookie, scheme=scheme, **kw)


def naive(model, colour, scheme, lower=None, upper=None):
    from problems.values import NaiveNumeric
    dr, da = bn.deltas(scheme)
    return NaiveNumeric(model, colour, scheme, dr, da, lower, upper)


class Stream:
    """a stream of the HIP runtime the library is linked against"""

    def __init__(self):
        self.L = capi.lib()
        self.h = C.c_void_p()
        assert self.L.hipStreamCreate(C.byref(self.h)) == 0 and self.h.value

    def sync(self):
        assert self.L.hipStreamSynchronize(self.h) == 0

    def close(self):
        assert self.L.hipStreamDestroy(self.h) == 0


def kernel_bounds(rng, p):
    """a third of the variables bounded: a narrow box around p, p on either bound, and one variable with lo == hi"""
    N = len(p)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    kind = rng.integers(0, 9, size=N)
    lo[kind == 0] = p[kind == 0] - 1e-9
    hi[kind == 0] = p[kind == 0] + 1e-10
    hi[kind == 1] = p[kind == 1]
    lo[kind == 2] = p[kind == 2]
    point = min(3, N - 1)
    lo[point] = hi[point] = p[point]
    return lo, hi, point


# ---- 1. the kernels alone ----
def check_one_invocation(stream, N, M, Jp, Ji, scheme, bounded, dense=False, seed=5):
    """one invocation on `stream`; everything the adapter wrote against the restatement.  dense: (Jp, Ji) is the full pattern the
    model needs, the adapter gets NJnnz = 0"""
    what = f"N {N} M {M} nnz {len(Ji)} scheme {scheme} bounded {bounded} dense {dense}"
    model, p = values_model(N, M, Jp, Ji, seed)
    nnz = 0 if dense else len(Ji)
    colour = np.arange(N, dtype=np.int32) if dense else jp.first_fit(N, M, Jp, Ji)
    ncol = int(colour.max()) + 1
    lo, hi, point = kernel_bounds(np.random.default_rng(100 * N + M), p) if bounded else (None, None, None)
    ad = adapter(model, nnz, scheme, lower=lo, upper=hi)
    K = no.n_copies(scheme, ncol)
    assert (ad.C, ad.K) == (ncol, K), what
    nJ = M * N if dense else nnz
    dp = capi.DeviceArray(p)
    dx, dJ = capi.DeviceArray(sentinel(M + PAD)), capi.DeviceArray(sentinel(nJ + PAD))
    ad.invoke(dp, dx, dJ, stream.h.value)
    stream.sync()
    x, J = dx.numpy(), dJ.numpy()
    pc, xc, div = ad.buffers()
    dr, da = bn.deltas(scheme)
    pc_want, div_want = no.copies_coloured(scheme, p, lo, hi, dr, da, colour, ncol)
    assert pc.tobytes() == pc_want.tobytes(), what + ": the copies"
    assert div.tobytes() == div_want.tobytes(), what + ": the divisors"
    # the model's own x: the numpy restatement to a few ulp of the row sums (sin may differ in the last bit)
    x_np = np.stack([jp.model(Jp, Ji, model.a, model.pstar, EPS, pc[k])[0] for k in range(0, K, max(1, K // 3))])
    assert np.all(np.isfinite(xc)) and np.max(np.abs(xc[::max(1, K // 3)] - x_np)) <= 1e-13, what + ": the model"
    J_want = no.jacobian_coloured(scheme, xc, div, Jp, Ji, colour, ncol)
    assert J[:nJ].tobytes() == J_want.tobytes(), what + ": J"
    assert x[:M].tobytes() == xc[0].tobytes(), what + ": x is copy 0's"
    assert x[M:].tobytes() == sentinel(PAD).tobytes() and J[nJ:].tobytes() == sentinel(PAD).tobytes(), what + ": a store past the end"
    if bounded:
        assert div[point] == 0.0 and np.all(J[:nJ][Ji == point] == 0.0) and not np.any(np.signbit(J[:nJ][Ji == point]))
        assert np.all(pc >= lo[None]) and np.all(pc <= hi[None])
    st = ad.stats()
    assert (st["invocations"], st["f_calls"], st["copies"], st["launches"]) == (1, 1, K, 2), what
    assert (model.ncalls(), model.ncopies()) == (1, K), what
    for a in (dp, dx, dJ):
        a.free()
    ad.close()
    model.close()
    return ncol


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_sparse_kernels_bit_for_bit(gpu, scheme, bounded):
    TR, lanes = NUMERIC_DEVICE_TILE_ROWS, NUMERIC_DEVICE_THREADS
    stream = Stream()
    # the ragged pattern (an empty row, a variable in no row) truncated and extended: one row, around half a tile and a whole
    # tile of the Jacobian kernel, a last tile of three rows
    Jp0, Ji0 = jp.ragged_pattern()
    for M in (1, 31, 32, 33, TR - 1, TR, TR + 1, 67, 2 * TR + 3):
        Jp, Ji = no.resized(Jp0, Ji0, M, N=40)
        check_one_invocation(stream, 40, M, Jp, Ji, scheme, bounded)
    # the small block-arrowhead pattern: 15 colours
    N, M, Jp, Ji = arrowhead((3, 8, 24))
    assert check_one_invocation(stream, N, M, Jp, Ji, scheme, bounded) == 15
    # a row longer than one workgroup's lanes (and, in either scheme, more colours than one LDS chunk stages)
    Jp, Ji = no.long_row_pattern(N=300, M=5, R=lanes + 24, long_row=2)
    assert np.diff(Jp).max() > lanes
    assert check_one_invocation(stream, 300, 5, Jp, Ji, scheme, bounded) > NUMERIC_DEVICE_LDS_SLOTS - 1
    stream.close()


def test_more_colours_than_one_lds_chunk(gpu):
    """the 100-entry-row pattern in the central scheme: the plan says that its copies do not fit one chunk of the LDS image"""
    Jp, Ji = no.long_row_pattern()
    N, M = 120, 40
    ncol, _, K, _ = capi.numeric_plan(N, M, len(Ji), Jp, Ji, NUMERIC_CENTRAL)
    chunk = (NUMERIC_DEVICE_LDS_SLOTS - 1) // 2
    assert ncol >= 100 and K >= 201 and K > NUMERIC_DEVICE_LDS_SLOTS and -(-ncol // chunk) >= 4
    stream = Stream()
    for bounded in (False, True):
        assert check_one_invocation(stream, N, M, Jp, Ji, NUMERIC_CENTRAL, bounded) == ncol
    stream.close()


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dense_kernels_bit_for_bit(gpu, scheme, bounded):
    stream = Stream()
    for N in (1, 7, 33, 64, 65, 130):
        for M in (1, 31, 33, 67):
            Jp, Ji = jp.full_pattern(M, N)
            check_one_invocation(stream, N, M, Jp, Ji, scheme, bounded, dense=True)
    stream.close()


# ---- 2. against the naive callback ----
def assert_same_solve(a, b, what):
    (ra, pa, ta), (rb, pb, tb) = a[:3], b[:3]
    assert ra == rb and ra >= 0, what + f": {ra} {rb}"
    assert pa.tobytes() == pb.tobytes(), what + ": p"
    n = ta.ntrials
    assert n == tb.ntrials and n > 1 and ta.ncallbacks == tb.ncallbacks, what + ": trial count"
    assert ta.step[:n].tobytes() == tb.step[:n].tobytes() and ta.p_trial[:n].tobytes() == tb.p_trial[:n].tobytes(), what + ": steps"
    assert bytes(ta._trials)[:n * C.sizeof(Trial)] == bytes(tb._trials)[:n * C.sizeof(Trial)], what + ": trials"


def solve_params(tr0=0.3):
    prm = oa.default_params()
    prm.max_iterations = 30
    prm.trustregion0 = tr0
    return prm


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/c/device_robust_abi.c as a shared library: the fields of a returned context through dogleg.h's own structs"""
    so = str(tmp_path_factory.mktemp("numeric") / "libdevice_robust_abi.so")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "device_robust_abi.c"), "-o", so, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    S = C.CDLL(so)
    S.robust_ctx_before.restype, S.robust_ctx_before.argtypes = C.c_void_p, [C.c_void_p]
    return S


@pytest.mark.parametrize("scheme", SCHEMES)
def test_sparse_solve_and_its_context_equal_the_naive_reference(gpu, shim, scheme):
    L = capi.lib()
    L.dogleg_amd_marginal_variances.argtypes = [C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    N, M, Jp, Ji = arrowhead((7, 50, 400))
    nnz = len(Ji)
    model, p0 = values_model(N, M, Jp, Ji)
    colour = jp.first_fit(N, M, Jp, Ji)
    ad, nv = adapter(model, nnz, scheme), naive(model, colour, scheme)
    prm = solve_params()
    a = capi.optimize_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, prm)
    b = capi.optimize_device(p0, N, M, nnz, Jp, Ji, nv.cb, nv.cookie, prm)
    assert_same_solve(a, b, f"sparse scheme {scheme}")
    assert np.max(np.abs(a[1] - model.pstar)) <= 1e-6
    # marginal variances from the factor the returned context holds
    var = []
    for cb in (ad, nv):
        p, ctx = p0.copy(), C.c_void_p()
        r = L.dogleg_optimize_device2(dptr(p), N, M, nnz, iptr(Jp), iptr(Ji), cb.cb, cb.cookie, C.byref(prm), C.byref(ctx))
        assert r == a[0] and ctx.value and p.tobytes() == a[1].tobytes()
        v = np.zeros(N)
        assert L.dogleg_amd_marginal_variances(dptr(v), shim.robust_ctx_before(ctx), ctx) == 0
        L.dogleg_freeContext(C.byref(ctx))
        var.append(v)
    assert var[0].tobytes() == var[1].tobytes() and np.all(var[0] > 0.0) and np.all(np.isfinite(var[0]))
    for o in (ad, nv, model):
        o.close()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_dense_solve_equals_the_naive_reference(gpu, scheme):
    N, M = 7, 33
    Jp, Ji = jp.full_pattern(M, N)
    model, p0 = values_model(N, M, Jp, Ji)
    ad, nv = adapter(model, 0, scheme), naive(model, np.arange(N), scheme)
    prm = solve_params()
    a = capi.optimize_device(p0, N, M, 0, None, None, ad.cb, ad.cookie, prm)
    b = capi.optimize_device(p0, N, M, 0, None, None, nv.cb, nv.cookie, prm)
    assert_same_solve(a, b, f"dense scheme {scheme}")
    assert np.max(np.abs(a[1] - model.pstar)) <= 1e-6
    for o in (ad, nv, model):
        o.close()


def box_bounds(model, p0):
    """variable i with i % 3 == 0 gets a bound half way between the optimum and the start, on the start's side -- it ends on that
    bound --, and variable 1 is held at its start by lo == hi"""
    N = model.N
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    third = np.arange(N) % 3 == 0
    mid = model.pstar + 0.5 * (p0 - model.pstar)
    up = p0 > model.pstar
    lo[third & up] = mid[third & up]
    hi[third & ~up] = mid[third & ~up]
    lo[1] = hi[1] = p0[1]
    return lo, hi, third


def test_robust_and_bounded_solves_equal_the_naive_reference(gpu):
    scheme = NUMERIC_FORWARD
    N, M, Jp, Ji = arrowhead((7, 50, 400))
    nnz = len(Ji)
    model, p0 = values_model(N, M, Jp, Ji)
    colour = jp.first_fit(N, M, Jp, Ji)
    prm = solve_params()
    ad, nv = adapter(model, nnz, scheme), naive(model, colour, scheme)
    loss = BatchLoss(LOSS_CAUCHY, 1.0, 1)
    a = capi.optimize_device_robust(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, loss, prm)
    b = capi.optimize_device_robust(p0, N, M, nnz, Jp, Ji, nv.cb, nv.cookie, loss, prm)
    assert_same_solve(a, b, "robust")
    assert a[3].tobytes() == b[3].tobytes() and np.all(a[3] > 0.0)
    ad.close()
    nv.close()
    lo, hi, third = box_bounds(model, p0)
    ad, nv = adapter(model, nnz, scheme, lower=lo, upper=hi), naive(model, colour, scheme, lo, hi)
    a = capi.optimize_device_bounded(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, lo, hi, None, prm)
    b = capi.optimize_device_bounded(p0, N, M, nnz, Jp, Ji, nv.cb, nv.cookie, lo, hi, None, prm)
    assert_same_solve(a, b, "bounded")
    p = a[1]
    assert a[4].tobytes() == b[4].tobytes() and np.all(p >= lo) and np.all(p <= hi) and p[1] == p0[1]
    on_bound = (p == lo) | (p == hi)
    print(f"bounded: {int(on_bound[third].sum())} of {int(third.sum())} bounded variables end on their bound")
    assert on_bound[third].any()
    for o in (ad, nv, model):
        o.close()


# ---- 3. against the reference's iterate sequence ----
def test_central_differences_follow_the_oracle(gpu):
    shape, eps, spread, seed, tr0, ulp_seed = ORACLE_CASE
    N, M, Jp, Ji = arrowhead(shape)
    nnz = len(Ji)
    a, pstar, p0 = no.coefficients(N, nnz, seed, spread)
    prm = solve_params(tr0)
    runs = []
    for rng in (None, np.random.default_rng(ulp_seed)):
        hp = no.NumericSparseHostProblem(N, M, Jp, Ji, a, pstar, eps, NUMERIC_CENTRAL, ulp_rng=rng)
        runs.append(oa.oracle_solve("sparse", p0, N, M, nnz, hp.cb, hp.cookie, prm))
    (ro, po, tro), (rm, pm, trm) = runs
    # the oracle with every x moved by up to one ulp: the same decisions on every trial (compare_traces asserts them)
    spread_seen = compare_traces(trm, tro, step_tol=1.0, what=("moved", "oracle"))
    tol = max(STEP_TOL, 10.0 * spread_seen)
    print(f"oracle against the oracle with x moved by an ulp: worst step difference {spread_seen:.3g} (recorded {ULP_SPREAD:.3g}), "
          f"step tolerance {tol:.3g}, {tro.ntrials} trials")
    assert tro.ntrials == 6 and abs(spread_seen - ULP_SPREAD) <= 0.05 * ULP_SPREAD, "the generator changed: choose the problem again"
    from problems.values import ValuesModel
    model = ValuesModel(N, M, Jp, Ji, a, pstar, eps)
    ad = adapter(model, nnz, NUMERIC_CENTRAL)
    rg, pg, trg = capi.optimize_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, prm)
    assert rg >= 0
    worst = compare_traces(trg, tro, step_tol=tol)
    print(f"the adapter against the oracle: worst step difference {worst:.3g}, max |p - p_oracle| {np.max(np.abs(pg - po)):.3g}")
    assert np.max(np.abs(pg - po)) <= 10.0 * tol
    assert ad.stats()["invocations"] == model.ncalls() >= trg.ncallbacks
    ad.close()
    model.close()


# ---- 4. bounds ----
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bounds_are_respected(gpu, scheme):
    N, M, Jp, Ji = arrowhead((3, 8, 24))
    nnz = len(Ji)
    model, p0 = values_model(N, M, Jp, Ji)
    lo, hi, third = box_bounds(model, p0)
    model.set_box(lo, hi)
    ad = adapter(model, nnz, scheme, lower=lo, upper=hi)
    prm = solve_params()
    r, p, tr, _, held = capi.optimize_device_bounded(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, lo, hi, None, prm)
    trials = tr.trials()
    assert r >= 0 and np.isfinite(r) and len(trials) > 1, "a point outside the box was evaluated"
    # (a trial that ends the solve before its point is evaluated carries NaN in the trace by design, so the model counts on the
    # device the points it was asked for outside the box: none, and every x of an evaluated trial is finite)
    assert model.noutside() == 0 and model.ncopies() == ad.K * model.ncalls() > 0
    assert sum(1 for t in trials if np.isfinite(t["norm2x_after"])) >= 2 and all(np.isfinite(t["norm2x_before"]) for t in trials)
    assert np.all(p >= lo) and np.all(p <= hi) and p[1] == p0[1]
    on_bound = (p == lo) | (p == hi)
    print(f"scheme {scheme}: {int(on_bound[third].sum())} of {int(third.sum())} bounded variables end on their bound, "
          f"{tr.ntrials} trials, {model.ncopies()} points evaluated")
    assert on_bound[third].any()
    # at the end point: finite everywhere, the held variable's entries exact zeros, every other variable of a row non-zero
    dp, dx, dJ = capi.DeviceArray(p), capi.DeviceArray(sentinel(M)), capi.DeviceArray(sentinel(nnz))
    ad.invoke(dp, dx, dJ)
    J = dJ.numpy()
    assert np.all(np.isfinite(J)) and np.all(J[Ji == 1] == 0.0) and np.any(Ji == 1) and np.all(J[Ji != 1] != 0.0)
    assert model.noutside() == 0
    ad.close()
    # the test can fail: the adapter WITHOUT the bounds steps outside the box there (central: on both sides of every variable
    # that sits on a bound) and the model answers NaN
    ad = adapter(model, nnz, NUMERIC_CENTRAL)
    ad.invoke(dp, dx, dJ)
    assert np.any(np.isnan(dJ.numpy())) and model.noutside() > 0
    for a in (dp, dx, dJ):
        a.free()
    ad.close()
    model.close()


# ---- 5. under the Jacobian check ----
def test_adapter_under_the_jacobian_check(gpu):
    """The forward numeric J against the checker's central differences.  The model is x_r = u + eps sin(u) with u = sum_t a_t
    (p_i - p*_i) over the at most R entries of a row, |a_t| <= 1, so |d2x_r / dp_j2| <= eps a^2 <= eps and |d3x_r / dp_j3| <= eps.
    With h = delta (|p| + 1), delta = 2^-26, the step of the adapter and D = 1e-6 the checker's (it compares the mean of the
    reported J at p -+ D / 2 with the difference of x between those points):
      truncation of the forward quotient            <= eps h_max / 2
      rounding of the forward quotient              <= 2 e_x / h_min
      truncation and rounding of the checker's own  <= eps D^2 / 24 + 2 e_x / D
      the mean of J at p -+ D / 2                   <= eps D^2 / 8 off J at p (a second difference)
    where e_x bounds the error of one computed x: R + 2 rounded additions and as many products over terms that sum to at most
    X = R max|p - p*| + eps, and sin to 2 ulp: e_x <= (2 R + 8) ulp(1) X / 2.  atol is their sum, rtol 0."""
    delta, D = 2.0 ** -26, 1e-6
    Jp_r, Ji_r = jp.ragged_pattern()
    for name, (N, M, Jp, Ji) in (("arrowhead", arrowhead((3, 8, 24))), ("ragged", (40, 70, Jp_r, Ji_r))):
        nnz, R = len(Ji), int(np.diff(Jp).max())
        model, p0 = values_model(N, M, Jp, Ji)
        ad = adapter(model, nnz, NUMERIC_FORWARD)
        h_max, h_min = delta * (np.max(np.abs(p0)) + D + 1.0), delta
        X = R * (np.max(np.abs(p0 - model.pstar)) + D + h_max) + EPS
        e_x = (2 * R + 8) * np.finfo(float).eps * X / 2.0
        atol = EPS * h_max / 2.0 + 2.0 * e_x / h_min + EPS * D * D * (1.0 / 24.0 + 1.0 / 8.0) + 2.0 * e_x / D
        out = capi.check_jacobian_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, delta=D, rtol=0.0, atol=atol)
        rep = out["report"]
        print(f"{name}: atol {atol:.3g} (e_x {e_x:.3g}), the largest |reported - observed| {rep['max_error']:.3g}")
        assert out["rc"] == 0 and (rep["nchecked"], rep["nbad"], rep["nnonfinite"], rep["noutside"]) == (nnz, 0, 0, 0), out["bad"][:4]
        assert rep["ncolours"] == ad.C and ad.stats()["invocations"] == 2 * ad.C
        if name == "ragged":
            # an undeclared dependence: the one way a wrong pattern shows.  w's colour is not among the row's, so the row must
            # not move with w's group -- and does
            colour = jp.first_fit(N, M, Jp, Ji)
            r_extra = 40
            row = Ji[Jp[r_extra]:Jp[r_extra + 1]]
            w = next(v for v in range(N) if colour[v] not in colour[row])
            model.set_faults(r_extra=r_extra, w=w, c=0.5)
            out = capi.check_jacobian_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, delta=D, rtol=0.0, atol=atol)
            print(out["report"], out["bad"][:2])
            assert out["report"]["noutside"] > 0 and out["rc"] > 0
        ad.close()
        model.close()


# ---- 6. costs ----
def test_costs_per_invocation_are_constant(gpu):
    figures = {}
    for shape, scheme in (((3, 8, 24), NUMERIC_FORWARD), ((7, 50, 400), NUMERIC_CENTRAL), ("long row", NUMERIC_FORWARD)):
        if shape == "long row":
            N, M = 120, 40
            Jp, Ji = no.long_row_pattern()
        else:
            N, M, Jp, Ji = arrowhead(shape)
        nnz = len(Ji)
        model, p0 = values_model(N, M, Jp, Ji)
        ad = adapter(model, nnz, scheme)
        r, p, tr = capi.optimize_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, solve_params())
        st = ad.stats()
        inv = st["invocations"]
        figures[(N, M, ad.C, scheme)] = (inv, st["f_calls"] / inv, st["launches"] / inv, st["copies"] / inv)
        assert np.isfinite(r) and inv >= tr.ncallbacks >= 2
        assert st["f_calls"] == inv == model.ncalls() and st["launches"] == 2 * inv
        assert st["copies"] == ad.K * inv == model.ncopies()
        assert st["ms_f"] == 0.0 and st["ms_library"] == 0.0                # no events without DOGLEG_AMD_NUMERIC_TIMING
        ad.close()
        model.close()
    print(figures)
    assert len({k[2] for k in figures}) == 2 and len({k[0] for k in figures}) == 3      # 15 and >= 100 colours, three sizes


# ---- 7. failures ----
def test_a_nan_row_fails_the_solve_as_the_analytic_callback_does(gpu):
    from problems import gradcheck as gp
    N, M, Jp, Ji = arrowhead((3, 8, 24))
    nnz = len(Ji)
    model, p0 = values_model(N, M, Jp, Ji)
    analytic = gp.SparseModel(N, M, Jp, Ji, model.a, model.pstar, EPS)
    ad = adapter(model, nnz, NUMERIC_FORWARD)
    prm = solve_params()
    good = capi.optimize_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, prm)
    assert good[0] >= 0 and good[2].ntrials > 1
    model.set_faults(r_nan=5)
    analytic.set_faults(r_nan=5)
    a = capi.optimize_device(p0, N, M, nnz, Jp, Ji, ad.cb, ad.cookie, prm)
    b = capi.optimize_device(p0, N, M, nnz, Jp, Ji, analytic.cb, analytic.cookie, prm)
    print(f"a NaN row: the adapter's solve returns {a[0]}, the analytic callback's {b[0]}")
    # neither returns a norm: the analytic model's NaN x with a finite J comes back as a NaN norm, the adapter's NaN x is also
    # a NaN row of J (the quotient of that row), which the factorisation refuses with -1.  Both leave p where it was.
    assert not (a[0] >= 0) and not (b[0] >= 0)
    assert a[1].tobytes() == b[1].tobytes() == p0.tobytes()
    for o in (ad, model, analytic):
        o.close()


def test_a_handle_is_destroyed_on_whatever_device_is_current(gpu):
    L = capi.lib()
    N, M, Jp, Ji = arrowhead((3, 8, 24))
    model, p0 = values_model(N, M, Jp, Ji)
    ad = adapter(model, len(Ji), NUMERIC_CENTRAL)
    dp, dx, dJ = capi.DeviceArray(p0), capi.DeviceArray(sentinel(M)), capi.DeviceArray(sentinel(len(Ji)))
    ad.invoke(dp, dx, dJ)
    assert np.all(np.isfinite(dJ.numpy()))
    home, cur = C.c_int(-1), C.c_int(-1)
    assert L.hipGetDevice(C.byref(home)) == 0
    other = (home.value + 1) % gpu.dlg_device_count()              # (one device: the same one)
    assert L.hipSetDevice(other) == 0
    ad.close()
    assert L.hipGetDevice(C.byref(cur)) == 0 and cur.value == other
    assert L.hipSetDevice(home.value) == 0
    for a in (dp, dx, dJ):
        a.free()
    model.close()
