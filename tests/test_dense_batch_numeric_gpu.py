"""The numeric-Jacobian adapter of the dense batch (dogleg_amd_batch_numeric_*) on the GPU, over the values-only model of
problems/device_batch_values.hip.

1. the adapter's two kernels alone against the numpy restatement (tests/batch_numeric_oracle.py), bit for bit;
2. whole solves through the adapter against the same solves through the naive reference callback (one launch of the values
   kernel per copy, one thread per entry of J), bit for bit;
3. central differences against the CPU oracle on the numeric host problem, with the tolerances of tests/test_dense_batch_gpu.py;
4. bounds: a model that is NaN outside the box solves under the bounded entry point, and fails without the adapter's bounds;
5. the costs per invocation do not depend on B;
6. the adapter under dogleg_amd_check_jacobian_device_batch;
7. a failing problem fails alone; a handle too small for the call fails every problem and touches nothing else.

The seeds of 3.  Device and host sin differ in last bits and a difference quotient amplifies that, so seed0 was chosen on the CPU
with batch_numeric_oracle.find_seed0 ON THE NUMERIC HOST PROBLEM (central differences, default deltas): seed0 = 1 for "diverse"
on (6, 40) (margin 2.71e-4) and on (7, 37) (6.73e-4), seed0 = 897 for "hard" on (6, 40) (4.51e-4), B = 257 each, all above
MARGIN_FLOOR = 1e-6.  The test also runs the oracle a second time with every x of the host model moved by -1, 0 or +1 ulp at
random and requires the same decisions and end points within the same tolerances: what the implementations may differ by does
not move these solves."""
import functools

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BatchLoss, LOSS_CAUCHY, NUMERIC_FORWARD, NUMERIC_CENTRAL,
                                       NUMERIC_TILE_ROWS)
from tests import batch_numeric_oracle as bn
from tests import test_dense_batch_gpu as tb

pytestmark = pytest.mark.gpu

TR = NUMERIC_TILE_ROWS
SENTINEL = 0xA5
# (set, (N, M)): (seed0, B, the margin the search recorded)
NUMERIC_SEEDS = {("diverse", (6, 40)): (1, 257, 2.71e-4), ("diverse", (7, 37)): (1, 257, 6.73e-4),
                 ("hard", (6, 40)): (897, 257, 4.51e-4)}


def values_batch(N, M, seeds, setname, **kw):
    from problems.batch_values import DeviceValuesBatch
    eps, noise, spread, _ = tb.SETS[setname]
    return DeviceValuesBatch(len(seeds), M, N, seeds=np.asarray(seeds, dtype=np.uint64), eps=kw.get("eps", eps),
                             noise=kw.get("noise", noise), p0_spread=kw.get("p0_spread", spread))


def adapter(vb, scheme=None, B=None, **kw):
    return capi.BatchNumeric(vb.B if B is None else B, vb.N, vb.M, vb.cb, vb.cookie, scheme=scheme, **kw)


def naive(vb, scheme, lower=None, upper=None):
    from problems.batch_values import NaiveNumeric
    dr, da = bn.deltas(scheme)
    return NaiveNumeric(vb, scheme, dr, da, lower, upper)


def sentinel(shape):
    return np.frombuffer(bytes([SENTINEL]) * (8 * int(np.prod(shape))), dtype=np.float64).reshape(shape).copy()


def dead_set(B):
    return {1: [], 3: [0, 2]}.get(B, [0, B // 2, B // 2 + 1, B - 1])


# ---- 1. the kernels alone ----
@pytest.mark.parametrize("scheme", [NUMERIC_FORWARD, NUMERIC_CENTRAL])
@pytest.mark.parametrize("N", [1, 7, 8, 33, 64])
def test_kernels_bit_for_bit(gpu, N, scheme):
    rng = np.random.default_rng(100 * N + scheme)
    for M in (1, TR - 1, TR, TR + 1, 2 * TR + 3):
        for B in (1, 3, 257):
            vb = values_batch(N, M, range(1, 1 + B), "default")
            p = vb.pstar() + rng.normal(size=(B, N))
            # a third of the entries bounded: boxes around p, p on either bound, and a box that is a point
            lo, hi = np.full((B, N), -np.inf), np.full((B, N), np.inf)
            kind = rng.integers(0, 12, size=(B, N))
            lo[kind == 0] = p[kind == 0] - 1e-9
            hi[kind == 0] = p[kind == 0] + 1e-10
            hi[kind == 1] = p[kind == 1]
            lo[kind == 2] = p[kind == 2]
            lo[kind == 3] = hi[kind == 3] = p[kind == 3]
            ad = adapter(vb, scheme, lower=lo, upper=hi)
            live = np.ones(B, dtype=np.uint8)
            live[dead_set(B)] = 0
            dp, dlive = capi.DeviceArray(p), capi.DeviceArray(live)
            dx, dJ = capi.DeviceArray(sentinel((B, M))), capi.DeviceArray(sentinel((B, M, N)))
            ad.invoke(dp, dx, dJ, dlive)
            x, J = dx.numpy((B, M)), dJ.numpy((B, M, N))
            pc, xc, div = ad.buffers()
            on = live.astype(bool)
            what = f"N {N} M {M} B {B} scheme {scheme}"
            dr, da = bn.deltas(scheme)
            pc_want, div_want = bn.copies(scheme, p, lo, hi, dr, da)
            assert pc.shape[0] == ad.K == (2 * N + 1 if scheme == NUMERIC_CENTRAL else N + 1)
            assert pc[:, on].tobytes() == pc_want[:, on].tobytes(), what + ": the copies"
            assert div[on].tobytes() == div_want[on].tobytes(), what + ": the divisors"
            assert np.all(div[on][kind[on] == 3] == 0.0)
            J_want = bn.jacobian(scheme, xc, div)
            assert np.all(np.isfinite(xc[:, on])) and J[on].tobytes() == J_want[on].tobytes(), what + ": J"
            assert np.all(J[on][:, :, :][np.broadcast_to((kind[on] == 3)[:, None, :], J[on].shape)] == 0.0)
            assert x[on].tobytes() == xc[0][on].tobytes(), what + ": x is copy 0's"
            assert x[~on].tobytes() == sentinel(x[~on].shape).tobytes(), what + ": x of a dead problem"
            assert J[~on].tobytes() == sentinel(J[~on].shape).tobytes(), what + ": J of a dead problem"
            st = ad.stats()
            assert (st["invocations"], st["f_calls"], st["copies"], st["launches"]) == (1, 1, ad.K * B, 2)
            assert vb.ncalls() == 1 and vb.ncopies() == ad.K * B and vb.nevals() == ad.K * int(on.sum())
            for a in (dp, dlive, dx, dJ):
                a.free()
            ad.close()
            vb.close()


# ---- 2. against the naive callback ----
def assert_same_solve(a, b, what):
    (pa, ra), (pb, rb) = a, b
    assert pa.tobytes() == pb.tobytes(), what + ": p"
    assert tb.bitwise_equal(ra, rb), what + ": results"


@pytest.mark.parametrize("scheme", [NUMERIC_FORWARD, NUMERIC_CENTRAL])
@pytest.mark.parametrize("case", [("diverse", (6, 40), 1), ("diverse", (7, 37), 1), ("hard", (6, 40), tb.HARD_SEED0)])
def test_solves_equal_the_naive_reference(gpu, case, scheme):
    setname, (N, M), seed0 = case
    B = 257
    vb = values_batch(N, M, range(seed0, seed0 + B), setname)
    ad, nv = adapter(vb, scheme), naive(vb, scheme)
    prm = tb.params(setname)
    rc1, p1, r1 = capi.optimize_dense_batch(vb.p0(), N, M, ad.cb, ad.cookie, prm)
    rc2, p2, r2 = capi.optimize_dense_batch(vb.p0(), N, M, nv.cb, nv.cookie, prm)
    assert rc1 == 0 and rc2 == 0 and np.all(r1["status"] != BATCH_FAILED) and len(set(r1["evaluations"])) > 1
    assert_same_solve((p1, r1), (p2, r2), f"{case} scheme {scheme}")
    for o in (ad, nv, vb):
        o.close()


def test_robust_bounded_and_uncertainty_equal_the_naive_reference(gpu):
    setname, (N, M), seed0, B = "diverse", (6, 40), 1, 257
    scheme = NUMERIC_FORWARD
    vb = values_batch(N, M, range(seed0, seed0 + B), setname)
    ad, nv = adapter(vb, scheme), naive(vb, scheme)
    prm = tb.params(setname)
    loss = BatchLoss(LOSS_CAUCHY, 0.5 * tb.SETS[setname][1], 1)
    a = capi.optimize_dense_batch_robust(vb.p0(), N, M, ad.cb, ad.cookie, loss, prm)
    b = capi.optimize_dense_batch_robust(vb.p0(), N, M, nv.cb, nv.cookie, loss, prm)
    assert a[0] == 0 and b[0] == 0 and np.all(a[2]["status"] != BATCH_FAILED)
    assert_same_solve(a[1:3], b[1:3], "robust")
    assert a[3].tobytes() == b[3].tobytes() and np.any(a[3] < 1.0)
    # the uncertainty call at the plain solve's end points
    rc, p, res = capi.optimize_dense_batch(vb.p0(), N, M, ad.cb, ad.cookie, prm)
    assert rc == 0
    ua = capi.dense_batch_uncertainty(p, N, M, ad.cb, ad.cookie, lam=res["lambda_"])
    ub = capi.dense_batch_uncertainty(p, N, M, nv.cb, nv.cookie, lam=res["lambda_"])
    assert ua["rc"] == 0 and ub["rc"] == 0 and not ua["status"].any()
    for k in ("status", "lam", "cov", "var", "factors", "scale"):
        assert ua[k].tobytes() == ub[k].tobytes(), k
    ad.close()
    nv.close()
    # bounded: the same bounds to the solve, to the adapter and to the naive reference
    lo, hi = box_bounds(vb)
    ad, nv = adapter(vb, scheme, lower=lo, upper=hi), naive(vb, scheme, lo, hi)
    a = capi.optimize_dense_batch_bounded(vb.p0(), N, M, ad.cb, ad.cookie, lo, hi, None, prm)
    b = capi.optimize_dense_batch_bounded(vb.p0(), N, M, nv.cb, nv.cookie, lo, hi, None, prm)
    assert a[0] == 0 and b[0] == 0 and np.all(a[2]["status"] != BATCH_FAILED)
    assert_same_solve(a[1:3], b[1:3], "bounded")
    assert a[3].tobytes() == b[3].tobytes() and np.any(a[3] != 0)
    for o in (ad, nv, vb):
        o.close()


# ---- 3. against the reference's iterate sequence ----
@functools.lru_cache(maxsize=None)
def numeric_oracle(setname, shape, ulp_seed=None):
    (N, M), (seed0, B, _) = shape, NUMERIC_SEEDS[(setname, shape)]
    eps, noise, spread, _ = tb.SETS[setname]
    rng = None if ulp_seed is None else np.random.default_rng(ulp_seed)
    return bn.solve_batch(M, N, range(seed0, seed0 + B), eps, noise, spread, tb.params(setname), want_margin=ulp_seed is None,
                          scheme=NUMERIC_CENTRAL, ulp_rng=rng)


@pytest.mark.parametrize("case", sorted(NUMERIC_SEEDS))
def test_central_differences_follow_the_oracle(gpu, case):
    setname, (N, M) = case
    seed0, B, recorded = NUMERIC_SEEDS[case]
    orc = numeric_oracle(setname, (N, M))
    m = tb.assert_margin(orc, f"numeric {case} seed0 {seed0}")
    assert abs(m - recorded) <= 0.05 * recorded, "the generator changed: search seed0 again"
    # the oracle again, every x of the host model moved by up to one ulp: the same decisions, the same end points
    moved = numeric_oracle(setname, (N, M), ulp_seed=7)
    res_moved = np.zeros(B, dtype=[("norm2_x", float), ("trustregion", float), ("lambda_", float), ("iterations", int),
                                   ("evaluations", int), ("status", int)])
    for b, o in enumerate(moved):
        res_moved[b] = tuple(o[k] for k in res_moved.dtype.names)
    tb.compare(np.array([o["p"] for o in moved]), res_moved, orc, f"numeric {case}: the oracle with x moved by an ulp")
    vb = values_batch(N, M, range(seed0, seed0 + B), setname)
    ad = adapter(vb, NUMERIC_CENTRAL)
    rc, p, res = capi.optimize_dense_batch(vb.p0(), N, M, ad.cb, ad.cookie, tb.params(setname))
    assert rc == 0
    tb.compare(p, res, orc, f"numeric {case}: the adapter")
    assert vb.ncalls() == int(res["evaluations"].max()) and vb.nevals() == ad.K * int(res["evaluations"].sum())
    ad.close()
    vb.close()


# ---- 4. bounds ----
def box_bounds(vb, point_every=5):
    """(lo, hi) (B, N): variable i of problem b with i % 3 == b % 3 gets a bound half way between the noise-free optimum and
    the start, on the start's side -- it ends on that bound --, and in every point_every-th problem the variable after it is
    held at its start by lo == hi"""
    p0, ps = vb.p0(), vb.pstar()
    lo, hi = np.full(p0.shape, -np.inf), np.full(p0.shape, np.inf)
    for b in range(vb.B):
        for i in range(vb.N):
            if i % 3 == b % 3:
                mid = ps[b, i] + 0.5 * (p0[b, i] - ps[b, i])
                if p0[b, i] > ps[b, i]:
                    lo[b, i] = mid
                else:
                    hi[b, i] = mid
        if b % point_every == 0:
            i = (b % 3 + 1) % vb.N
            lo[b, i] = hi[b, i] = p0[b, i]
    return lo, hi


@pytest.mark.parametrize("scheme", [NUMERIC_FORWARD, NUMERIC_CENTRAL])
def test_bounds_are_respected(gpu, scheme):
    from problems.batch import DeviceBatch
    from problems.batch_values import MODE_BOX_NAN
    setname, (N, M), seed0, B = "default", (6, 40), 1, 96
    eps, noise, spread, _ = tb.SETS[setname]
    prm = tb.params(setname)
    vb = values_batch(N, M, range(seed0, seed0 + B), setname)
    lo, hi = box_bounds(vb)
    vb.set_box(lo, hi)
    vb.set_mode(np.full(B, MODE_BOX_NAN, dtype=np.uint8))
    p0 = vb.p0()
    ad = adapter(vb, scheme, lower=lo, upper=hi)
    rc, p, res, held, _ = capi.optimize_dense_batch_bounded(p0, N, M, ad.cb, ad.cookie, lo, hi, None, prm)
    assert rc == 0
    assert not np.any(res["status"] == BATCH_FAILED), "a point outside the box was evaluated"
    assert np.all(p >= lo) and np.all(p <= hi)
    # the analytic callback on the same problems and bounds: the same held set, the same optimum to the accuracy of J
    db = DeviceBatch(B, M, N, seeds=vb.seeds, eps=eps, noise=noise, p0_spread=spread)
    rc, pa, resa, helda, _ = capi.optimize_dense_batch_bounded(p0, N, M, db.cb, db.cookie, lo, hi, None, prm)
    assert rc == 0 and not np.any(resa["status"] == BATCH_FAILED)
    # (held codes a variable on a bound whose gradient entry pushes outward.  A variable with lo == hi has a column of exact zeros
    # under the adapter, so its gradient entry is exactly 0 and its code is 0, whatever the analytic gradient says there)
    point = lo == hi
    assert np.array_equal(held[~point], helda[~point]) and not held[point].any()
    third = np.array([[i % 3 == b % 3 for i in range(N)] for b in range(B)])
    on_bound = (p == lo) | (p == hi)
    print(f"scheme {scheme}: {int(on_bound[third].sum())} of {int(third.sum())} bounded variables end on their bound, "
          f"max |p - p_analytic| {np.max(np.abs(p - pa)):.3g}")
    # (the test's own inputs: nearly all of that third -- holding a neighbour at its start moves a few optima off their bound --
    # and the analytic run ends on the same bounds)
    pa_on_bound = (pa == lo) | (pa == hi)
    assert on_bound[third].mean() > 0.9 and np.array_equal(on_bound, pa_on_bound) and np.all(held[on_bound & third & ~point] != 0)
    # a variable with lo == hi: a zero column (the divisor is 0) and it stays put
    assert point.any() and np.array_equal(p[point], p0[point])
    dp, dlive = capi.DeviceArray(p), capi.DeviceArray(np.ones(B, dtype=np.uint8))
    dx, dJ = capi.DeviceArray(sentinel((B, M))), capi.DeviceArray(sentinel((B, M, N)))
    ad.invoke(dp, dx, dJ, dlive)
    J = dJ.numpy((B, M, N))
    assert np.all(np.isfinite(J)) and np.all(J[np.broadcast_to(point[:, None, :], J.shape)] == 0.0)
    assert np.all(np.any(J != 0.0, axis=1)[~point])
    for a in (dp, dlive, dx, dJ):
        a.free()
    ad.close()
    # the adapter WITHOUT the bounds steps outside the box: the model answers NaN there and those problems fail
    ad = adapter(vb, scheme)
    rc, p2, res2, _, _ = capi.optimize_dense_batch_bounded(p0, N, M, ad.cb, ad.cookie, lo, hi, None, prm)
    assert rc == 0
    failed = res2["status"] == BATCH_FAILED
    print(f"scheme {scheme}: without the adapter's bounds {int(failed.sum())} of {B} problems fail")
    # exactly the problems the rule predicts: the solve itself keeps p inside, so a point outside is the adapter's p + h above an
    # active upper bound or a held variable (forward), or p -+ h beyond any active bound (central)
    hi_active = np.any(third & np.isfinite(hi), axis=1)
    predicted = np.ones(B, dtype=bool) if scheme == NUMERIC_CENTRAL else (hi_active | point.any(axis=1))
    assert np.array_equal(failed, predicted) and failed.sum() >= B // 2
    ad.close()
    db.close()
    vb.close()


# ---- 5. costs ----
def test_costs_do_not_depend_on_the_batch_size(gpu):
    """(the rounds are compared with the analytic run's: on the CPU the oracle's smallest decision margin over the problems 1 ..
    4096 of this set is 5.3e-4 with the analytic and 5.1e-4 with the forward numeric Jacobian, four decades over the 1e-8 by which
    a forward quotient is off, and both make the same decisions)"""
    from problems.batch import DeviceBatch
    setname, (N, M) = "default", (6, 40)
    eps, noise, spread, _ = tb.SETS[setname]
    figures, analytic_rounds = {}, {}
    for B in (1, 64, 4096):
        db = DeviceBatch(B, M, N, seeds=1, eps=eps, noise=noise, p0_spread=spread)
        rc, _, resa = capi.optimize_dense_batch(db.p0(), N, M, db.cb, db.cookie, tb.params(setname))
        assert rc == 0
        analytic_rounds[B] = capi.batch_last_stats()["rounds"]
        assert analytic_rounds[B] == db.ncalls()
        db.close()
    for scheme in (NUMERIC_FORWARD, NUMERIC_CENTRAL):
        for B in (1, 64, 4096):
            vb = values_batch(N, M, range(1, 1 + B), setname)
            ad = adapter(vb, scheme)
            rc, p, res = capi.optimize_dense_batch(vb.p0(), N, M, ad.cb, ad.cookie, tb.params(setname))
            assert rc == 0 and np.all(res["status"] != BATCH_FAILED)
            rounds = capi.batch_last_stats()["rounds"]
            st = ad.stats()
            inv = st["invocations"]
            figures[(scheme, B)] = (inv, st["f_calls"] / inv, st["launches"] / inv, st["copies"] / inv / B, rounds)
            # the analytic run's accounting holds for the adapter as it is: one invocation per round, rounds = most evaluations
            assert inv == rounds == int(res["evaluations"].max()) == analytic_rounds[B]
            assert st["f_calls"] == inv == vb.ncalls() and st["launches"] == 2 * inv
            assert st["copies"] == ad.K * B * inv == vb.ncopies()
            assert vb.nevals() == ad.K * int(res["evaluations"].sum())          # live problems only
            assert st["ms_f"] == 0.0 and st["ms_library"] == 0.0                # no events without DOGLEG_AMD_BATCH_TIMING
            ad.close()
            vb.close()
    print(figures)


# ---- 6. under the Jacobian check ----
def test_adapter_under_the_jacobian_check(gpu):
    """The forward numeric J against the checker's central differences.  The model is x_r = u + eps sin(u) - noise n_r with
    u = sum_j c_rj (p_j - p*_j), |c_rj| <= 1 / sqrt(N), so |d2x_r / dp_j2| <= eps c_rj^2 <= eps / N and |d3x_r / dp_j3| <= eps /
    N^1.5.  With h = delta (|p| + 1), delta = 2^-26, the step of the adapter and D = 1e-6 the checker's:
      truncation of the forward quotient            <= (eps / N) h_max / 2
      rounding of the forward quotient              <= 2 e_x / h_min
      truncation and rounding of the checker's own  <= (eps / N^1.5) D^2 / 24 + 2 e_x / D
      reported is the mean of J at p -+ D / 2       <= (eps / N^1.5) D^2 / 8 off J at p (a second difference)
    where e_x bounds the error of one computed x: N + 2 rounded additions and as many products over terms that sum to at most
    X = sqrt(N) max|p - p*| + eps + noise, and sin to 2 ulp: e_x <= (2 N + 8) ulp(1) X / 2.  atol is their sum, rtol 0."""
    setname, (N, M), B = "default", (6, 40), 64
    eps, noise, spread, _ = tb.SETS[setname]
    vb = values_batch(N, M, range(1, 1 + B), setname)
    ad = adapter(vb, NUMERIC_FORWARD)
    p0 = vb.p0()
    delta, D = 2.0 ** -26, 1e-6
    h_max, h_min = delta * (np.max(np.abs(p0)) + D + 1.0), delta
    X = np.sqrt(N) * (np.max(np.abs(p0 - vb.pstar())) + D + h_max) + eps + noise
    e_x = (2 * N + 8) * np.finfo(float).eps * X / 2.0
    atol = (eps / N) * h_max / 2.0 + 2.0 * e_x / h_min + (eps / N ** 1.5) * D * D * (1.0 / 24.0 + 1.0 / 8.0) + 2.0 * e_x / D
    out = capi.check_jacobian_device_batch(p0, N, M, ad.cb, ad.cookie, delta=D, rtol=0.0, atol=atol)
    worst = max(r["max_error"] for r in out["reports"])
    print(f"atol {atol:.3g} (e_x {e_x:.3g}), the largest |reported - observed| {worst:.3g}")
    assert out["rc"] == 0
    assert all(r["nchecked"] == N * M and r["nbad"] == 0 and r["nnonfinite"] == 0 for r in out["reports"]), out["bad"][:4]
    assert ad.stats()["invocations"] == 2 * N
    # the check can fail: a step a thousand times larger leaves a truncation error above atol
    coarse = adapter(vb, NUMERIC_FORWARD, delta_rel=2.0 ** -6, delta_abs=2.0 ** -6)
    out = capi.check_jacobian_device_batch(p0, N, M, coarse.cb, coarse.cookie, delta=D, rtol=0.0, atol=atol)
    assert out["rc"] == 0 and sum(r["nbad"] for r in out["reports"]) > 0
    coarse.close()
    ad.close()
    vb.close()


# ---- 7. failures ----
def test_a_failing_problem_fails_alone(gpu):
    from problems.batch_values import MODE_NAN
    setname, (N, M), B = "default", (6, 40), 64
    vb = values_batch(N, M, range(1, 1 + B), setname)
    ad = adapter(vb, NUMERIC_FORWARD)
    prm = tb.params(setname)
    p0 = vb.p0()
    rc, pg, rg = capi.optimize_dense_batch(p0, N, M, ad.cb, ad.cookie, prm)
    assert rc == 0 and np.all(rg["status"] != BATCH_FAILED)
    mode = np.zeros(B, dtype=np.uint8)
    bad = [1, 5, 63]
    mode[bad] = MODE_NAN
    vb.set_mode(mode)
    rc, p, res = capi.optimize_dense_batch(p0, N, M, ad.cb, ad.cookie, prm)
    assert rc == 0
    for b in bad:
        assert res["status"][b] == BATCH_FAILED and res["norm2_x"][b] < 0 and np.array_equal(p[b], p0[b])
    good = [b for b in range(B) if b not in bad]
    assert p[good].tobytes() == pg[good].tobytes() and tb.bitwise_equal(res[good], rg[good])
    ad.close()
    vb.close()


def test_a_variable_the_model_ignores_gives_a_zero_column(gpu):
    """the model's MODE_ZERO_COLUMN: both x of the quotient are the same bits, so the column is exactly zero and the solve takes
    the lambda path there (as tests/test_dense_batch_gpu.py::test_lambda_is_per_problem with the analytic zero column)"""
    from problems.batch_values import MODE_ZERO_COLUMN
    setname, (N, M), B, chosen, zero_col = "default", (6, 40), 32, [3, 17, 30], 2
    vb = values_batch(N, M, range(1, 1 + B), setname)
    mode = np.zeros(B, dtype=np.uint8)
    mode[chosen] = MODE_ZERO_COLUMN
    vb.set_mode(mode, zero_col)
    ad, nv = adapter(vb, NUMERIC_FORWARD), naive(vb, NUMERIC_FORWARD)
    rc, p, res = capi.optimize_dense_batch(vb.p0(), N, M, ad.cb, ad.cookie, tb.params(setname))
    rc2, p2, res2 = capi.optimize_dense_batch(vb.p0(), N, M, nv.cb, nv.cookie, tb.params(setname))
    assert rc == 0 and rc2 == 0 and np.all(res["status"] != BATCH_FAILED)
    assert_same_solve((p, res), (p2, res2), "zero columns")
    want = np.where(np.isin(np.arange(B), chosen), 1e-10, 0.0)
    assert np.array_equal(res["lambda_"], want)
    assert np.array_equal(p[chosen, zero_col], vb.p0()[chosen, zero_col])
    for o in (ad, nv, vb):
        o.close()


def test_a_handle_too_small_fails_every_problem(gpu, capfd):
    setname, (N, M), B, Bh = "default", (6, 40), 8, 4
    vb = values_batch(N, M, range(1, 1 + B), setname)
    ad = adapter(vb, NUMERIC_FORWARD, B=Bh)
    p0 = vb.p0()
    capfd.readouterr()
    rc, p, res = capi.optimize_dense_batch(p0, N, M, ad.cb, ad.cookie, tb.params(setname))
    assert rc == 0 and np.all(res["status"] == BATCH_FAILED) and np.array_equal(p, p0)
    st = ad.stats()
    assert vb.ncalls() == 0 and st["f_calls"] == 0 and st["copies"] == 0 and st["launches"] == st["invocations"] >= 1
    # the adapter directly: NaN into x of the live problems and nothing else; the handle's own buffers stay as they were
    before = ad.buffers(B=Bh)
    live = np.ones(B, dtype=np.uint8)
    live[[0, 5]] = 0
    dp, dlive = capi.DeviceArray(p0), capi.DeviceArray(live)
    dx, dJ = capi.DeviceArray(sentinel((B, M))), capi.DeviceArray(sentinel((B, M, N)))
    ad.invoke(dp, dx, dJ, dlive, B=B)
    x, J = dx.numpy((B, M)), dJ.numpy((B, M, N))
    on = live.astype(bool)
    assert np.all(np.isnan(x[on])) and x[~on].tobytes() == sentinel(x[~on].shape).tobytes()
    assert J.tobytes() == sentinel(J.shape).tobytes()
    after = ad.buffers(B=Bh)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after)) and vb.ncalls() == 0
    err = capfd.readouterr().err
    assert err.count("dogleg_amd_batch_numeric_callback") == 1, "one message, however often it happens"
    # the same handle still serves a call it is large enough for
    vs = values_batch(N, M, range(1, 1 + Bh), setname)
    a2 = adapter(vs, NUMERIC_FORWARD)
    rc, p2, r2 = capi.optimize_dense_batch(vs.p0(), N, M, a2.cb, a2.cookie, tb.params(setname))
    assert rc == 0 and np.all(r2["status"] != BATCH_FAILED)
    for a in (dp, dlive, dx, dJ):
        a.free()
    for o in (a2, vs, ad, vb):
        o.close()


def test_device_bounds_are_read_where_they_lie(gpu):
    """(the refusals of create are decided from the arguments: tests/test_dense_batch_numeric_cpu.py)"""
    setname, (N, M), B = "default", (6, 40), 5
    vb = values_batch(N, M, range(1, 1 + B), setname)
    p = vb.p0()
    lo, hi = p - 1e-9, p.copy()
    dlo, dhi = capi.DeviceArray(lo), capi.DeviceArray(hi)
    a_dev = adapter(vb, NUMERIC_CENTRAL, lower=dlo, upper=dhi, bounds_on_device=True)
    a_host = adapter(vb, NUMERIC_CENTRAL, lower=lo, upper=hi)
    outs = []
    for ad in (a_dev, a_host):
        dp, dlive = capi.DeviceArray(p), capi.DeviceArray(np.ones(B, dtype=np.uint8))
        dx, dJ = capi.DeviceArray(sentinel((B, M))), capi.DeviceArray(sentinel((B, M, N)))
        ad.invoke(dp, dx, dJ, dlive)
        outs.append((dJ.numpy((B, M, N)),) + ad.buffers())
        for a in (dp, dlive, dx, dJ):
            a.free()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
    assert np.all(outs[0][1] <= hi[None]) and np.all(outs[0][1] >= lo[None])
    for o in (a_dev, a_host, dlo, dhi):
        (o.close if hasattr(o, "close") else o.free)()
    vb.close()
