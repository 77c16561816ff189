"""dogleg_amd_optimize_dense_batch against the CPU oracle: one oa.oracle_solve("dense", ...) per problem of the batch with
the host callback of the same DenseProblem (tests/batch_oracle.py).  Tolerances: |p_batch - p_oracle|_inf <= 1e-10
(tests/parity.py STEP_TOL), norm2_x and the trust region to 1e-8 relative (compare_traces' rel_scalar_tol), lambda,
iterations, evaluations and status equal.

The seeds.  A problem whose decision sits on a rounding edge can flip a branch on any implementation, so seed0 of every
shape was chosen on the CPU, with the oracle alone (batch_oracle.find_seed0), such that every problem's smallest decision
margin is above MARGIN_FLOOR = 1e-6, four decades over the 1e-10 by which the implementations may differ; the margin each
seed0 gave is written in SETS / SHAPES below and every test asserts the floor on the oracle side before it compares.
seed0 = 1 passed for all five shapes under both prescribed parameter sets (B = 257, and B = 2048 for (6, 40)).  Those
sets -- the model x = u + eps sin(u) is monotone for eps < 1 -- have no rejected trial in them, so the rejection (and
with it the retry from the cached steps and the TRUSTREGION stop) is covered by a third set of this file's own: eps =
0.95, p0_spread = 6, the default trustregion0 on the (6, 40) shape, where the search gave seed0 = 897 (3 rejected trials
in 257 problems, margin 4.5e-4).  Rejected trials are rare in this model, and where they are frequent (eps > 1) they come
with solves that creep for a hundred iterations on improvements at the rounding level of norm2(x): there rho differs
between any two implementations by more than its distance to the thresholds.  So the margin counts |rho - t| less the
rounding error of rho itself (batch_oracle.margin): such solves fall under the floor and the search passes them by."""
import ctypes as C
import functools

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS, BATCH_FAILED,
                                       BATCH_MAX_NSTATE)
from tests import oracle_api as oa
from tests import batch_oracle as bo
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu

MARGIN_FLOOR = 1e-6
REL_SCALAR_TOL = 1e-8
# name: (eps, noise, p0_spread, trustregion0)
SETS = {"diverse": (0.9, 0.01, 2.0, 1.0), "default": (0.3, 0.01, 0.5, 1.0e3), "hard": (0.95, 0.01, 6.0, 1.0e3)}
# (N, M): (B, seed0, {set: the margin the search recorded})
SHAPES = {
    (3, 12): (257, 1, {"diverse": 2.05e-3, "default": 3.22e-3}),
    (6, 40): (2048, 1, {"diverse": 1.2e-4, "default": 5.27e-4}),
    (16, 96): (257, 1, {"diverse": 1.71e-2, "default": 1.39e-2}),
    (32, 200): (257, 1, {"diverse": 2.03e-3, "default": 1.68e-3}),
    (7, 37): (257, 1, {"diverse": 6.73e-4, "default": 8.04e-4}),
}
HARD_SEED0, HARD_B, HARD_MARGIN = 897, 257, 4.51e-4


def params(setname, **over):
    prm = oa.default_params()
    prm.trustregion0 = SETS[setname][3]
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def device_batch(N, M, seeds, setname, **kw):
    from problems.batch import DeviceBatch
    eps, noise, spread, _ = SETS[setname]
    return DeviceBatch(len(seeds), M, N, seeds=np.asarray(seeds, dtype=np.uint64), eps=kw.get("eps", eps),
                       noise=kw.get("noise", noise), p0_spread=kw.get("p0_spread", spread))


@functools.lru_cache(maxsize=None)
def oracle_batch(N, M, seed0, B, setname, over=()):
    """the oracle on problems seed0 .. seed0 + B - 1 (cached: several tests share a batch)"""
    eps, noise, spread, _ = SETS[setname]
    return bo.solve_batch(M, N, range(seed0, seed0 + B), eps, noise, spread, params(setname, **dict(over)))


def assert_margin(orc, what):
    m = min(r["margin"] for r in orc)
    print(f"{what}: smallest decision margin of the oracle's solves {m:.3g}")
    assert m > MARGIN_FLOOR, f"{what}: margin {m:.3g}: the seeds no longer keep the decisions off the rounding edges"
    return m


def compare(p, res, orc, what, idx=None, p_tol=STEP_TOL):
    """every problem of the batch result against its oracle solve; prints the figures, then asserts"""
    idx = range(len(orc)) if idx is None else idx
    dp = max(float(np.max(np.abs(p[k] - orc[b]["p"]))) for k, b in enumerate(idx))
    dn = max(abs(res["norm2_x"][k] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for k, b in enumerate(idx))
    dt = max(abs(res["trustregion"][k] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for k, b in enumerate(idx))
    print(f"{what}: {len(list(idx))} problems, max |p - p_oracle| {dp:.3g}, norm2_x rel {dn:.3g}, trust region rel {dt:.3g}")
    for k, b in enumerate(idx):
        o = orc[b]
        got = (int(res["iterations"][k]), int(res["evaluations"][k]), int(res["status"][k]), float(res["lambda_"][k]))
        want = (o["iterations"], o["evaluations"], o["status"], o["lambda_"])
        assert got == want, f"{what}: problem {b}: (iterations, evaluations, status, lambda) {got}, the oracle {want}"
    assert dp <= p_tol and dn <= REL_SCALAR_TOL and dt <= REL_SCALAR_TOL


def run(db, prm):
    db.reset_counters()
    rc, p, res = capi.optimize_dense_batch(db.p0(), db.N, db.M, db.cb, db.cookie, prm)
    assert rc == 0
    # one batched callback per round, live problems only
    assert db.ncalls() == int(res["evaluations"].max()) and db.nevals() == int(res["evaluations"].sum())
    return p, res


@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_parity_over_a_batch(shape, setname):
    N, M = shape
    B, seed0, recorded = SHAPES[shape]
    orc = oracle_batch(N, M, seed0, B, setname)
    m = assert_margin(orc, f"{shape} {setname} seed0 {seed0}")
    assert abs(m - recorded[setname]) <= 0.05 * recorded[setname], "the generator changed: search seed0 again"
    types = set().union(*[o["step_types"] for o in orc])
    evals = {o["evaluations"] for o in orc}
    print(f"step types {sorted(types)}, evaluations {min(evals)} .. {max(evals)}")
    if setname == "diverse":
        assert types == {0, 1, 2} and len(evals) > 1      # (the rejected trials: test_rejected_trials_and_the_retry)
    for nb in (1, 2, B):
        db = device_batch(N, M, range(seed0, seed0 + nb), setname)
        p, res = run(db, params(setname))
        compare(p, res, orc, f"{shape} {setname} B = {nb}", idx=range(nb))
        db.close()


def test_rejected_trials_and_the_retry():
    N, M = 6, 40
    orc = oracle_batch(N, M, HARD_SEED0, HARD_B, "hard")
    m = assert_margin(orc, "hard set")
    assert abs(m - HARD_MARGIN) <= 0.05 * HARD_MARGIN
    assert sum(o["rejected"] for o in orc) >= 1 and set().union(*[o["step_types"] for o in orc]) == {0, 1, 2}
    assert len({o["evaluations"] for o in orc}) > 1
    db = device_batch(N, M, range(HARD_SEED0, HARD_SEED0 + HARD_B), "hard")
    p, res = run(db, params("hard"))
    compare(p, res, orc, "hard set")
    db.close()


@pytest.mark.parametrize("max_iterations", [1, 2, 3, 5])
def test_iterate_sequence(max_iterations):
    N, M, B, seed0 = 6, 40, 257, 1
    over = (("max_iterations", max_iterations),)
    orc = oracle_batch(N, M, seed0, B, "diverse", over)
    assert_margin(orc, f"max_iterations {max_iterations}")
    db = device_batch(N, M, range(seed0, seed0 + B), "diverse")
    p, res = run(db, params("diverse", **dict(over)))
    compare(p, res, orc, f"max_iterations {max_iterations}")
    cut = [b for b in range(B) if orc[b]["status"] == BATCH_MAX_ITERATIONS]
    assert all(orc[b]["iterations"] == max_iterations for b in cut) and (max_iterations > 2 or cut)
    assert all(res["status"][b] == BATCH_MAX_ITERATIONS for b in cut)
    db.close()


def test_all_four_stops():
    N, M = 6, 40
    # started at the optimum of a noise-free problem: x(p*) = 0
    B = 8
    db = device_batch(N, M, range(1, 1 + B), "default", noise=0.0, p0_spread=0.0)
    p0 = db.p0()
    p, res = run(db, params("default"))
    assert np.all(res["status"] == BATCH_JTX) and np.all(res["evaluations"] == 1) and np.all(res["iterations"] == 0)
    assert np.array_equal(p, p0) and np.all(res["norm2_x"] == 0.0)
    db.close()
    # ordinary solves end with a small step
    orc = oracle_batch(N, M, 1, 2048, "default")
    assert BATCH_SMALL_STEP in {o["status"] for o in orc}      # (compared in test_parity_over_a_batch)
    # a large trustregion_threshold: the first rejected trial ends the solve
    over = (("trustregion_threshold", 100.0),)
    orc = oracle_batch(N, M, HARD_SEED0, HARD_B, "hard", over)
    assert_margin(orc, "trustregion_threshold 100")
    assert BATCH_TRUSTREGION in {o["status"] for o in orc}
    db = device_batch(N, M, range(HARD_SEED0, HARD_SEED0 + HARD_B), "hard")
    p, res = run(db, params("hard", **dict(over)))
    compare(p, res, orc, "trustregion_threshold 100")
    db.close()
    # max_iterations cuts some problems and not others
    over = (("max_iterations", 4),)
    orc = oracle_batch(N, M, 1, 257, "diverse", over)
    assert_margin(orc, "max_iterations 4")
    st = {o["status"] for o in orc}
    assert BATCH_MAX_ITERATIONS in st and len(st) > 1
    db = device_batch(N, M, range(1, 258), "diverse")
    p, res = run(db, params("diverse", **dict(over)))
    compare(p, res, orc, "max_iterations 4")
    db.close()


def zero_column_oracle(prm, B=32, chosen=(3, 17, 30), zero_col=2, shape=(6, 40), seed0=1):
    """the oracle on the "default" problems seed0 .. seed0 + B - 1 of `shape`, column zero_col of J exactly zero in the chosen"""
    N, M = shape
    eps, noise, spread, _ = SETS["default"]
    return bo.solve_batch(M, N, range(seed0, seed0 + B), eps, noise, spread, prm, zero_cols={b: zero_col for b in chosen})


def _zero_column_batch(prm, B=32, chosen=(3, 17, 30), zero_col=2, shape=(6, 40)):
    from problems.batch import MODE_ZERO_COLUMN
    (N, M), seed0 = shape, 1
    orc = zero_column_oracle(prm, B, chosen, zero_col, shape, seed0)
    assert_margin(orc, f"zero-column batch {shape}")
    db = device_batch(N, M, range(seed0, seed0 + B), "default")
    mode = np.zeros(B, dtype=np.uint8)
    mode[list(chosen)] = MODE_ZERO_COLUMN
    db.set_mode(mode, zero_col)
    p, res = run(db, prm)
    db.close()
    return p, res, orc


def test_lambda_is_per_problem():
    chosen = (3, 17, 30)
    p, res, orc = _zero_column_batch(params("default"), chosen=chosen)
    for b in range(len(orc)):
        assert orc[b]["lambda_"] == (1e-10 if b in chosen else 0.0)
    # (1e-9: the tolerance tests/test_dense_gpu.py::test_dense_lambda_path uses for the singular case)
    compare(p, res, orc, "zero columns", p_tol=1e-9)


def test_lambda_moves_only_when_the_reference_would_factorise():
    # a small trust region: the first trials are clipped Cauchy steps, at a point where JtJ is singular -- no factorisation
    # is attempted, so lambda stays 0 (tests/test_edge_cases_gpu.py::test_cauchy_step_at_a_singular_point_leaves_lambda_alone)
    chosen = (3, 17, 30)
    p, res, orc = _zero_column_batch(params("default", trustregion0=1e-3, max_iterations=3), chosen=chosen)
    for b in chosen:
        assert orc[b]["step_types"] == {0} and orc[b]["lambda_"] == 0.0 and orc[b]["iterations"] == 3
    compare(p, res, orc, "clipped Cauchy steps at singular points", p_tol=1e-9)
    assert np.all(res["lambda_"] == 0.0)


def test_a_failing_problem_fails_alone():
    from problems.batch import MODE_NAN
    N, M, B, seed0 = 6, 40, 64, 1
    orc = oracle_batch(N, M, seed0, 2048, "default")[:B]
    db = device_batch(N, M, range(seed0, seed0 + B), "default")
    mode = np.zeros(B, dtype=np.uint8)
    bad = [1, 5, 63]
    mode[bad] = MODE_NAN
    db.set_mode(mode)
    p0 = db.p0()
    p, res = run(db, params("default"))
    for b in bad:
        assert res["status"][b] == BATCH_FAILED and res["norm2_x"][b] < 0 and np.array_equal(p[b], p0[b])
    good = [b for b in range(B) if b not in bad]
    compare(p[good], res[good], orc, "beside failing problems", idx=good)
    db.close()


def test_launches_do_not_depend_on_the_batch_size():
    N, M = 6, 40
    calls = {}
    for B in (1, 2048):
        db = device_batch(N, M, range(1, 1 + B), "default")
        p, res = run(db, params("default"))          # (run asserts calls == max evaluations, evaluations done == their sum)
        calls[B] = (db.ncalls(), int(res["evaluations"].max()), capi.batch_last_stats()["rounds"])
        db.close()
    print(calls)
    for B, (ncalls, emax, rounds) in calls.items():
        assert ncalls == emax == rounds


def bitwise_equal(a, b):
    """record arrays of results, field by field (the struct's padding bytes are nobody's)"""
    return all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in a.dtype.names)


def test_order_and_neighbours_do_not_matter():
    N, M, B = 6, 40, 2048
    seeds = np.arange(1, 1 + B)
    db = device_batch(N, M, seeds, "diverse")
    p, res = run(db, params("diverse"))
    db.close()
    perm = np.random.default_rng(5).permutation(B)
    db = device_batch(N, M, seeds[perm], "diverse")
    pp, resp = run(db, params("diverse"))
    db.close()
    assert pp.tobytes() == p[perm].tobytes() and bitwise_equal(resp, res[perm])
    for b in (0, 777, B - 1):
        db = device_batch(N, M, seeds[b:b + 1], "diverse")
        p1, res1 = run(db, params("diverse"))
        db.close()
        assert p1.tobytes() == p[b:b + 1].tobytes() and bitwise_equal(res1, res[b:b + 1])


def test_second_leg_single_problem_device_solves():
    """weaker: it shares the product's code.  dogleg_optimize_device2 (dense) on 32 problems of the (16, 96) batch, one
    at a time: the same end point, the same number of trials"""
    N, M, B, seed0 = 16, 96, 32, 1
    eps, noise, spread, _ = SETS["diverse"]
    db = device_batch(N, M, range(seed0, seed0 + B), "diverse")
    p, res = run(db, params("diverse"))
    db.close()
    worst = 0.0
    for b in range(B):
        prob = oa.DenseProblem(M, N, seed=seed0 + b, eps=eps, noise=noise, p0_spread=spread)
        twin = oa.DeviceTwin(prob)
        r, p1, tr = capi.optimize_device(prob.p0(), N, M, 0, None, None, twin.cb, twin.cookie, params("diverse"))
        assert r >= 0
        worst = max(worst, float(np.max(np.abs(p1 - p[b]))))
        assert tr.ntrials == int(res["evaluations"][b]) - 1 + (res["status"][b] == BATCH_SMALL_STEP)
        twin.close()
        prob.close()
    print(f"batch against single-problem device solves: max |dp| {worst:.3g}")
    assert worst <= STEP_TOL


def test_refusals_on_the_gpu():
    N, M = 6, 40
    db = device_batch(N, M, range(1, 3), "default")
    p0 = db.p0()
    rc, p, _ = capi.optimize_dense_batch(np.zeros((2, BATCH_MAX_NSTATE + 1)), BATCH_MAX_NSTATE + 1, M, db.cb, db.cookie)
    assert rc == -1 and not p.any()
    L = capi.lib()
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        rc, p, _ = capi.optimize_dense_batch(p0, N, M, db.cb, db.cookie)
        assert rc == -1 and np.array_equal(p, p0) and db.ncalls() == 0
    finally:
        L.dogleg_amd_clear_communicator()
    rc, p, res = capi.optimize_dense_batch(p0, N, M, db.cb, db.cookie)
    assert rc == 0 and np.all(res["status"] > 0)
    db.close()


def test_release_cache_between_batch_calls():
    N, M, B, seed0 = 6, 40, 64, 1
    orc = oracle_batch(N, M, seed0, 2048, "default")[:B]
    db = device_batch(N, M, range(seed0, seed0 + B), "default")
    p, res = run(db, params("default"))
    compare(p, res, orc, "before the release")
    capi.lib().dogleg_amd_release_cache()
    p, res = run(db, params("default"))
    compare(p, res, orc, "after the release")
    db.close()
    dp = oa.DenseProblem(M=96, N=16, seed=3)
    prm = oa.default_params()
    ro, po, tro = oa.oracle_solve("dense", dp.p0(), dp.N, dp.M, 0, dp.cb, dp.cookie, prm)
    rg, pg, trg = capi.optimize("dense", dp.p0(), dp.N, dp.M, 0, dp.cb, dp.cookie, prm)
    assert rg >= 0 and np.max(np.abs(pg - po)) <= STEP_TOL and trg.ntrials == tro.ntrials
