"""dogleg_amd_optimize_dense_batch_bounded and its device twin.

The reference is the NumPy oracle of tests/batch_bounds_oracle.py on the host model of the same problems (tests/
test_dense_batch_bounds_cpu.py holds it against the robust oracle, against exact bounded solutions and on the fallback
example).  Tolerances, the project's: |p - p_oracle|_inf <= STEP_TOL = 1e-10, F (norm2_x), the trust region and every weight
to REL_SCALAR_TOL = 1e-8 relative; lambda, iterations, evaluations, status and held equal.  The figures are printed before
they are asserted.

The bounds of the synthetic batches.  With p* the optimum the unbounded oracle finds from the start point p0, problem b gets
a bound on its variables i = b mod 3 (on every variable where a case says so), half way between start and optimum:
p*_i + 0.5 (p0_i - p*_i), a lower bound where the start lies above the optimum and an upper bound where it lies below.  The
start point is feasible, the unbounded optimum is not, so the solve has to run into the bound and hold it.

The seeds.  Every batch was chosen on the CPU, with the oracle alone, such that every problem's smallest decision margin
(the plain loop's, and those of the held set, the clip and the fallback: tests/batch_bounds_oracle.py) is above MARGIN_FLOOR =
1e-6 -- no problem is left out; the margin each batch gave is written beside it and asserted, to 5 %, before anything is
compared.  Seeds 1 .. B passed wherever they are used.

The stopping thresholds.  A problem that ends on a bound ends with a large residual (the bound keeps it half way from its
optimum), and on a large-residual problem Gauss-Newton converges linearly, not quadratically.  Solved to the default 1e-8 the
last steps improve F by less than its rounding error: their gain ratios are noise on any implementation (negative margins on
the oracle, on seeds 1 .. 65 and on every other range).  As the planted batch of tests/test_dense_batch_robust_gpu.py does for
the same reason, the batches here stop at update_threshold = Jt_x_threshold = 1e-6 (STOP_OVER), before that; the "hard" batch
of the rejected trials, whose residuals are larger still, at 1e-5."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BATCH_JTX, BATCH_NOT_RUN, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BatchLoss,
                                       LOSS_TRIVIAL, LOSS_HUBER)
from problems.batch_linear import LinearDeviceBatch, exact_bounded_solution, from_normal_equations
from tests import batch_oracle as bo
from tests import batch_bounds_oracle as bb
from tests import batch_robust_oracle as ro
from tests import dense_batch_shapes as ds
from tests import dense_batch_wide_shapes as ws
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MARGIN_FLOOR, REL_TOL = tb.MARGIN_FLOOR, tb.REL_SCALAR_TOL
GUARD = td.GUARD
HELD_GUARD = 0x5A
KKT_TOL = 1e-9
STOP_OVER = (("update_threshold", 1e-6), ("Jt_x_threshold", 1e-6))
NEAR = 0.5                              # Huber's scale in units of noise sqrt(featureSize), as tests/test_dense_batch_robust_gpu.py


def params(setname, over=STOP_OVER):
    return tb.params(setname, **dict(over))


def loss_pair(setname, kind, fs):
    """(the oracle's loss, the library's loss or None)"""
    if kind is None:
        return ro.Loss(LOSS_TRIVIAL, 1.0, 1), None
    scale = NEAR * tb.SETS[setname][1] * float(np.sqrt(fs))
    return ro.Loss(kind, scale, fs), BatchLoss(kind, scale, fs)


def bounds_between(p0, pstar, b, every=False, frac=0.5):
    """(lo, hi) of problem b: the module's docstring; frac: where between the optimum (0) and the start (1) the bound lies"""
    N = len(p0)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    for i in range(N):
        if every or i % 3 == b % 3:
            mid = pstar[i] + frac * (p0[i] - pstar[i]) if frac != 1.0 else p0[i]
            if p0[i] > pstar[i]:
                lo[i] = mid
            else:
                hi[i] = mid
    return lo, hi


@functools.lru_cache(maxsize=None)
def oracle_batch(N, M, seeds, setname, kind=None, fs=1, every=False, over=STOP_OVER, frac=0.5):
    """(the bounded oracle's solves, lo (B, N), hi (B, N)) of the problems `seeds` (a tuple); cached: the tests share batches.
    p* is the optimum of the unbounded oracle under the set's own parameters, the bounded solve runs under `over`"""
    eps, noise, spread, _ = tb.SETS[setname]
    loss = loss_pair(setname, kind, fs)[0]
    out, los, his = [], [], []
    for b, s in enumerate(seeds):
        hp = bo.HostProblem(M, N, int(s), eps, noise, spread)
        free = ro.solve_one(hp, tb.params(setname), loss)
        lo, hi = bounds_between(hp.p0(), free["p"], b, every, frac)
        out.append(bb.solve_one(hp, tb.params(setname, **dict(over)), loss, lo, hi))
        los.append(lo)
        his.append(hi)
        hp.dp.close()
    return out, np.array(los), np.array(his)


def run(db, prm, lo, hi, loss=None, p0=None):
    """the host-pointer call: (p, results, held, weights); one batched callback per round, live problems only"""
    db.reset_counters()
    rc, p, res, held, w = capi.optimize_dense_batch_bounded(db.p0() if p0 is None else p0, db.N, db.M, db.cb, db.cookie, lo, hi,
                                                            loss, prm)
    assert rc == 0
    assert db.ncalls() == int(res["evaluations"].max()) == capi.batch_last_stats()["rounds"]
    assert db.nevals() == int(res["evaluations"].sum())
    return p, res, held, w


def assert_margin(orc, recorded, what):
    m = min(r["margin"] for r in orc)
    print(f"{what}: smallest decision margin of the oracle's solves {m:.3g} (recorded {recorded:.3g})")
    assert m > MARGIN_FLOOR, f"{what}: margin {m:.3g}: the seeds no longer keep the decisions off the rounding edges"
    assert abs(m - recorded) <= 0.05 * recorded, "the generator or the oracle changed: choose the seeds again"


def compare(p, res, held, w, orc, what):
    """every problem against its oracle solve; prints the figures, then asserts"""
    nb = len(p)
    dp = max(float(np.max(np.abs(p[b] - orc[b]["p"]))) for b in range(nb))
    dn = max(abs(res["norm2_x"][b] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for b in range(nb))
    dt = max(abs(res["trustregion"][b] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for b in range(nb))
    dw = 0.0 if w is None else max(float(np.max(np.abs(w[b] - orc[b]["weights"]) / orc[b]["weights"])) for b in range(nb))
    print(f"{what}: {nb} problems, max |p - p_oracle| {dp:.3g}, F rel {dn:.3g}, trust region rel {dt:.3g}, weights rel {dw:.3g}")
    for b in range(nb):
        o = orc[b]
        got = (int(res["iterations"][b]), int(res["evaluations"][b]), int(res["status"][b]), float(res["lambda_"][b]))
        want = (o["iterations"], o["evaluations"], o["status"], o["lambda_"])
        assert got == want, f"{what}: problem {b}: (iterations, evaluations, status, lambda) {got}, the oracle {want}"
        assert held[b].tolist() == o["held"].tolist(), f"{what}: problem {b}: held {held[b].tolist()}, the oracle {o['held'].tolist()}"
    assert dp <= STEP_TOL and dn <= REL_TOL and dt <= REL_TOL and dw <= REL_TOL


# ---------------------------------------------------------------- 1. bounds that clamp nothing: the plain solve, bit for bit
@pytest.mark.parametrize("shape", [(6, 40), (64, 128)], ids=str)
def test_infinite_bounds_are_the_plain_solve_bit_for_bit(shape):
    N, M = shape
    nb = 9
    db = tb.device_batch(N, M, range(1, 1 + nb), "diverse")
    prm = tb.params("diverse")
    pp, rp = tb.run(db, prm)
    inf = np.full((nb, N), np.inf)
    for what, lo, hi in (("NULL", None, None), ("infinite", -inf, inf), ("a box 1e300 wide", np.full((nb, N), -5e299),
                                                                      np.full((nb, N), 5e299)), ("lower only", -inf, None)):
        p, res, held, w = run(db, prm, lo, hi)
        assert p.tobytes() == pp.tobytes() and tb.bitwise_equal(res, rp), what
        assert not held.any() and w is None, what
    loss = loss_pair("diverse", LOSS_HUBER, 2)[1]
    rc, pr, rr, wr = capi.optimize_dense_batch_robust(db.p0(), N, M, db.cb, db.cookie, loss, prm)
    assert rc == 0
    for lo, hi in ((None, None), (-inf, inf)):
        p, res, held, w = run(db, prm, lo, hi, loss)
        assert p.tobytes() == pr.tobytes() and tb.bitwise_equal(res, rr) and w.tobytes() == wr.tobytes() and not held.any()
    db.close()


# ---------------------------------------------------------------- 2. parity over a batch
PARITY_SHAPE, PARITY_B = (6, 40), 65
PARITY_MARGIN = 1.86e-3


def parity_batch():
    (N, M), nb = PARITY_SHAPE, PARITY_B
    return N, M, tuple(range(1, 1 + nb)), oracle_batch(N, M, tuple(range(1, 1 + nb)), "diverse")


def test_parity_over_a_batch():
    N, M, seeds, (orc, lo, hi) = parity_batch()
    nheld = sum(bool(o["held"].any()) for o in orc)
    types = set().union(*[o["step_types"] for o in orc])
    nclipped, nfallbacks = sum(o["clipped"] for o in orc), sum(o["fallbacks"] for o in orc)
    print(f"{nheld} of {len(orc)} problems end with a held variable, step types {sorted(types)}, {nclipped} clipped steps, "
          f"{nfallbacks} fallbacks, evaluations {sorted({o['evaluations'] for o in orc})}")
    assert 2 * nheld >= len(orc) and types == {0, 1, 2} and nclipped > 0 and len({o["evaluations"] for o in orc}) > 1
    assert_margin(orc, PARITY_MARGIN, "diverse, bounded")
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res, held, w = run(db, params("diverse"), lo, hi)
    compare(p, res, held, w, orc, "diverse, bounded")
    assert np.all(p >= lo) and np.all(p <= hi)
    db.close()


# ---------------------------------------------------------------- 3. rejected trials
# Bounds half way to the optimum are met late, trials are rejected early: seeds 1 .. 3000 of the "hard" set reject no trial with
# a variable held.  Here the bound lies AT the start point (on the optimum's side of it), so the bounded variables are held from
# the first step on.  Seeds 446 (at b = 0) and 1398 (at b = 2), found among 1 .. 1500, reject a trial and step again with held
# variables, between problems that do not.  REJECT_OVER: the module's docstring
REJECT_SEEDS = (446, 1, 1398, 2, 3)
REJECT_OVER = (("update_threshold", 1e-5), ("Jt_x_threshold", 1e-5))
# trustregion_threshold or None: the margin recorded
REJECT_MARGIN = {None: 4.27e-3, 100.0: 4.27e-3}


@pytest.mark.parametrize("threshold", [None, 100.0], ids=str)
def test_rejected_trials(threshold):
    """threshold None: a rejected trial steps again from the cached steps, the held set formed again from p_before and g;
    threshold 100: the first rejected trial ends the solve (TRUSTREGION), held is that of the point before it"""
    N, M = 6, 40
    over = REJECT_OVER + (() if threshold is None else (("trustregion_threshold", threshold),))
    orc, lo, hi = oracle_batch(N, M, REJECT_SEEDS, "hard", over=over, frac=1.0)
    assert_margin(orc, REJECT_MARGIN[threshold], f"hard, bounded, threshold {threshold}")
    assert sum(o["rejected"] for o in orc) >= 2
    if threshold is None:
        print(f"steps behind a rejected trial with a held variable: {[o['held_resteps'] for o in orc]}")
        assert sum(o["held_resteps"] for o in orc) >= 1
    else:
        stopped = [o for o in orc if o["status"] == BATCH_TRUSTREGION]
        assert len(stopped) >= 1 and all(o["rejected"] == 1 for o in stopped) and any(o["held"].any() for o in stopped)
    db = tb.device_batch(N, M, REJECT_SEEDS, "hard")
    p, res, held, w = run(db, tb.params("hard", **dict(over)), lo, hi)
    compare(p, res, held, w, orc, f"hard, bounded, threshold {threshold}")
    db.close()


# ---------------------------------------------------------------- 4. the branches, one per problem of a linear batch
def branch_batch():
    """(A (8, 2, 2), y (8, 2), p0 (8, 2), lo, hi, trustregion0): problems 0 .. 7 as the test names them"""
    Af, yf = from_normal_equations([[1.0, 0.95], [0.95, 1.0]], [-0.14, -0.25])
    Ao, yo = from_normal_equations([[2.0, 0.3], [0.3, 1.0]], [-1.0, 0.5])        # unbounded optimum (0.602, -0.681)
    inf = np.inf
    rows = [
        (Af, yf, (0.0, 0.0), (-inf, -inf), (inf, 0.1)),          # 0: the fallback example
        (Ao, yo, (0.0, 0.0), (-inf, 0.25), (inf, 0.25)),         # 1: lo == hi in variable 1
        (Af, yf, (0.0, 0.0), (-1.0, -1.0), (0.0, 0.0)),          # 2: g(0) < 0 and upper = 0: everything held at the start
        (Ao, yo, (5.0, -7.0), (-0.5, -0.5), (0.5, 0.5)),         # 3: an infeasible start
        (Ao, yo, (0.1, 0.1), (0.0, 1.0), (1.0, 0.5)),            # 4: lo > hi
        (Ao, yo, (0.1, 0.1), (0.0, np.nan), (1.0, 1.0)),         # 5: a NaN bound
        (Ao, yo, (0.2, -0.1), (-inf, -0.3), (0.4, inf)),         # 6: ordinary
        (Af, yf, (0.5, 0.5), (0.1, -inf), (inf, inf)),           # 7: ordinary
    ]
    A, y, p0, lo, hi = (np.array([r[k] for r in rows], dtype=np.float64) for k in range(5))
    return A, y, p0, lo, hi, 10.0


def test_branches_on_the_linear_problem():
    A, y, p0, lo, hi, tr0 = branch_batch()
    nb, N = p0.shape
    prm = tb.params("default")
    prm.trustregion0 = tr0
    db = LinearDeviceBatch(A, y, p0)
    orc = [bb.solve_one(db.host(b), prm, ro.Loss(LOSS_TRIVIAL), lo[b], hi[b]) for b in range(nb)]
    margin = min(o["margin"] for o in orc)
    print(f"the oracle: fallbacks {[o['fallbacks'] for o in orc]}, clipped {[o['clipped'] for o in orc]}, statuses "
          f"{[o['status'] for o in orc]}, smallest margin {margin:.3g}")
    assert orc[0]["fallbacks"] == 1 and margin > MARGIN_FLOOR
    p, res, held, w = run(db, prm, lo, hi)
    first = db.first_p()
    compare(p, res, held, w, orc, "branches")
    good = [0, 1, 2, 3, 6, 7]
    for b in good:
        assert float(np.max(np.abs(p[b] - exact_bounded_solution(A[b], y[b], lo[b], hi[b])))) <= KKT_TOL, b
        assert np.all(first[b] >= lo[b]) and np.all(first[b] <= hi[b]), b
    assert p[1][1] == 0.25
    # everything held at the start
    assert (res["status"][2], res["evaluations"][2], res["iterations"][2]) == (BATCH_JTX, 1, 0)
    assert p[2].tobytes() == p0[2].tobytes() and held[2].tolist() == [2, 2]
    # the infeasible start was clamped before the first evaluation
    assert first[3].tolist() == [0.5, -0.5]
    # bad bounds: FAILED alone, nothing evaluated, nothing written but the record
    for b in (4, 5):
        assert (res["status"][b], res["evaluations"][b], res["iterations"][b], res["norm2_x"][b]) == (BATCH_FAILED, 0, 0, -1.0)
        assert p[b].tobytes() == p0[b].tobytes() and not held[b].any()
    db.close()
    # the two ordinary problems alone: the same bits
    for b in (6, 7):
        d1 = LinearDeviceBatch(A[b:b + 1], y[b:b + 1], p0[b:b + 1])
        p1, r1, h1, _ = run(d1, prm, lo[b:b + 1], hi[b:b + 1])
        assert p1.tobytes() == p[b:b + 1].tobytes() and tb.bitwise_equal(r1, res[b:b + 1]) and h1.tobytes() == held[b:b + 1].tobytes()
        d1.close()


# ---------------------------------------------------------------- 5. every size class
# (N, M, every variable bounded): the margin recorded.  The smallest M of the class in tests/dense_batch_shapes.py and
# tests/dense_batch_wide_shapes.py; N = 64 with all 64 variables bounded: bit 63 of the ballot; N = 33: the first of <48>
CLASS_CASES = {
    (1, 5, False): 9.57e-2, (16, 50, False): 2.65e-3, (17, 40, False): 1.18e-3, (31, 47, False): 1.81e-3, (33, 70, False): 2.41e-3,
    (49, 103, False): 6.36e-3, (64, 128, True): 1.34e-3,
}
CLASS_B = 5


def test_the_class_table_is_what_it_says():
    assert sorted(ws.size_class(N) for N, _, _ in CLASS_CASES) == [8, 16, 24, 32, 48, 64, 64]
    shapes = list(ds.CASES) + list(ws.CASES)
    for N, M, every in CLASS_CASES:
        if every:
            assert (N, M) == (64, 128)
            continue
        assert M == min(m for n, m in shapes if ws.size_class(n) == ws.size_class(N)), (N, M)


@pytest.mark.parametrize("case", sorted(CLASS_CASES), ids=str)
def test_every_size_class(case):
    N, M, every = case
    seeds = tuple(range(1, 1 + CLASS_B))
    orc, lo, hi = oracle_batch(N, M, seeds, "diverse", every=every)
    assert_margin(orc, CLASS_CASES[case], str(case))
    assert sum(bool(o["held"].any()) for o in orc) >= 2
    if every:
        assert any(o["held"][N - 1] for o in orc), "no problem holds the last variable: the top bit of the mask is not exercised"
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res, held, w = run(db, params("diverse"), lo, hi)
    compare(p, res, held, w, orc, str(case))
    db.close()


# ---------------------------------------------------------------- 6. a loss and bounds together
HUBER_B, HUBER_FS, HUBER_MARGIN = 33, 2, 3.04e-4


def test_loss_and_bounds_together():
    N, M = 6, 40
    seeds = tuple(range(1, 1 + HUBER_B))
    orc, lo, hi = oracle_batch(N, M, seeds, "diverse", LOSS_HUBER, HUBER_FS)
    assert_margin(orc, HUBER_MARGIN, "huber, bounded")
    assert 2 * sum(bool(o["held"].any()) for o in orc) >= len(orc)
    assert float(np.mean([np.mean(o["weights"] < 1.0) for o in orc])) >= 0.1
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res, held, w = run(db, params("diverse"), lo, hi, loss_pair("diverse", LOSS_HUBER, HUBER_FS)[1])
    compare(p, res, held, w, orc, "huber, bounded")
    db.close()


# ---------------------------------------------------------------- 7. the device twin
def solve_dev(db, prm, lo, hi, loss=None, mask=None, stream=None, want_held=True):
    """the device-resident bounded solve under prefilled sentinels: (p, results, lambda, held, weights, counts); lo, hi: arrays or
    None"""
    nb, N = db.B, db.N
    P = td.Buf(db.p0())
    R = td.Buf(np.full(nb * td.RSIZE, td.PAD, dtype=np.uint8))
    Lm = td.Buf(np.full(nb, GUARD))
    Lo = None if lo is None else td.Buf(np.ascontiguousarray(lo, dtype=np.float64))
    Hi = None if hi is None else td.Buf(np.ascontiguousarray(hi, dtype=np.float64))
    H = td.Buf(np.full((nb, N), HELD_GUARD, dtype=np.uint8)) if want_held else None
    W = td.Buf(np.full((nb, db.M // max(loss.featureSize, 1)), GUARD)) if loss is not None else None
    A = td.mask_dev(mask)
    db.reset_counters()
    rc = capi.optimize_dense_batch_bounded_device(P.ptr, nb, N, db.M, db.cb, db.cookie, prm, loss, Lo.ptr if Lo else None,
                                                  Hi.ptr if Hi else None, H.ptr if H else None, R.ptr, Lm.ptr,
                                                  W.ptr if W else None, A.ptr if A else None, stream)
    assert rc == 0
    counts = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    if A is not None:
        assert np.array_equal(A.get(), np.asarray(mask, dtype=np.uint8))
    # (Buf.get checks the guard behind each array: the bounds are read only, held is written within its span)
    if Lo is not None:
        assert Lo.get().tobytes() == np.ascontiguousarray(lo, dtype=np.float64).tobytes()
    if Hi is not None:
        assert Hi.get().tobytes() == np.ascontiguousarray(hi, dtype=np.float64).tobytes()
    return P.get(), td.results_of(R, nb), Lm.get(), H.get() if H else None, W.get() if W else None, counts


@pytest.mark.parametrize("kind", [None, LOSS_HUBER], ids=str)
def test_device_twin_equals_host_twin(kind):
    N, M, seeds, _ = parity_batch()
    fs = 2 if kind is not None else 1
    nb = HUBER_B if kind is not None else len(seeds)
    seeds = seeds[:nb]
    orc, lo, hi = oracle_batch(N, M, seeds, "diverse", kind, fs)
    loss = loss_pair("diverse", kind, fs)[1]
    db = tb.device_batch(N, M, seeds, "diverse")
    prm = params("diverse")
    ph, rh, hh, wh = run(db, prm, lo, hi, loss)
    ch = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    pd, rd, ld, hd, wd, cd = solve_dev(db, prm, lo, hi, loss)
    assert pd.tobytes() == ph.tobytes() and tb.bitwise_equal(rd, rh) and hd.tobytes() == hh.tobytes() and cd == ch
    assert ld.tobytes() == np.ascontiguousarray(rh["lambda_"]).tobytes() and hh.any()
    assert (wd is None and wh is None) or wd.tobytes() == wh.tobytes()
    # no held asked for, one side of the box only: the same solves
    pn, rn, _, hn, _, _ = solve_dev(db, prm, lo, hi, loss, want_held=False)
    assert pn.tobytes() == ph.tobytes() and tb.bitwise_equal(rn, rh) and hn is None
    p1, r1, h1, _ = run(db, prm, lo, None, loss)
    pd1, rd1, _, hd1, _, _ = solve_dev(db, prm, lo, None, loss)
    assert pd1.tobytes() == p1.tobytes() and tb.bitwise_equal(rd1, r1) and hd1.tobytes() == h1.tobytes()
    db.close()


@pytest.mark.parametrize("shape", [(6, 40), (64, 128)], ids=str)
def test_mask(shape):
    N, M = shape
    nb = td.B if N == 6 else 9
    seeds = tuple(range(1, 1 + nb))
    every = N == 64
    orc, lo, hi = oracle_batch(N, M, seeds, "diverse", every=every)
    db = tb.device_batch(N, M, seeds, "diverse")
    prm = params("diverse")
    p0 = db.p0()
    pf, rf, lf, hf, _, _ = solve_dev(db, prm, lo, hi)
    m = td.the_mask(N, nb)
    on, off = np.flatnonzero(m), np.flatnonzero(m == 0)
    # a problem that is not run is not checked either: bad bounds in one of them
    lo2 = lo.copy()
    lo2[off[0], 0] = np.nan
    pm, rm, lm, hm, _, cm = solve_dev(db, prm, lo2, hi, mask=m)
    assert pm[on].tobytes() == pf[on].tobytes() and tb.bitwise_equal(rm[on], rf[on]) and lm[on].tobytes() == lf[on].tobytes()
    assert hm[on].tobytes() == hf[on].tobytes() and hf.any()
    assert pm[off].tobytes() == p0[off].tobytes() and np.all(hm[off] == HELD_GUARD)
    assert np.all(rm["norm2_x"][off] == -1.0) and np.all(rm["status"][off] == BATCH_NOT_RUN)
    for k in ("trustregion", "lambda_", "iterations", "evaluations"):
        assert not rm[k][off].any(), k
    assert cm["nevals"] == int(rm["evaluations"].sum()) and cm["ncalls"] == int(rm["evaluations"].max()) == cm["rounds"]
    db.close()


STREAM_CHILD = r'''
import sys
import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded
sys.path.insert(0, sys.argv[1])
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_bounds_gpu as tbb
from tests import test_dense_batch_gpu as tb
from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchResult

N, M, B = 6, 40, 33
seeds = tuple(range(1, 1 + B))
orc, lo, hi = tbb.oracle_batch(N, M, seeds, "diverse")
db = tb.device_batch(N, M, seeds, "diverse")
prm = tbb.params("diverse")
p0 = db.p0()
pn, rn, ln, hn, _, cn = tbb.solve_dev(db, prm, lo, hi)          # hip_stream NULL
s = torch.cuda.Stream()
host = torch.from_numpy(p0.copy()).pin_memory()
hlo, hhi = torch.from_numpy(lo.copy()).pin_memory(), torch.from_numpy(hi.copy()).pin_memory()
dev = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
dlo = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
dhi = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
held = torch.full((B * N + 64,), tbb.HELD_GUARD, dtype=torch.uint8, device="cuda")
res = torch.full((B * td.RSIZE + 512,), td.PAD, dtype=torch.uint8, device="cuda")
lam = torch.full((B + 64,), td.GUARD, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(s):
    # asynchronous, on s; no synchronisation before the call
    dev[:B * N].copy_(host.reshape(-1), non_blocking=True)
    dlo[:B * N].copy_(hlo.reshape(-1), non_blocking=True)
    dhi[:B * N].copy_(hhi.reshape(-1), non_blocking=True)
rc = capi.optimize_dense_batch_bounded_device(dev.data_ptr(), B, N, M, db.cb, db.cookie, prm, None, dlo.data_ptr(), dhi.data_ptr(),
                                              held.data_ptr(), res.data_ptr(), lam.data_ptr(), None, None, s.cuda_stream)
assert rc == 0
torch.cuda.synchronize()
ps, ls, hs, raw = dev.cpu().numpy(), lam.cpu().numpy(), held.cpu().numpy(), res.cpu().numpy()
assert np.all(ps[B * N:] == td.GUARD) and np.all(ls[B:] == td.GUARD) and np.all(raw[B * td.RSIZE:] == td.PAD)
assert np.all(hs[B * N:] == tbb.HELD_GUARD) and np.all(dlo.cpu().numpy()[B * N:] == td.GUARD)
rs = capi._batch_results((BatchResult * B).from_buffer_copy(raw[:B * td.RSIZE].tobytes()), B)
assert ps[:B * N].tobytes() == pn.tobytes() and ls[:B].tobytes() == ln.tobytes() and tb.bitwise_equal(rs, rn)
assert hs[:B * N].tobytes() == hn.tobytes() and hn.any()
assert np.all(rs["status"] > 0)
db.close()
print("STREAM OK")
'''


def test_stream(tmp_path):
    """in a process of its own, as tests/test_dense_batch_device_gpu.py::test_stream: torch is loaded before the library there"""
    src = tmp_path / "stream_child.py"
    src.write_text(STREAM_CHILD)
    r = subprocess.run([sys.executable, str(src), ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "STREAM OK" in r.stdout, r.stdout + r.stderr


def test_refusals_on_the_gpu():
    N, M, nb = 6, 40, 4
    db = tb.device_batch(N, M, range(1, 1 + nb), "default")
    db.reset_counters()
    P = td.Buf(db.p0())
    R = td.Buf(np.full(nb * td.RSIZE, td.PAD, dtype=np.uint8))
    Lm = td.Buf(np.full(nb, GUARD))
    Lo, Hi = td.Buf(np.full((nb, N), -50.0)), td.Buf(np.full((nb, N), 50.0))
    H = td.Buf(np.full((nb, N), HELD_GUARD, dtype=np.uint8))
    W = td.Buf(np.full((nb, M), GUARD))
    short = capi.DeviceArray(nbytes=nb * N - 1)
    pageable = np.full((nb, N), -50.0)
    prm = tb.params("default")

    def dev(lo=Lo.ptr, hi=Hi.ptr, h=H.ptr, loss=None, w=None, p=P.ptr, r=R.ptr):
        return capi.optimize_dense_batch_bounded_device(p, nb, N, M, db.cb, db.cookie, prm, loss, lo, hi, h, r, Lm.ptr, w)

    assert capi.batch_device_span_ok(H.ptr, nb * N) and not capi.batch_device_span_ok(short.ptr, nb * N)
    assert not capi.batch_device_span_ok(pageable.ctypes.data, 8 * nb * N)
    assert dev(lo=pageable.ctypes.data) == -1                   # a pageable-host lower
    assert dev(hi=pageable.ctypes.data) == -1
    assert dev(h=short.ptr) == -1                               # a held one byte short
    assert dev(h=np.zeros((nb, N), dtype=np.uint8).ctypes.data) == -1   # a held on another kind of memory
    assert dev(w=W.ptr) == -1                                   # weights without a loss
    assert dev(p=None) == -1 and dev(r=None) == -1
    L = capi.lib()
    assert L.dogleg_amd_optimize_dense_batch_bounded_device(P.ptr, nb, N, M, db.cb, db.cookie, None, None, None, R.ptr, Lm.ptr,
                                                            None, None, None) == -1      # a NULL bounds
    assert db.ncalls() == 0
    assert np.all(R.get() == td.PAD) and np.all(Lm.get() == GUARD) and np.all(W.get() == GUARD) and np.all(H.get() == HELD_GUARD)
    assert P.get().tobytes() == db.p0().tobytes()
    # and the valid call behind them
    assert dev() == 0 and np.all(td.results_of(R, nb)["status"] > 0) and not H.get().any()
    short.free()
    db.close()


# ---------------------------------------------------------------- 8. independence
def test_order_size_and_neighbours_do_not_matter():
    N, M, seeds, (orc, lo, hi) = parity_batch()
    nb = len(seeds)
    prm = params("diverse")
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res, held, _ = run(db, prm, lo, hi)
    db.close()
    # reversed, every neighbour's bounds another problem's
    rev = tuple(reversed(seeds))
    db = tb.device_batch(N, M, rev, "diverse")
    pr, rr, hr, _ = run(db, prm, lo[::-1], hi[::-1])
    db.close()
    assert pr[::-1].tobytes() == p.tobytes() and tb.bitwise_equal(rr[::-1], res) and hr[::-1].tobytes() == held.tobytes()
    # the neighbours' bounds changed (none at all), one problem's kept
    for b in (0, 31, nb - 1):
        lo2, hi2 = np.full_like(lo, -np.inf), np.full_like(hi, np.inf)
        lo2[b], hi2[b] = lo[b], hi[b]
        db = tb.device_batch(N, M, seeds, "diverse")
        p2, r2, h2, _ = run(db, prm, lo2, hi2)
        db.close()
        assert p2[b].tobytes() == p[b].tobytes() and tb.bitwise_equal(r2[b:b + 1], res[b:b + 1]) and h2[b].tobytes() == held[b].tobytes()
        # alone
        db = tb.device_batch(N, M, seeds[b:b + 1], "diverse")
        p1, r1, h1, _ = run(db, prm, lo[b:b + 1], hi[b:b + 1])
        db.close()
        assert p1[0].tobytes() == p[b].tobytes() and tb.bitwise_equal(r1, res[b:b + 1]) and h1[0].tobytes() == held[b].tobytes()


# ---------------------------------------------------------------- 9. round accounting
def test_round_accounting():
    """run() asserts, for every batch above, one callback per round and live problems only; here also against the oracle's
    counts and with problems that never start"""
    N, M, seeds, (orc, lo, hi) = parity_batch()
    db = tb.device_batch(N, M, seeds, "diverse")
    lo2 = lo.copy()
    lo2[[0, 17]] = np.nan
    p, res, held, _ = run(db, params("diverse"), lo2, hi)
    want = [0 if b in (0, 17) else o["evaluations"] for b, o in enumerate(orc)]
    assert res["evaluations"].tolist() == want and db.ncalls() == max(want) and db.nevals() == sum(want)
    assert capi.batch_last_stats()["rounds"] == max(want)
    assert res["status"][0] == res["status"][17] == BATCH_FAILED
    db.close()
