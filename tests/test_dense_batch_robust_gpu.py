"""dogleg_amd_optimize_dense_batch_robust and its device twin.

The reference is the NumPy oracle of tests/batch_robust_oracle.py on the host model of the same problems (tests/
test_dense_batch_robust_cpu.py holds it against the C oracle under LOSS_TRIVIAL).  Tolerances: |p - p_oracle|_inf <= STEP_TOL =
1e-10, F (norm2_x), the trust region and every weight to 1e-8 relative, lambda, iterations, evaluations and status equal.
Every shape here holds them (the figures are printed before they are asserted).

The seeds.  Every batch was chosen on the CPU, with the oracle alone, such that every problem's smallest decision margin is
above MARGIN_FLOOR = 1e-6 (no problem is left out); the margin each batch gave is written beside it and asserted, to 5 %,
before anything is compared.  Seeds 1 .. B passed wherever they are used.  With a concave loss the Gauss-Newton model
majorises F along the step where the model is linear, so trials are hardly ever rejected: seeds 1 .. 1500 of the "hard" set
reject none with a scale near the noise.  The batches with rejected trials therefore use a wide scale (300 x the noise: the
loss bends at the far start points and is the plain one at the optimum) and the seeds found there; with
trustregion_threshold = 100 their first rejected trial ends the solve, so the returned point is not the last one evaluated.

The shapes.  T = min(64, 256 / N) rows a tile, T' = T - T mod featureSize.  Up to the class of 16 a tile holds more rows than
the problem has variables, and M runs below one tile, at exactly one tile and at T' + featureSize.  From the class of 24 on a
tile is shorter than N, so a problem of one tile would be underdetermined (lambda decisions on a singular H sit on rounding
edges, which no margin keeps apart): there M is a whole number of tiles, and that plus one feature."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BATCH_NOT_RUN, BATCH_TRUSTREGION, BATCH_MAX_NSTATE, BatchLoss, BatchResult,
                                       LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY)
from problems.batch import MODE_NAN
from problems.batch_offsets import OffsetDeviceBatch, OffsetHostProblem, planted_offsets
from tests import batch_oracle as bo
from tests import batch_robust_oracle as ro
from tests import dense_batch_wide_shapes as ws
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MARGIN_FLOOR, REL_TOL = tb.MARGIN_FLOOR, tb.REL_SCALAR_TOL
KINDS = {"huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}
NEAR, WIDE = 0.5, 300.0                 # the scale in units of noise sqrt(featureSize)
OUTLIER_FRACTION, OUTLIER_SIZE, OUTLIER_SEED = 0.1, 50.0, 7
GUARD = td.GUARD


def scale_of(setname, fs, factor):
    return factor * tb.SETS[setname][1] * float(np.sqrt(fs))


def loss_of(kind, setname, fs, factor):
    return BatchLoss(KINDS.get(kind, LOSS_TRIVIAL), scale_of(setname, fs, factor), fs)


def offsets_of(nb, M, fs, setname):
    return planted_offsets(nb, M, fs, OUTLIER_FRACTION, OUTLIER_SIZE * tb.SETS[setname][1], OUTLIER_SEED)[0]


@functools.lru_cache(maxsize=None)
def oracle_batch(N, M, fs, kind, seeds, setname, factor=NEAR, planted=False, over=()):
    """the NumPy oracle on the problems `seeds` (a tuple) of a batch (cached: the tests share the batches)"""
    eps, noise, spread, _ = tb.SETS[setname]
    prm = tb.params(setname, **dict(over))
    loss = ro.Loss(KINDS[kind], scale_of(setname, fs, factor), fs)
    off = offsets_of(len(seeds), M, fs, setname) if planted else None
    out = []
    for b, s in enumerate(seeds):
        hp = bo.HostProblem(M, N, int(s), eps, noise, spread)
        out.append(ro.solve_one(hp if off is None else OffsetHostProblem(hp, off[b]), prm, loss))
        hp.dp.close()
    return out


def device_batch(N, M, fs, seeds, setname, planted=False, nb=None):
    """the first nb problems of the batch `seeds`"""
    nb = len(seeds) if nb is None else nb
    db = tb.device_batch(N, M, seeds[:nb], setname)
    return OffsetDeviceBatch(db, offsets_of(len(seeds), M, fs, setname)[:nb]) if planted else db


def run(db, prm, loss):
    """the host-pointer call: (p, results, weights); one batched callback per round, live problems only"""
    db.reset_counters()
    rc, p, res, w = capi.optimize_dense_batch_robust(db.p0(), db.N, db.M, db.cb, db.cookie, loss, prm)
    assert rc == 0
    assert db.ncalls() == int(res["evaluations"].max()) == capi.batch_last_stats()["rounds"]
    assert db.nevals() == int(res["evaluations"].sum())
    return p, res, w


def assert_margin(orc, recorded, what):
    m = min(r["margin"] for r in orc)
    print(f"{what}: smallest decision margin of the oracle's solves {m:.3g} (recorded {recorded:.3g})")
    assert m > MARGIN_FLOOR, f"{what}: margin {m:.3g}: the seeds no longer keep the decisions off the rounding edges"
    assert abs(m - recorded) <= 0.05 * recorded, "the generator or the oracle changed: choose the seeds again"


def compare(p, res, w, orc, what):
    """every problem against its oracle solve; prints the figures, then asserts"""
    nb = len(p)
    dp = max(float(np.max(np.abs(p[b] - orc[b]["p"]))) for b in range(nb))
    dn = max(abs(res["norm2_x"][b] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for b in range(nb))
    dt = max(abs(res["trustregion"][b] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for b in range(nb))
    dw = max(float(np.max(np.abs(w[b] - orc[b]["weights"]) / orc[b]["weights"])) for b in range(nb))
    print(f"{what}: {nb} problems, max |p - p_oracle| {dp:.3g}, F rel {dn:.3g}, trust region rel {dt:.3g}, weights rel {dw:.3g}")
    for b in range(nb):
        o = orc[b]
        got = (int(res["iterations"][b]), int(res["evaluations"][b]), int(res["status"][b]), float(res["lambda_"][b]))
        want = (o["iterations"], o["evaluations"], o["status"], o["lambda_"])
        assert got == want, f"{what}: problem {b}: (iterations, evaluations, status, lambda) {got}, the oracle {want}"
    assert dp <= STEP_TOL and dn <= REL_TOL and dt <= REL_TOL and dw <= REL_TOL


# ---------------------------------------------------------------- 1. parity over a batch, every loss
PARITY_SHAPE, PARITY_FS, PARITY_B = (6, 40), 2, 65
PARITY_MARGIN = {"huber": 7.59e-5, "soft_l1": 3.02e-4, "cauchy": 5.97e-3}
# With the planted outliers F is dominated by their rho, so that the last steps of a solve to 1e-8 improve F by less than
# its rounding error: their gain ratios are noise on any implementation (negative margins on the oracle).  The planted batch
# stops at 1e-6 instead, before that.
PLANTED_B, PLANTED_OVER = 33, (("update_threshold", 1e-6), ("Jt_x_threshold", 1e-6))
PLANTED_MARGIN = {"huber": 5.83e-4, "soft_l1": 2.62e-4, "cauchy": 7.88e-3}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_parity_over_a_batch(kind):
    (N, M), fs, nb = PARITY_SHAPE, PARITY_FS, PARITY_B
    seeds = tuple(range(1, 1 + nb))
    orc = oracle_batch(N, M, fs, kind, seeds, "diverse")
    assert_margin(orc, PARITY_MARGIN[kind], f"{kind} diverse")
    # (Huber's weights are exactly 1 up to c; the other two losses have w < 1 everywhere, so they are asked for w < 0.9)
    below = 1.0 if kind == "huber" else 0.9
    share = float(np.mean([np.mean(o["weights"] < below) for o in orc]))
    types = set().union(*[o["step_types"] for o in orc])
    print(f"share of features with w < {below} at the optimum {share:.2f}, step types {sorted(types)}")
    assert share >= 0.25 and types == {0, 1, 2} and len({o["evaluations"] for o in orc}) > 1
    db = device_batch(N, M, fs, seeds, "diverse")
    p, res, w = run(db, tb.params("diverse"), loss_of(kind, "diverse", fs, NEAR))
    compare(p, res, w, orc, f"{kind} diverse")
    db.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_parity_with_planted_outliers(kind):
    """a tenth of the features displaced by 50 x the noise through problems/batch_offsets.py"""
    (N, M), fs, nb = PARITY_SHAPE, PARITY_FS, PLANTED_B
    seeds = tuple(range(1, 1 + nb))
    orc = oracle_batch(N, M, fs, kind, seeds, "default", NEAR, True, PLANTED_OVER)
    assert_margin(orc, PLANTED_MARGIN[kind], f"{kind} planted")
    _, planted = planted_offsets(nb, M, fs, OUTLIER_FRACTION, OUTLIER_SIZE * tb.SETS["default"][1], OUTLIER_SEED)
    worst_planted = max(float(o["weights"][planted[b]].max()) for b, o in enumerate(orc))
    print(f"the largest weight of a planted feature {worst_planted:.3g}")
    assert worst_planted < 0.1
    db = device_batch(N, M, fs, seeds, "default", planted=True)
    p, res, w = run(db, tb.params("default", **dict(PLANTED_OVER)), loss_of(kind, "default", fs, NEAR))
    compare(p, res, w, orc, f"{kind} planted")
    db.close()


# ---------------------------------------------------------------- 2. the shapes at which the sweep can go wrong
# (N, featureSize, M, kind): the margin recorded.  B = problems a workgroup + 1, seeds 1 ..; "diverse"
SHAPES = {
    (5, 3, 48, "huber"): 6.77e-04, (5, 3, 51, "soft_l1"): 9.19e-02, (5, 3, 54, "cauchy"): 4.29e-02,         # <8>, T 51 -> 51
    (5, 4, 44, "cauchy"): 9.88e-03, (5, 4, 48, "huber"): 5.02e-03, (5, 4, 52, "soft_l1"): 3.05e-02,         # <8>, T 51 -> 48
    (12, 2, 18, "soft_l1"): 6.96e-02, (12, 2, 20, "cauchy"): 5.29e-02, (12, 2, 22, "huber"): 1.19e-03,      # <16>, T 21 -> 20
    (24, 4, 56, "huber"): 5.75e-04, (24, 4, 60, "cauchy"): 3.01e-02,                                   # <24>, T 10 -> 8: 7 tiles, + 4 rows
    (32, 3, 66, "soft_l1"): 8.99e-03, (32, 3, 69, "huber"): 5.87e-04,                                  # <32>, T 8 -> 6: 11 tiles, + 3 rows
    (48, 2, 100, "cauchy"): 5.54e-02, (48, 2, 102, "soft_l1"): 1.43e-01,                               # <48>, T 5 -> 4: 25 tiles, + 2 rows
    (48, 4, 100, "huber"): 7.86e-03, (48, 4, 104, "cauchy"): 3.99e-02,                                 # <48>, T 5 -> 4: 25 tiles, + 4 rows
    (64, 3, 129, "soft_l1"): 1.50e-01, (64, 3, 132, "huber"): 5.81e-04,                                # <64>, T 4 -> 3: 43 tiles, + 3 rows
    (64, 1, 130, "cauchy"): 4.04e-01,                                                             # <64>, T 4: 32 tiles + 2 rows
}


def tile_rows(N, fs):
    t = min(64, 256 // N)
    return t - t % fs


def test_the_shape_table_is_what_it_says():
    assert {ws.size_class(N) for N, _, _, _ in SHAPES} == {8, 16, 24, 32, 48, 64}
    assert tile_rows(48, 2) == tile_rows(48, 4) == 4 and tile_rows(64, 3) == 3 and tile_rows(5, 3) == 51 and tile_rows(5, 4) == 48
    for N, fs in {(N, fs) for N, fs, _, _ in SHAPES if fs > 1}:
        Ms = sorted(M for n, f, M, _ in SHAPES if (n, f) == (N, fs))
        t = tile_rows(N, fs)
        assert all(M % fs == 0 and M > N for M in Ms)
        if t > N + fs:
            assert Ms[0] < t and Ms[1] == t and Ms[2] == t + fs, (N, fs, Ms)
        else:
            assert Ms[0] % t == 0 and Ms[1] == Ms[0] + fs, (N, fs, Ms)


@pytest.mark.parametrize("case", sorted(SHAPES), ids=str)
def test_shapes(case):
    N, fs, M, kind = case
    nb = ws.problems_per_workgroup(N) + 1
    seeds = tuple(range(1, 1 + nb))
    orc = oracle_batch(N, M, fs, kind, seeds, "diverse")
    assert_margin(orc, SHAPES[case], str(case))
    # (M is about 2 N here: the fit takes up much of the noise, fewer features end above Huber's c than in the batch above)
    assert float(np.mean([np.mean(o["weights"] < 1.0) for o in orc])) >= 0.1
    for b in (1, 2, nb):
        db = device_batch(N, M, fs, seeds, "diverse", nb=b)
        p, res, w = run(db, tb.params("diverse"), loss_of(kind, "diverse", fs, NEAR))
        compare(p, res, w, orc, f"{case} B = {b}")
        db.close()


# ---------------------------------------------------------------- 3. TRIVIAL is the plain solve, bit for bit
@pytest.mark.parametrize("shape,setname,seed0,nb", [((6, 40), "diverse", 1, 65), ((6, 40), "hard", tb.HARD_SEED0, tb.HARD_B),
                                                    ((33, 70), "hard", 1, 33), ((48, 100), "diverse", 1, 33),
                                                    ((64, 128), "diverse", 1, 33)], ids=str)
def test_trivial_is_the_plain_solve_bit_for_bit(shape, setname, seed0, nb):
    """featureSize 1: the tiles of the plain sweep.  The "hard" batches reject trials (tests/test_dense_batch_gpu.py,
    tests/dense_batch_wide_shapes.py)"""
    N, M = shape
    db = tb.device_batch(N, M, range(seed0, seed0 + nb), setname)
    prm = tb.params(setname)
    pp, rp = tb.run(db, prm)
    p, res, w = run(db, prm, BatchLoss(LOSS_TRIVIAL, 0.0, 1))
    assert p.tobytes() == pp.tobytes() and tb.bitwise_equal(res, rp)
    assert w.shape == (nb, M) and np.all(w == 1.0)
    if setname == "hard":
        assert np.any(rp["evaluations"] > rp["iterations"] + 1)
    # featureSize 2 divides the tile height of N = 6 (T 42) and of N = 64 (T 4): the same tiles, the same bits
    if N in (6, 64):
        p2, res2, w2 = run(db, prm, BatchLoss(LOSS_TRIVIAL, 0.0, 2))
        assert p2.tobytes() == pp.tobytes() and tb.bitwise_equal(res2, rp) and w2.shape == (nb, M // 2) and np.all(w2 == 1.0)
    db.close()


# ---------------------------------------------------------------- 4. rejected trials
# seeds of the "hard" set whose solves reject a trial at the WIDE scale, between problems that do not
REJECT_SEEDS = {"huber": (1, 95, 276, 2, 682, 1055, 1090, 1096, 3), "soft_l1": (1, 682, 2, 1090, 3)}
# (kind, trustregion_threshold or None): the margin recorded
REJECT_MARGIN = {("huber", None): 1.14e-3, ("huber", 100.0): 1.14e-3, ("soft_l1", None): 3.13e-2, ("soft_l1", 100.0): 3.13e-2}


@pytest.mark.parametrize("kind,threshold", sorted(REJECT_MARGIN, key=str), ids=str)
def test_rejected_trials(kind, threshold):
    """threshold 100: the first rejected trial ends the solve (TRUSTREGION), so the weights returned must be those of the point
    before it, which the oracle keeps apart from the trial's"""
    (N, M), fs = (6, 40), 2
    over = () if threshold is None else (("trustregion_threshold", threshold),)
    seeds = REJECT_SEEDS[kind]
    orc = oracle_batch(N, M, fs, kind, seeds, "hard", WIDE, False, over)
    assert_margin(orc, REJECT_MARGIN[(kind, threshold)], f"{kind} rejected, threshold {threshold}")
    assert sum(o["rejected"] for o in orc) >= 2
    if threshold is not None:
        stopped = [o for o in orc if o["status"] == BATCH_TRUSTREGION]
        assert len(stopped) >= 2 and all(o["rejected"] == 1 and o["weights"].min() < 0.99 for o in stopped)
        # the rejected trial's weights are not the returned point's: five decades over the tolerance of the comparison below
        apart = min(float(np.max(np.abs(o["last_weights"] - o["weights"]) / o["weights"])) for o in stopped)
        print(f"weights of the rejected trial against those of the returned point: at least {apart:.3g} apart")
        assert apart > 1e-3
    db = device_batch(N, M, fs, seeds, "hard")
    p, res, w = run(db, tb.params("hard", **dict(over)), loss_of(kind, "hard", fs, WIDE))
    compare(p, res, w, orc, f"{kind} rejected, threshold {threshold}")
    db.close()


# ---------------------------------------------------------------- 5. the device twin
def solve_dev(db, prm, loss, mask=None, stream=None, want_weights=True):
    """the device-resident robust solve under prefilled sentinels: (p, results, lambda, weights, counts)"""
    nb, N, NF = db.B, db.N, db.M // max(loss.featureSize, 1)
    P = td.Buf(db.p0())
    R = td.Buf(np.full(nb * td.RSIZE, td.PAD, dtype=np.uint8))
    Lm = td.Buf(np.full(nb, GUARD))
    W = td.Buf(np.full((nb, NF), GUARD)) if want_weights else None
    A = td.mask_dev(mask)
    db.reset_counters()
    rc = capi.optimize_dense_batch_robust_device(P.ptr, nb, N, db.M, db.cb, db.cookie, prm, loss, R.ptr, Lm.ptr,
                                                 W.ptr if W else None, A.ptr if A else None, stream)
    assert rc == 0
    counts = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    if A is not None:
        assert np.array_equal(A.get(), np.asarray(mask, dtype=np.uint8))
    return P.get(), td.results_of(R, nb), Lm.get(), W.get() if W else None, counts


DEVICE_CASES = [(6, 2, 40, "huber", True), (12, 2, 22, "cauchy", False), (48, 4, 104, "soft_l1", False),
                (64, 3, 132, "cauchy", True)]


@pytest.mark.parametrize("case", DEVICE_CASES, ids=str)
def test_device_twin_equals_host_twin(case):
    N, fs, M, kind, planted = case
    nb = td.B
    seeds = tuple(range(1, 1 + nb))
    db = device_batch(N, M, fs, seeds, "diverse", planted=planted)
    prm, loss = tb.params("diverse"), loss_of(kind, "diverse", fs, NEAR)
    ph, rh, wh = run(db, prm, loss)
    ch = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    pd, rd, ld, wd, cd = solve_dev(db, prm, loss)
    assert pd.tobytes() == ph.tobytes() and tb.bitwise_equal(rd, rh) and wd.tobytes() == wh.tobytes()
    assert ld.tobytes() == np.ascontiguousarray(rh["lambda_"]).tobytes() and cd == ch
    assert np.all(rh["status"] > 0) and np.all((wh > 0) & (wh <= 1))
    # no weights asked for: the same solve
    pn, rn, ln, wn, _ = solve_dev(db, prm, loss, want_weights=False)
    assert pn.tobytes() == ph.tobytes() and tb.bitwise_equal(rn, rh) and wn is None
    rc, p2, r2, w2 = capi.optimize_dense_batch_robust(db.p0(), N, M, db.cb, db.cookie, loss, prm, want_weights=False)
    assert rc == 0 and p2.tobytes() == ph.tobytes() and tb.bitwise_equal(r2, rh) and w2 is None
    db.close()


@pytest.mark.parametrize("case", [(6, 2, 40, "cauchy"), (48, 4, 104, "huber"), (64, 3, 132, "soft_l1")], ids=str)
def test_mask(case):
    N, fs, M, kind = case
    nb = td.B
    db = device_batch(N, M, fs, tuple(range(1, 1 + nb)), "diverse")
    prm, loss = tb.params("diverse"), loss_of(kind, "diverse", fs, NEAR)
    p0 = db.p0()
    pf, rf, lf, wf, _ = solve_dev(db, prm, loss)
    m = td.the_mask(N)
    on, off = np.flatnonzero(m), np.flatnonzero(m == 0)
    pm, rm, lm, wm, cm = solve_dev(db, prm, loss, mask=m)
    assert pm[on].tobytes() == pf[on].tobytes() and tb.bitwise_equal(rm[on], rf[on]) and lm[on].tobytes() == lf[on].tobytes()
    assert wm[on].tobytes() == wf[on].tobytes()
    # not run: p and the weights untouched, the record of a problem that is not run
    assert pm[off].tobytes() == p0[off].tobytes() and np.all(wm[off] == GUARD)
    assert np.all(rm["norm2_x"][off] == -1.0) and np.all(rm["status"][off] == BATCH_NOT_RUN)
    for k in ("trustregion", "lambda_", "iterations", "evaluations"):
        assert not rm[k][off].any(), k
    assert not lm[off].any()
    assert cm["nevals"] == int(rm["evaluations"].sum()) and cm["ncalls"] == int(rm["evaluations"].max()) == cm["rounds"]
    pz, rz, lz, wz, cz = solve_dev(db, prm, loss, mask=np.zeros(nb, dtype=np.uint8))
    assert pz.tobytes() == p0.tobytes() and cz["ncalls"] <= 1 and cz["nevals"] == 0 and np.all(wz == GUARD)
    assert np.all(rz["status"] == BATCH_NOT_RUN) and np.all(rz["norm2_x"] == -1.0) and not lz.any()
    db.close()


def test_a_failing_problem_fails_alone():
    N, fs, M, kind = 6, 2, 40, "cauchy"
    nb = td.B
    bad = [0, 31, nb - 1]
    db = device_batch(N, M, fs, tuple(range(1, 1 + nb)), "diverse")
    prm, loss = tb.params("diverse"), loss_of(kind, "diverse", fs, NEAR)
    pg, rg, wg = run(db, prm, loss)
    mode = np.zeros(nb, dtype=np.uint8)
    mode[bad] = MODE_NAN
    db.set_mode(mode)
    p0 = db.p0()
    good = np.setdiff1d(np.arange(nb), bad)
    ph, rh, wh = run(db, prm, loss)
    pd, rd, ld, wd, _ = solve_dev(db, prm, loss)
    for p, r, w in ((ph, rh, wh), (pd, rd, wd)):
        assert p[bad].tobytes() == p0[bad].tobytes() and np.all(np.isnan(w[bad]))
        assert np.all(r["norm2_x"][bad] == -1.0) and np.all(r["status"][bad] == BATCH_FAILED)
        assert p[good].tobytes() == pg[good].tobytes() and tb.bitwise_equal(r[good], rg[good])
        assert w[good].tobytes() == wg[good].tobytes()
    db.close()


STREAM_CHILD = r'''
import sys
import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded
sys.path.insert(0, sys.argv[1])
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_robust_gpu as tr
from tests import test_dense_batch_gpu as tb
from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchResult

N, fs, M, B = 6, 2, 40, td.B
NF = M // fs
db = tr.device_batch(N, M, fs, tuple(range(1, 1 + B)), "diverse")
prm, loss = tb.params("diverse"), tr.loss_of("cauchy", "diverse", fs, tr.NEAR)
p0 = db.p0()
pn, rn, ln, wn, cn = tr.solve_dev(db, prm, loss)          # hip_stream NULL
s = torch.cuda.Stream()
host = torch.from_numpy(p0.copy()).pin_memory()
dev = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
res = torch.full((B * td.RSIZE + 512,), td.PAD, dtype=torch.uint8, device="cuda")
lam = torch.full((B + 64,), td.GUARD, dtype=torch.float64, device="cuda")
wts = torch.full((B * NF + 64,), td.GUARD, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(s):
    dev[:B * N].copy_(host.reshape(-1), non_blocking=True)      # asynchronous, on s; no synchronisation before the call
rc = capi.optimize_dense_batch_robust_device(dev.data_ptr(), B, N, M, db.cb, db.cookie, prm, loss, res.data_ptr(), lam.data_ptr(),
                                             wts.data_ptr(), None, s.cuda_stream)
assert rc == 0
torch.cuda.synchronize()
ps, ls, ww, raw = dev.cpu().numpy(), lam.cpu().numpy(), wts.cpu().numpy(), res.cpu().numpy()
assert np.all(ps[B * N:] == td.GUARD) and np.all(ls[B:] == td.GUARD) and np.all(raw[B * td.RSIZE:] == td.PAD)
assert np.all(ww[B * NF:] == td.GUARD)
rs = capi._batch_results((BatchResult * B).from_buffer_copy(raw[:B * td.RSIZE].tobytes()), B)
assert ps[:B * N].tobytes() == pn.tobytes() and ls[:B].tobytes() == ln.tobytes() and tb.bitwise_equal(rs, rn)
assert ww[:B * NF].tobytes() == wn.tobytes()
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


# ---------------------------------------------------------------- 6. refusals: -1, no invocation, nothing written
def test_refusals_on_the_gpu():
    N, fs, M, nb = 6, 2, 40, 4
    NF = M // fs
    db = tb.device_batch(N, M, range(1, 1 + nb), "default")
    db.reset_counters()
    P = td.Buf(db.p0())
    R = td.Buf(np.full(nb * td.RSIZE, td.PAD, dtype=np.uint8))
    Lm = td.Buf(np.full(nb, GUARD))
    W = td.Buf(np.full((nb, NF), GUARD))
    short = capi.DeviceArray(nbytes=8 * (nb * NF - 1))
    prm = tb.params("default")
    good = BatchLoss(LOSS_HUBER, 0.5, fs)

    def dev(p=P.ptr, b=nb, n=N, m=M, f=db.cb, r=R.ptr, loss=good, w=W.ptr):
        return capi.optimize_dense_batch_robust_device(p, b, n, m, f, db.cookie, prm, loss, r, Lm.ptr, w)

    def host(loss=good, m=M, n=N):
        rc, p, res, w = capi.optimize_dense_batch_robust(np.full((nb, n), 2.5), n, m, db.cb, db.cookie, loss, prm)
        assert np.all(p == 2.5) and np.all(w == -1.0) and not res["status"].any()
        return rc

    for call in (dev, host):
        assert call(loss=None) == -1 and call(loss=BatchLoss(7, 0.5, fs)) == -1 and call(loss=BatchLoss(-1, 0.5, fs)) == -1
        for scale in (0.0, -2.0, np.inf, np.nan):
            assert call(loss=BatchLoss(LOSS_CAUCHY, scale, fs)) == -1, scale
        assert call(loss=BatchLoss(LOSS_SOFT_L1, 0.5, 5)) == -1 and call(loss=BatchLoss(LOSS_SOFT_L1, 0.5, 3)) == -1
    assert dev(p=None) == -1 and dev(r=None) == -1 and dev(f=None) == -1 and dev(b=0) == -1
    assert host(n=BATCH_MAX_NSTATE + 1) == -1
    assert dev(w=short.ptr) == -1                               # the weights' span is checked as the others are
    assert dev(w=np.zeros((nb, NF)).ctypes.data) == -1          # pageable host memory
    L = capi.lib()
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert dev() == -1 and host() == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert db.ncalls() == 0
    assert np.all(R.get() == td.PAD) and np.all(Lm.get() == GUARD) and np.all(W.get() == GUARD)
    assert P.get().tobytes() == db.p0().tobytes()
    # and the valid call behind them
    assert dev() == 0 and np.all(td.results_of(R, nb)["status"] > 0) and np.all((W.get() > 0) & (W.get() <= 1))
    short.free()
    db.close()
