"""dogleg_amd_optimize_dense_products_batch against the CPU oracle: one oa.oracle_solve("products", ...) per problem, packed
upper, with a host products callback over the problem's own M[b] rows (tests/batch_products_oracle.py); on the device the
fused callback of problems/device_batch_products.hip.  Tolerances, those of tests/test_dense_batch_gpu.py:
|p - p_oracle|_inf <= 1e-10, norm2_x and the trust region to 1e-8 relative, lambda, iterations, evaluations and status equal.

Every test first asserts, on the oracle side, that the smallest decision margin of its problems is above MARGIN_FLOOR = 1e-6
and equals, to 5 %, the value recorded in batch_products_oracle (computed on the CPU with the products oracle alone;
tests/test_dense_products_batch_cpu.py reproduces all of them without a GPU).  The cases: the shapes of the J-form files, all
four kernel size classes with a packed triangle of at most 64 entries (one pass of the loader) and of more (several),
ragged batches whose problems have their own number of measurements, the "hard" set with its rejected trials, and zero
columns that send three problems of 32 through the lambda loop."""
import ctypes as C

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_FAILED, BATCH_MAX_ITERATIONS
from tests import batch_products_oracle as po
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu

REL_SCALAR_TOL = 1e-8


def device_batch(N, Ms, seeds, setname, layout=None):
    from problems.batch import DeviceProductsBatch, LAYOUT_PACKED_UPPER
    eps, noise, spread, _ = po.SETS[setname]
    return DeviceProductsBatch(len(seeds), Ms, N, seeds=np.asarray(seeds, dtype=np.uint64), eps=eps, noise=noise,
                               p0_spread=spread, layout=LAYOUT_PACKED_UPPER if layout is None else layout)


def run(db, prm):
    """a solve of the batch in the layout it is set to; one callback per round, live problems only"""
    db.reset_counters()
    rc, p, res = capi.optimize_dense_products_batch(db.p0(), db.N, db.cb, db.cookie, db.set_params(prm))
    assert rc == 0
    rounds = capi.batch_last_stats()["rounds"]
    assert db.ncalls() == int(res["evaluations"].max()) == rounds and db.nevals() == int(res["evaluations"].sum())
    return p, res


def compare(p, res, orc, what, idx=None, p_tol=STEP_TOL):
    """every problem of the batch result against its oracle solve; prints the figures, then asserts"""
    idx = list(range(len(orc)) if idx is None else idx)
    dp = max(float(np.max(np.abs(p[k] - orc[b]["p"]))) for k, b in enumerate(idx))
    dn = max(abs(res["norm2_x"][k] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for k, b in enumerate(idx))
    dt = max(abs(res["trustregion"][k] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for k, b in enumerate(idx))
    print(f"{what}: {len(idx)} problems, max |p - p_oracle| {dp:.3g}, norm2_x rel {dn:.3g}, trust region rel {dt:.3g}")
    for k, b in enumerate(idx):
        o = orc[b]
        got = (int(res["iterations"][k]), int(res["evaluations"][k]), int(res["status"][k]), float(res["lambda_"][k]))
        want = (o["iterations"], o["evaluations"], o["status"], o["lambda_"])
        assert got == want, f"{what}: problem {b}: (iterations, evaluations, status, lambda) {got}, the oracle {want}"
    assert dp <= p_tol and dn <= REL_SCALAR_TOL and dt <= REL_SCALAR_TOL


def bitwise_equal(a, b):
    """record arrays of results, field by field (the struct's padding bytes are nobody's)"""
    return all(np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes() for f in a.dtype.names)


def parity(N, Ms, B, orc, setname, what, **over):
    """the batch at B = 1, 2 (a workgroup of one wave, then of two) and the full B against the oracle"""
    Ms = np.broadcast_to(Ms, (B,))
    for nb in (1, 2, B):
        db = device_batch(N, Ms[:nb], range(1, 1 + nb), setname)
        p, res = run(db, po.params(setname, **over))
        compare(p, res, orc, f"{what} B = {nb}", idx=range(nb))
        db.close()


# ---------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(po.PARITY))
def test_parity_over_a_batch(shape, setname):
    N, M = shape
    B, want = po.PARITY[shape]
    orc = po.oracle_batch(N, M, 1, B, setname)
    po.assert_margin(orc, f"{shape} {setname}", want[setname])
    types = set().union(*[o["step_types"] for o in orc])
    evals = {o["evaluations"] for o in orc}
    print(f"step types {sorted(types)}, evaluations {min(evals)} .. {max(evals)}")
    if setname == "diverse":
        assert types == ({0, 1, 2} if N >= 2 else {0, 1})
    parity(N, M, B, orc, setname, f"{shape} {setname}")


@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("N", sorted(po.RAGGED))
def test_parity_over_a_ragged_batch(N, setname):
    (Mmin, Mmax), want = po.RAGGED[N]
    orc = po.oracle_batch(N, 0, 1, po.B, setname, ragged=(Mmin, Mmax))
    po.assert_margin(orc, f"ragged N {N} {setname}", want[setname])
    parity(N, po.ragged_M(po.B, Mmin, Mmax), po.B, orc, setname, f"ragged N {N} {setname}")


def test_rejected_trials_and_the_retry():
    N, M = po.HARD_SHAPE
    orc = po.oracle_batch(N, M, po.HARD_SEED0, po.HARD_B, "hard")
    po.assert_margin(orc, "hard set", po.HARD_MARGIN)
    assert sum(o["rejected"] for o in orc) == po.HARD_REJECTED
    ev = [o["evaluations"] for o in orc]
    assert (min(ev), max(ev)) == po.HARD_EVALS
    db = device_batch(N, M, range(po.HARD_SEED0, po.HARD_SEED0 + po.HARD_B), "hard")
    p, res = run(db, po.params("hard"))
    compare(p, res, orc, "hard set")
    db.close()


@pytest.mark.parametrize("shape", sorted(po.ZERO_COLUMN))
def test_lambda_is_per_problem(shape):
    from problems.batch import MODE_ZERO_COLUMN
    N, M = shape
    col, want = po.ZERO_COLUMN[shape]
    orc = po.oracle_batch(N, M, 1, po.ZERO_B, "default", zero=(po.ZERO_CHOSEN, col))
    po.assert_margin(orc, f"zero column {shape}", want)
    assert [o["lambda_"] for o in orc] == [1e-10 if b in po.ZERO_CHOSEN else 0.0 for b in range(po.ZERO_B)]
    db = device_batch(N, M, range(1, 1 + po.ZERO_B), "default")
    mode = np.zeros(po.ZERO_B, dtype=np.uint8)
    mode[list(po.ZERO_CHOSEN)] = MODE_ZERO_COLUMN
    db.set_mode(mode, col)
    p, res = run(db, po.params("default"))
    db.close()
    compare(p, res, orc, f"zero columns {shape}")


@pytest.mark.parametrize("max_iterations", [1, 2, 3, 5])
def test_iterate_sequence(max_iterations):
    N, M, B = 6, 40, po.B
    over = (("max_iterations", max_iterations),)
    orc = po.oracle_batch(N, M, 1, B, "diverse", over)
    po.assert_margin(orc, f"max_iterations {max_iterations}")
    db = device_batch(N, M, range(1, 1 + B), "diverse")
    p, res = run(db, po.params("diverse", **dict(over)))
    compare(p, res, orc, f"max_iterations {max_iterations}")
    cut = [b for b in range(B) if orc[b]["status"] == BATCH_MAX_ITERATIONS]
    assert all(orc[b]["iterations"] == max_iterations for b in cut) and (max_iterations > 2 or cut)
    assert all(res["status"][b] == BATCH_MAX_ITERATIONS for b in cut)
    db.close()


# ---------------------------------------------------------------- layouts, neighbours, the J form
@pytest.mark.parametrize("shape", [(6, 40), (25, 81)])
def test_the_three_layouts_give_the_same_bits(shape):
    """packed upper, unpacked, and unpacked with the strict lower triangle NaN: only the entries [i][j], j >= i, are read"""
    from problems.batch import LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER
    N, M = shape
    B = po.B_SMALL
    got = {}
    for layout in (LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        db = device_batch(N, M, range(1, 1 + B), "diverse", layout)
        got[layout] = run(db, po.params("diverse"))
        db.close()
    p, res = got[LAYOUT_PACKED_UPPER]
    assert np.all(res["status"] != BATCH_FAILED) and len(set(res["evaluations"])) > 1
    for layout in (LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        assert got[layout][0].tobytes() == p.tobytes() and bitwise_equal(got[layout][1], res), layout


def test_order_and_neighbours_do_not_matter():
    N, M, B = 24, 73, po.B
    seeds = np.arange(1, 1 + B)
    db = device_batch(N, M, seeds, "diverse")
    p, res = run(db, po.params("diverse"))
    db.close()
    db = device_batch(N, M, seeds[::-1], "diverse")
    pr, resr = run(db, po.params("diverse"))
    db.close()
    assert pr.tobytes() == np.ascontiguousarray(p[::-1]).tobytes() and bitwise_equal(resr, res[::-1])
    for b in (0, 100, 256):
        db = device_batch(N, M, seeds[b:b + 1], "diverse")
        p1, res1 = run(db, po.params("diverse"))
        db.close()
        assert p1.tobytes() == p[b:b + 1].tobytes() and bitwise_equal(res1, res[b:b + 1])


def test_against_the_j_form():
    """the same 257 problems through dogleg_amd_optimize_dense_batch with the J-form twin"""
    from problems.batch import DeviceBatch
    N, M, B = 16, 96, po.B
    eps, noise, spread, _ = po.SETS["diverse"]
    db = device_batch(N, M, range(1, 1 + B), "diverse")
    p, res = run(db, po.params("diverse"))
    db.close()
    dj = DeviceBatch(B, M, N, seeds=1, eps=eps, noise=noise, p0_spread=spread)
    rc, pj, resj = capi.optimize_dense_batch(dj.p0(), N, M, dj.cb, dj.cookie, po.params("diverse"))
    dj.close()
    assert rc == 0
    for f in ("iterations", "evaluations", "status", "lambda_"):
        assert np.array_equal(res[f], resj[f]), f
    d = float(np.max(np.abs(p - pj)))
    print(f"products form against the J form: max |dp| {d:.3g}")
    assert d <= STEP_TOL and len(set(res["evaluations"])) > 1


# ---------------------------------------------------------------- failures
@pytest.mark.parametrize("mode_name", ["MODE_NAN", "MODE_NAN_OFFDIAGONAL"])
def test_a_failing_problem_fails_alone(mode_name):
    """x[0] = NaN (norm2x and xtJ non-finite), or a NaN in one off-diagonal entry of JtJ and nowhere else"""
    from problems import batch
    N, M, B = 6, 40, 32
    bad = [3, 17, 30]
    good = [b for b in range(B) if b not in bad]
    db = device_batch(N, M, [1 + b for b in good], "default")        # a run without the three
    plain_p, plain = run(db, po.params("default"))
    db.close()
    db = device_batch(N, M, range(1, 1 + B), "default")
    p0 = db.p0()
    mode = np.zeros(B, dtype=np.uint8)
    mode[bad] = getattr(batch, mode_name)
    db.set_mode(mode)
    p, res = run(db, po.params("default"))
    db.close()
    for b in bad:
        assert res["status"][b] == BATCH_FAILED and res["norm2_x"][b] < 0 and np.array_equal(p[b], p0[b])
        assert res["evaluations"][b] == 1
    assert np.all(plain["status"] != BATCH_FAILED)
    assert p[good].tobytes() == plain_p.tobytes() and bitwise_equal(res[good], plain)


def test_refusals_on_the_gpu():
    N, M = 6, 40
    db = device_batch(N, M, range(1, 3), "default")
    p0 = db.p0()
    prm = po.params("default")
    prm.JtJ_packed, prm.JtJ_upper = True, False                  # packed lower
    db.reset_counters()
    rc, p, _ = capi.optimize_dense_products_batch(p0, N, db.cb, db.cookie, prm)
    assert rc == -1 and np.array_equal(p, p0) and db.ncalls() == 0
    L = capi.lib()
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        rc, p, _ = capi.optimize_dense_products_batch(p0, N, db.cb, db.cookie, po.params("default"))
        assert rc == -1 and np.array_equal(p, p0) and db.ncalls() == 0
    finally:
        L.dogleg_amd_clear_communicator()
    p, res = run(db, po.params("default"))
    assert np.all(res["status"] > 0) and np.all(res["status"] != BATCH_FAILED)
    db.close()
