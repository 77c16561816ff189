"""dogleg_amd_optimize_dense_batch and dogleg_amd_dense_batch_uncertainty at every size class, dispatch edge and tile edge of
dense_batch.hip: the case table of tests/dense_batch_shapes.py, whose coverage, decision margins and reference accuracy
tests/test_dense_batch_shapes_cpu.py asserts with the oracle alone.  The references and the tolerances are those of
tests/test_dense_batch_gpu.py (the CPU oracle per problem: |p - p_oracle|_inf <= 1e-10, norm2_x and the trust region 1e-8
relative, iterations, evaluations, status and lambda equal) and of tests/test_dense_batch_uncertainty_gpu.py (Sigma and the
variances 1e-9 scaled, the factors rtol 1e-9 / atol 1e-12, a computed scale 1e-12); nothing of the library under test
computes what is checked.

What the cases are there for.  k_batch_round<NMAX> and k_batch_uncertainty<NMAX> exist for NMAX = 8, 16, 24, 32 (N <= 8 / 16
/ 24 / else): the table has N on both sides of every edge, N = 1 and 2, and of the row tile T = min(64, 256 / N) of the sweep
a partial tile, exactly one tile, one tile and a row, and several tiles with a ragged last one; the uncertainty table adds odd
M (a trailing measurement that featureSize 2 does not cover) and N = 11 and 17, where the second sweep's tile is rounded down
to an even number of rows.  The rejected trial's reload of JtJ, the lambda loop and "the neighbours do not matter" run at N =
24, 31, 32, where the packed triangle has more entries than a wavefront has lanes and each wavefront's LDS slice is the
<24> or <32> carve-up, and two batches are under-determined (M < N: the lambda loop at the first factorisation of every problem).

Measured on the CPU for the uncertainty cases, at the oracle's end points of problems 1 .. 65 (asserted in the CPU file): two
independent host computations (LAPACK inverse, the oracle's packed Cholesky) agree to 5.5e-15 scaled on Sigma and 1.9e-14 on
the factors; cond(JtJ) <= 173, the largest leverage is 0.90, min |det(A_f - I)| = 0.026, so no reference value is DBL_MAX;
lambda is 0 throughout.  The under-determined shape (24, 9) is left out: its decision margin, 1.3e-3, does not stand a decade
over the 1e-3 to which p is compared there; (20, 9), margin 0.25, runs the <24> instantiation in its place.

Measured on an MI355X, B = 65 (margins: diverse / default; |p - p_oracle|: the larger of the two sets; Sigma scaled and factors
relative: the larger of featureSize 1 and 2):
  (N, M)     margins              |p - p_oracle|   Sigma     factors
  (1, 1)     8.21e-3 / 8.67e-2    0                -         -
  (1, 5)     1.21e-2 / 1.70e-2    0                5.5e-16   1.1e-13
  (2, 9)     8.91e-3 / 3.04e-2    5.6e-17          1.0e-15   3.7e-14
  (5, 103)   1.06e-2 / 3.14e-3    1.1e-16          5.3e-16   6.4e-14
  (8, 32)    7.26e-5 / 1.09e-2    1.1e-16          8.1e-16   5.1e-15
  (8, 33)    5.19e-3 / 3.54e-2    1.1e-16          1.0e-15   5.7e-15
  (9, 55)    3.96e-3 / 1.40e-2    1.1e-16          8.9e-16   7.1e-15
  (11, 47)   -                    -                9.4e-16   6.9e-15
  (16, 50)   8.41e-2 / 1.55e-2    1.1e-16          1.2e-15   2.9e-15
  (17, 40)   2.30e-2 / 5.96e-3    1.1e-16          -         -
  (17, 41)   -                    -                1.7e-15   3.7e-15
  (24, 73)   9.57e-3 / 7.50e-3    1.1e-16          1.5e-15   3.0e-15
  (25, 81)   2.91e-3 / 7.31e-5    1.1e-16          1.2e-15   3.0e-15
  (31, 47)   5.35e-3 / 2.76e-2    2.2e-16          5.8e-15   1.3e-14
norm2_x agreed to 8.2e-16 relative and the trust region exactly at every case.  The "hard" batches (32, 70) and (24, 73),
margins 7.70e-3 and 1.07e-2: |p - p_oracle| 1.1e-16, trust region 4.9e-15 relative; the zero-column batches, margins 7.83e-3
and 1.30e-2: 1.1e-16; the under-determined (10, 6) and (20, 9): 7.8e-7 and 8.1e-7 against the 1e-3 allowed."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, dptr
from tests import dense_batch_shapes as ds
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 2. parity of the solve at every case
def parity(shape, setname, want):
    N, M = shape
    orc = tb.oracle_batch(N, M, ds.SEED0, ds.B, setname)
    m = tb.assert_margin(orc, f"{shape} {setname} seed0 {ds.SEED0}")
    assert ds.recorded(m, want), "the generator changed: search seed0 again"
    types = set().union(*[o["step_types"] for o in orc])
    print(f"<{ds.size_class(N)}>, T {ds.T(N)}, step types {sorted(types)}")
    if setname == "diverse":
        assert types == ({0, 1, 2} if N >= 2 else {0, 1})
    for nb in (1, 2, ds.B):
        db = tb.device_batch(N, M, range(ds.SEED0, ds.SEED0 + nb), setname)
        p, res = tb.run(db, tb.params(setname))
        db.close()
        tb.compare(p, res, orc, f"{shape} {setname} B = {nb}", idx=range(nb))


@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(ds.CASES))
def test_parity_of_the_solve(shape, setname):
    parity(shape, setname, ds.CASES[shape][setname])


@pytest.mark.parametrize("setname", ["diverse", "default"])
def test_parity_with_one_measurement_of_one_state(setname):
    parity((1, 1), setname, ds.ONE_BY_ONE[(1, 1)][setname])


# ---------------------------------------------------------------- 3. the paths tested at (6, 40) only, where their loops make several passes
@pytest.mark.parametrize("shape", sorted(ds.RETRY))
def test_rejected_trials_and_the_retry(shape):
    N, M = shape
    seed0, B, want, rejected = ds.RETRY[shape]
    orc = tb.oracle_batch(N, M, seed0, B, "hard")
    m = tb.assert_margin(orc, f"hard set {shape}")
    assert ds.recorded(m, want) and sum(o["rejected"] for o in orc) == rejected >= 1
    db = tb.device_batch(N, M, range(seed0, seed0 + B), "hard")
    p, res = tb.run(db, tb.params("hard"))
    db.close()
    tb.compare(p, res, orc, f"hard set {shape}")


@pytest.mark.parametrize("shape", sorted(ds.ZERO_COLUMN))
def test_lambda_is_per_problem(shape):
    col, want = ds.ZERO_COLUMN[shape]
    p, res, orc = tb._zero_column_batch(tb.params("default"), B=ds.ZERO_B, chosen=ds.ZERO_CHOSEN, zero_col=col, shape=shape)
    assert ds.recorded(min(o["margin"] for o in orc), want)
    for b in range(len(orc)):
        assert orc[b]["lambda_"] == (1e-10 if b in ds.ZERO_CHOSEN else 0.0)
    # (1e-9: the tolerance of tests/test_dense_batch_gpu.py::test_lambda_is_per_problem, for the singular problems)
    tb.compare(p, res, orc, f"zero column {col} of {shape}", p_tol=1e-9)


@pytest.mark.parametrize("shape", sorted(ds.UNDER))
def test_underdetermined_batches(shape):
    """M < N: JtJ is singular, every problem's first factorisation fails and lambda goes to 1e-10.  cond(JtJ + 1e-10 I) ~
    1e11, so two Cholesky factorisations agree to ~1e-5 at best: p to 1e-3, as
    tests/test_edge_cases_gpu.py::test_underdetermined_system_takes_the_lambda_path, the decisions exactly (the CPU file
    asserts their margin above 1e-2)"""
    N, M = shape
    orc = ds.under_oracle(shape)
    m = min(o["margin"] for o in orc)
    assert m > ds.UNDER_MARGIN_FLOOR and ds.recorded(m, ds.UNDER[shape])
    db = tb.device_batch(N, M, range(1, 1 + ds.UNDER_B), "default")
    p, res = tb.run(db, tb.params("default", **dict(ds.UNDER_OVER)))
    db.close()
    dp = max(float(np.max(np.abs(p[b] - o["p"]))) for b, o in enumerate(orc))
    print(f"{shape}: margin {m:.3g}, max |p - p_oracle| {dp:.3g}, largest norm2_x {float(res['norm2_x'].max()):.3g} "
          f"(the oracle's {max(o['norm2_x'] for o in orc):.3g}), iterations {sorted(set(res['iterations'].tolist()))}")
    for b, o in enumerate(orc):
        got = (int(res["iterations"][b]), int(res["evaluations"][b]), int(res["status"][b]), float(res["lambda_"][b]))
        assert got == (o["iterations"], o["evaluations"], o["status"], o["lambda_"]), f"problem {b}: {got}"
        assert o["lambda_"] == 1e-10
    assert dp <= ds.UNDER_P_TOL


@pytest.mark.parametrize("shape", ds.NEIGHBOUR_SHAPES)
def test_order_and_neighbours_do_not_matter_to_the_solve(shape):
    N, M = shape
    B = ds.NEIGHBOUR_B
    seeds = np.arange(1, 1 + B)
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res = tb.run(db, tb.params("diverse"))
    db.close()
    perm = np.random.default_rng(5).permutation(B)
    db = tb.device_batch(N, M, seeds[perm], "diverse")
    pp, resp = tb.run(db, tb.params("diverse"))
    db.close()
    assert pp.tobytes() == p[perm].tobytes() and tb.bitwise_equal(resp, res[perm])
    for b in ds.NEIGHBOUR_ALONE:
        db = tb.device_batch(N, M, seeds[b:b + 1], "diverse")
        p1, res1 = tb.run(db, tb.params("diverse"))
        db.close()
        assert p1.tobytes() == p[b:b + 1].tobytes() and tb.bitwise_equal(res1, res[b:b + 1]), b


@pytest.mark.parametrize("shape", ds.NEIGHBOUR_SHAPES)
def test_order_and_neighbours_do_not_matter_to_the_uncertainty(shape):
    N, M = shape
    B = ds.NEIGHBOUR_B
    seeds = np.arange(1, 1 + B)
    db, p, lam = tu.solved(N, M, seeds)
    base = {fs: tu.unc(db, p, lam, fs=fs) for fs in (1, 2)}
    db.close()
    perm = np.random.default_rng(9).permutation(B)
    db = tu.device_batch(N, M, seeds[perm])
    for fs in (1, 2):
        assert np.all(base[fs]["status"] == BATCH_UNC_OK)
        assert tu.same_bits(base[fs], tu.unc(db, p[perm], lam[perm], fs=fs), idx_a=perm), fs
    db.close()
    for b in ds.NEIGHBOUR_ALONE:
        db = tu.device_batch(N, M, seeds[b:b + 1])
        for fs in (1, 2):
            assert tu.same_bits(base[fs], tu.unc(db, p[b:b + 1], lam[b:b + 1], fs=fs), idx_a=slice(b, b + 1)), (b, fs)
        db.close()


# ---------------------------------------------------------------- 4. parity of the uncertainty call at every case
GUARD = -7.5


def factors_with_a_guard(db, p, lam, fs):
    """the call itself with 64 doubles behind the factors: (factors (B, M // fs), the 64 doubles)"""
    B, NF = p.shape[0], db.M // fs
    fac = np.full(B * NF + 64, GUARD)
    lam, scale, status = lam.copy(), np.full(B, -1.0), np.full(B, -1, dtype=np.int32)
    rc = capi.lib().dogleg_amd_dense_batch_uncertainty(dptr(np.ascontiguousarray(p)), B, db.N, db.M, db.cb, db.cookie, dptr(lam),
                                                       None, None, dptr(fac), dptr(scale), fs, capi.iptr(status))
    assert rc == 0 and np.all(status == BATCH_UNC_OK)
    return fac[:B * NF].reshape(B, NF), fac[B * NF:]


@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("shape", ds.UNC_CASES)
def test_parity_of_the_uncertainty(shape, fs):
    N, M = shape
    B = ds.UNC_B
    seeds = np.arange(ds.SEED0, ds.SEED0 + B)
    db, p, lam = tu.solved(N, M, seeds)
    out = tu.unc(db, p, lam, fs=fs)
    fac, behind = factors_with_a_guard(db, p, lam, fs)
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK) and np.array_equal(out["lam"], lam) and np.all(lam == 0.0)
    # with an odd M and fs = 2 the last measurement belongs to no feature: M // 2 factors, and nothing behind them
    assert out["factors"].shape == (B, M // fs)
    assert np.all(behind == GUARD) and fac.tobytes() == out["factors"].tobytes()
    print(f"<{ds.size_class(N)}>, T {ds.T(N)}, T2 {ds.T2(N, fs)}, {M // fs} features")
    nmax = tu.check_against_reference(out, N, M, seeds, p, lam, fs, f"{shape} fs {fs}")
    assert nmax == 0


def test_lambda_loop_of_the_uncertainty_on_a_zero_column():
    N, M = ds.UNC_ZERO_SHAPE
    tu.check_lambda_loop_on_a_zero_column(N, M, ds.UNC_ZERO_COLUMN, B=ds.ZERO_B, chosen=ds.ZERO_CHOSEN)
