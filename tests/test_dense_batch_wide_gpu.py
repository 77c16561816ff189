"""The batch entry points at 33 .. 64 variables: the size classes <48> and <64> of k_batch_round and k_batch_uncertainty in
both forms, dogleg_amd_check_jacobian_device_batch at 64 variables and the refusal of 65.  The case table is
tests/dense_batch_wide_shapes.py, whose coverage, decision margins and reference accuracy
tests/test_dense_batch_wide_cpu.py asserts with the oracles alone.  References and tolerances are those of the files the
helpers come from, unchanged: the CPU oracle per problem (|p - p_oracle|_inf <= 1e-10, norm2_x and the trust region 1e-8
relative, iterations, evaluations, status and lambda equal; p to 1e-3 with the decisions exact on the under-determined
batches), the host reference of the uncertainty call (Sigma and the variances 1e-9 scaled, the factors rtol 1e-9 / atol
1e-12).  Nothing of the library under test computes what is checked.

What the cases are there for.  The dispatch is N <= 32 / <= 48 / else: N = 33 and 48, 49 and 64 stand on both sides of the
new edges (32 itself runs in tests/test_dense_batch_shapes_gpu.py), 63 and 64 end the range.  The first sweep's tile is
T = 256 / N = 7 / 6 / 5 / 5 / 4 / 4 rows: (33, 70), (48, 100), (64, 128) are whole tiles, (40, 97), (49, 103), (63, 131) end
on a ragged one and give the uncertainty call an odd M.  <48> runs two problems per workgroup and <64> one, so B = 1, 2, 33
and 65 give a workgroup of one wavefront, a full one, and a last one half empty.

Measured on the CPU (asserted in the CPU file), at the oracle's end points of problems 1 .. 33: two independent host
computations agree to 2.7e-15 scaled on Sigma and 3.5e-15 on the factors; cond(JtJ) <= 41.9, the largest leverage is 0.81,
min |det(A_f - I)| = 0.108, no reference value is DBL_MAX, lambda is 0 throughout.

Measured on an MI355X, B = 33: |p - p_oracle| <= 2.2e-16 and norm2_x 2.2e-15 relative at every solve in both forms (the
trust region exact but for the "hard" batches, 5.7e-15); the under-determined (40, 12) and (64, 20): 8.5e-7 and 1.1e-6
against the 1e-3 allowed; Sigma 1.7e-15 .. 2.3e-15 scaled and the factors 1.1e-15 .. 4.1e-15 relative at the six shapes,
Sigma of the ragged products batches 5.5e-15 / 7.7e-15 / 1.7e-14 at N = 33 / 48 / 64; the whole file runs in 2 s."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, BATCH_UNC_FAILED, BATCH_FAILED, BatchResult, dptr
from problems import gradcheck as gp
from tests import dense_batch_wide_shapes as ws
from tests import batch_products_oracle as po
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu
from tests import test_dense_products_batch_gpu as tp
from tests import test_dense_products_batch_uncertainty_gpu as tpu
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. parity of the solve
@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(ws.CASES))
def test_parity_of_the_solve(shape, setname):
    N, M = shape
    orc = tb.oracle_batch(N, M, ws.SEED0, ws.B, setname)
    m = tb.assert_margin(orc, f"{shape} {setname} seed0 {ws.SEED0}")
    assert ws.recorded(m, ws.CASES[shape][setname]), "the generator changed: record the margin again"
    types = set().union(*[o["step_types"] for o in orc])
    print(f"<{ws.size_class(N)}>, {ws.problems_per_workgroup(N)} per workgroup, T {ws.T(N)}, step types {sorted(types)}")
    if setname == "diverse":
        assert types == {0, 1, 2}
    for nb in (1, 2, ws.B):
        db = tb.device_batch(N, M, range(ws.SEED0, ws.SEED0 + nb), setname)
        p, res = tb.run(db, tb.params(setname))
        db.close()
        tb.compare(p, res, orc, f"{shape} {setname} B = {nb}", idx=range(nb))


# ---------------------------------------------------------------- 2. rejected trials: the reload of JtJ
@pytest.mark.parametrize("shape", sorted(ws.RETRY))
def test_rejected_trials_and_the_retry(shape):
    N, M = shape
    want, rejected = ws.RETRY[shape]
    orc = tb.oracle_batch(N, M, ws.SEED0, ws.B, "hard")
    m = tb.assert_margin(orc, f"hard set {shape}")
    assert ws.recorded(m, want) and sum(o["rejected"] for o in orc) == rejected >= 1
    db = tb.device_batch(N, M, range(ws.SEED0, ws.SEED0 + ws.B), "hard")
    p, res = tb.run(db, tb.params("hard"))
    db.close()
    tb.compare(p, res, orc, f"hard set {shape}")


# ---------------------------------------------------------------- 3. lambda per problem
@pytest.mark.parametrize("shape", sorted(ws.ZERO_COLUMN))
def test_lambda_is_per_problem(shape):
    col, want = ws.ZERO_COLUMN[shape]
    p, res, orc = tb._zero_column_batch(tb.params("default"), B=ws.ZERO_B, chosen=ws.ZERO_CHOSEN, zero_col=col, shape=shape)
    assert ws.recorded(min(o["margin"] for o in orc), want)
    for b in range(len(orc)):
        assert orc[b]["lambda_"] == (1e-10 if b in ws.ZERO_CHOSEN else 0.0)
    # (1e-9: the tolerance of tests/test_dense_batch_gpu.py::test_lambda_is_per_problem, for the singular problems)
    tb.compare(p, res, orc, f"zero column {col} of {shape}", p_tol=1e-9)


# ---------------------------------------------------------------- 4. under-determined batches
@pytest.mark.parametrize("shape", sorted(ws.UNDER))
def test_underdetermined_batches(shape):
    """M < N: every problem's first factorisation fails and lambda goes to 1e-10; p to 1e-3 and the decisions exactly, as
    tests/test_dense_batch_shapes_gpu.py::test_underdetermined_batches"""
    N, M = shape
    orc = ws.under_oracle(shape)
    m = min(o["margin"] for o in orc)
    assert m > ws.UNDER_MARGIN_FLOOR and ws.recorded(m, ws.UNDER[shape])
    db = tb.device_batch(N, M, range(1, 1 + ws.UNDER_B), "default")
    p, res = tb.run(db, tb.params("default", **dict(ws.UNDER_OVER)))
    db.close()
    dp = max(float(np.max(np.abs(p[b] - o["p"]))) for b, o in enumerate(orc))
    print(f"{shape}: margin {m:.3g}, max |p - p_oracle| {dp:.3g}, iterations {sorted(set(res['iterations'].tolist()))}")
    for b, o in enumerate(orc):
        got = (int(res["iterations"][b]), int(res["evaluations"][b]), int(res["status"][b]), float(res["lambda_"][b]))
        assert got == (o["iterations"], o["evaluations"], o["status"], o["lambda_"]), f"problem {b}: {got}"
        assert o["lambda_"] == 1e-10
    assert dp <= ws.UNDER_P_TOL


# ---------------------------------------------------------------- 5. neighbours and order, bit for bit
@pytest.mark.parametrize("shape", ws.NEIGHBOUR_SHAPES)
def test_order_and_neighbours_do_not_matter_to_the_solve(shape):
    N, M = shape
    B = ws.NEIGHBOUR_B
    seeds = np.arange(1, 1 + B)
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res = tb.run(db, tb.params("diverse"))
    db.close()
    perm = np.random.default_rng(5).permutation(B)
    db = tb.device_batch(N, M, seeds[perm], "diverse")
    pp, resp = tb.run(db, tb.params("diverse"))
    db.close()
    assert pp.tobytes() == p[perm].tobytes() and tb.bitwise_equal(resp, res[perm])
    for b in ws.NEIGHBOUR_ALONE:
        db = tb.device_batch(N, M, seeds[b:b + 1], "diverse")
        p1, res1 = tb.run(db, tb.params("diverse"))
        db.close()
        assert p1.tobytes() == p[b:b + 1].tobytes() and tb.bitwise_equal(res1, res[b:b + 1]), b


@pytest.mark.parametrize("shape", ws.NEIGHBOUR_SHAPES)
def test_order_and_neighbours_do_not_matter_to_the_uncertainty(shape):
    N, M = shape
    B = ws.NEIGHBOUR_B
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
    for b in ws.NEIGHBOUR_ALONE:
        db = tu.device_batch(N, M, seeds[b:b + 1])
        for fs in (1, 2):
            assert tu.same_bits(base[fs], tu.unc(db, p[b:b + 1], lam[b:b + 1], fs=fs), idx_a=slice(b, b + 1)), (b, fs)
        db.close()


# ---------------------------------------------------------------- 6. the uncertainty call
@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("shape", ws.UNC_CASES)
def test_parity_of_the_uncertainty(shape, fs):
    N, M = shape
    seeds = np.arange(ws.SEED0, ws.SEED0 + ws.B)
    db, p, lam = tu.solved(N, M, seeds)
    out = tu.unc(db, p, lam, fs=fs)
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK) and np.array_equal(out["lam"], lam) and np.all(lam == 0.0)
    # with an odd M and fs = 2 the last measurement belongs to no feature
    assert out["factors"].shape == (ws.B, M // fs)
    assert out["var"].tobytes() == np.ascontiguousarray(np.einsum("bii->bi", out["cov"])).tobytes()
    print(f"<{ws.size_class(N)}>, T {ws.T(N)}, T2 {ws.T2(N, fs)}, {M // fs} features")
    nmax = tu.check_against_reference(out, N, M, seeds, p, lam, fs, f"{shape} fs {fs}")
    assert nmax == 0


def test_lambda_loop_of_the_uncertainty_on_a_zero_column():
    N, M = ws.UNC_ZERO_SHAPE
    tu.check_lambda_loop_on_a_zero_column(N, M, ws.UNC_ZERO_COLUMN, B=ws.ZERO_B, chosen=ws.ZERO_CHOSEN)


def test_a_failing_problem_of_64_variables_gets_nan_and_fails_alone():
    from problems.batch import MODE_NAN
    (N, M), B, bad = ws.UNC_NAN_SHAPE, ws.UNC_NAN_B, list(ws.UNC_NAN_BAD)
    db, p, lam = tu.solved(N, M, np.arange(1, 1 + B))
    plain = tu.unc(db, p, lam, fs=2)
    mode = np.zeros(B, dtype=np.uint8)
    mode[bad] = MODE_NAN
    db.set_mode(mode)
    out = tu.unc(db, p, lam, fs=2)
    db.close()
    good = [b for b in range(B) if b not in bad]
    assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
    for k in ("cov", "var", "factors"):
        assert np.all(np.isnan(out[k][bad])), k
    assert tu.same_bits(plain, out, idx_a=good, idx_b=good)


# ---------------------------------------------------------------- 7. the products form
@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("N", sorted(ws.RAGGED))
def test_products_parity_over_a_ragged_batch(N, setname):
    (Mmin, Mmax), want = ws.RAGGED[N]
    orc = ws.ragged_oracle(N, setname)
    po.assert_margin(orc, f"ragged N {N} {setname}", want[setname])
    tp.parity(N, po.ragged_M(ws.B, Mmin, Mmax), ws.B, orc, setname, f"ragged N {N} {setname}")


@pytest.mark.parametrize("shape", ws.PRODUCTS_SHAPES)
def test_products_layouts_give_the_same_bits(shape):
    """packed upper, unpacked, and unpacked with the strict lower triangle NaN: only the entries [i][j], j >= i, are read"""
    from problems.batch import LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER
    N, M = shape
    got = {}
    for layout in (LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        db = tp.device_batch(N, np.full(ws.B, M), range(1, 1 + ws.B), "diverse", layout)
        got[layout] = tp.run(db, po.params("diverse"))
        db.close()
    p, res = got[LAYOUT_PACKED_UPPER]
    assert np.all(res["status"] != BATCH_FAILED)
    for layout in (LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        assert got[layout][0].tobytes() == p.tobytes() and tp.bitwise_equal(got[layout][1], res), layout


@pytest.mark.parametrize("shape", ws.PRODUCTS_SHAPES)
def test_products_against_the_j_form(shape):
    """the same 33 problems through both forms, as tests/test_dense_products_batch_gpu.py::test_against_the_j_form: the
    decisions equal, p to 1e-10; and both against the J-form oracle, whose margin stands over the floor"""
    N, M = shape
    orc = tb.oracle_batch(N, M, ws.SEED0, ws.B, "diverse")
    tb.assert_margin(orc, f"{shape} diverse")
    db = tp.device_batch(N, np.full(ws.B, M), range(1, 1 + ws.B), "diverse")
    p, res = tp.run(db, po.params("diverse"))
    db.close()
    dj = tb.device_batch(N, M, range(1, 1 + ws.B), "diverse")
    pj, resj = tb.run(dj, tb.params("diverse"))
    dj.close()
    for f in ("iterations", "evaluations", "status", "lambda_"):
        assert np.array_equal(res[f], resj[f]), f
    d = float(np.max(np.abs(p - pj)))
    print(f"{shape}: products form against the J form: max |dp| {d:.3g}")
    assert d <= STEP_TOL
    tb.compare(p, res, orc, f"{shape} products form against the J-form oracle")


@pytest.mark.parametrize("N", sorted(ws.RAGGED))
def test_products_uncertainty(N):
    """Sigma and the variances of a ragged products batch against the host reference on each problem's own rows, in the
    three layouts, and against the J form's call where the problems have equal M"""
    from problems.batch import LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER
    B = ws.B
    seeds, Ms = np.arange(1, 1 + B), po.ragged_M(B, *ws.RAGGED[N][0])
    db, p, lam = tpu.solved(N, Ms, seeds)
    db.reset_counters()
    out = tpu.unc(db, p, lam)
    assert db.ncalls() == 1 and db.nevals() == B
    assert np.all(out["status"] == BATCH_UNC_OK) and np.array_equal(out["lam"], lam) and np.all(lam == 0.0)
    ecov, evar = tpu.errors(out, N, Ms, seeds, p, lam)
    print(f"ragged N {N}: {B} problems: Sigma scaled error {ecov:.3g}, variances rel {evar:.3g}")
    assert ecov <= tu.COV_TOL and evar <= tu.VAR_TOL
    assert out["var"].tobytes() == np.ascontiguousarray(np.einsum("bii->bi", out["cov"])).tobytes()
    for layout in (LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        db.set_layout(layout)
        assert tpu.same_bits(out, tpu.unc(db, p, lam)), layout
    db.close()
    # equal M: the J form's Sigma at the same points, to the tolerance each has against the host
    M = [m for n, m in ws.PRODUCTS_SHAPES if n == N][0]
    dj, pj, lamj = tu.solved(N, M, seeds)
    outj = tu.unc(dj, pj, lamj, want=("cov", "var"))
    dj.close()
    dbp = tpu.device_batch(N, np.full(B, M), seeds)
    outp = tpu.unc(dbp, pj, lamj)
    dbp.close()
    assert np.all(outp["status"] == BATCH_UNC_OK)
    d = np.sqrt(outj["var"])
    e = float(np.max(np.abs(outp["cov"] - outj["cov"]) / (d[:, :, None] * d[:, None, :])))
    print(f"({N}, {M}): products form against the J form: Sigma scaled {e:.3g}")
    assert e <= 2 * tu.COV_TOL


# ---------------------------------------------------------------- 8. the Jacobian check of a batch callback
def test_jacobian_check_of_a_batch_at_64_variables():
    """tests/test_jacobian_check_gpu.py::test_batch at (64, 70): delta 1e-6, atol 1e-7, a factor of 1.01 on one entry"""
    DELTA, ATOL, FACTOR, eps = 1e-6, 1e-7, 1.01, 0.3
    (N, M), B = ws.GRADCHECK_SHAPE, ws.GRADCHECK_B
    rng = np.random.default_rng(164)
    coef = rng.uniform(0.1, 1.0, (B, M, N)) * rng.choice([-1.0, 1.0], (B, M, N))
    pstar = rng.uniform(-1.0, 1.0, (B, N))
    p0 = pstar + 0.3 * rng.uniform(-1.0, 1.0, (B, N))
    model = gp.BatchModel(coef, pstar, eps)
    out = capi.check_jacobian_device_batch(p0, N, M, model.cb, model.cookie, delta=DELTA, atol=ATOL)
    assert out["rc"] == 0 and not out["bad"]
    assert model.ncalls() == 2 * N and model.notlive() == 0
    for rep in out["reports"]:
        assert (rep["nbad"], rep["noutside"], rep["nnonfinite"]) == (0, 0, 0), rep
        assert rep["nchecked"] == M * N and rep["ncolours"] == N and rep["evaluations"] == 2 * N, rep
        assert 0.0 < rep["max_error"] <= ATOL, rep
    honest = out["reports"]
    bs, r, v = ws.GRADCHECK_FAULT
    model.set_fault(bs, r, v, FACTOR)
    out = capi.check_jacobian_device_batch(p0, N, M, model.cb, model.cookie, delta=DELTA, atol=ATOL)
    model.close()
    assert out["rc"] == 0 and len(out["bad"]) == 1
    assert all(out["reports"][b] == honest[b] for b in range(B) if b != bs)
    rep = out["reports"][bs]
    assert rep["nbad"] == 1 and rep["nnonfinite"] == 0 and (rep["worst_var"], rep["worst_meas"]) == (v, r)
    problem, bvar, bmeas, reported, observed = out["bad"][0]
    assert (problem, bvar, bmeas) == (bs, v, r)
    u = np.sum(coef[bs, r] * (p0[bs] - pstar[bs]))
    want = (FACTOR - 1.0) * coef[bs, r, v] * (1.0 + eps * np.cos(u))
    assert abs(want) >= 6e-4 and abs((reported - observed) - want) <= 1e-7


# ---------------------------------------------------------------- 9. 65 variables are refused
def test_65_variables_are_refused_by_all_five_entry_points():
    N, M, B = ws.REFUSED_NSTATE, 140, 2
    L = capi.lib()
    dj = tb.device_batch(64, M, range(1, 1 + B), "default")           # callbacks that must never be called
    dpr = tp.device_batch(64, np.full(B, M), range(1, 1 + B), "default")
    mark = np.arange(B * N, dtype=np.float64).reshape(B, N) + 0.5
    p = mark.copy()
    res = (BatchResult * B)()
    assert L.dogleg_amd_optimize_dense_batch(dptr(p), B, N, M, dj.cb, dj.cookie, None, res) == -1
    prm = po.params("default")
    rc, pp, _ = capi.optimize_dense_products_batch(p, N, dpr.cb, dpr.cookie, prm)
    assert rc == -1 and np.array_equal(pp, mark)
    out = capi.dense_batch_uncertainty(p, N, M, dj.cb, dj.cookie, lam=np.zeros(B))
    assert out["rc"] == -1 and not out["cov"].any() and not out["var"].any() and not out["factors"].any()
    out = capi.dense_products_batch_uncertainty(p, N, dpr.cb, dpr.cookie, prm, lam=np.zeros(B))
    assert out["rc"] == -1 and not out["cov"].any() and not out["var"].any()
    out = capi.check_jacobian_device_batch(p, N, M, dj.cb, dj.cookie, delta=1e-6, atol=1e-7)
    assert out["rc"] == -1
    assert np.array_equal(p, mark) and dj.ncalls() == 0 and dpr.ncalls() == 0
    # and 64 is taken by the same objects
    rc, p64, r64 = capi.optimize_dense_batch(dj.p0(), 64, M, dj.cb, dj.cookie, tb.params("default"))
    assert rc == 0 and np.all(r64["status"] > 0) and np.all(r64["status"] != BATCH_FAILED)
    dj.close()
    dpr.close()
