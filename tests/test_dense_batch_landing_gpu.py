"""The fallback's landing in the bounded batch kernels (step 6: the component that sets alpha ends ON its bound), every BOUNDED
form of k_batch_round against the oracle that states the rule (tests/batch_bounds_oracle.fallback_step).  The cases and why the
linear family's landing is the same on every implementation: tests/batch_landing_cases.py; what the rule changes, with the oracle
alone: tests/test_dense_batch_landing_cpu.py.

The linear family, 16 upper bounds (9 "short", 4 "on", 3 "beyond" under the plain sum), the J form, the J form with a loss
(Huber at a scale that leaves every weight 1), the products form packed and unpacked, host and device twins, in every size class
with the pair in the first and in the last two variables: status, iterations, evaluations, lambda and held equal to the oracle,
|p - p_oracle| <= STEP_TOL = 1e-10, F and the trust region to REL_SCALAR_TOL = 1e-8, p[:, pair + 1] == u bit for bit and p
within KKT_TOL = 1e-9 of the exact bounded solution.  The model and the Poisson form: a batch of 65 with cut landings each, at
the tolerances of tests/test_dense_batch_model_gpu.py and tests/test_dense_batch_poisson_gpu.py.

MEASURED on an MI355X against the kernel before the rule (step 6 as s = alpha d, clipped): 52 of the 56 tests here fail and 4
pass.  In every one of the 52 tests of the linear family (13 placements x J form, J form with Huber, products packed, products
unpacked) exactly the 9 "short" problems differ from the oracle -- status SMALL_STEP after 1 iteration and 2 evaluations, p one
ulp below the bound, 0.06 from the exact bounded solution -- and the 7 "on" and "beyond" problems agree: the GPU's arithmetic
is what tests/batch_landing_cases.py assumes, the prediction made on the CPU holds problem for problem.  The 4 model and
Poisson tests pass on that kernel too: their 55 cut landings start from points of the size of the bound, where the plain sum
lands on the bound's bits (all 55 are "on" in the oracle), so they check the rule's text in those two forms, not the defect."""
import numpy as np
import pytest

from libdogleg_amd.ctypes_defs import BATCH_JTX, BatchLoss, LOSS_HUBER, LOSS_TRIVIAL
from problems.batch import LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED
from problems.batch_linear import LinearDeviceBatch, LinearHostProblem
from problems.batch_linear_products import LinearProductsBatch
from tests import batch_bounds_oracle as bb
from tests import batch_landing_cases as lc
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_bounds_gpu as tbd
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_model_gpu as tm
from tests import test_dense_batch_poisson_gpu as tp
from tests import test_dense_products_batch_bounds_gpu as tpb
from tests.parity import STEP_TOL

pytestmark = pytest.mark.gpu

REL_TOL = tb.REL_SCALAR_TOL
HUBER_SCALE = 1024.0             # every residual of the family is below 1: every weight is 1 and the products are the plain ones
CASES = [(N, at) for N in lc.SIZES for at in lc.placements(N)]
U = np.array([u for u, _ in lc.LANDING_U])


def check(p, res, held, w, N, at, orc, what):
    """the oracle, the bound's bits and the exact bounded solution; the figures first"""
    A, y, p0, lo, hi = lc.linear_batch(N, at)
    off = [b for b in range(len(U)) if p[b, at + 1] != U[b]]
    kkt = max(float(np.max(np.abs(p[b] - lc.exact_embedded(N, at, U[b])))) for b in range(len(U)))
    wrong = [(c, int(res["status"][b]), int(res["iterations"][b])) for b, (_, c) in enumerate(lc.LANDING_U)
             if (int(res["status"][b]), int(res["iterations"][b])) != (orc[b]["status"], orc[b]["iterations"])]
    print(f"{what}: problems whose p is not on the bound's bits {off}, worst |p - exact| {kkt:.3g}, (class, status, iterations) "
          f"where they are not the oracle's: {wrong}")
    tbd.compare(p, res, held, w, orc, what)
    assert not off and kkt <= lc.KKT_TOL
    assert np.all(res["status"] == BATCH_JTX) and np.all(held[:, at + 1] == bb.AT_UPPER) and int(held.sum()) == 2 * len(U)


# ---------------------------------------------------------------- 1. the J form, with and without a loss, both twins
@pytest.mark.parametrize("case", CASES, ids=str)
def test_j_form(case):
    N, at = case
    A, y, p0, lo, hi = lc.linear_batch(N, at)
    orc = lc.linear_oracle(N, at)
    assert min(o["margin"] for o in orc) > lc.MARGIN_FLOOR
    db = LinearDeviceBatch(A, y, p0)
    prm = lc.params()
    p, res, held, w = tbd.run(db, prm, lo, hi)
    assert w is None
    check(p, res, held, None, N, at, orc, f"J form, N = {N}, the pair at {at}")
    pd, rd, ld, hd, _, _ = tbd.solve_dev(db, prm, lo, hi)
    assert pd.tobytes() == p.tobytes() and tb.bitwise_equal(rd, res) and hd.tobytes() == held.tobytes()
    assert ld.tobytes() == np.ascontiguousarray(res["lambda_"]).tobytes()
    db.close()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_j_form_with_a_loss(case):
    N, at = case
    A, y, p0, lo, hi = lc.linear_batch(N, at)
    loss = ro.Loss(LOSS_HUBER, HUBER_SCALE, 1)
    orc = [bb.solve_one(LinearHostProblem(A[b], y[b], p0[b]), lc.params(), loss, lo[b], hi[b]) for b in range(len(U))]
    plain = lc.linear_oracle(N, at)
    for o, o2 in zip(orc, plain):
        assert np.all(o["weights"] == 1.0) and o["p"].tobytes() == o2["p"].tobytes() and o["landings"] == o2["landings"]
    assert min(o["margin"] for o in orc) > lc.MARGIN_FLOOR
    db = LinearDeviceBatch(A, y, p0)
    prm = lc.params()
    dl = BatchLoss(LOSS_HUBER, HUBER_SCALE, 1)
    p, res, held, w = tbd.run(db, prm, lo, hi, dl)
    assert np.all(w == 1.0)
    check(p, res, held, w, N, at, orc, f"J form with Huber, N = {N}, the pair at {at}")
    pd, rd, ld, hd, wd, _ = tbd.solve_dev(db, prm, lo, hi, dl)
    assert pd.tobytes() == p.tobytes() and tb.bitwise_equal(rd, res) and hd.tobytes() == held.tobytes() and wd.tobytes() == w.tobytes()
    db.close()


# ---------------------------------------------------------------- 2. the products form, packed and unpacked, both twins
@pytest.mark.parametrize("layout", [LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED], ids=["packed", "unpacked"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_products_form(case, layout):
    N, at = case
    A, y, p0, lo, hi = lc.linear_batch(N, at)
    orc = lc.linear_oracle(N, at)
    db = LinearProductsBatch(list(A), list(y), p0, layout=layout)
    prm = lc.params()
    p, res, held = tpb.run(db, prm, lo, hi)
    check(p, res, held, None, N, at, orc, f"products form, layout {layout}, N = {N}, the pair at {at}")
    pd, rd, ld, hd, _ = tpb.solve_dev(db, prm, lo, hi)
    assert pd.tobytes() == p.tobytes() and tb.bitwise_equal(rd, res) and hd.tobytes() == held.tobytes()
    assert ld.tobytes() == np.ascontiguousarray(res["lambda_"]).tobytes()
    db.close()


# ---------------------------------------------------------------- 3. the model form and the Poisson form
def compare_fit(p, res, held, orc, what, relative):
    nb = len(orc)
    den = (lambda o: np.maximum(1.0, np.abs(o["p"]))) if relative else (lambda o: 1.0)
    dp = max(float(np.max(np.abs(p[b] - orc[b]["p"]) / den(orc[b]))) for b in range(nb))
    dn = max(abs(res["norm2_x"][b] - orc[b]["norm2_x"]) / max(abs(orc[b]["norm2_x"]), 1e-300) for b in range(nb))
    dt = max(abs(res["trustregion"][b] - orc[b]["trustregion"]) / abs(orc[b]["trustregion"]) for b in range(nb))
    bad = [b for b in range(nb) if (int(res["status"][b]), int(res["iterations"][b]), int(res["evaluations"][b]),
                                    float(res["lambda_"][b])) != (orc[b]["status"], orc[b]["iterations"], orc[b]["evaluations"],
                                                                  orc[b]["lambda_"]) or held[b].tolist() != orc[b]["held"].tolist()]
    print(f"{what}: max |p - p_oracle| {dp:.3g}, F rel {dn:.3g}, trust region rel {dt:.3g}; problems whose status, counts, lambda "
          f"or held are not the oracle's: {bad} (problems with a cut landing: {[b for b in range(nb) if orc[b]['landings']]})")
    assert not bad
    assert dp <= STEP_TOL and dn <= REL_TOL and dt <= REL_TOL
    for b in range(nb):
        on = orc[b]["held"] != bb.FREE
        assert p[b][on].tobytes() == orc[b]["p"][on].tobytes(), (b, "a held variable is not on its bound's bits")


@pytest.mark.parametrize("case", lc.FIT_CASES, ids=mz.case_id)
def test_model_form(case):
    orc = lc.fit_oracle("model", case)
    assert sum(len(o["landings"]) for o in orc) >= lc.MIN_LANDINGS and min(o["margin"] for o in orc) > lc.MARGIN_FLOOR
    bt = lc.fit_batch("model", case)
    dm = tm.DevModel(bt)
    p, res, held = tm.fused(dm, bt["p0"], bt["lo"], bt["hi"], True)
    compare_fit(p, res, held, orc, f"model form, {mz.case_id(case)}", relative=False)
    d = tm.device_route(dm, bt["p0"], bt["lo"], bt["hi"], True, None, True)
    tm.same_bits((p, res, held), (d[0], d[1], d[3]), "the device twin")


@pytest.mark.parametrize("case", lc.FIT_CASES, ids=mz.case_id)
def test_poisson_form(case):
    orc = lc.fit_oracle("poisson", case)
    assert sum(len(o["landings"]) for o in orc) >= lc.MIN_LANDINGS and min(o["margin"] for o in orc) > lc.MARGIN_FLOOR
    assert max(o["cost_error"] for o in orc) <= po.COST_TOL
    bt = lc.fit_batch("poisson", case)
    dm = tm.DevModel(bt)
    p, res, held = tp.mle(dm, bt["p0"], bt["lo"], bt["hi"], True)
    compare_fit(p, res, held, orc, f"Poisson form, {mz.case_id(case)}", relative=True)
    d = tp.mle_device(dm, bt["p0"], bt["lo"], bt["hi"], True)
    tm.same_bits((p, res, held), d[:3], "the device twin")
