"""Branches of the host driver (driver.hip: eval_point, take_step, run_optimizer; driver_comm.cpp: attach_communicator)
that no other test of the suite walks, each as a whole solve against the oracle's trace (profiles/driver_refactor.md has the
table of branches and the tests that execute them)."""
import ctypes as C
import numpy as np
import pytest

from libdogleg_amd import capi
from tests import oracle_api as oa
from tests.parity import compare_traces
from tests.test_shard_gpu import _multi_rank_solve, _check_ranks_against_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["device sparse", "device dense", "host"])
def test_terminal_step_carries_its_expected_improvement(gpu, kind):
    """A device-callback solve keeps the expected improvement of a step on its way until the trial point is evaluated
    (dlg_backend_set_defer_tail).  A step that ends the solve on update_threshold (dogleg.c:1289-1296) has no evaluation
    behind it: take_step fetches the value itself (fetch_deferred_improvement), and the terminal record carries it --
    the oracle's number, not the NaN the step returned in its place.  host: the same end with nothing deferred."""
    sparse = kind != "device dense"
    prob = oa.BAProblem(4, 20, 60, seed=2, eps=0.4, p0_spread=0.8) if sparse else oa.DenseProblem(M=60, N=6, seed=3)
    nnz = prob.nnz if sparse else 0
    prm = oa.default_params()
    prm.max_iterations = 40
    prm.trustregion0 = 3.0
    prm.update_threshold = 1e-3
    prm.Jt_x_threshold = 1e-300
    p0 = prob.p0()
    ro, po, tro = oa.oracle_solve("sparse" if sparse else "dense", p0, prob.N, prob.M, nnz, prob.cb, prob.cookie, prm)
    if kind == "host":
        rg, pg, trg = capi.optimize("sparse", p0, prob.N, prob.M, nnz, prob.cb, prob.cookie, prm)
    else:
        twin = oa.DeviceTwin(prob)
        Jp, Ji = prob.pattern() if sparse else (None, None)
        rg, pg, trg = capi.optimize_device(p0, prob.N, prob.M, nnz, Jp, Ji, twin.cb, twin.cookie, prm)
    assert rg >= 0
    compare_traces(trg, tro)
    last = trg.trials()[-1]
    assert last["accepted"] == 2, "the solve must end on the step that is not applied"
    assert last["step_type"] != 0, "the terminal step must be one that needed the Gauss-Newton step (the fused path defers)"
    assert np.isfinite(last["expected_improvement"]) and last["expected_improvement"] >= 0.0
    assert np.max(np.abs(pg - po)) <= 1e-10


def test_host_solves_in_a_row_of_one_shape_same_and_another_pattern(gpu):
    """Host-callback solves of one (N, M, nnz) in a row: pattern A, A again (the parked backend is taken over as it is:
    set_pattern finds its own pattern), then B (one camera less, two points more: replace_pattern drops and analyses) -- each the oracle's trace."""
    probs = [oa.BAProblem(4, 20, 60, seed=2, eps=0.4, p0_spread=0.8), oa.BAProblem(4, 20, 60, seed=2, eps=0.4, p0_spread=0.8),
             oa.BAProblem(3, 22, 60, seed=5, eps=0.4, p0_spread=0.8)]
    assert (probs[0].N, probs[0].M, probs[0].nnz) == (probs[2].N, probs[2].M, probs[2].nnz)
    assert not np.array_equal(probs[0].pattern()[1], probs[2].pattern()[1])
    prm = oa.default_params()
    prm.max_iterations = 8
    prm.trustregion0 = 3.0
    for k, prob in enumerate(probs):
        p0 = prob.p0()
        ro, po, tro = oa.oracle_solve("sparse", p0, prob.N, prob.M, prob.nnz, prob.cb, prob.cookie, prm)
        rg, pg, trg = capi.optimize("sparse", p0, prob.N, prob.M, prob.nnz, prob.cb, prob.cookie, prm)
        assert rg >= 0, k
        compare_traces(trg, tro)
        assert np.max(np.abs(pg - po)) <= 1e-10, k


def test_dense_device_callback_on_two_logical_ranks(gpu):
    """dogleg_optimize_device2, dense, as one rank of two: the callback writes ALL rows into the slot's buffers, the rank's
    rows are a contiguous slice of them (bind at row0; 61 rows: 30 and 31) -- the oracle's trace on every rank, the same
    bits on both."""
    dp = oa.DenseProblem(M=61, N=6, seed=3)
    prm = oa.default_params()
    prm.max_iterations = 8
    twin = oa.DeviceTwin(dp)
    try:
        res = _multi_rank_solve("dense", dp, 2, prm, twin=twin)
    finally:
        twin.close()
    _check_ranks_against_oracle("dense", dp, prm, res)


def test_a_step_redone_behind_the_between_callback_evaluates_its_point_again(gpu):
    """A device model whose every point but the start has two zero columns in J.  The first step needs the Gauss-Newton
    step at lambda = 0; the next one is dlg_take_step from a singular point: the factorisation fails, lambda is raised and
    the step made again -- behind the callback that ran from inside the first attempt (driver_between), for a trial point
    that has moved since.  eval_point must not take that evaluation (dlg_backend_between_redone): the model runs again.
    Against the oracle with the same model on the host."""
    dp = oa.DenseProblem(M=60, N=6, seed=3)
    twin = oa.DeviceTwin(dp)
    M, N, cols = dp.M, dp.N, (1, 4)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemset2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    DEV = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    inner_dev, inner_host = DEV(twin.cb.value), capi.CB_DENSE(dp.cb.value)
    calls = {"device": 0, "host": 0, "errors": 0}

    @DEV
    def cb_dev(p, x, J, stream, cookie):
        inner_dev(p, x, J, stream, cookie)
        calls["device"] += 1
        if calls["device"] > 1:                     # (on the callback's stream, behind the model's kernels: J is [M][N] row-major)
            for c in cols:
                calls["errors"] += hip.hipMemset2DAsync(J + 8 * c, 8 * N, 0, 8, M, stream) != 0

    @capi.CB_DENSE
    def cb_host(p, x, J, cookie):
        inner_host(p, x, J, cookie)
        calls["host"] += 1
        if calls["host"] > 1:
            Jv = np.ctypeslib.as_array(J, shape=(M, N))
            for c in cols:
                Jv[:, c] = 0.0

    prm = oa.default_params()
    prm.max_iterations = 4
    prm.trustregion0 = 1e3
    p0 = dp.p0()
    ro, po, tro = oa.oracle_solve("dense", p0, N, M, 0, C.cast(cb_host, C.c_void_p), dp.cookie, prm)
    rg, pg, trg = capi.optimize_device(p0, N, M, 0, None, None, C.cast(cb_dev, C.c_void_p), twin.cookie, prm)
    assert rg >= 0 and calls["errors"] == 0
    tg = trg.trials()
    print("lambda per trial", [t["lambda_"] for t in tg], "step types", [t["step_type"] for t in tg],
          "device evaluations", calls["device"], "callbacks", trg.ncallbacks)
    assert tg[0]["lambda_"] == 0.0 and tg[0]["step_type"] != 0 and tg[0]["accepted"] == 1, "the scenario: a GN step from a regular start, accepted"
    assert tg[1]["lambda_"] > 0.0, "the scenario: the second step starts from a singular point"
    compare_traces(trg, tro)
    assert np.max(np.abs(pg - po)) <= 1e-10
    # the model ran once more than the driver counts: the evaluation behind the first attempt was thrown away
    assert calls["device"] > trg.ncallbacks == tro.ncallbacks
