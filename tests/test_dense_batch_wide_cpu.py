"""What tests/test_dense_batch_wide_gpu.py presupposes, asserted without a GPU: the limit of 64 variables in the header and
in ctypes, that the case table of tests/dense_batch_wide_shapes.py reaches both new size classes, their dispatch edges and
both kinds of last tile, every recorded decision margin and rejected-trial count (the CPU oracles alone), and that the host
reference of the uncertainty call is three decades more exact than the tolerances it is used with."""
import os
import re

import pytest

from libdogleg_amd import ctypes_defs
from libdogleg_amd.ctypes_defs import BATCH_JTX, BATCH_SMALL_STEP
from tests import dense_batch_shapes as ds
from tests import dense_batch_wide_shapes as ws
from tests import batch_products_oracle as po
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the limit
def test_the_limit_is_64_in_the_header_and_in_ctypes():
    text = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    m = re.search(r"^#define\s+DOGLEG_AMD_BATCH_MAX_NSTATE\s+(\d+)\s*$", text, re.M)
    assert m and int(m.group(1)) == 64
    assert ctypes_defs.BATCH_MAX_NSTATE == 64 and ws.REFUSED_NSTATE == 65


# ---------------------------------------------------------------- 2. the table covers what it is there for
def test_the_tiling_restated():
    Ns = (33, 40, 48, 49, 63, 64)
    assert [ws.size_class(N) for N in (32,) + Ns] == [32, 48, 48, 48, 64, 64, 64]
    assert [ws.problems_per_workgroup(N) for N in (32,) + Ns] == [4, 2, 2, 2, 1, 1, 1]
    assert [ws.T(N) for N in Ns] == [7, 6, 5, 5, 4, 4]
    assert [ws.T2(N, 1) for N in Ns] == [35, 28, 24, 42, 33, 32]
    assert [ws.T2(N, 2) for N in Ns] == [34, 28, 24, 42, 32, 32]
    # the second sweep's tile, T2 rows at stride N | 1, fits the region the factor lay in: NP(NMAX) doubles
    for N in range(33, 65):
        for fs in (1, 2):
            assert ws.T2(N, fs) >= 24 and ws.T2(N, fs) * (N | 1) <= ds.n_packed(ws.size_class(N))
    # a wavefront's LDS in the J form, NP + max(NP, 320) + NMAX doubles, and four workgroups of a class in a CU's 160 KB
    for nmax, want in ((48, 19200), (64, 33792)):
        lds = 8 * (2 * ds.n_packed(nmax) + nmax)
        assert lds == want and 4 * (ws.problems_per_workgroup(nmax) * lds + 8) <= 160 * 1024


def test_the_tables_cover_both_classes_and_every_edge():
    cases = list(ws.CASES)
    Ns = {N for N, _ in cases}
    assert {33, 48, 49, 63, 64} <= Ns and {ws.size_class(N) for N in Ns} == {48, 64}
    for cls in (48, 64):
        mine = [(N, M) for N, M in cases if ws.size_class(N) == cls]
        assert any(M % ws.T(N) == 0 for N, M in mine) and any(M % ws.T(N) != 0 for N, M in mine)
        assert any(M % 2 == 1 for N, M in mine)
    assert ws.UNC_CASES == sorted(cases) and all(M > N + 1 for N, M in cases)
    # the second sweep: several tiles with a ragged last one in both classes and for both feature sizes, and a tile that
    # the rounding to an even number of rows changed
    for fs in (1, 2):
        for cls in (48, 64):
            assert any((M // fs) * fs > 2 * ws.T2(N, fs) and 0 < ((M // fs) * fs) % ws.T2(N, fs)
                       for N, M in cases if ws.size_class(N) == cls)
    assert any(ws.T2(N, 2) < ws.T2(N, 1) for N, _ in cases)
    for table in (ws.RETRY, ws.ZERO_COLUMN, ws.UNDER, dict.fromkeys(ws.NEIGHBOUR_SHAPES), dict.fromkeys(ws.PRODUCTS_SHAPES)):
        assert {ws.size_class(N) for N, _ in table} == {48, 64}
    assert {ws.size_class(N) for N in ws.RAGGED} == {48, 64} and set(ws.RAGGED) == {33, 48, 64}
    assert all((Mmin, Mmax) == (N + 7, 2 * N + 12) for N, ((Mmin, Mmax), _) in ws.RAGGED.items())
    assert all(col == N - 1 for (N, _), (col, _) in ws.ZERO_COLUMN.items()) and all(M < N for N, M in ws.UNDER)
    assert ws.B == 33 and ws.SEED0 == 1 and ws.NEIGHBOUR_B == 65 and max(ws.NEIGHBOUR_ALONE) == ws.NEIGHBOUR_B - 1
    assert ws.size_class(ws.UNC_ZERO_SHAPE[0]) == 48 and ws.UNC_NAN_SHAPE[0] == 64 and ws.GRADCHECK_SHAPE == (64, 70)
    assert ws.GRADCHECK_FAULT[0] == 2 and ws.GRADCHECK_FAULT[2] == 63 and ws.GRADCHECK_B == 3


# ---------------------------------------------------------------- 3. the margins
@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(ws.CASES))
def test_margins_and_step_types(shape, setname):
    N, M = shape
    orc = tb.oracle_batch(N, M, ws.SEED0, ws.B, setname)
    m = tb.assert_margin(orc, f"{shape} {setname} seed0 {ws.SEED0}")
    assert ws.recorded(m, ws.CASES[shape][setname]), "the generator changed: record the margin again"
    if setname == "diverse":
        assert set().union(*[o["step_types"] for o in orc]) == {0, 1, 2}
    assert {o["status"] for o in orc} <= {BATCH_JTX, BATCH_SMALL_STEP} and all(o["lambda_"] == 0.0 for o in orc)


@pytest.mark.parametrize("shape", sorted({**ws.RETRY, **ws.RETRY_CPU_ONLY}))
def test_rejected_trials_are_there(shape):
    want, rejected = {**ws.RETRY, **ws.RETRY_CPU_ONLY}[shape]
    orc = tb.oracle_batch(*shape, ws.SEED0, ws.B, "hard")
    m = tb.assert_margin(orc, f"hard set {shape}")
    assert ws.recorded(m, want)
    assert sum(o["rejected"] for o in orc) == rejected >= 1


def test_the_default_set_at_64_by_200_stays_out():
    # its margin is negative: should this start to pass, (64, 200) may join the table
    m = min(o["margin"] for o in tb.oracle_batch(64, 200, ws.SEED0, ws.B, "default"))
    assert m < 0.0 and (64, 200) not in ws.CASES


@pytest.mark.parametrize("shape", sorted(ws.ZERO_COLUMN))
def test_zero_column_problems_end_with_a_lambda(shape):
    orc = ws.zero_oracle(shape)
    m = tb.assert_margin(orc, f"zero-column batch {shape}")
    assert ws.recorded(m, ws.ZERO_COLUMN[shape][1])
    assert [o["lambda_"] for o in orc] == [1e-10 if b in ws.ZERO_CHOSEN else 0.0 for b in range(ws.ZERO_B)]


@pytest.mark.parametrize("shape", sorted(ws.UNDER))
def test_underdetermined_batches_start_in_the_lambda_loop(shape):
    orc = ws.under_oracle(shape)
    m = min(o["margin"] for o in orc)
    print(f"{shape}: margin {m:.3g}")
    assert m > ws.UNDER_MARGIN_FLOOR >= 10 * ws.UNDER_P_TOL and ws.recorded(m, ws.UNDER[shape])
    assert all(o["lambda_"] == 1e-10 and o["status"] == BATCH_JTX and 2 <= o["iterations"] <= 3 for o in orc)
    assert all(o["evaluations"] == o["iterations"] + 1 for o in orc)


@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("N", sorted(ws.RAGGED))
def test_margins_of_the_ragged_products_batches(N, setname):
    orc = ws.ragged_oracle(N, setname)
    po.assert_margin(orc, f"ragged N {N} {setname}", ws.RAGGED[N][1][setname])
    assert all(o["lambda_"] == 0.0 for o in orc)


@pytest.mark.parametrize("shape", ws.PRODUCTS_SHAPES)
def test_the_products_oracle_decides_as_the_j_form_oracle(shape):
    # what test_products_against_the_j_form leans on: on equal M the two oracles take the same decisions
    N, M = shape
    oj, op = tb.oracle_batch(N, M, ws.SEED0, ws.B, "diverse"), po.oracle_batch(N, M, ws.SEED0, ws.B, "diverse")
    po.assert_margin(op, f"{shape} diverse, products oracle", ws.CASES[shape]["diverse"])
    for a, b in zip(oj, op):
        assert all(a[k] == b[k] for k in ("iterations", "evaluations", "status", "lambda_"))


# ---------------------------------------------------------------- 4. the host reference of the uncertainty call
@pytest.mark.parametrize("shape", ws.UNC_CASES)
def test_two_host_computations_agree_three_decades_under_the_tolerances(shape):
    a = ws.host_agreement(shape)
    print(f"{shape}: Sigma {a['sigma']:.3g}, factors {a['factors']:.3g}, cond(JtJ) {a['cond']:.4g}, largest leverage "
          f"{a['leverage']:.3g}, min |det(A_f - I)| {a['mindet']:.3g}")
    assert a["sigma"] <= 1e-3 * min(tu.COV_TOL, tu.VAR_TOL) and a["factors"] <= 1e-3 * tu.FAC_RTOL
    assert a["n_dbl_max"] == 0 and a["mindet"] > 1e-8 and a["lambda_max"] == 0.0
    assert a["cond"] <= 50 and a["leverage"] <= 0.85            # (measured: 41.9 and 0.81)
