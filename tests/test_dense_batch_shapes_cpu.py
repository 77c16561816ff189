"""What tests/test_dense_batch_shapes_gpu.py presupposes, asserted with the CPU oracle alone (no GPU): that its case table
reaches every size class, dispatch edge and tile edge of dense_batch.hip, that every recorded decision margin still holds,
that the rejected trials, the lambda loops and the under-determined solves are where the table says, and that the host
reference of the uncertainty call is three decades more exact than the tolerances it is used with."""
import pytest

from tests import dense_batch_shapes as ds
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu
from libdogleg_amd.ctypes_defs import BATCH_JTX, BATCH_SMALL_STEP


# ---------------------------------------------------------------- 1. the table covers what it is there for
def test_the_tiling_restated():
    assert [ds.T(N) for N in (1, 2, 4, 5, 8, 9, 16, 17, 24, 25, 31, 32)] == [64, 64, 64, 51, 32, 28, 16, 15, 10, 10, 8, 8]
    assert [ds.T2(N, 1) for N in (1, 5, 8, 11, 16, 17, 24, 25, 31, 32)] == [64, 51, 32, 23, 16, 15, 10, 10, 8, 8]
    assert [ds.T2(N, 2) for N in (1, 5, 8, 11, 16, 17, 24, 25, 31, 32)] == [64, 50, 32, 22, 16, 14, 10, 10, 8, 8]
    assert [ds.size_class(N) for N in (1, 8, 9, 16, 17, 24, 25, 32)] == [8, 8, 16, 16, 24, 24, 32, 32]
    # the second sweep's tile, T2 rows at stride N | 1, fits the BATCH_TILE + 64 doubles the first sweep's tile has
    assert all(ds.T2(N, fs) >= fs and ds.T2(N, fs) * (N | 1) <= ds.BATCH_TILE + 64 for N in range(1, 33) for fs in (1, 2))


def test_the_solve_table_covers_every_class_and_edge():
    cases = list(ds.CASES)
    Ns = {N for N, _ in cases}
    assert {ds.size_class(N) for N in Ns} == {8, 16, 24, 32}
    assert {8, 9, 16, 17, 24, 25} <= Ns and {1, 2} <= Ns
    assert any(M < ds.T(N) for N, M in cases)
    assert any(M == ds.T(N) for N, M in cases)
    assert any(M == ds.T(N) and N < 16 for N, M in cases)
    assert any(M % ds.T(N) == 1 and M > ds.T(N) for N, M in cases)
    assert any(M > 2 * ds.T(N) and 1 < M % ds.T(N) < ds.T(N) for N, M in cases)
    # M = 1, and more entries of JtJ than lanes in every class above <8>
    assert (1, 1) in ds.ONE_BY_ONE
    assert {ds.size_class(N) for N, _ in cases if ds.n_packed(N) > 64} == {16, 24, 32}


def test_the_uncertainty_table_covers_every_class_and_edge():
    cases = ds.UNC_CASES
    Ns = {N for N, _ in cases}
    assert {ds.size_class(N) for N in Ns} == {8, 16, 24, 32}
    assert {8, 9, 16, 17, 24, 25} <= Ns and {1, 2} <= Ns
    assert all(M > N + 1 for N, M in cases)
    assert any(M % 2 == 1 for N, M in cases)
    assert any(ds.T2(N, 2) < ds.T2(N, 1) for N, M in cases)
    # a trailing odd measurement in every class, and one behind a tile that the rounding changed
    assert {ds.size_class(N) for N, M in cases if M % 2 == 1} == {8, 16, 24, 32}
    assert any(ds.T2(N, 2) < ds.T2(N, 1) and M % 2 == 1 and M > 2 * ds.T2(N, 2) for N, M in cases)
    # several tiles of the second sweep with a ragged last one, for both feature sizes
    for fs in (1, 2):
        assert any((M // fs) * fs > 2 * ds.T2(N, fs) and 0 < ((M // fs) * fs) % ds.T2(N, fs) for N, M in cases)


def test_the_other_tables_reach_the_loops_of_several_passes():
    # for(e = lane; e < NP; e += 64): more than one pass, in <24> and in <32>
    for table in (ds.RETRY, ds.ZERO_COLUMN):
        assert {ds.size_class(N) for N, _ in table if ds.n_packed(N) > 64} == {24, 32}
    assert {ds.size_class(N) for N, _ in ds.NEIGHBOUR_SHAPES if ds.n_packed(N) > 64} == {24, 32}
    assert all(M < N for N, M in ds.UNDER) and {ds.size_class(N) for N, _ in ds.UNDER} >= {16, 24}
    assert all(0 <= col < N for (N, _), (col, _) in ds.ZERO_COLUMN.items())
    # a last wavefront alone in its workgroup, and problems 0, 100, B - 1 exist
    assert ds.B % 4 == 1 and ds.NEIGHBOUR_B % 4 == 1 and max(ds.NEIGHBOUR_ALONE) == ds.NEIGHBOUR_B - 1


# ---------------------------------------------------------------- 2. the margins of the parity cases
@pytest.mark.parametrize("setname", ["diverse", "default"])
@pytest.mark.parametrize("shape", sorted(ds.CASES) + sorted(ds.ONE_BY_ONE))
def test_margins_and_step_types(shape, setname):
    N, M = shape
    want = {**ds.CASES, **ds.ONE_BY_ONE}[shape][setname]
    orc = tb.oracle_batch(N, M, ds.SEED0, ds.B, setname)
    m = tb.assert_margin(orc, f"{shape} {setname} seed0 {ds.SEED0}")
    assert ds.recorded(m, want), "the generator changed: search seed0 again"
    types = set().union(*[o["step_types"] for o in orc])
    if setname == "diverse":
        assert types == ({0, 1, 2} if N >= 2 else {0, 1})
    assert {o["status"] for o in orc} <= {BATCH_JTX, BATCH_SMALL_STEP} and all(o["lambda_"] == 0.0 for o in orc)


# ---------------------------------------------------------------- 3. the paths that the old suite ran at (6, 40) only
@pytest.mark.parametrize("shape", sorted(ds.RETRY))
def test_rejected_trials_are_there(shape):
    seed0, B, want, rejected = ds.RETRY[shape]
    orc = tb.oracle_batch(*shape, seed0, B, "hard")
    m = tb.assert_margin(orc, f"hard set {shape}")
    assert ds.recorded(m, want)
    assert sum(o["rejected"] for o in orc) == rejected >= 1


@pytest.mark.parametrize("shape", sorted(ds.ZERO_COLUMN))
def test_zero_column_problems_end_with_a_lambda(shape):
    orc = ds.zero_oracle(shape)
    m = tb.assert_margin(orc, f"zero-column batch {shape}")
    assert ds.recorded(m, ds.ZERO_COLUMN[shape][1])
    assert [o["lambda_"] for o in orc] == [1e-10 if b in ds.ZERO_CHOSEN else 0.0 for b in range(ds.ZERO_B)]


@pytest.mark.parametrize("shape", sorted(ds.UNDER))
def test_underdetermined_batches_start_in_the_lambda_loop(shape):
    orc = ds.under_oracle(shape)
    m = min(o["margin"] for o in orc)
    print(f"{shape}: margin {m:.3g}")
    assert m > ds.UNDER_MARGIN_FLOOR >= 10 * ds.UNDER_P_TOL and ds.recorded(m, ds.UNDER[shape])
    assert all(o["lambda_"] == 1e-10 and o["status"] == BATCH_JTX and 2 <= o["iterations"] <= 3 for o in orc)
    assert all(o["evaluations"] == o["iterations"] + 1 for o in orc)


def test_the_underdetermined_shape_left_out_is_still_under_the_floor():
    # should this start to pass, (24, 9) belongs in ds.UNDER
    for shape, want in ds.UNDER_LEFT_OUT.items():
        m = min(o["margin"] for o in ds.under_oracle(shape))
        assert ds.recorded(m, want) and m <= ds.UNDER_MARGIN_FLOOR


# ---------------------------------------------------------------- 4. the host reference of the uncertainty call
@pytest.mark.parametrize("shape", ds.UNC_CASES)
def test_two_host_computations_agree_three_decades_under_the_tolerances(shape):
    a = ds.host_agreement(shape)
    print(f"{shape}: Sigma {a['sigma']:.3g}, factors {a['factors']:.3g}, cond(JtJ) {a['cond']:.4g}, largest leverage "
          f"{a['leverage']:.3g}, min |det(A_f - I)| {a['mindet']:.3g}")
    assert a["sigma"] <= 1e-3 * min(tu.COV_TOL, tu.VAR_TOL) and a["factors"] <= 1e-3 * tu.FAC_RTOL
    assert a["n_dbl_max"] == 0 and a["mindet"] > 1e-8
    assert a["cond"] <= 200 and a["leverage"] <= 0.91           # (measured: 173 and 0.90)


def test_zero_column_of_the_uncertainty_case_is_in_range():
    N, M = ds.UNC_ZERO_SHAPE
    assert ds.size_class(N) == 24 and ds.n_packed(N) > 64 and 0 <= ds.UNC_ZERO_COLUMN < N and M > N + 1
