"""What tests/test_dense_shapes_gpu.py presupposes, asserted without a GPU: that the constants and rules restated in
tests/dense_shapes.py are the ones in kernels_dense.hip and dense_diag.hip, that every N and M of its tables sits on the
edge its comment claims, that the CPU oracle's own float64 route (which substitutes where the kernels multiply by inverse
blocks: c = 1) meets every bound the kernels are held to -- the bounds are not vacuous and the reference alone passes
them --, that the inputs meet c <= 64, and that the oracle's lambda columns and step kinds on the problems with failing
pivots are the recorded ones."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libdogleg_amd.ctypes_defs import dptr
from tests import dense_shapes as ds
from tests import exact_ei
from tests import oracle_api as oa

CSRC = os.path.join(oa.ROOT, "libdogleg_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, f"the source no longer has a line like /{pattern}/: restate the rule in tests/dense_shapes.py"
    return int(m.group(1))


# ---------------------------------------------------------------- 1. the constants are the source's
def test_long_double_is_extended_precision():
    ds.require_long_double()


def test_restated_constants_are_those_of_the_source():
    kd, dd = _text("kernels_dense.hip"), _text("dense_diag.hip")
    assert _int(r"constexpr int TPB = (\d+);", kd) == ds.TPB
    assert _int(r"constexpr int KC = (\d+);", kd) == ds.KC
    assert _int(r"constexpr int NB = (\d+);", kd) == ds.NB == _int(r"constexpr int NB = (\d+);", dd)
    assert _int(r"constexpr int BT = (\d+)\*WT;", kd) * ds.SYRK_WT == ds.BT
    # the JtJ SYRK is the <64> instantiation, through the slabs
    assert _int(r"DLG_CHECK\(launch_syrk<(\d+)>\(b->stream, b->G, b->N, S\.Jin\(\)", kd) == ds.SYRK_WT
    assert _int(r"constexpr int S = (\d+);", kd) == ds.SUPER
    m = re.search(r"const int r = pos & (\d+), q = pos >> (\d+);", kd)
    assert m and int(m.group(1)) == ds.GROUP - 1 and 1 << int(m.group(2)) == ds.GROUP
    m = re.search(r"idx \+= \(ntl - x \+ (\d+)\) >> (\d+);", kd)
    assert m and int(m.group(1)) == ds.GROUP - 1 and 1 << int(m.group(2)) == ds.GROUP
    assert _int(r"constexpr int SYRK_RSUB = (\d+);", kd) == ds.SYRK_RSUB
    assert _int(r"if\(rem >= (\d+)\) rc = launch_syrk<64>", kd) == ds.STEP_REM_WIDE
    # syrk_nsplit and the kper rule
    assert re.search(r"static int syrk_nsplit\(int ntiles, int K, int resident = 512\)", kd)
    assert re.search(r"int nom = dlg_cdiv\(1536, ntiles\);", kd) and re.search(r"const int maxs = K/\(4\*KC\);", kd)
    assert re.search(r"lo = std::max\(1, 2\*nom/3\), hi = std::max\(lo, std::min\(std::max\(maxs, 1\), nom \+ nom/2 \+ 1\)\);", kd)
    assert re.search(r"if\(eff\(ns\) >= beff - 0\.03\) return ns;", kd)
    assert re.search(r"if\(ks < 2\) ks = 2;", kd)
    assert re.search(r"int kper = dlg_cdiv\(dlg_cdiv\(K, ks\), KC\)\*KC;\s*if\(kper < KC\) kper = KC;", kd)
    # dense_eval, dense_norm2_Jv
    assert _int(r"int rpc = (\d+);", kd) == ds.EVAL_RPC0
    m = re.search(r"while\(rpc > (\d+) && \(long\)dlg_cdiv\(M, rpc\)\*dlg_cdiv\(N, TPB\) < (\d+)\) rpc >>= 1;", kd)
    assert m and (int(m.group(1)), int(m.group(2))) == (ds.EVAL_RPC_MIN, ds.EVAL_WG)
    assert _int(r"const int nsl = \(nchunks >= (\d+)\) \? 32 : 0;", kd) == ds.EVAL_TWO_STAGE
    m = re.search(r"int g = dlg_cdiv\(M, (\d+)\); if\(g > (\d+)\) g = \2;", kd)
    assert m and (int(m.group(1)), int(m.group(2))) == (ds.NORM2_WAVES, ds.NORM2_G_MAX)
    # which form runs
    assert re.search(r"if\(!b->knobs\.potrf_steps && T >= 2\)", kd)
    assert re.search(r"if\(T >= 2 && T <= b->ncu/2 && !b->knobs\.trsv_steps\)", kd)
    assert _int(r"const bool ffold = i >= (\d+);", dd) == ds.FOLD_FWD_FROM
    assert _int(r"const bool b_early = T - 1 - i < (\d+);", dd) == ds.FOLD_BWD_WITHIN


def test_the_lds_attribute_of_the_syrk_is_set_per_device():
    """a function attribute is a property of (function, device): k_syrk_lower<64> needs 73 728 B of dynamic LDS on every
    device it is launched on, not only on the first one of the process"""
    kd = _text("kernels_dense.hip")
    assert "static bool attr_set" not in kd
    assert re.search(r"static bool attr\[DLG_MAX_DEV\] = \{\};[^\n]*\n\s*dlg_func_lds_once\(attr, reinterpret_cast<const void\*>\(&k_syrk_lower<WT>\)", kd)
    assert 4 * ds.KC * (ds.BT + 16) * 8 == 73728


# ---------------------------------------------------------------- 2. every case sits on the edge its comment claims
def test_every_N_sits_on_its_edge():
    for N, claim in ds.N_CASES.items():
        got = (ds.tiles(N), ds.last_tile(N), ds.block_tiles(N), ds.last_block_tile(N), ds.super_tiles(N), ds.trsv_regime(N))
        assert got == claim, (N, got, claim)
        assert ds.default_M(N) >= 2 * N and ds.default_M(N) % 2 == 1 and ds.default_M(N) % 16 != 0
        assert ds.default_M(N) == 2 * N + 3 or N < 256
    Ns = set(ds.N_CASES)
    # one short of, on and one past every 64-column tile up to four, and the 128-row block tile up to two
    for edge in (64, 128, 192, 256):
        assert {edge - 1, edge, edge + 1} <= Ns
    assert all(not ds.one_launch_potrf(N) for N in (1, 2, 15, 16, 17, 63, 64)) and ds.one_launch_potrf(65)
    assert all(ds.one_launch_trsv(N) for N in Ns if N >= 65)
    # a last tile of one column, a whole one, one short of whole: in both one-launch kernels
    assert {ds.last_tile(N) for N in Ns if N >= 65} >= {1, 63, 64}
    assert {ds.last_block_tile(N) for N in Ns if ds.block_tiles(N) > 1} >= {1, 63, 64, 65, 127, 128}
    # every regime of k_trsv_tiles on both sides of its threshold
    assert (ds.trsv_regime(512), ds.trsv_regime(513)) == ("plain", "fold")
    assert (ds.trsv_regime(1024), ds.trsv_regime(1025)) == ("fold", "fold+")
    # the super-tile list changes shape at 4 -> 5 and at 8 -> 9 block tiles
    assert [(ds.block_tiles(N), ds.super_tiles(N)) for N in (512, 513, 1024, 1025)] == [(4, 1), (5, 2), (8, 2), (9, 3)]
    # groups of eight positions: a tile count below 8 (empty groups), and counts that are no multiple of 8
    counts = {N: ds.block_tiles(N) * (ds.block_tiles(N) + 1) // 2 for N in Ns}
    assert min(counts.values()) == 1 and 0 in ds.group_sizes(1) and any(c % 8 for c in counts.values() if c > 8)
    assert all(sum(ds.group_sizes(c)) == c for c in counts.values())
    # the step form: launch_syrk<64> only with rem >= 1024, which 1089 reaches in its first step and 1025 never does
    assert ds.step_form_rems(1089)[0] == 1025 and max(ds.step_form_rems(1025)) < ds.STEP_REM_WIDE
    assert set(ds.STEP_FORM_ONLY) == {1089}
    # odd N: the pair-of-rows loop of k_syrk_reduce stores one row only in the last row
    assert sum(N % 2 for N in Ns) >= 8
    # the SYRK at these shapes: several splits, also empty ones
    assert any(ds.syrk_split(N, ds.default_M(N))[2] > 0 for N in Ns) and any(ds.syrk_split(N, ds.default_M(N))[0] > 8 for N in Ns)


def test_every_M_of_the_sweep_sits_on_its_edge():
    for N in ds.M_SWEEP_N:
        assert ds.one_launch_potrf(N) and ds.block_tiles(N) in (1, 2)
        for M in ds.M_SWEEP:
            assert (ds.syrk_split(N, M), ds.eval_chunks(M, N)) == ds.m_sweep_claim(N, M), (N, M)
    Ms = set(ds.M_SWEEP)
    assert {1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025} <= Ms
    # both sides of nchunks >= 64, and a last chunk of one row on the far side
    assert not ds.eval_chunks(1008, 65)[2] and ds.eval_chunks(1023, 65)[2] and ds.eval_chunks(1025, 65)[1] == 65
    # empty splits, a split of one row
    assert ds.syrk_split(65, 16)[2] == 1 and ds.syrk_split(65, 17) == (2, 16, 0)
    # rows per wave of k_norm2_Jv_part above 1
    for M, rows in ds.M_SWEEP_LONG.items():
        assert ds.norm2_rows_per_wave(M) == rows
    assert set(ds.M_SWEEP_LONG.values()) == {1, 2}
    assert all(ds.norm2_rows_per_wave(M) == 1 for M in ds.M_SWEEP)


def test_the_failing_pivot_cases_are_where_the_table_says():
    Ns = {N for N, _, _ in ds.ZERO_CASES.values()}
    assert Ns == {65, 130, 193, 257, 513} and all(ds.one_launch_potrf(N) and ds.one_launch_trsv(N) for N in Ns)
    cols = [(N, z) for N, _, z in ds.ZERO_CASES.values()]
    assert any(z == (0,) for _, z in cols) and any(z == (63,) for _, z in cols) and any(z == (64,) for _, z in cols)
    assert any(z == (N - 1,) for N, z in cols)
    assert any(len({c // ds.NB for c in z}) >= 2 for _, z in cols)
    assert ds.trsv_regime(513) == "fold"
    assert set(ds.ZERO_SOLVES) <= set(ds.ZERO_CASES) and {ds.ZERO_CASES[n][0] for n in ds.ZERO_SOLVES} == Ns
    for N, k in ds.NEG_CASES:
        assert ds.one_launch_potrf(N) and k in (63, N - 1)


# ---------------------------------------------------------------- 3. the oracle's float64 route meets every bound with c = 1
def oracle_route(R):
    """orc_step_dense on the inputs of the reference R: (jtx, cauchy, gn, step, L, out8) or None where it does not factorise"""
    O = oa.oracle()
    N, M = R.N, R.M
    dfac, work, o8 = np.zeros(N * (N + 1) // 2), np.zeros(5 * N), np.zeros(8)
    if O.orc_step_dense(N, M, dptr(R.J), dptr(R.x), dptr(R.p), R.lam, dptr(dfac), dptr(work), dptr(o8)) != 0:
        return None
    return work[:N].copy(), work[N:2 * N].copy(), work[2 * N:3 * N].copy(), work[3 * N:4 * N].copy(), ds.unpack_factor(dfac, N), o8


def route_ratios(R):
    """every bound of tests/dense_shapes.py on the oracle's route, c = 1: {check: observed / bound}"""
    g, cauchy, gn, step, L, o8 = oracle_route(R)
    out = ds.check_eval(R, g, o8[0], o8[6])
    out.update(ds.check_cauchy(R, g, cauchy, o8[1]))
    out["factor"] = ds.check_factor(R, L, 1.0)
    out["gn"] = ds.check_gn(R, L, gn, 1.0)
    out["norm2_gn"] = ds.check_norm2(gn, o8[2])
    # the step of orc_step_dense: interpolated where the trust region mean(|cauchy|, |gn|) lies between the two
    tr = 0.5 * (np.sqrt(o8[1]) + np.sqrt(o8[2]))
    if o8[1] < tr * tr < o8[2]:
        sref, sb, k, dk = ds.step_reference(2, cauchy, gn, o8[1], tr)
        out["step"] = ds._ratio(step.astype(ds.LD) - sref, sb)
        out["k"] = ds._ratio(ds.LD(o8[3]) - k, dk)
    if R.N <= 129:
        ei = exact_ei.expected_improvement(R.J, R.x, step)
        _, b = ds.ei_bound(R, g, step)
    else:
        ei, b = ds.ei_bound(R, g, step)
    out["ei"] = ds._ratio(ds.LD(o8[5]) - ds.LD(ei), b)
    return out


@pytest.mark.parametrize("N", list(ds.N_CASES))
def test_the_oracle_route_meets_the_bounds_at_every_N(N):
    M = ds.default_M(N)
    worst_c = 0.0
    for lam in ds.LAMBDAS:
        R = ds.reference(N, M, lam)
        assert R.L is not None and R.c <= ds.C_MAX, (N, lam, R.c)
        worst_c = max(worst_c, R.c)
        ratios = route_ratios(R)
        print(f"N {N} lambda {lam:g}: c {R.c:.1f}", {k: f"{v:.3f}" for k, v in ratios.items()})
        assert all(v <= 1.0 for v in ratios.values()), (N, lam, ratios)
        assert max(ratios.values()) > 0.0 or N == 1
    assert abs(worst_c - ds.C_RECORDED[N]) <= 0.06, (worst_c, ds.C_RECORDED[N])


@pytest.mark.parametrize("N", ds.M_SWEEP_N + (ds.M_SWEEP_LONG_N,))
def test_the_oracle_route_meets_the_bounds_over_the_M_sweep(N):
    sweep = [(M, ds.M_SWEEP_SIGMA) for M in ds.M_SWEEP] if N in ds.M_SWEEP_N else [(M, 1.0) for M in ds.M_SWEEP_LONG]
    for M, sigma in sweep:
        R = ds.reference(N, M, ds.M_SWEEP_LAMBDA, (), 0, sigma)
        assert R.L is not None and R.c <= ds.C_MAX, (N, M, R.c)
        ratios = route_ratios(R)
        assert all(v <= 1.0 for v in ratios.values()), (N, M, ratios)


@pytest.mark.parametrize("N", ds.PRODUCTS_N)
def test_the_oracle_route_meets_the_bounds_on_the_products_form(N):
    O = oa.oracle()
    for lam in ds.PRODUCTS_LAMBDAS:
        R = ds.products_reference(N, ds.default_M(N), lam, True)
        assert R.L is not None and R.c <= ds.C_MAX
        ap = R.upload.copy()
        ap[np.cumsum([0] + [N - i for i in range(N - 1)])] += lam
        assert O.orc_dpptrf_L(N, dptr(ap)) == 0
        gn = R.g64.copy()
        O.orc_dpptrs_L(N, dptr(ap), dptr(gn))
        gn *= -1
        L = ds.unpack_factor(ap, N)
        assert ds.check_factor(R, L, 1.0) <= 1.0 and ds.check_gn(R, L, gn, 1.0) <= 1.0
        val, b = ds.ei_products_bound(R, gn)
        got = -2.0 * O.orc_inner(dptr(R.g64), dptr(gn), N) - O.orc_xt_Apacked_upper_x(dptr(gn), dptr(R.upload), N)
        assert ds._ratio(ds.LD(got) - ds.LD(val), b) <= 1.0
        if N <= 129:
            exact = exact_ei.expected_improvement_products(R.g64, R.H64, gn)
            assert ds._ratio(ds.LD(exact) - ds.LD(val), b) <= 1e-3          # the two references agree far inside the bound


# ---------------------------------------------------------------- 4. the lambda cases
@pytest.mark.parametrize("name", list(ds.ZERO_CASES))
def test_zero_columns_fail_the_pivot_and_decouple(name):
    N, M, zero = ds.ZERO_CASES[name]
    R0 = ds.reference(N, M, 0.0, zero)
    assert R0.L is None and R0.bad + 1 == ds.first_bad_pivot(zero)
    R = ds.reference(N, M, ds.ZERO_LAMBDA, zero)
    assert R.L is not None and R.c <= ds.C_MAX, R.c
    assert all(R.gn[c] == 0 for c in zero) and all(R.g[c] == 0 for c in zero)
    assert oracle_route(R0) is None
    ratios = route_ratios(R)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # the positive definite upload that follows the failure in the GPU test
    Rpd = ds.reference(N, M, 0.0)
    assert Rpd.L is not None and Rpd.c <= ds.C_MAX, Rpd.c


@pytest.mark.parametrize("N", [1, 17, 65, 257, 1089])
def test_the_check_of_lambda_on_the_diagonal_is_sharp(N):
    """on the scaled inputs the two factors' bounds together stay below DIAG_SHARP lambda, the reference's own row sums
    differ by lambda far inside them, and a factor of a matrix with lambda missing from ONE diagonal entry -- the last
    row -- is outside"""
    M = ds.default_M(N)
    R0 = ds.reference(N, M, 0.0, (), 0, ds.DIAG_SIGMA)
    R1 = ds.reference(N, M, ds.DIAG_LAMBDA, (), 0, ds.DIAG_SIGMA)
    assert R0.c <= ds.C_MAX
    (s0, b0), (s1, b1) = ds.diag_rows_bound(R0, R0.L.astype(np.float64)), ds.diag_rows_bound(R0, R1.L.astype(np.float64))
    assert float(np.max(b0 + b1)) <= ds.DIAG_SHARP * ds.DIAG_LAMBDA
    assert float(np.max(np.abs((s1 - s0) - ds.LD(ds.DIAG_LAMBDA)) / (b0 + b1))) <= 1.0
    A = R1.A.copy()
    A[N - 1, N - 1] -= ds.LD(ds.DIAG_LAMBDA)
    Lbad, _ = ds.cholesky(A)
    sb, bb = ds.diag_rows_bound(R0, Lbad.astype(np.float64))
    miss = np.abs((sb - s0) - ds.LD(ds.DIAG_LAMBDA)) / (b0 + bb)
    assert float(miss[N - 1]) >= 1.0 / ds.DIAG_SHARP and float(np.max(miss[:N - 1], initial=0)) <= 1.0


def _trials(tr):
    return [(t["lambda_"], t["step_type"]) for t in tr.trials()]


@pytest.mark.parametrize("name", ds.ZERO_SOLVES)
def test_the_oracle_takes_the_recorded_steps_behind_a_failed_pivot(name):
    N, M, _ = ds.ZERO_CASES[name]
    J0, xs, p0 = ds.zero_solve(name)
    cb = ds.dense_cb(J0, xs)
    for tr0, want in ((None, ds.ZERO_TRIALS[name]), (ds.ZERO_SMALL_TRUSTREGION, ds.ZERO_TRIALS_SMALL[name])):
        prm = oa.default_params()
        prm.max_iterations = ds.ZERO_MAX_ITERATIONS
        if tr0 is not None:
            prm.trustregion0 = tr0
        r, p, tr = oa.oracle_solve("dense", p0, N, M, 0, C.cast(cb, C.c_void_p), None, prm)
        assert r >= 0 and _trials(tr) == want
    kinds = {k for n in ds.ZERO_SOLVES for _, k in ds.ZERO_TRIALS_SMALL[n]}
    assert kinds == {0, 1, 2}


@pytest.mark.parametrize("N,k", ds.NEG_CASES)
def test_the_oracle_raises_lambda_four_times_over_a_negative_pivot(N, k):
    for packed in (True, False):
        cb, H = ds.neg_products(N, k, packed)
        for lam in (0.0, 1e-10, 1e-9, 1e-8):
            assert ds.cholesky(np.tril(H).astype(ds.LD) + ds.LD(lam) * np.eye(N, dtype=ds.LD))[0] is None
        assert ds.cholesky(np.tril(H).astype(ds.LD) + ds.LD(1e-7) * np.eye(N, dtype=ds.LD))[0] is not None
        prm = oa.default_params()
        prm.max_iterations = ds.ZERO_MAX_ITERATIONS
        prm.JtJ_packed = prm.JtJ_upper = packed
        r, p, tr = oa.oracle_solve("products", np.zeros(N), N, 0, 0, C.cast(cb, C.c_void_p), None, prm)
        assert [t["lambda_"] for t in tr.trials()] == ds.NEG_LAMBDA_COLUMN
