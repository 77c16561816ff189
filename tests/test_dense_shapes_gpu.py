"""The single-problem dense path (DLG_DENSE, DLG_DENSE_PRODUCTS: kernels_dense.hip, dense_diag.hip) at every tile edge and
change of regime that tests/dense_shapes.py lists, operation by operation through the C-ABI against long-double
references under derived rounding bounds, in the one-launch forms and in both step forms; and a pivot that fails INSIDE
the one-launch factorisation (N >= 65), with the lambda loop, the speculative solve and a whole solve behind it.

Every check prints `ratio <check> <where> <observed / bound>`; the bounds (tests/dense_shapes.py) do not depend on them.
tests/test_dense_shapes_cpu.py asserts without a GPU what this file presupposes."""
import ctypes as C

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import dptr
from tests import dense_shapes as ds
from tests import exact_ei
from tests import oracle_api as oa
from tests.parity import compare_traces

pytestmark = pytest.mark.gpu

MODES = {"default": (), "potrf-steps": ("DOGLEG_AMD_POTRF_STEPS",), "trsv-steps": ("DOGLEG_AMD_TRSV_STEPS",)}
STEP_FORM = ("DOGLEG_AMD_POTRF_STEPS", "DOGLEG_AMD_TRSV_STEPS")
EXACT_EI_MAX_N = 129
WORST = {}


def set_form(monkeypatch, names):
    """the knobs are read when a backend is created"""
    for k in STEP_FORM:
        monkeypatch.delenv(k, raising=False)
    for k in names:
        monkeypatch.setenv(k, "1")


def held(check, ratio, where):
    """observed / bound of one check: printed, kept for the summary line, asserted"""
    print(f"ratio {check} {where} {ratio:.4f}")
    if ratio > WORST.get(check, (-1.0, None))[0]:
        WORST[check] = (ratio, where)
    assert ratio <= 1.0, (check, where, ratio)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print("\nworst observed / bound per check: " + "; ".join(f"{k} {v[0]:.4f} at {v[1]}" for k, v in sorted(WORST.items())))


def backend(R, kind=capi.DLG_DENSE, flags=0, device=-1):
    be = capi.Backend(kind, R.N, R.M, 0, flags, device)
    be.set_p(0, R.p)
    return be


def device_factor(be, N, full=False):
    """L from dlg_factor_download_dense: the packed triangle, or (DLG_DENSE_PRODUCTS with an unpacked JtJ) the N x N
    column-major array whose lower triangle holds L"""
    if full:
        return np.tril(be.factor_dense(N * N).reshape(N, N).T)
    return ds.unpack_factor(be.factor_dense(N * (N + 1) // 2), N)


def point_ops(be, P, where):
    """K1 and K3 of the uploaded point against the long-double reference: (jtx, cauchy, |cauchy|^2) as the device holds them"""
    n2x, gmax = be.eval(0)
    jtx = be.download(0, capi.VEC_JTX)
    for k, v in ds.check_eval(P, jtx, n2x, gmax).items():
        held(k, v, where)
    n2c = be.cauchy(0)
    cauchy = be.download(0, capi.VEC_CAUCHY)
    for k, v in ds.check_cauchy(P, jtx, cauchy, n2c).items():
        held(k, v, where)
    return jtx, cauchy, n2c


def factor_and_solve(be, R, where, want_factor_check=True, full=False):
    """factorize(0, R.lam) + factor_dense + solve_gn under the factor's and the residual's bound: (L, gn, |gn|^2)"""
    assert be.factorize(0, R.lam), (where, "a pivot failed")
    L = device_factor(be, R.N, full)
    if want_factor_check:
        held("factor", ds.check_factor(R, L, R.c), where)
    n2gn = be.solve_gn(0)
    gn = be.download(0, capi.VEC_GN)
    held("gn", ds.check_gn(R, L, gn, R.c), where)
    held("norm2_gn", ds.check_norm2(gn, n2gn), where)
    return L, gn, n2gn


def ei_check(be, P, jtx, step, where):
    ei = be.expected_improvement(0, 1)
    ref, bound = ds.ei_bound(P, jtx, step)
    if P.N <= EXACT_EI_MAX_N:
        ref = exact_ei.expected_improvement(P.J, P.x, step)
    held("ei", ds._ratio(ds.LD(ei) - ds.LD(ref), bound), where)


def steps_and_ei(be, P, jtx, cauchy, n2c, gn, n2gn, where, kinds=(capi.KIND_CAUCHY, capi.KIND_GN, capi.KIND_INTERP)):
    """K7 in the kinds asked for, at trust radii from the norms of the two steps, and K8 of each"""
    rc, rg = np.sqrt(n2c), np.sqrt(n2gn)
    radius = {capi.KIND_CAUCHY: 0.5 * rc, capi.KIND_GN: 2.0 * rg, capi.KIND_INTERP: 0.5 * (rc + rg)}
    for kind in kinds:
        if kind == capi.KIND_INTERP and not rc < (1 - 1e-6) * rg:
            assert P.N == 1 or P.M < P.N            # one variable: the Cauchy step IS the Gauss-Newton step
            continue
        tr = radius[kind]
        n2s, k, amax, pnew = be.make_step(0, 1, kind, tr)
        step = be.download(1, capi.VEC_STEP)
        sref, sb, kref, dk = ds.step_reference(kind, cauchy, gn, n2c, tr)
        w = f"{where} kind {kind}"
        held("step", ds._ratio(step.astype(ds.LD) - sref, sb), w)
        assert amax == np.max(np.abs(step))                                    # a maximum rounds nothing
        # p_new = p + step: one rounding per entry; 4 U (|p| + |step|) with the margin of sum_bound
        held("p_new", ds._ratio(pnew.astype(ds.LD) - (P.p.astype(ds.LD) + step.astype(ds.LD)),
                                4 * ds.U * (np.abs(P.p) + np.abs(step)).astype(ds.LD)), w)
        if kind == capi.KIND_INTERP:
            held("k", ds._ratio(ds.LD(k) - kref, dk), w)
            held("norm2_step", ds.check_norm2(step, n2s), w)
        else:
            assert n2s == (n2c if kind == capi.KIND_CAUCHY else n2gn)          # dogleg.c:1200: the unscaled norm
        ei_check(be, P, jtx, step, w)


def diagonal_lambda(be, N, M, where, upload):
    """sum_k L_ik^2 at lambda = 1e-10 exceeds the value at lambda = 0 by 1e-10 in EVERY row i, to within the two factors'
    bounds (ds.diag_rows_bound; the inputs scaled so that the bounds stay below half of lambda): a lambda that
    k_syrk_reduce / k_unpack_to_G leaves off one diagonal entry fails here by name -- the last row of an odd N included"""
    R0 = ds.reference(N, M, 0.0, (), 0, ds.DIAG_SIGMA)
    upload(R0)
    rows = []
    for lam in (0.0, ds.DIAG_LAMBDA):
        assert be.factorize(0, lam)
        rows.append(ds.diag_rows_bound(R0, ds.unpack_factor(be.factor_dense(N * (N + 1) // 2), N)))
    (s0, b0), (s1, b1) = rows
    assert float(np.max(b0 + b1)) <= ds.DIAG_SHARP * ds.DIAG_LAMBDA
    per_row = np.abs((s1 - s0) - ds.LD(ds.DIAG_LAMBDA)) / (b0 + b1)
    held("lambda_on_the_diagonal", float(np.max(per_row)), f"{where} row {int(np.argmax(per_row))}")


def oracle_agreement(R, gn, n2c):
    """the project's own agreement with the CPU oracle (as test_dense_stream_variants_match_oracle asks it)"""
    O = oa.oracle()
    N, M = R.N, R.M
    dfac, work, o8 = np.zeros(N * (N + 1) // 2), np.zeros(5 * N), np.zeros(8)
    assert O.orc_step_dense(N, M, dptr(R.J), dptr(R.x), dptr(R.p), 0.0, dptr(dfac), dptr(work), dptr(o8)) == 0
    assert np.linalg.norm(gn - work[2 * N:3 * N]) <= 1e-10
    assert abs(n2c - o8[1]) <= 1e-10 * o8[1]


# ---------------------------------------------------------------- 1. operations one at a time, at every N
@pytest.mark.parametrize("N", list(ds.N_CASES))
def test_operations_one_at_a_time(gpu, N, monkeypatch):
    set_form(monkeypatch, STEP_FORM if N in ds.STEP_FORM_ONLY else ())
    M = ds.default_M(N)
    P = ds.point(N, M)
    be = backend(P)
    try:
        be.upload(0, P.x, P.J)
        jtx, cauchy, n2c = point_ops(be, P, f"N {N}")
        for lam in (1.0, 1e-10, 0.0):
            R = ds.reference(N, M, lam)
            L, gn, n2gn = factor_and_solve(be, R, f"N {N} lambda {lam:g}")
        steps_and_ei(be, P, jtx, cauchy, n2c, gn, n2gn, f"N {N}")
        if N <= ds.ORACLE_AGREEMENT_MAX_N:
            oracle_agreement(R, gn, n2c)
    finally:
        be.close()


@pytest.mark.parametrize("N", list(ds.N_CASES))
def test_lambda_reaches_every_diagonal_entry(gpu, N, monkeypatch):
    """the SYRK's reduce adds lambda to the diagonal (k_syrk_reduce, a pair of rows a thread): row by row, see
    diagonal_lambda"""
    set_form(monkeypatch, STEP_FORM if N in ds.STEP_FORM_ONLY else ())
    M = ds.default_M(N)
    be = capi.Backend(capi.DLG_DENSE, N, M)
    try:
        diagonal_lambda(be, N, M, f"N {N}", lambda R0: (be.set_p(0, R0.p), be.upload(0, R0.x, R0.J), be.eval(0)))
    finally:
        be.close()


# ---------------------------------------------------------------- the M sweep
@pytest.mark.parametrize("N", ds.M_SWEEP_N + (ds.M_SWEEP_LONG_N,))
def test_the_M_sweep(gpu, N, monkeypatch):
    set_form(monkeypatch, ())
    sweep = [(M, ds.M_SWEEP_SIGMA) for M in ds.M_SWEEP] if N in ds.M_SWEEP_N else [(M, 1.0) for M in ds.M_SWEEP_LONG]
    for M, sigma in sweep:
        R = ds.reference(N, M, ds.M_SWEEP_LAMBDA, (), 0, sigma)
        be = backend(R)
        try:
            be.upload(0, R.x, R.J)
            where = f"M {M} N {N}"
            jtx, cauchy, n2c = point_ops(be, R, where)
            L, gn, n2gn = factor_and_solve(be, R, where)
            steps_and_ei(be, R, jtx, cauchy, n2c, gn, n2gn, where, kinds=(capi.KIND_GN, capi.KIND_CAUCHY))
        finally:
            be.close()


# ---------------------------------------------------------------- 2. both forms
@pytest.mark.parametrize("N", [N for N in ds.N_CASES if N not in ds.STEP_FORM_ONLY])
def test_the_one_launch_forms_and_the_step_forms(gpu, N, monkeypatch):
    """factor and solve by default (k_potrf_tiles / k_trsv_tiles from T = 2 on), under DOGLEG_AMD_POTRF_STEPS and under
    DOGLEG_AMD_TRSV_STEPS: the same bounds for all three, agreement with one another to 1e-11 max(1, |gn|_inf) (as
    test_one_launch_potrf_matches_the_step_form_and_reproduces_its_bits asks), and two repetitions over two alternating
    inputs reproduce their bits"""
    M = ds.default_M(N)
    draws = [ds.inputs(N, M, (), alt) for alt in (0, 1)]
    got = {}
    checked = {}                                           # factor bits -> its ratio: the same factor is checked once
    for mode, names in MODES.items():
        set_form(monkeypatch, names)
        be = capi.Backend(capi.DLG_DENSE, N, M)
        try:
            be.set_p(0, draws[0][2])
            runs = []
            for rep in range(2):
                for alt, (x, J, p) in enumerate(draws):
                    be.upload(0, x, J)
                    be.eval(0)
                    for lam in ds.LAMBDAS:
                        assert be.factorize(0, lam)
                        fac = be.factor_dense(N * (N + 1) // 2)
                        n2gn = be.solve_gn(0)
                        runs.append((alt, lam, fac, n2gn, be.download(0, capi.VEC_GN)))
        finally:
            be.close()
        half = len(runs) // 2
        for a, b in zip(runs[:half], runs[half:]):
            assert a[3] == b[3] and np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4]), (mode, a[0], a[1])
        for alt, lam, fac, n2gn, gn in runs[:half]:
            if alt == 0:
                R = ds.reference(N, M, lam)
                L = ds.unpack_factor(fac, N)
                key = (lam, fac.tobytes())
                if key not in checked:
                    checked[key] = ds.check_factor(R, L, R.c)
                held("factor", checked[key], f"N {N} lambda {lam:g} {mode}")
                held("gn", ds.check_gn(R, L, gn, R.c), f"N {N} lambda {lam:g} {mode}")
                held("norm2_gn", ds.check_norm2(gn, n2gn), f"N {N} lambda {lam:g} {mode}")
        got[mode] = runs[:half]
    for mode in ("potrf-steps", "trsv-steps"):
        for a, b in zip(got["default"], got[mode]):
            assert np.max(np.abs(a[4] - b[4])) <= 1e-11 * max(1.0, np.max(np.abs(a[4]))), (mode, a[0], a[1])


# ---------------------------------------------------------------- 3. DLG_DENSE_PRODUCTS
@pytest.mark.parametrize("packed", [True, False], ids=["packed-upper", "unpacked"])
@pytest.mark.parametrize("N", ds.PRODUCTS_N)
def test_the_products_form(gpu, N, packed, monkeypatch):
    set_form(monkeypatch, ())
    M = ds.default_M(N)
    flags = (capi.FLAG_PACKED | capi.FLAG_UPPER) if packed else 0
    be = capi.Backend(capi.DLG_DENSE_PRODUCTS, N, M, 0, flags)
    try:
        for lam in ds.PRODUCTS_LAMBDAS:
            R = ds.products_reference(N, M, lam, packed)
            where = f"products N {N} lambda {lam:g} {'packed' if packed else 'full'}"
            be.set_p(0, R.p)
            be.upload_products(0, R.n2x64, R.g64, R.upload)
            n2x, gmax = be.eval(0)
            assert n2x == R.n2x64 and gmax == np.max(np.abs(R.g64))              # handed through
            L, gn, n2gn = factor_and_solve(be, R, where, full=not packed)
            n2s, k, amax, pnew = be.make_step(0, 1, capi.KIND_GN, 2.0 * np.sqrt(n2gn))
            step = be.download(1, capi.VEC_STEP)
            assert np.array_equal(step, gn)
            ei = be.expected_improvement(0, 1)
            ref, bound = ds.ei_products_bound(R, step)
            if N <= EXACT_EI_MAX_N:
                ref = exact_ei.expected_improvement_products(R.g64, R.H64, step)
            held("ei_products", ds._ratio(ds.LD(ei) - ds.LD(ref), bound), where)
    finally:
        be.close()


@pytest.mark.parametrize("packed", [True, False], ids=["packed-upper", "unpacked"])
@pytest.mark.parametrize("N", ds.PRODUCTS_N)
def test_lambda_reaches_every_diagonal_entry_of_the_products(gpu, N, packed, monkeypatch):
    """k_unpack_to_G's lambda, row by row: the products scaled by 2^-12 (exactly), as diagonal_lambda scales J"""
    set_form(monkeypatch, ())
    M = ds.default_M(N)
    R0 = ds.products_reference(N, M, 0.0, packed)
    be = capi.Backend(capi.DLG_DENSE_PRODUCTS, N, M, 0, (capi.FLAG_PACKED | capi.FLAG_UPPER) if packed else 0)
    try:
        be.set_p(0, R0.p)
        diagonal_lambda_products(be, R0, ds.DIAG_SIGMA ** 2, f"products N {N} {'packed' if packed else 'full'}", not packed)
    finally:
        be.close()


def diagonal_lambda_products(be, R0, s2, where, full):
    N = R0.N
    be.upload_products(0, R0.n2x64 * s2, R0.g64 * s2, R0.upload * s2)
    be.eval(0)
    rows = []
    for lam in (0.0, ds.DIAG_LAMBDA):
        assert be.factorize(0, lam)
        rows.append(ds.diag_rows_bound(R0, device_factor(be, N, full)))
    (s0, b0), (s1, b1) = rows
    assert float(np.max(b0 + b1)) <= ds.DIAG_SHARP * ds.DIAG_LAMBDA
    per_row = np.abs((s1 - s0) - ds.LD(ds.DIAG_LAMBDA)) / (b0 + b1)
    held("lambda_on_the_diagonal", float(np.max(per_row)), f"{where} row {int(np.argmax(per_row))}")


# ---------------------------------------------------------------- 4. a pivot that fails inside the one-launch factorisation
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(ds.ZERO_CASES))
def test_a_zero_column_fails_the_pivot_and_lambda_repairs_it(gpu, name, mode, monkeypatch):
    """factorize(0, 0) reports the failure; factorize(0, 1e-10) gives a factor within the bound; the backend that has just
    had a failed factorisation factorises another, positive definite upload correctly (the pivot word, the flags and the
    epoch do not stick); gauss_newton(0, 0) raises lambda to 1e-10 itself and its step meets the residual's bound"""
    set_form(monkeypatch, MODES[mode])
    N, M, zero = ds.ZERO_CASES[name]
    R = ds.reference(N, M, ds.ZERO_LAMBDA, zero)
    Rpd = ds.reference(N, M, 0.0)
    be = backend(R)
    try:
        be.upload(0, R.x, R.J)
        be.eval(0)
        assert not be.factorize(0, 0.0)
        assert be.factorize(0, ds.ZERO_LAMBDA)
        L = ds.unpack_factor(be.factor_dense(N * (N + 1) // 2), N)
        held("factor", ds.check_factor(R, L, R.c), f"{name} {mode} lambda 1e-10")
        # a failure, then another matrix
        assert not be.factorize(0, 0.0)
        be.upload(0, Rpd.x, Rpd.J)
        be.eval(0)
        factor_and_solve(be, Rpd, f"{name} {mode} behind a failed pivot")
        # the lambda loop re-entering the kernels
        be.upload(0, R.x, R.J)
        be.eval(0)
        lam, n2gn = be.gauss_newton(0, 0.0)
        assert lam == ds.ZERO_LAMBDA
        gn = be.download(0, capi.VEC_GN)
        L2 = ds.unpack_factor(be.factor_dense(N * (N + 1) // 2), N)
        assert np.array_equal(L2, L)
        assert all(gn[c] == 0.0 for c in zero)
        held("gn", ds.check_gn(R, L2, gn, R.c), f"{name} {mode} gauss_newton")
        held("norm2_gn", ds.check_norm2(gn, n2gn), f"{name} {mode} gauss_newton")
    finally:
        be.close()


@pytest.mark.parametrize("defer", [False, True], ids=["inline-tail", "deferred-tail"])
@pytest.mark.parametrize("name", list(ds.ZERO_CASES))
def test_take_step_behind_a_failed_pivot(gpu, name, defer, monkeypatch):
    """dlg_take_step from lambda = 0: the Cauchy step, the factorisation, the speculative solve behind the factor that
    failed, the retry at 1e-10 and the step, behind one synchronisation"""
    set_form(monkeypatch, ())
    N, M, zero = ds.ZERO_CASES[name]
    R = ds.reference(N, M, ds.ZERO_LAMBDA, zero)
    be = backend(R)
    try:
        be.set_defer_tail(defer)
        for rep in range(2):                                   # the second one starts from flags a failure has left
            be.upload(0, R.x, R.J)
            be.eval(0)
            lam, r, pnew = be.take_step(0, 1, 2.0 * float(np.sqrt(R.n2gn)), 0.0)
            assert lam == ds.ZERO_LAMBDA and r["kind"] == capi.KIND_GN
            step = be.download(1, capi.VEC_STEP)
            L = ds.unpack_factor(be.factor_dense(N * (N + 1) // 2), N)
            where = f"{name} take_step {'deferred' if defer else 'inline'} {rep}"
            held("factor", ds.check_factor(R, L, R.c), where)
            held("gn", ds.check_gn(R, L, step, R.c), where)
            held("norm2_gn", ds.check_norm2(step, r["n2g"]), where)
            assert np.isfinite(r["ei"]) and r["ei"] > 0.0
    finally:
        be.close()


def _lambda_column(tr):
    return [t["lambda_"] for t in tr.trials()]


@pytest.mark.parametrize("small", [False, True], ids=["trustregion0-default", "trustregion0-small"])
@pytest.mark.parametrize("name", ds.ZERO_SOLVES)
def test_a_whole_solve_behind_a_failed_pivot(gpu, name, small, monkeypatch):
    set_form(monkeypatch, ())
    N, M, _ = ds.ZERO_CASES[name]
    J0, xs, p0 = ds.zero_solve(name)
    cb = ds.dense_cb(J0, xs)
    addr = C.cast(cb, C.c_void_p)
    prm = oa.default_params()
    prm.max_iterations = ds.ZERO_MAX_ITERATIONS
    if small:
        prm.trustregion0 = ds.ZERO_SMALL_TRUSTREGION
    ro, po, tro = oa.oracle_solve("dense", p0, N, M, 0, addr, None, prm)
    rg, pg, trg = capi.optimize("dense", p0, N, M, 0, addr, None, prm)
    want = (ds.ZERO_TRIALS_SMALL if small else ds.ZERO_TRIALS)[name]
    assert [(t["lambda_"], t["step_type"]) for t in tro.trials()] == want
    assert rg >= 0 and _lambda_column(trg) == _lambda_column(tro)
    compare_traces(trg, tro, step_tol=1e-9)
    assert np.max(np.abs(pg - po)) <= 1e-9


@pytest.mark.parametrize("packed", [True, False], ids=["packed-upper", "unpacked"])
@pytest.mark.parametrize("N,k", ds.NEG_CASES)
def test_several_failed_pivots_in_a_row(gpu, N, k, packed, monkeypatch):
    """a negative pivot of -3e-8: lambda = 0, 1e-10, 1e-9 and 1e-8 all fail inside k_potrf_tiles before 1e-7 factorises"""
    set_form(monkeypatch, ())
    cb, H = ds.neg_products(N, k, packed)
    addr = C.cast(cb, C.c_void_p)
    prm = oa.default_params()
    prm.max_iterations = ds.ZERO_MAX_ITERATIONS
    prm.JtJ_packed = prm.JtJ_upper = packed
    ro, po, tro = oa.oracle_solve("products", np.zeros(N), N, 0, 0, addr, None, prm)
    rg, pg, trg = capi.optimize("products", np.zeros(N), N, 0, 0, addr, None, prm)
    assert _lambda_column(tro) == ds.NEG_LAMBDA_COLUMN
    assert rg >= 0 and _lambda_column(trg) == _lambda_column(tro)
    compare_traces(trg, tro, step_tol=1e-9)
    assert np.max(np.abs(pg - po)) <= 1e-9


# ---------------------------------------------------------------- 5. two devices
def test_a_second_device_then_the_first(gpu, monkeypatch):
    """a function attribute is a property of (function, device): k_syrk_lower<64> gets its 73 728 B of dynamic LDS on the
    device of the second backend of the process too"""
    if gpu.dlg_device_count() < 2:
        pytest.skip("one visible device: the dense path on a second device cannot run here")
    set_form(monkeypatch, ())
    N = 257
    M = ds.default_M(N)
    R = ds.reference(N, M, 0.0)
    for device in (1, 0):
        be = backend(R, device=device)
        try:
            be.upload(0, R.x, R.J)
            be.eval(0)
            factor_and_solve(be, R, f"N {N} device {device}")
        finally:
            be.close()
