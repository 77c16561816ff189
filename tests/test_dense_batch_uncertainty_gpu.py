"""dogleg_amd_dense_batch_uncertainty: Sigma_b = (JtJ + lambda I)^-1, its diagonal and the outlierness factors of every
problem of a batch, against values computed on the host for each problem from HostProblem.eval(p[b]) at the very p[b] handed
to the call: Sigma from the oracle's orc_dense_JtJ_packed_upper + lambda on the diagonal + orc_dpptrf_L / orc_dpptrs_L on
unit columns (the recipe of tests/test_outliers_gpu.py::test_dense_leverage_matches_oracle), the factors from a numpy
restatement of the formulas in include/dogleg.h.  Nothing of the library under test computes what is checked.

Tolerances (those of the single-problem entry points): max |Sigma - ref|_ij / sqrt(Sigma_ii Sigma_jj) <= 1e-9, variances
1e-9 relative, factors rtol 1e-9 / atol 1e-12 where the reference value is not DBL_MAX, a computed scale 1e-12 relative.
For the parity cases two independent host computations (LAPACK inverse, the oracle's packed Cholesky) agree to 2e-15
scaled on Sigma and 3.5e-14 on the factors; cond(JtJ) <= 51, the largest leverage is 0.79, lambda is 0 throughout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, BATCH_UNC_FAILED, dptr
from tests import oracle_api as oa
from tests import batch_oracle as bo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
COV_TOL, VAR_TOL, SCALE_TOL = 1e-9, 1e-9, 1e-12
FAC_RTOL, FAC_ATOL = 1e-9, 1e-12
SHAPES = [(3, 12), (6, 40), (16, 96), (32, 200), (32, 64)]
OUT_KEYS = ("cov", "var", "factors", "scale", "lam", "status")


# ---------------------------------------------------------------- the batch and the host reference
def device_batch(N, M, seeds):
    from problems.batch import DeviceBatch
    return DeviceBatch(len(seeds), M, N, seeds=np.asarray(seeds, dtype=np.uint64), eps=EPS, noise=NOISE, p0_spread=SPREAD)


def solved(N, M, seeds):
    """(DeviceBatch, p, lambda) of a batch solve with the default parameters"""
    db = device_batch(N, M, seeds)
    rc, p, res = capi.optimize_dense_batch(db.p0(), N, M, db.cb, db.cookie, oa.default_params())
    assert rc == 0 and np.all(res["norm2_x"] >= 0)
    return db, p, np.ascontiguousarray(res["lambda_"])


def ref_sigma(J, lam):
    M, N = J.shape
    O = oa.oracle()
    ap = np.zeros(N * (N + 1) // 2)
    O.orc_dense_JtJ_packed_upper(dptr(ap), dptr(np.ascontiguousarray(J)), M, N)
    ap[np.cumsum(np.r_[0, np.arange(N, 1, -1)])] += lam          # diagonal of the row-major packed upper triangle
    assert O.orc_dpptrf_L(N, dptr(ap)) == 0
    S = np.zeros((N, N))
    for c in range(N):
        e = np.zeros(N)
        e[c] = 1.0
        O.orc_dpptrs_L(N, dptr(ap), dptr(e))
        S[:, c] = e
    return S


def ref_scale(M, N, norm2_x):
    return M / (4.0 * ((N + 1) * norm2_x / (M - N - 1)))


def ref_factors(S, x, J, fs, scale):
    """include/dogleg.h above dogleg_getOutliernessFactors, A_f = J_f Sigma J_f^T"""
    k = scale / 8.0
    out = np.zeros(len(x) // fs)
    for f in range(len(out)):
        Jf, xf = J[f * fs:(f + 1) * fs], x[f * fs:(f + 1) * fs]
        A = Jf @ S @ Jf.T
        if fs == 1:
            den = 1.0 - A[0, 0]
            out[f] = DBL_MAX if abs(den) < 1e-8 else xf[0] * xf[0] / den * k
        else:
            Mx = A - np.eye(2)
            if abs(np.linalg.det(Mx)) < 1e-8:
                out[f] = DBL_MAX
            else:
                Bm = np.linalg.inv(Mx)
                out[f] = float(xf @ (Bm + Bm @ Bm) @ xf) * k
    return out


def reference(N, M, seed, p, lam, zero_col=-1):
    """(x, J, Sigma) of one problem on the host at p"""
    hp = bo.HostProblem(M, N, int(seed), EPS, NOISE, SPREAD, zero_col)
    x, J = hp.eval(np.ascontiguousarray(p))
    hp.dp.close()
    return x, J, ref_sigma(J, lam)


def check_against_reference(out, N, M, seeds, p, lam, fs, what, scale_given=None):
    """every problem of `out` against the host; prints the figures, then asserts"""
    ecov = evar = efac = esc = 0.0
    nmax = 0
    fac_ok = True
    for b, s in enumerate(seeds):
        x, J, S = reference(N, M, s, p[b], lam[b])
        d = np.sqrt(np.diag(S))
        ecov = max(ecov, float(np.max(np.abs(out["cov"][b] - S) / np.outer(d, d))))
        evar = max(evar, float(np.max(np.abs(out["var"][b] - np.diag(S)) / np.diag(S))))
        sc = ref_scale(M, N, float(x @ x)) if scale_given is None else scale_given
        esc = max(esc, abs(out["scale"][b] - sc) / sc)
        want = ref_factors(S, x, J, fs, sc)
        got = out["factors"][b]
        big = want == DBL_MAX
        nmax += int(big.sum())
        fac_ok = fac_ok and bool(np.all(got[big] == DBL_MAX)) and bool(np.allclose(got[~big], want[~big], rtol=FAC_RTOL, atol=FAC_ATOL))
        if np.any(~big):
            efac = max(efac, float(np.max(np.abs(got[~big] - want[~big]) / np.maximum(np.abs(want[~big]), FAC_ATOL / FAC_RTOL))))
    print(f"{what}: {len(seeds)} problems: Sigma scaled error {ecov:.3g}, variances rel {evar:.3g}, factors rel {efac:.3g} "
          f"({nmax} DBL_MAX in the reference), scale rel {esc:.3g}")
    assert ecov <= COV_TOL and evar <= VAR_TOL and esc <= SCALE_TOL and fac_ok
    return nmax


def same_bits(a, b, keys=OUT_KEYS, idx_a=None, idx_b=None):
    for k in keys:
        if k not in a and k not in b:
            continue
        x = a[k] if idx_a is None else a[k][idx_a]
        y = b[k] if idx_b is None else b[k][idx_b]
        if np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():
            return False
    return True


def unc(db, p, lam, **kw):
    out = capi.dense_batch_uncertainty(p, db.N, db.M, db.cb, db.cookie, lam=lam, **kw)
    assert out["rc"] == 0
    return out


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity(shape, fs):
    N, M = shape
    seeds = np.arange(1, 65)
    db, p, lam = solved(N, M, seeds)
    out = unc(db, p, lam, fs=fs)
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK) and np.array_equal(out["lam"], lam) and np.all(lam == 0.0)
    assert out["factors"].shape == (64, M // fs)
    nmax = check_against_reference(out, N, M, seeds, p, lam, fs, f"{shape} fs {fs}")
    assert nmax == 0


# ---------------------------------------------------------------- 2. subsets and repetition
def test_variances_are_the_diagonal_and_subsets_give_the_same_bits():
    N, M = 16, 96
    db, p, lam = solved(N, M, np.arange(1, 65))
    full = unc(db, p, lam, fs=2)
    assert np.array_equal(full["var"], np.einsum("bii->bi", full["cov"]))
    assert full["var"].tobytes() == np.ascontiguousarray(np.einsum("bii->bi", full["cov"])).tobytes()
    again = unc(db, p, lam, fs=2)
    assert same_bits(full, again)
    for want in (("cov",), ("var",), ("factors",), ("cov", "var"), ("var", "factors"), ("cov", "factors")):
        part = unc(db, p, lam, fs=2, want=want)
        keys = list(want) + (["scale"] if "factors" in want else []) + ["lam", "status"]
        assert [k for k in ("cov", "var", "factors") if k in part] == [k for k in ("cov", "var", "factors") if k in want]
        assert same_bits(full, part, keys=keys), want
    # lambda == NULL starts at 0 and reports nothing: the same numbers here, where lambda is 0
    nolam = unc(db, p, None, fs=2)
    assert nolam["lam"] is None and same_bits(full, nolam, keys=("cov", "var", "factors", "scale", "status"))
    db.close()


# ---------------------------------------------------------------- 3. position independence
def test_position_and_neighbours_do_not_matter():
    N, M = 6, 40
    seeds = np.arange(1, 65)
    db, p, lam = solved(N, M, seeds)
    base = unc(db, p, lam, fs=2)
    db.close()
    big_seeds = np.arange(1001, 2001)
    pos = np.random.default_rng(9).permutation(1000)[:64]
    big_seeds[pos] = seeds
    dbb, pb, lamb = solved(N, M, big_seeds)
    assert pb[pos].tobytes() == p.tobytes() and lamb[pos].tobytes() == lam.tobytes()
    big = unc(dbb, pb, lamb, fs=2)
    dbb.close()
    assert same_bits(base, big, idx_b=pos)
    for b in range(64):
        db1 = device_batch(N, M, seeds[b:b + 1])
        one = unc(db1, p[b:b + 1], lam[b:b + 1], fs=2)
        db1.close()
        assert same_bits(base, one, idx_a=slice(b, b + 1))


# ---------------------------------------------------------------- 4. one callback, launches constant in B
def test_one_callback_and_constant_launches():
    N, M = 6, 40
    stats = {}
    for B in (1, 64, 4096):
        db, p, lam = solved(N, M, np.arange(1, 1 + B))
        db.reset_counters()
        out = unc(db, p, lam, fs=1)
        assert db.ncalls() == 1 and db.nevals() == B
        assert np.all(out["status"] == BATCH_UNC_OK)
        s = capi.batch_uncertainty_last_stats()
        stats[B] = (s["launches"], s["syncs"], s["copies"])
        db.close()
    print(stats)
    assert len(set(stats.values())) == 1 and stats[1][0] == 1 and stats[1][1] == 1


# ---------------------------------------------------------------- 5. the lambda loop
def test_lambda_loop_on_a_zero_column():
    check_lambda_loop_on_a_zero_column(6, 40, 2)


def check_lambda_loop_on_a_zero_column(N, M, c, B=32, chosen=(3, 17, 30)):
    from problems.batch import MODE_ZERO_COLUMN
    chosen = list(chosen)
    seeds = np.arange(1, 1 + B)
    db, p, _ = solved(N, M, seeds)
    lam0 = np.zeros(B)
    plain = unc(db, p, lam0, fs=1)
    mode = np.zeros(B, dtype=np.uint8)
    mode[chosen] = MODE_ZERO_COLUMN
    db.set_mode(mode, c)
    out = unc(db, p, lam0, fs=1)
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK)
    others = [b for b in range(B) if b not in chosen]
    assert np.all(out["lam"][others] == 0.0) and same_bits(plain, out, idx_a=others, idx_b=others)
    for b in chosen:
        lam = out["lam"][b]
        var, cov = out["var"][b], out["cov"][b]
        print(f"problem {b}: lambda {lam:g}, variance of the zero column {var[c]:.6g}")
        assert lam == 1e-10
        assert np.allclose(var[c], 1.0 / lam, rtol=1e-9, atol=0)
        off = [j for j in range(N) if j != c]
        assert np.all(np.abs(cov[c, off]) <= 1e-12 * np.sqrt(var[c] * var[off]))
        assert np.all(np.abs(cov[off, c]) <= 1e-12 * np.sqrt(var[c] * var[off]))
    # and the whole of those problems against the host at the lambda that was used
    sel = np.array(chosen)
    ecov = 0.0
    for b in chosen:
        x, J, S = reference(N, M, seeds[b], p[b], out["lam"][b], zero_col=c)
        d = np.sqrt(np.diag(S))
        ecov = max(ecov, float(np.max(np.abs(out["cov"][b] - S) / np.outer(d, d))))
    print(f"zero-column problems {sel}: Sigma scaled error {ecov:.3g}")
    assert ecov <= COV_TOL


# ---------------------------------------------------------------- 6. DBL_MAX
def test_square_problems_give_dbl_max():
    N = M = 6
    db, p, _ = solved(N, M, np.arange(1, 33))
    for fs in (1, 2):
        out = unc(db, p, None, fs=fs, scale=1.0)
        assert np.all(out["status"] == BATCH_UNC_OK) and np.all(out["scale"] == 1.0)
        assert out["factors"].shape == (32, M // fs) and np.all(out["factors"] == DBL_MAX)
    # a scale to be computed needs Nmeas > Nstate + 1
    db.reset_counters()
    out = capi.dense_batch_uncertainty(p, N, M, db.cb, db.cookie, fs=1)
    assert out["rc"] == -1 and db.ncalls() == 0
    assert not out["cov"].any() and not out["var"].any() and not out["factors"].any() and np.all(out["scale"] == -1.0)
    db.close()


# ---------------------------------------------------------------- 7. failure isolation
def test_a_failing_problem_fails_alone():
    from problems.batch import MODE_NAN
    N, M, B = 6, 40, 64
    db, p, lam = solved(N, M, np.arange(1, 1 + B))
    plain = unc(db, p, lam, fs=2)
    bad = [1, 5, 63]
    mode = np.zeros(B, dtype=np.uint8)
    mode[bad] = MODE_NAN
    db.set_mode(mode)
    out = unc(db, p, lam, fs=2)            # (unc asserts rc == 0)
    db.close()
    good = [b for b in range(B) if b not in bad]
    assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
    for k in ("cov", "var", "factors"):
        assert np.all(np.isnan(out[k][bad])), k
    assert same_bits(plain, out, idx_a=good, idx_b=good)


def test_a_negative_or_nan_lambda_fails_that_problem_alone():
    N, M, B = 6, 40, 16
    db, p, lam = solved(N, M, np.arange(1, 1 + B))
    plain = unc(db, p, lam, fs=1)
    bad_lam = lam.copy()
    bad_lam[2], bad_lam[9] = -1.0, np.nan
    out = unc(db, p, bad_lam, fs=1)
    db.close()
    bad = [2, 9]
    good = [b for b in range(B) if b not in bad]
    assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
    assert out["lam"][2] == -1.0 and np.isnan(out["lam"][9])
    for k in ("cov", "var", "factors"):
        assert np.all(np.isnan(out[k][bad])), k
    assert same_bits(plain, out, idx_a=good, idx_b=good)


# ---------------------------------------------------------------- 8. the single-problem route
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bunc") / "batch_uncertainty_harness")
    cmd = ["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "batch_uncertainty_harness.c"), "-o", exe,
           "-L", os.path.join(ROOT, "libdogleg_amd"), "-ldogleg_amd",
           "-L", os.path.join(ROOT, "problems"), "-lproblems", "-lm",
           "-Wl,-rpath," + os.path.join(ROOT, "libdogleg_amd"), "-Wl,-rpath," + os.path.join(ROOT, "problems")]
    subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("fs", [1, 2])
def test_against_the_single_problem_route(harness, fs):
    N, M, B = 6, 40, 8
    seeds = np.arange(1, 1 + B)
    db, p, lam = solved(N, M, seeds)
    out = unc(db, p, lam, fs=fs)
    db.close()
    evar = efac = esc = 0.0
    for b in range(B):
        r = subprocess.run([harness, str(M), str(N), str(seeds[b]), repr(EPS), repr(NOISE), repr(SPREAD), str(fs)]
                           + [float(v).hex() for v in p[b]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        o = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines() if ln.strip()}
        assert o.get("alive") == ["1"] and o["rc_var"] == ["0"] and o["ok"] == ["1"]
        f = lambda key: np.array([float.fromhex(v) for v in o[key]])
        assert np.array_equal(f("p"), p[b]), "the single-problem solve moved away from p[b]"
        assert f("lambda")[0] == lam[b]
        evar = max(evar, float(np.max(np.abs(out["var"][b] - f("var")) / f("var"))))
        esc = max(esc, abs(out["scale"][b] - f("scale")[0]) / f("scale")[0])
        want = f("factors")
        assert np.all(want != DBL_MAX)
        efac = max(efac, float(np.max(np.abs(out["factors"][b] - want) / np.maximum(np.abs(want), FAC_ATOL / FAC_RTOL))))
        assert np.allclose(out["factors"][b], want, rtol=FAC_RTOL, atol=FAC_ATOL)
    print(f"fs {fs}: against dogleg_optimize_dense2 + marginal variances + outlierness factors: variances rel {evar:.3g}, "
          f"scale rel {esc:.3g}, factors rel {efac:.3g}")
    assert evar <= VAR_TOL and esc <= SCALE_TOL


# ---------------------------------------------------------------- refusals with a device present
def test_refusals_on_the_gpu():
    N, M = 6, 40
    db, p, lam = solved(N, M, np.arange(1, 3))
    db.reset_counters()
    assert capi.dense_batch_uncertainty(p, N, M, db.cb, db.cookie, lam=lam, fs=3)["rc"] == -1
    assert capi.dense_batch_uncertainty(p, N, M, db.cb, db.cookie, lam=lam, want=())["rc"] == -1
    L = capi.lib()
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert capi.dense_batch_uncertainty(p, N, M, db.cb, db.cookie, lam=lam)["rc"] == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert db.ncalls() == 0
    out = unc(db, p, lam)
    assert np.all(out["status"] == BATCH_UNC_OK) and db.ncalls() == 1
    L.dogleg_amd_release_cache()
    again = unc(db, p, lam)
    assert same_bits(out, again)
    db.close()
