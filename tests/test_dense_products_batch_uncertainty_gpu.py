"""dogleg_amd_dense_products_batch_uncertainty: Sigma_b = (JtJ + lambda I)^-1 and its diagonal for every problem of a products
batch, against the host reference of tests/test_dense_batch_uncertainty_gpu.py built on the problem's own M[b] rows:
HostProblem.eval(p[b]), the oracle's orc_dense_JtJ_packed_upper + lambda on the diagonal, orc_dpptrf_L / orc_dpptrs_L on
unit columns.  Evaluated at the p and lambda the products solve returned.  Tolerances, that file's:
max |Sigma - ref|_ij / sqrt(Sigma_ii Sigma_jj) <= 1e-9, variances 1e-9 relative.  Nothing of the library under test
computes what is checked."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, BATCH_UNC_FAILED
from tests import batch_oracle as bo
from tests import batch_products_oracle as po
from tests.test_dense_batch_uncertainty_gpu import ref_sigma, COV_TOL, VAR_TOL

pytestmark = pytest.mark.gpu
SET = "default"
EPS, NOISE, SPREAD, _ = po.SETS[SET]
B = po.B_SMALL
OUT_KEYS = ("cov", "var", "lam", "status")
# (N, M or (Mmin, Mmax))
SHAPES = [(3, 12), (8, 33), (17, 41), (32, 200), (16, (20, 96))]


def Ms_of(M, nb=B):
    return po.ragged_M(nb, *M) if isinstance(M, tuple) else np.full(nb, M)


def device_batch(N, Ms, seeds, layout=None):
    from problems.batch import DeviceProductsBatch, LAYOUT_PACKED_UPPER
    return DeviceProductsBatch(len(seeds), Ms, N, seeds=np.asarray(seeds, dtype=np.uint64), eps=EPS, noise=NOISE,
                               p0_spread=SPREAD, layout=LAYOUT_PACKED_UPPER if layout is None else layout)


def solved(N, Ms, seeds, layout=None):
    """(batch, p, lambda) of a products solve"""
    db = device_batch(N, Ms, seeds, layout)
    rc, p, res = capi.optimize_dense_products_batch(db.p0(), N, db.cb, db.cookie, db.set_params(po.params(SET)))
    assert rc == 0 and np.all(res["norm2_x"] >= 0)
    return db, p, np.ascontiguousarray(res["lambda_"])


def unc(db, p, lam, **kw):
    out = capi.dense_products_batch_uncertainty(p, db.N, db.cb, db.cookie, db.set_params(po.params(SET)), lam=lam, **kw)
    assert out["rc"] == 0
    return out


def reference(N, M, seed, p, lam, zero_col=-1):
    hp = bo.HostProblem(int(M), N, int(seed), EPS, NOISE, SPREAD, zero_col)
    x, J = hp.eval(np.ascontiguousarray(p))
    hp.dp.close()
    return ref_sigma(J, lam)


def errors(out, N, Ms, seeds, p, lam, idx=None, zero_col=-1):
    ecov = evar = 0.0
    for b in (range(len(seeds)) if idx is None else idx):
        S = reference(N, Ms[b], seeds[b], p[b], lam[b], zero_col)
        d = np.sqrt(np.diag(S))
        ecov = max(ecov, float(np.max(np.abs(out["cov"][b] - S) / np.outer(d, d))))
        evar = max(evar, float(np.max(np.abs(out["var"][b] - np.diag(S)) / np.diag(S))))
    return ecov, evar


def same_bits(a, b, keys=OUT_KEYS, idx_a=None, idx_b=None):
    for k in keys:
        if a.get(k) is None and b.get(k) is None:
            continue
        x = a[k] if idx_a is None else a[k][idx_a]
        y = b[k] if idx_b is None else b[k][idx_b]
        if np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes():
            return False
    return True


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parity(shape):
    N, M = shape
    seeds, Ms = np.arange(1, 1 + B), Ms_of(M)
    db, p, lam = solved(N, Ms, seeds)
    db.reset_counters()
    out = unc(db, p, lam)
    assert db.ncalls() == 1 and db.nevals() == B              # one callback, every live byte 1
    assert np.all(out["status"] == BATCH_UNC_OK) and np.array_equal(out["lam"], lam) and np.all(lam == 0.0)
    ecov, evar = errors(out, N, Ms, seeds, p, lam)
    print(f"{shape}: {B} problems: Sigma scaled error {ecov:.3g}, variances rel {evar:.3g}")
    assert ecov <= COV_TOL and evar <= VAR_TOL
    # the variances are the diagonal, and each output alone gives the bits of both together
    assert out["var"].tobytes() == np.ascontiguousarray(np.einsum("bii->bi", out["cov"])).tobytes()
    for want in (("cov",), ("var",)):
        part = unc(db, p, lam, want=want)
        assert [k for k in ("cov", "var") if k in part] == list(want)
        assert same_bits(out, part, keys=list(want) + ["lam", "status"]), want
    # lambda == NULL starts at 0 and reports nothing
    nolam = unc(db, p, None)
    assert nolam["lam"] is None and same_bits(out, nolam, keys=("cov", "var", "status"))
    db.close()


def test_the_unpacked_layouts_give_the_same_bits():
    from problems.batch import LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER
    N, M = 17, 41
    seeds, Ms = np.arange(1, 1 + B), Ms_of(M)
    db, p, lam = solved(N, Ms, seeds)
    base = unc(db, p, lam)
    for layout in (LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        db.set_layout(layout)
        assert same_bits(base, unc(db, p, lam)), layout
    db.close()


def test_lambda_loop_on_a_zero_column():
    from problems.batch import MODE_ZERO_COLUMN
    N, M, c, nb, chosen = 24, 73, 17, 32, [3, 17, 30]
    seeds, Ms = np.arange(1, 1 + nb), Ms_of(M, 32)
    db, p, _ = solved(N, Ms, seeds)
    lam0 = np.zeros(nb)
    plain = unc(db, p, lam0)
    mode = np.zeros(nb, dtype=np.uint8)
    mode[chosen] = MODE_ZERO_COLUMN
    db.set_mode(mode, c)
    out = unc(db, p, lam0)
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK)
    others = [b for b in range(nb) if b not in chosen]
    assert np.all(out["lam"][others] == 0.0) and same_bits(plain, out, idx_a=others, idx_b=others)
    for b in chosen:
        lam, var, cov = out["lam"][b], out["var"][b], out["cov"][b]
        print(f"problem {b}: lambda {lam:g}, variance of the zero column {var[c]:.6g}")
        assert lam == 1e-10
        assert np.allclose(var[c], 1.0 / lam, rtol=1e-9, atol=0)
        off = [j for j in range(N) if j != c]
        assert np.all(np.abs(cov[c, off]) <= 1e-12 * np.sqrt(var[c] * var[off]))
        assert np.all(np.abs(cov[off, c]) <= 1e-12 * np.sqrt(var[c] * var[off]))
    # and the whole of those problems against the host at the lambda that was used (the bound of
    # tests/test_dense_batch_uncertainty_gpu.py::check_lambda_loop_on_a_zero_column: Sigma only, COV_TOL)
    ecov = 0.0
    for b in chosen:
        S = reference(N, M, seeds[b], p[b], out["lam"][b], zero_col=c)
        d = np.sqrt(np.diag(S))
        ecov = max(ecov, float(np.max(np.abs(out["cov"][b] - S) / np.outer(d, d))))
    print(f"zero-column problems {chosen}: Sigma scaled error {ecov:.3g}")
    assert ecov <= COV_TOL


def test_a_negative_or_nan_lambda_fails_that_problem_alone():
    N, M, nb = 8, 33, 16
    db, p, lam = solved(N, Ms_of(M, nb), np.arange(1, 1 + nb))
    plain = unc(db, p, lam)
    bad_lam = lam.copy()
    bad_lam[2], bad_lam[9] = -1.0, np.nan
    out = unc(db, p, bad_lam)
    db.close()
    bad = [2, 9]
    good = [b for b in range(nb) if b not in bad]
    assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
    assert out["lam"][2] == -1.0 and np.isnan(out["lam"][9])
    for k in ("cov", "var"):
        assert np.all(np.isnan(out[k][bad])), k
    assert same_bits(plain, out, idx_a=good, idx_b=good)


@pytest.mark.parametrize("mode_name", ["MODE_NAN", "MODE_NAN_OFFDIAGONAL"])
def test_a_failing_problem_fails_alone(mode_name):
    from problems import batch
    N, M, nb = 8, 33, 32
    db, p, lam = solved(N, Ms_of(M, nb), np.arange(1, 1 + nb))
    plain = unc(db, p, lam)
    bad = [1, 5, 31]
    mode = np.zeros(nb, dtype=np.uint8)
    mode[bad] = getattr(batch, mode_name)
    db.set_mode(mode)
    out = unc(db, p, lam)
    db.close()
    good = [b for b in range(nb) if b not in bad]
    assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
    for k in ("cov", "var"):
        assert np.all(np.isnan(out[k][bad])), k
    assert same_bits(plain, out, idx_a=good, idx_b=good)


def test_neighbours_and_the_batch_size_do_not_matter():
    N, M = 17, 41
    seeds, Ms = np.arange(1, 1 + B), Ms_of(M)
    db, p, lam = solved(N, Ms, seeds)
    base = unc(db, p, lam)
    stats = {B: capi.batch_uncertainty_last_stats()}
    db.close()
    for b in (0, 33, B - 1):
        db1 = device_batch(N, Ms[b:b + 1], seeds[b:b + 1])
        one = unc(db1, p[b:b + 1], lam[b:b + 1])
        stats[1] = capi.batch_uncertainty_last_stats()
        db1.close()
        assert same_bits(base, one, idx_a=slice(b, b + 1))
    # launches, synchronisations and copies do not depend on B
    print(stats)
    key = lambda s: (s["launches"], s["syncs"], s["copies"])
    assert key(stats[1]) == key(stats[B]) and stats[1]["launches"] == 1 and stats[1]["syncs"] == 1
