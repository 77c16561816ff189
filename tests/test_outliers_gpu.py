"""The outlier API (reference dogleg.h:331-392, dogleg.c:2294-3149) and the leverage blocks behind it.

dlg_feature_leverage (A_f = J_f inv(JtJ + lambda I) J_f^T from the forward solves of the factor held on the device) is
checked against independent solves with the ORACLE's factor (orc_sparse_solve, orc_dpptrs_L) and against the full
solves of dlg_pseudoinverse_chunk; the public entry points, driven from C by tests/c/outlier_harness.c, against a numpy
restatement of the formulas on the point the solve left behind."""
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import dptr, iptr
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max


# ---------------------------------------------------------------- numpy restatements
def _packed(A, fs):
    return np.array([A[0, 0]]) if fs == 1 else np.array([A[0, 0], A[0, 1], A[1, 1]])


def _factor(Ap, x, fs, scale):
    k = scale / 8.0
    if fs == 1:
        den = 1.0 - Ap[0]
        return DBL_MAX if abs(den) < 1e-8 else x[0] * x[0] / den * k
    M = np.array([[Ap[0] - 1.0, Ap[1]], [Ap[1], Ap[2] - 1.0]])
    if abs(np.linalg.det(M)) < 1e-8:
        return DBL_MAX
    B = np.linalg.inv(M)
    return float(x @ (B + B @ B) @ x) * k


def _scale(M, N, nout, fs, norm2_x):
    nn = M - nout * fs
    return nn / (4.0 * ((N + 1) * norm2_x / (nn - N - 1)))


def _dense_J(Jp, Ji, Jx, M, N):
    J = np.zeros((M, N))
    for r in range(M):
        J[r, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
    return J


def _oracle_leverage_sparse(prob, Jp, Ji, Jx, lam, fs, feats):
    O = oa.oracle()
    F = O.orc_sparse_analyze(prob.N, prob.M, iptr(Jp), iptr(Ji))
    assert O.orc_sparse_factorize(F, iptr(Jp), iptr(Ji), dptr(Jx), lam) == prob.N
    out = []
    for f in feats:
        rows = np.zeros((fs, prob.N))
        for a in range(fs):
            r = f * fs + a
            rows[a, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
        sol = np.zeros_like(rows)
        for a in range(fs):
            O.orc_sparse_solve(F, dptr(np.ascontiguousarray(rows[a])), dptr(sol[a]))
        out.append(_packed(rows @ sol.T, fs))
    O.orc_sparse_free(F)
    return np.array(out)


def _sparse_backend(prob, lam):
    p = prob.p0()
    x, Jx = prob.eval(p)
    Jp, Ji = prob.pattern()
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_pattern(Jp, Ji)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    assert be.factorize(0, lam)
    return be, x, Jp, Ji, Jx


def _as2d(A, fs):
    return np.asarray(A).reshape(-1, 1 if fs == 1 else 3)


# ---------------------------------------------------------------- C-ABI: leverage blocks
@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("shape,nsample", [((5, 40, 300), None), ((49, 900, 10000), 200), ((199, 3600, 40000), 200)],
                         ids=["tiny", "medium", "large"])
def test_sparse_leverage_matches_oracle(gpu, shape, nsample, lam, fs):
    prob = oa.BAProblem(*shape, seed=11)
    be, x, Jp, Ji, Jx = _sparse_backend(prob, lam)
    nf = prob.M // fs
    A = _as2d(be.feature_leverage(0, fs, 0, nf), fs)
    feats = np.arange(nf) if nsample is None else np.sort(np.random.default_rng(7).choice(nf, nsample, replace=False))
    ref = _oracle_leverage_sparse(prob, Jp, Ji, Jx, lam, fs, feats)
    err = np.max(np.abs(A[feats] - ref))
    print(f"{shape} lambda={lam} fs={fs}: max |A - oracle| = {err:.2e} over {len(feats)} features")
    assert err <= 1e-10
    assert np.all(A[:, 0] >= -1e-12) and np.all(A[:, -1] <= 1.0 + 1e-12)
    # the same blocks from the full solves of dlg_pseudoinverse_chunk
    for f in feats[:24]:
        U = be.pseudoinverse_chunk(0, f * fs, (f + 1) * fs)
        J_f = _dense_J(Jp[f * fs:(f + 1) * fs + 1] - Jp[f * fs], Ji[Jp[f * fs]:Jp[(f + 1) * fs]],
                       Jx[Jp[f * fs]:Jp[(f + 1) * fs]], fs, prob.N)
        assert np.max(np.abs(_packed(J_f @ U.T, fs) - A[f])) <= 1e-10
    # a sub-range is the same numbers
    f0 = nf // 3
    assert np.array_equal(_as2d(be.feature_leverage(0, fs, f0, 5), fs), A[f0:f0 + 5])
    be.close()


def test_sparse_leverage_reproducible_and_equal_to_full_sweep(gpu, monkeypatch):
    prob = oa.BAProblem(49, 900, 10000, seed=5)
    be, *_ = _sparse_backend(prob, 0.0)
    nf = prob.M // 2
    A1 = be.feature_leverage(0, 2, 0, nf)
    A2 = be.feature_leverage(0, 2, 0, nf)
    assert np.array_equal(A1, A2), "two calls differ"
    nch, visits, nsn = be.leverage_stats(2)
    assert nch == (nf + 7) // 8 and 0 < visits < nch * nsn
    print(f"reach: {visits / nch:.1f} of {nsn} supernodes per chunk")
    monkeypatch.setenv("DOGLEG_AMD_LEVERAGE_SWEEP", "1")
    A3 = be.feature_leverage(0, 2, 0, nf)
    monkeypatch.delenv("DOGLEG_AMD_LEVERAGE_SWEEP")
    err = np.max(np.abs(A1 - A3))
    print(f"reach-restricted against the full sweep: {err:.2e}")
    assert err <= 1e-12
    be.close()


def test_config3_sample_matches_oracle(gpu):
    """config #3 at full size: 256 random observations against the oracle"""
    prob = oa.BAProblem(499, 9000, 100000, seed=1)
    be, x, Jp, Ji, Jx = _sparse_backend(prob, 0.0)
    nf = prob.M // 2
    A = be.feature_leverage(0, 2, 0, nf)
    feats = np.sort(np.random.default_rng(3).choice(nf, 256, replace=False))
    ref = _oracle_leverage_sparse(prob, Jp, Ji, Jx, 0.0, 2, feats)
    err = np.max(np.abs(A[feats] - ref))
    print(f"config #3: max |A - oracle| = {err:.2e}")
    assert err <= 1e-10
    be.close()


@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_dense_leverage_matches_oracle(gpu, fs, lam):
    dp = oa.DenseProblem(M=1201, N=150, seed=2)
    p = dp.p0()
    x, J = dp.eval(p)
    be = capi.Backend(capi.DLG_DENSE, dp.N, dp.M)
    be.set_p(0, p)
    be.upload(0, x, J)
    be.eval(0)
    assert be.factorize(0, lam)
    nf = dp.M // fs
    A = _as2d(be.feature_leverage(0, fs, 0, nf), fs)
    O = oa.oracle()
    ap = np.zeros(dp.N * (dp.N + 1) // 2)
    O.orc_dense_JtJ_packed_upper(dptr(ap), dptr(J), dp.M, dp.N)
    ap[np.cumsum(np.r_[0, np.arange(dp.N, 1, -1)])] += lam          # diagonal of the row-major packed upper triangle
    assert O.orc_dpptrf_L(dp.N, dptr(ap)) == 0
    feats = np.arange(0, nf, 7)
    ref = []
    for f in feats:
        rows = J[f * fs:(f + 1) * fs].copy()
        sol = rows.copy()
        for a in range(fs):
            O.orc_dpptrs_L(dp.N, dptr(ap), dptr(sol[a]))
        ref.append(_packed(rows @ sol.T, fs))
    err = np.max(np.abs(A[feats] - np.array(ref)))
    print(f"dense fs={fs} lambda={lam}: max |A - oracle| = {err:.2e}")
    assert err <= 1e-10
    assert np.array_equal(A, _as2d(be.feature_leverage(0, fs, 0, nf), fs))
    be.close()


def _lonely_problem():
    """a random sparse J in which state N-1 is touched by measurement 5 alone: its leverage is 1 at lambda = 0"""
    rng = np.random.default_rng(4)
    N, M = 40, 200
    rows = []
    for r in range(M):
        cols = np.sort(rng.choice(N - 1, 6, replace=False))
        if r == 5:
            cols = np.r_[cols, N - 1]
        rows.append(cols.astype(np.int32))
    Jp = np.zeros(M + 1, dtype=np.int32)
    Jp[1:] = np.cumsum([len(c) for c in rows])
    Ji = np.concatenate(rows).astype(np.int32)
    Jx = rng.standard_normal(len(Ji))
    x = rng.standard_normal(M)
    return N, M, Jp, Ji, Jx, x


@pytest.mark.parametrize("fs", [1, 2])
def test_factors_capi_and_dbl_max(gpu, fs):
    N, M, Jp, Ji, Jx, x = _lonely_problem()
    be = capi.Backend(capi.DLG_SPARSE, N, M, len(Ji))
    be.set_pattern(Jp, Ji)
    be.set_p(0, np.zeros(N))
    be.upload(0, x, Jx)
    be.eval(0)
    assert be.factorize(0, 0.0)
    nf = M // fs
    J = _dense_J(Jp, Ji, Jx, M, N)
    H = J.T @ J
    A = _as2d(be.feature_leverage(0, fs, 0, nf), fs)
    ref = np.array([_packed(J[f * fs:(f + 1) * fs] @ np.linalg.solve(H, J[f * fs:(f + 1) * fs].T), fs) for f in range(nf)])
    assert np.max(np.abs(A - ref)) <= 1e-10
    scale = 0.37
    fac = be.outlierness_factors(0, fs, nf, scale)
    want = np.array([_factor(A[f], x[f * fs:(f + 1) * fs], fs, scale) for f in range(nf)])
    lonely = 5 // fs
    assert fac[lonely] == DBL_MAX, fac[lonely]
    ok = want != DBL_MAX
    assert np.all(fac[~ok] == DBL_MAX)
    assert np.allclose(fac[ok], want[ok], rtol=1e-9, atol=1e-12)
    be.close()


def test_refusals_capi(gpu):
    prob = oa.BAProblem(5, 40, 300, seed=11)
    be, *_ = _sparse_backend(prob, 0.0)
    with pytest.raises(capi.DlgError):
        be.feature_leverage(0, 3, 0, 4)
    with pytest.raises(capi.DlgError):
        be.feature_leverage(1, 2, 0, 4)               # slot 1 holds no factor (and no inputs)
    with pytest.raises(capi.DlgError):
        be.feature_leverage(0, 2, 0, prob.M)          # more rows than there are
    be.close()


# ---------------------------------------------------------------- the public API from C
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("outl") / "outlier_harness")
    cmd = ["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "outlier_harness.c"), "-o", exe,
           "-L", os.path.join(ROOT, "libdogleg_amd"), "-ldogleg_amd",
           "-L", os.path.join(ROOT, "problems"), "-lproblems", "-lm",
           "-Wl,-rpath," + os.path.join(ROOT, "libdogleg_amd"), "-Wl,-rpath," + os.path.join(ROOT, "problems")]
    subprocess.run(cmd, check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    out = {}
    for line in r.stdout.splitlines():
        if line.strip():
            k, *v = line.split()
            out[k] = v
    assert out.get("alive") == ["1"]
    return out, r.stderr


def _f(vals):
    return np.array([float.fromhex(v) for v in vals])


def _point(out):
    N, M, nnz = map(int, out["dims"])
    Jp = np.array(out["Jt_p"], dtype=np.int32)
    Ji = np.array(out["Jt_i"], dtype=np.int32)
    J = _dense_J(Jp, Ji, _f(out["Jt_x_vals"]), M, N)
    lam = _f(out["lambda"])[0]
    return N, M, J, _f(out["x"]), _f(out["norm2_x"])[0], lam


def _np_factors(out, fs, nout, scale):
    N, M, J, x, n2, lam = _point(out)
    H = J.T @ J + lam * np.eye(N)
    nf = M // fs
    if scale <= 0:
        scale = _scale(M, N, nout, fs, n2)
    fac = []
    for f in range(nf):
        Jf = J[f * fs:(f + 1) * fs]
        fac.append(_factor(_packed(Jf @ np.linalg.solve(H, Jf.T), fs), x[f * fs:(f + 1) * fs], fs, scale))
    return np.array(fac), scale


@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("nout,scale_in", [(0, -1.0), (3, -1.0), (0, 0.37)])
def test_factors_and_scale(gpu, harness, fs, nout, scale_in):
    out, _ = _run(harness, "factors", fs, nout, scale_in)
    assert out["ok"] == ["1"] and out["repeat_same"] == ["1"]
    got, scale = _f(out["factors"]), _f(out["scale"])[0]
    want, wscale = _np_factors(out, fs, nout, scale_in)
    if scale_in > 0:
        assert scale == scale_in
    else:
        assert abs(scale - wscale) <= np.spacing(wscale), (scale, wscale)
    assert np.allclose(got, want, rtol=1e-8, atol=1e-12)
    # with the scale computed, the corrupted measurements (7, 40, 81) stand out
    if scale_in <= 0:
        for r in (7, 40, 81):
            assert got[r // fs] >= 1.0, (r, got[r // fs])
    print(f"fs={fs} nout={nout}: scale {scale:.6g}, {np.sum(got >= 1)} of {len(got)} factors >= 1")


def _candidates(factors, premarked):
    return [i for i in range(len(factors)) if i not in premarked and factors[i] >= 1.0]


def test_mark_outliers(gpu, harness):
    # which features are candidates (factor >= 1): from a first run that chooses none
    out, _ = _run(harness, "mark", 2, "-", "-", -1)
    fac = _f(out["factors"])
    cand = _candidates(fac, set())
    assert len(cand) >= 3, cand
    assert out["ret"] == ["0"] and out["noutliers"] == ["0"] and out["marked"] == []
    assert int(out["calls"][0]) == 1 + len(cand)
    # two candidates and one feature that is no candidate are "cheap"; feature 0 was marked before
    chosen = [cand[0], cand[-1]] + [i for i in range(len(fac)) if i not in cand and i != 0][:1]
    pre = [0] if 0 not in cand else [1]
    out, _ = _run(harness, "mark", 2, ",".join(map(str, chosen)), ",".join(map(str, pre)), -1)
    fac = _f(out["factors"])
    cand = _candidates(fac, set(pre))
    want_marked = sorted(set(pre) | {c for c in chosen if c in cand})
    assert [int(v) for v in out["marked"]] == want_marked
    assert int(out["noutliers"][0]) == len(want_marked)
    assert out["ret"] == ["1"]
    assert int(out["calls"][0]) == 1 + len(cand)


def test_mark_outliers_early_exits(gpu, harness):
    # the initial confidence is negative: false, nothing counted, one call
    out, _ = _run(harness, "mark", 2, "-", "2", -2)
    assert out["ret"] == ["0"] and out["noutliers"] == ["1"] and out["calls"] == ["1"]
    # a candidate's confidence is negative: false at once, the count so far
    out, _ = _run(harness, "mark", 2, "-", "-", -1)
    cand = _candidates(_f(out["factors"]), set())
    stop = cand[1]
    chosen = cand[0]
    out, _ = _run(harness, "mark", 2, str(chosen), "-", stop)
    assert out["ret"] == ["0"]
    assert out["noutliers"] == ["1"]                  # cand[0] was marked before the exit
    assert [int(v) for v in out["marked"]] == [chosen]
    assert out["calls"] == ["3"]                      # initial, cand[0], cand[1]


def test_report_outliers(gpu, harness):
    out, err = _run(harness, "report", 2)
    N, M = map(int, out["dims"][:2])
    nf = M // 2
    assert int(out["calls"][0]) == nf + 1
    lines = [ln.split(": ", 1)[1] for ln in err.splitlines() if ": " in ln]
    i = lines.index("## Outlier statistics")
    assert lines[i + 1] == "# i_feature outlier_factor confidence_drop_relative_if_removed"
    rows = lines[i + 2:i + 2 + nf]
    want, _ = _np_factors(out, 2, 0, -1.0)
    for k, ln in enumerate(rows):
        assert ln == "%5d %9.3g %9.3g" % (k, float(ln.split()[1]), 0.5), ln
        assert float(ln.split()[1]) == pytest.approx(want[k], rel=6e-3, abs=1e-300)     # (three digits printed)


def test_trace_query(gpu, harness):
    out, _ = _run(harness, "trace", 11, 10, 40)
    N, M, J, x, n2, lam = _point(out)
    Jq = _f(out["Jq"]).reshape(2, 40)
    H = J.T @ J + lam * np.eye(N)
    Jfull = np.zeros((2, N))
    Jfull[:, 10:50] = Jq
    A = Jfull @ np.linalg.solve(H, Jfull.T)
    tr = np.trace(np.linalg.inv(np.eye(2) + A))
    for key, nout in (("trace", 0), ("trace_nout3", 3)):
        want = _scale(M, N, nout, 2, n2) * (2.0 - tr)
        got = _f(out[key])[0]
        assert got == pytest.approx(want, rel=1e-9), (key, got, want)
    assert _f(out["trace_fs3"])[0] == -1.0
    assert _f(out["trace_noJ"])[0] == -1.0


def test_refusals_public(gpu, harness):
    out, err = _run(harness, "refuse")
    assert out["fs3"] == ["0"] and out["too_many"] == ["0"] and out["products"] == ["0"]
