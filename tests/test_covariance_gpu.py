"""Covariance blocks and marginal variances of Sigma = inv(JtJ + lambda I) from the factor held on the device.

dlg_covariance_blocks / dlg_marginal_variances are checked against numpy's inverse formed from J on the host (small
problems), against dlg_solve_multi with unit columns (the same factor, full solves) and the ORACLE's own factor
(orc_sparse_solve) on the benchmark configurations, on a singular JtJ, on the dense and dense-products backends, for
reproducibility and independence of the other requests, against the full-sweep route, and for their refusals.  The
public entry points run from C (tests/c/covariance_harness.c) on the point dogleg_optimize2 left behind."""
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import dptr, iptr
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, BC, BP = 6, 6, 3


def _dense_J(Jp, Ji, Jx, M, N):
    J = np.zeros((M, N))
    for r in range(M):
        J[r, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
    return J


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
    return be, Jp, Ji, Jx


def _ba_requests(Nc, Np, Jp, Ji, rng, n_obs=None, n_unobs=None):
    """every global, camera and point diagonal block; camera x point blocks of observed and unobserved pairs; global x
    camera blocks.  Lists (r0, nr, c0, nc)."""
    cam0, pt0 = G, G + BC * Nc
    req = [(0, G, 0, G)]
    req += [(cam0 + BC * c, BC, cam0 + BC * c, BC) for c in range(Nc)]
    req += [(pt0 + BP * p, BP, pt0 + BP * p, BP) for p in range(Np)]
    obs = set()
    for r in range(0, len(Jp) - 1, 2):
        cols = Ji[Jp[r]:Jp[r + 1]]
        obs.add(((int(cols[G]) - cam0) // BC, (int(cols[G + BC]) - pt0) // BP))
    obs = sorted(obs)
    if n_obs is not None:
        obs = [obs[i] for i in rng.choice(len(obs), min(n_obs, len(obs)), replace=False)]
    req += [(cam0 + BC * c, BC, pt0 + BP * p, BP) for c, p in obs]
    unobs = []
    allobs = set(obs)
    while len(unobs) < (n_unobs if n_unobs is not None else 2 * Nc):
        c, p = int(rng.integers(Nc)), int(rng.integers(Np))
        if (c, p) not in allobs:
            unobs.append((c, p))
    req += [(pt0 + BP * p, BP, cam0 + BC * c, BC) for c, p in unobs]       # (point rows, camera columns)
    req += [(0, G, cam0 + BC * c, BC) for c in range(0, Nc, max(1, Nc // 16))]
    return req


def _call(be, req, slot=0):
    r0, nr, c0, nc = (np.array(a, dtype=np.int32) for a in zip(*req))
    return be.covariance_blocks(slot, r0, nr, c0, nc)


def _scaled_err(blocks, req, S, d):
    worst = 0.0
    for B, (r0, nr, c0, nc) in zip(blocks, req):
        ref = S[r0:r0 + nr, c0:c0 + nc]
        sc = np.sqrt(np.outer(d[r0:r0 + nr], d[c0:c0 + nc]))
        worst = max(worst, float(np.max(np.abs(B - ref) / sc)))
    return worst


def _unit_solve(be, N, cols):
    """Sigma[:, cols] through dlg_solve_multi on unit columns (the same factor, full solves)"""
    out = np.zeros((len(cols), N))
    for i in range(0, len(cols), 128):
        cc = cols[i:i + 128]
        E = np.zeros((len(cc), N))
        E[np.arange(len(cc)), cc] = 1.0
        X = np.zeros_like(E)
        be.L.dlg_solve_multi(be.h, 0, dptr(E), dptr(X), len(cc))
        out[i:i + len(cc)] = X
    return out


def _check_against_columns(blocks, req, cols, X, diag, tol):
    pos = {c: i for i, c in enumerate(cols)}
    worst = 0.0
    for B, (r0, nr, c0, nc) in zip(blocks, req):
        ref = np.array([[X[pos[c0 + j], r0 + i] for j in range(nc)] for i in range(nr)])
        sc = np.sqrt(np.outer(diag[r0:r0 + nr], diag[c0:c0 + nc]))
        worst = max(worst, float(np.max(np.abs(B - ref) / sc)))
    assert worst <= tol, worst
    return worst


# ---------------------------------------------------------------- small problems against numpy
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("shape", [(12, 120, 720), (49, 900, 10000)], ids=["small", "medium"])
def test_sparse_blocks_match_numpy(gpu, shape, lam):
    prob = oa.BAProblem(*shape, seed=3)
    be, Jp, Ji, Jx = _sparse_backend(prob, lam)
    J = _dense_J(Jp, Ji, Jx, prob.M, prob.N)
    S = np.linalg.inv(J.T @ J + lam * np.eye(prob.N))
    d = np.diag(S)
    req = _ba_requests(shape[0], shape[1], Jp, Ji, np.random.default_rng(1))
    blocks = _call(be, req)
    err = _scaled_err(blocks, req, S, d)
    var = be.marginal_variances(0)
    verr = float(np.max(np.abs(var - d) / d))
    nch, visits, nsn = be.covariance_stats()
    print(f"{shape} lambda={lam}: {len(req)} requests, scaled error {err:.2e}, variances {verr:.2e}; "
          f"marginal plan {nch} chunks, {visits / nch:.1f} of {nsn} supernodes per chunk")
    assert err <= 1e-9 and verr <= 1e-9
    assert np.all(var > 0)
    be.close()


# ---------------------------------------------------------------- config #3: the same factor, an independent factor
def test_config3_against_full_solves_and_oracle(gpu):
    Nc, Np = 499, 9000
    prob = oa.BAProblem(Nc, Np, 100000, seed=1)
    be, Jp, Ji, Jx = _sparse_backend(prob, 0.0)
    rng = np.random.default_rng(5)
    allreq = _ba_requests(Nc, Np, Jp, Ji, rng, n_obs=400, n_unobs=200)
    req = [allreq[i] for i in rng.choice(len(allreq), 256, replace=False)]
    blocks = _call(be, req)
    var = be.marginal_variances(0)
    cols = sorted({c0 + j for (_, _, c0, nc) in req for j in range(nc)} | {r0 + i for (r0, nr, _, _) in req for i in range(nr)})
    X = _unit_solve(be, prob.N, np.array(cols))
    diag = var.copy()
    err = _check_against_columns(blocks, req, cols, X, diag, 1e-12)
    print(f"config #3: 256 requests against dlg_solve_multi on {len(cols)} unit columns: {err:.2e}")
    # the oracle's own factor on a part of them
    O = oa.oracle()
    F = O.orc_sparse_analyze(prob.N, prob.M, iptr(Jp), iptr(Ji))
    assert O.orc_sparse_factorize(F, iptr(Jp), iptr(Ji), dptr(Jx), 0.0) == prob.N
    sub = req[:24]
    ocols = sorted({c0 + j for (_, _, c0, nc) in sub for j in range(nc)} | {r0 + i for (r0, nr, _, _) in sub for i in range(nr)})
    Xo = np.zeros((len(ocols), prob.N))
    for i, c in enumerate(ocols):
        e = np.zeros(prob.N)
        e[c] = 1.0
        O.orc_sparse_solve(F, dptr(e), dptr(Xo[i]))
    O.orc_sparse_free(F)
    oerr = _check_against_columns(blocks[:24], sub, ocols, Xo, diag, 1e-9)
    print(f"config #3: 24 requests against the oracle's factor: {oerr:.2e}")
    be.close()


# ---------------------------------------------------------------- config #4
def test_config4_sample_and_marginals(gpu):
    Nc, Np = 2499, 45000
    prob = oa.BAProblem(Nc, Np, 500000, seed=1)
    be, Jp, Ji, Jx = _sparse_backend(prob, 0.0)
    var = be.marginal_variances(0)
    assert np.all(np.isfinite(var)) and np.all(var > 0)
    # the diagonals of every 6 x 6 and 3 x 3 block: the same bits
    cam0, pt0 = G, G + BC * Nc
    diag_req = [(0, G, 0, G)] + [(cam0 + BC * c, BC, cam0 + BC * c, BC) for c in range(Nc)] + \
               [(pt0 + BP * p, BP, pt0 + BP * p, BP) for p in range(Np)]
    blocks = _call(be, diag_req)
    dvar = np.concatenate([np.diag(B) for B in blocks])
    nbad = int(np.sum(dvar != var))
    print(f"config #4: {nbad} of {prob.N} marginal variances differ from the block diagonals "
          f"(max rel {np.max(np.abs(dvar - var) / var):.1e})")
    assert nbad == 0
    rng = np.random.default_rng(9)
    allreq = _ba_requests(Nc, Np, Jp, Ji, rng, n_obs=300, n_unobs=100)
    req = [allreq[i] for i in rng.choice(len(allreq), 128, replace=False)]
    blocks = _call(be, req)
    cols = sorted({c0 + j for (_, _, c0, nc) in req for j in range(nc)} | {r0 + i for (r0, nr, _, _) in req for i in range(nr)})
    X = _unit_solve(be, prob.N, np.array(cols))
    err = _check_against_columns(blocks, req, cols, X, var, 1e-12)
    print(f"config #4: 128 requests against dlg_solve_multi: {err:.2e}")
    be.close()


# ---------------------------------------------------------------- singular JtJ
def test_singular_columns(gpu):
    lam = 1e-6
    prob = oa.BAProblem(12, 120, 720, seed=2, n_zero_cols=3)
    be, Jp, Ji, Jx = _sparse_backend(prob, lam)
    J = _dense_J(Jp, Ji, Jx, prob.M, prob.N)
    zero = np.where(~np.any(J != 0.0, axis=0))[0]
    assert len(zero) == 3, zero
    var = be.marginal_variances(0)
    assert np.allclose(var[zero], 1.0 / lam, rtol=1e-9, atol=0)
    other = [v for v in range(0, prob.N, 7) if v not in set(zero)][:12]
    req = [(int(z), 1, int(o), 1) for z in zero for o in other] + [(int(z), 1, int(z), 1) for z in zero]
    blocks = _call(be, req)
    vals = np.array([B[0, 0] for B in blocks])
    n = len(zero) * len(other)
    assert np.all(np.abs(vals[:n]) <= 1e-12 * np.sqrt(var[np.repeat(zero, len(other))] * var[np.tile(other, len(zero))]))
    assert np.allclose(vals[n:], 1.0 / lam, rtol=1e-9, atol=0)
    S = np.linalg.inv(J.T @ J + lam * np.eye(prob.N))
    assert np.max(np.abs(var - np.diag(S)) / np.diag(S)) <= 1e-9
    be.close()


# ---------------------------------------------------------------- dense and dense-products
@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("kind", ["dense", "products_packed_upper", "products_unpacked"])
def test_dense_blocks_match_numpy(gpu, kind, lam):
    dp = oa.DenseProblem(M=1201, N=150, seed=2)
    p = dp.p0()
    x, J = dp.eval(p)
    N = dp.N
    H = J.T @ J
    if kind == "dense":
        be = capi.Backend(capi.DLG_DENSE, N, dp.M)
        be.set_p(0, p)
        be.upload(0, x, J)
    else:
        packed = kind == "products_packed_upper"
        be = capi.Backend(capi.DLG_DENSE_PRODUCTS, N, dp.M, 0, (capi.FLAG_PACKED | capi.FLAG_UPPER) if packed else 0)
        be.set_p(0, p)
        JtJ = H[np.triu_indices(N)].copy() if packed else H.copy()
        be.upload_products(0, float(x @ x), J.T @ x, JtJ)
    be.eval(0)
    assert be.factorize(0, lam)
    S = np.linalg.inv(H + lam * np.eye(N))
    d = np.diag(S)
    rng = np.random.default_rng(4)
    req = [(v, 6, v, 6) for v in range(0, N - 6, 6)]
    req += [(int(a), 6, int(b), 9) for a, b in zip(rng.integers(0, N - 6, 40), rng.integers(0, N - 9, 40)) if abs(int(a) - int(b)) >= 9]
    req += [(0, 16, 0, 16), (N - 16, 16, N - 16, 16), (10, 12, 14, 12)]
    blocks = _call(be, req)
    err = _scaled_err(blocks, req, S, d)
    var = be.marginal_variances(0)
    verr = float(np.max(np.abs(var - d) / d))
    print(f"{kind} lambda={lam}: scaled error {err:.2e}, variances {verr:.2e}")
    assert err <= 1e-9 and verr <= 1e-9
    for B, r in zip(blocks, req):
        if r[0] == r[2] and r[1] == r[3]:
            assert np.array_equal(B, B.T)
    assert all(np.array_equal(a, b) for a, b in zip(blocks, _call(be, req)))
    be.close()


# ---------------------------------------------------------------- reproducibility, independence, full-sweep route
def test_reproducible_order_independent_and_sweep(gpu, monkeypatch):
    Nc, Np = 49, 900
    prob = oa.BAProblem(Nc, Np, 10000, seed=5)
    be, Jp, Ji, Jx = _sparse_backend(prob, 1e-3)
    rng = np.random.default_rng(2)
    req = _ba_requests(Nc, Np, Jp, Ji, rng, n_obs=500, n_unobs=100)
    B1 = _call(be, req)
    B2 = _call(be, req)
    assert all(np.array_equal(a, b) for a, b in zip(B1, B2)), "two calls differ"
    perm = rng.permutation(len(req))
    B3 = _call(be, [req[i] for i in perm])
    ndiff = sum(not np.array_equal(B1[i], B3[k]) for k, i in enumerate(perm))
    assert ndiff == 0, f"{ndiff} of {len(req)} requests changed with the order"
    # a request alone: the same bits as among the others
    for i in (0, 7, len(req) - 1):
        assert np.array_equal(_call(be, [req[i]])[0], B1[i])
    var = be.marginal_variances(0)
    monkeypatch.setenv("DOGLEG_AMD_LEVERAGE_SWEEP", "1")
    B4 = _call(be, req)
    var4 = be.marginal_variances(0)
    monkeypatch.delenv("DOGLEG_AMD_LEVERAGE_SWEEP")
    d = var
    err = max(float(np.max(np.abs(a - b) / np.sqrt(np.outer(d[r[0]:r[0] + r[1]], d[r[2]:r[2] + r[3]]))))
              for a, b, r in zip(B1, B4, req))
    print(f"reach-restricted against the full sweep: {err:.2e}")
    assert err <= 1e-12
    assert np.max(np.abs(var - var4) / var) <= 1e-12
    # the blocked plan is still cached and gives the same bits
    assert all(np.array_equal(a, b) for a, b in zip(B1, _call(be, req)))
    be.close()


def test_refusals(gpu):
    prob = oa.BAProblem(5, 40, 300, seed=11)
    be, *_ = _sparse_backend(prob, 0.0)
    N = prob.N
    ok = (0, 6, 0, 6)
    for bad in [(0, 17, 0, 17), (0, 9, 20, 8), (0, 0, 0, 6), (0, 6, 0, 0), (N - 3, 6, 0, 6), (-1, 2, 0, 2), (0, 2, N - 1, 2)]:
        with pytest.raises(capi.DlgError):
            _call(be, [ok, bad])
    assert _call(be, [(0, 9, 4, 11)])[0].shape == (9, 11)          # overlapping ranges: 15 distinct variables
    z = np.zeros(1, dtype=np.int32)
    assert be.L.dlg_covariance_blocks(be.h, 0, 0, iptr(z), iptr(z), iptr(z), iptr(z), None) == 0      # nreq == 0
    assert be.L.dlg_covariance_blocks(be.h, 0, 1, None, iptr(z), iptr(z), iptr(z), dptr(np.zeros(4))) != 0
    assert be.L.dlg_marginal_variances(be.h, 0, None) != 0
    with pytest.raises(capi.DlgError):
        be.marginal_variances(1)                                   # slot 1 holds no factor
    with pytest.raises(capi.DlgError):
        _call(be, [ok], slot=1)
    be.close()
    # a partitioned backend: refused as such (before anything looks at the factor)
    prob = oa.BAProblem(49, 900, 10000, seed=5)
    Jp, Ji = prob.pattern()
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_partition(0, 2)
    be.set_pattern(Jp, Ji)
    for call in (lambda: be.marginal_variances(0), lambda: _call(be, [ok])):
        with pytest.raises(capi.DlgError, match="sharded or partitioned"):
            call()
    be.close()


# ---------------------------------------------------------------- the pattern dropped and set again on one backend
@pytest.mark.parametrize("sym_cache", [True, False], ids=["sym-cache", "no-sym-cache"])
def test_plans_follow_the_pattern(gpu, monkeypatch, sym_cache):
    """a backend whose pattern is dropped and set again (as the driver does with a parked backend): the same pattern
    (a new symbolic phase) and another pattern of the same sizes, each factorised and checked against numpy"""
    if not sym_cache:
        monkeypatch.setenv("DOGLEG_AMD_NO_SYM_CACHE", "1")
    Nc, Np, Nobs = 12, 120, 720
    prob = oa.BAProblem(Nc, Np, Nobs, seed=3)
    Jp, Ji = prob.pattern()
    # another pattern of the same sizes: the same measurements with the points relabelled
    pt0 = G + BC * Nc
    relabel = np.random.default_rng(6).permutation(Np)
    Ji2 = Ji.copy()
    pts = Ji >= pt0
    Ji2[pts] = pt0 + BP * relabel[(Ji[pts] - pt0) // BP] + (Ji[pts] - pt0) % BP
    assert not np.array_equal(Ji, Ji2)
    pats = [(Jp, Ji), (Jp, Ji2)]
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    p = prob.p0()
    x, Jx = prob.eval(p)
    req = _ba_requests(Nc, Np, Jp, Ji, np.random.default_rng(1), n_obs=200, n_unobs=20)
    for k, i in enumerate([0, 1, 0, 0, 1]):
        Jpk, Jik = pats[i]
        if k > 0:
            assert be.L.dlg_sparse_drop_pattern(be.h) == 0
        be.set_pattern(Jpk, Jik)
        be.set_p(0, p)
        be.upload(0, x, Jx)
        be.eval(0)
        lam = 1e-3 * k
        assert be.factorize(0, lam)
        J = _dense_J(Jpk, Jik, Jx, prob.M, prob.N)
        S = np.linalg.inv(J.T @ J + lam * np.eye(prob.N))
        d = np.diag(S)
        var = be.marginal_variances(0)
        if k != 3:                                     # (k = 3: the variances alone)
            blocks = _call(be, req)
            assert _scaled_err(blocks, req, S, d) <= 1e-9, (k, i)
        assert np.max(np.abs(var - d) / d) <= 1e-9, (k, i)
    be.close()


# ---------------------------------------------------------------- the public API from C
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cov") / "covariance_harness")
    cmd = ["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "covariance_harness.c"), "-o", exe,
           "-L", os.path.join(ROOT, "libdogleg_amd"), "-ldogleg_amd",
           "-L", os.path.join(ROOT, "problems"), "-lproblems", "-lm",
           "-Wl,-rpath," + os.path.join(ROOT, "libdogleg_amd"), "-Wl,-rpath," + os.path.join(ROOT, "problems")]
    subprocess.run(cmd, check=True)
    return exe


def _f(vals):
    return np.array([float.fromhex(v) for v in vals])


def test_public_api_end_to_end(gpu, harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    out = {}
    for line in r.stdout.splitlines():
        if line.strip():
            k, *v = line.split()
            out[k] = v
    assert out.get("alive") == ["1"]
    N, M, nnz = map(int, out["dims"])
    req = np.array(out["req"], dtype=int).reshape(-1, 4)
    for tag in ("before", "fresh"):
        assert out[f"{tag}_rc"] == ["0", "0"], (tag, out[f"{tag}_rc"])
        J = _dense_J(np.array(out[f"{tag}_Jp"], dtype=np.int32), np.array(out[f"{tag}_Ji"], dtype=np.int32),
                     _f(out[f"{tag}_Jx"]), M, N)
        lam = _f(out[f"{tag}_lambda"])[0]
        S = np.linalg.inv(J.T @ J + lam * np.eye(N))
        d = np.diag(S)
        got = _f(out[f"{tag}_blocks"])
        o = 0
        worst = 0.0
        for r0, nr, c0, nc in req:
            B = got[o:o + nr * nc].reshape(nr, nc)
            o += nr * nc
            worst = max(worst, float(np.max(np.abs(B - S[r0:r0 + nr, c0:c0 + nc]) / np.sqrt(np.outer(d[r0:r0 + nr], d[c0:c0 + nc])))))
        verr = float(np.max(np.abs(_f(out[f"{tag}_var"]) - d) / d))
        print(f"{tag}: lambda {lam:.3g}, blocks {worst:.2e}, variances {verr:.2e}")
        assert worst <= 1e-9 and verr <= 1e-9
    assert out["refuse"] == ["-1", "-1"]
