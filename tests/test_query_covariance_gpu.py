"""Query covariance Jq Sigma Jq^T (and the observation form Jq Sigma J_obs^T J_obs Sigma Jq^T) from the factor held on the
device.

dlg_query_covariance is checked against numpy's inverse formed from J on the host (small problems, both forms, several
lambdas, every row count, unsorted / duplicated indices, empty rows), against dlg_solve_multi on the columns of Jq^T on
configs #3 and #4, against the existing calls it generalises (dlg_covariance_blocks, dlg_feature_leverage,
dlg_leverage_query), on the dense and dense-products backends, for reproducibility and independence of the other queries,
against the full-sweep route, for plans that follow the values and the pattern, and for its refusals.  The public entry
point runs from C (tests/c/query_harness.c) on the point dogleg_optimize2 left behind."""
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


def _csr(queries):
    """queries: lists of rows, each row a list of (var, val) -> (qrow, rowptr, var, val)"""
    qrow, rowptr, var, val = [0], [0], [], []
    for rows in queries:
        for row in rows:
            var += [int(v) for v, _ in row]
            val += [float(x) for _, x in row]
            rowptr.append(len(var))
        qrow.append(len(rowptr) - 1)
    return (np.array(qrow, dtype=np.int32), np.array(rowptr, dtype=np.int32), np.array(var, dtype=np.int32),
            np.array(val, dtype=np.float64))


def _call(be, queries, nobs=-1, slot=0):
    return be.query_covariance(slot, *_csr(queries), nobs=nobs)


def _dense_rows(rows, N):
    Q = np.zeros((len(rows), N))
    for i, row in enumerate(rows):
        for v, x in row:
            Q[i, v] += x
    return Q


def _check(blocks, queries, S, N, tol, what=""):
    worst = 0.0
    for B, rows in zip(blocks, queries):
        Q = _dense_rows(rows, N)
        ref = Q @ S @ Q.T
        sc = max(float(np.max(np.abs(ref))), 1e-300)
        worst = max(worst, float(np.max(np.abs(B - ref))) / sc)
    assert worst <= tol, (what, worst)
    return worst


def _random_queries(N, rng, sizes, nnz=(1, 20), pool=None):
    """random rows: unsorted, some indices duplicated, some rows empty"""
    queries = []
    for fs in sizes:
        rows = []
        for _ in range(fs):
            k = int(rng.integers(nnz[0], nnz[1] + 1))
            src = pool if pool is not None else np.arange(N)
            vs = list(rng.choice(src, k))
            if rng.random() < 0.3:
                vs.append(vs[0])                              # a duplicate
            rows.append([(int(v), float(rng.standard_normal())) for v in vs])
        if fs > 1 and rng.random() < 0.3:
            rows[int(rng.integers(fs))] = []                   # an empty row
        queries.append(rows)
    return queries


def _pixel_queries(Nc, Np, rng, n, rows=2, cams=None):
    """rows over the globals, one camera and one point (15 variables), pairs observed or not"""
    cam0, pt0 = G, G + BC * Nc
    out = []
    for _ in range(n):
        c = int(rng.integers(Nc)) if cams is None else int(rng.choice(cams))
        p = int(rng.integers(Np))
        vs = list(range(G)) + list(range(cam0 + BC * c, cam0 + BC * c + BC)) + list(range(pt0 + BP * p, pt0 + BP * p + BP))
        out.append([[(v, float(rng.standard_normal())) for v in vs] for _ in range(rows)])
    return out


# ---------------------------------------------------------------- small sparse problems against numpy
@pytest.mark.parametrize("lam", [0.0, 1e-6, 1.0])
def test_sparse_match_numpy(gpu, lam):
    prob = oa.BAProblem(12, 120, 720, seed=3)
    be, Jp, Ji, Jx = _sparse_backend(prob, lam)
    N = prob.N
    J = _dense_J(Jp, Ji, Jx, prob.M, N)
    S = np.linalg.inv(J.T @ J + lam * np.eye(N))
    rng = np.random.default_rng(1)
    queries = _random_queries(N, rng, [1, 2, 3, 7, 16, 2, 1, 16, 3, 7, 2, 2, 5])
    queries += _pixel_queries(12, 120, rng, 20)
    blocks = _call(be, queries)
    err = _check(blocks, queries, S, N, 1e-10, "plain")
    for B in blocks:
        assert np.array_equal(B, B.T)
    # the observation form with a nobs that leaves rows out
    nobs = prob.M - 37
    Jo = J[:nobs]
    So = S @ Jo.T @ Jo @ S
    blocks = _call(be, queries, nobs=nobs)
    erro = _check(blocks, queries, So, N, 1e-10, "observation form")
    nch, visits, nsn = be.query_covariance_stats()
    print(f"lambda={lam}: plain {err:.2e}, observation form {erro:.2e}; {nch} chunks")
    be.close()


# ---------------------------------------------------------------- configs #3 and #4 against dlg_solve_multi
def _solve_multi_route(be, N, queries):
    """Jq Sigma Jq^T through dlg_solve_multi on the columns of Jq^T and a host product"""
    out = []
    rows = [r for q in queries for r in q]
    cols = np.zeros((len(rows), N))
    for i, r in enumerate(rows):
        for v, x in r:
            cols[i, v] += x
    X = np.zeros_like(cols)
    for i in range(0, len(rows), 128):
        assert be.L.dlg_solve_multi(be.h, 0, dptr(np.ascontiguousarray(cols[i:i + 128])), dptr(X[i:i + 128]),
                                    len(cols[i:i + 128])) == 0
    o = 0
    for q in queries:
        fs = len(q)
        out.append(cols[o:o + fs] @ X[o:o + fs].T)
        o += fs
    return out


@pytest.mark.parametrize("config", ["3", "4"])
def test_configs_against_solve_multi(gpu, config):
    Nc, Np, Nobs = (499, 9000, 100000) if config == "3" else (2499, 45000, 500000)
    prob = oa.BAProblem(Nc, Np, Nobs, seed=1)
    be, Jp, Ji, Jx = _sparse_backend(prob, 0.0)
    rng = np.random.default_rng(11)
    queries = _pixel_queries(Nc, Np, rng, 400) + _pixel_queries(Nc, Np, rng, 16, rows=16)
    blocks = _call(be, queries)
    ref = _solve_multi_route(be, prob.N, queries)
    worst = max(float(np.max(np.abs(a - b))) / float(np.max(np.abs(b))) for a, b in zip(blocks, ref))
    nch, visits, nsn = be.query_covariance_stats()
    print(f"config #{config}: {len(queries)} queries, {worst:.2e} against dlg_solve_multi; {nch} chunks, "
          f"{visits / nch:.1f} of {nsn} supernodes per chunk")
    assert worst <= 1e-10
    assert visits < 0.2 * nch * nsn
    be.close()


# ---------------------------------------------------------------- identities against the existing calls
def test_identities_with_existing_calls(gpu):
    lam = 1e-3
    prob = oa.BAProblem(49, 900, 10000, seed=5)
    be, Jp, Ji, Jx = _sparse_backend(prob, lam)
    N = prob.N
    rng = np.random.default_rng(4)
    # unit rows: the covariance blocks of the same variables
    req = [(int(a), 6, int(a), 6) for a in rng.integers(0, N - 6, 30)]
    cov = be.covariance_blocks(0, *(np.array(x, dtype=np.int32) for x in zip(*req)))
    unit = [[[(r0 + i, 1.0)] for i in range(nr)] for (r0, nr, _, _) in req]
    qb = _call(be, unit)
    for a, b in zip(qb, cov):
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b))
    # J's own rows grouped by 1 and 2: the feature leverages
    nf = 300
    for fs in (1, 2):
        rows = [[(int(v), float(x)) for v, x in zip(Ji[Jp[r]:Jp[r + 1]], Jx[Jp[r]:Jp[r + 1]])] for r in range(nf * fs)]
        qs = [rows[f * fs:(f + 1) * fs] for f in range(nf)]
        qb = _call(be, qs)
        lev = be.feature_leverage(0, fs, 0, nf)
        got = np.array([B[0, 0] for B in qb]) if fs == 1 else np.array([[B[0, 0], B[0, 1], B[1, 1]] for B in qb])
        assert np.max(np.abs(got - lev)) <= 1e-10 * np.max(np.abs(lev)), fs
    # one 2-row query on a contiguous range: dlg_leverage_query gives the numpy value
    J = _dense_J(Jp, Ji, Jx, prob.M, N)
    S = np.linalg.inv(J.T @ J + lam * np.eye(N))
    istate, ns = 40, 30
    Jq = rng.standard_normal((2, ns))
    A = be.leverage_query(0, Jq, istate)
    ref = Jq @ S[istate:istate + ns, istate:istate + ns] @ Jq.T
    assert np.max(np.abs(A - ref[np.triu_indices(2)])) <= 1e-10 * np.max(np.abs(ref))
    q = [[[(istate + j, Jq[i, j]) for j in range(ns)] for i in range(2)]]
    assert np.max(np.abs(_call(be, q)[0] - ref)) <= 1e-10 * np.max(np.abs(ref))
    be.close()


# ---------------------------------------------------------------- the observation form
def test_observation_form_identities(gpu):
    prob = oa.BAProblem(12, 120, 720, seed=7)
    N, M = prob.N, prob.M
    rng = np.random.default_rng(2)
    queries = _random_queries(N, rng, [1, 2, 3, 16, 7, 2]) + _pixel_queries(12, 120, rng, 30)
    be, Jp, Ji, Jx = _sparse_backend(prob, 0.0)
    plain = _call(be, queries)
    full = _call(be, queries, nobs=M)
    for a, b in zip(full, plain):
        assert np.max(np.abs(a - b)) <= 1e-10 * np.max(np.abs(b))
    zero = _call(be, queries, nobs=0)
    assert all(np.all(B == 0.0) for B in zero)
    lam = 0.5
    assert be.factorize(0, lam)
    J = _dense_J(Jp, Ji, Jx, M, N)
    S = np.linalg.inv(J.T @ J + lam * np.eye(N))
    _check(_call(be, queries, nobs=M), queries, S - lam * S @ S, N, 1e-10, "Sigma - lambda Sigma^2")
    be.close()


# ---------------------------------------------------------------- dense and dense-products
@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("kind", ["dense", "products"])
def test_dense(gpu, kind, lam):
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
        be = capi.Backend(capi.DLG_DENSE_PRODUCTS, N, dp.M, 0, capi.FLAG_PACKED | capi.FLAG_UPPER)
        be.set_p(0, p)
        be.upload_products(0, float(x @ x), J.T @ x, H[np.triu_indices(N)].copy())
    be.eval(0)
    assert be.factorize(0, lam)
    S = np.linalg.inv(H + lam * np.eye(N))
    rng = np.random.default_rng(4)
    queries = _random_queries(N, rng, [1, 2, 3, 7, 16, 2, 2, 5, 16, 1] * 3)
    blocks = _call(be, queries)
    _check(blocks, queries, S, N, 1e-10, kind)
    assert all(np.array_equal(a, b) for a, b in zip(blocks, _call(be, queries)))
    nobs = dp.M - 100
    if kind == "dense":
        So = S @ J[:nobs].T @ J[:nobs] @ S
        _check(_call(be, queries, nobs=nobs), queries, So, N, 1e-10, "dense observation form")
    else:
        with pytest.raises(capi.DlgError, match="dense-products"):
            _call(be, queries, nobs=nobs)
    be.close()


# ---------------------------------------------------------------- reproducibility, independence, full-sweep route
def test_reproducible_independent_and_sweep(gpu, monkeypatch):
    Nc, Np = 49, 900
    prob = oa.BAProblem(Nc, Np, 10000, seed=5)
    be, Jp, Ji, Jx = _sparse_backend(prob, 1e-3)
    rng = np.random.default_rng(2)
    queries = _pixel_queries(Nc, Np, rng, 300) + _random_queries(prob.N, rng, [1, 3, 7, 16, 5] * 4)
    B1 = _call(be, queries)
    B2 = _call(be, queries)
    assert all(np.array_equal(a, b) for a, b in zip(B1, B2)), "two calls differ"
    perm = rng.permutation(len(queries))
    B3 = _call(be, [queries[i] for i in perm])
    ndiff = sum(not np.array_equal(B1[i], B3[k]) for k, i in enumerate(perm))
    assert ndiff == 0, f"{ndiff} of {len(queries)} queries changed with the order"
    extra = _pixel_queries(Nc, Np, rng, 50, rows=3)
    B4 = _call(be, extra[:25] + queries + extra[25:])
    assert all(np.array_equal(a, b) for a, b in zip(B1, B4[25:25 + len(queries)]))
    for i in (0, 7, len(queries) - 1):
        assert np.array_equal(_call(be, [queries[i]])[0], B1[i])
    O1 = _call(be, queries, nobs=prob.M - 5)
    assert all(np.array_equal(a, b) for a, b in zip(O1, _call(be, queries, nobs=prob.M - 5)))
    monkeypatch.setenv("DOGLEG_AMD_LEVERAGE_SWEEP", "1")
    B5 = _call(be, queries)
    monkeypatch.delenv("DOGLEG_AMD_LEVERAGE_SWEEP")
    err = max(float(np.max(np.abs(a - b))) / float(np.max(np.abs(a))) for a, b in zip(B1, B5))
    print(f"reach-restricted against the full sweep: {err:.2e}")
    assert err <= 1e-12
    be.close()


# ---------------------------------------------------------------- plans follow the values and the pattern
def test_plans_follow_values_and_pattern(gpu):
    Nc, Np, Nobs = 12, 120, 720
    prob = oa.BAProblem(Nc, Np, Nobs, seed=3)
    be, Jp, Ji, Jx = _sparse_backend(prob, 1e-3)
    N = prob.N
    J = _dense_J(Jp, Ji, Jx, prob.M, N)
    S = np.linalg.inv(J.T @ J + 1e-3 * np.eye(N))
    rng = np.random.default_rng(8)
    queries = _pixel_queries(Nc, Np, rng, 40)
    qrow, rowptr, var, val = _csr(queries)
    B1 = be.query_covariance(0, qrow, rowptr, var, val)
    assert be.query_covariance_plan_seconds() > 0.0
    val2 = rng.standard_normal(len(val))
    B2 = be.query_covariance(0, qrow, rowptr, var, val2)
    assert be.query_covariance_plan_seconds() == 0.0
    q2 = [[[(v, x) for v, x in zip(var[rowptr[r]:rowptr[r + 1]], val2[rowptr[r]:rowptr[r + 1]])]
           for r in range(qrow[k], qrow[k + 1])] for k in range(len(qrow) - 1)]
    _check(B2, q2, S, N, 1e-10, "new values")
    assert not all(np.array_equal(a, b) for a, b in zip(B1, B2))
    # the pattern dropped and set again: the plan is rebuilt, the values right
    assert be.L.dlg_sparse_drop_pattern(be.h) == 0
    with pytest.raises(capi.DlgError):
        be.query_covariance_stats()
    be.set_pattern(Jp, Ji)
    p = prob.p0()
    x, Jx = prob.eval(p)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    assert be.factorize(0, 1e-3)
    B3 = be.query_covariance(0, qrow, rowptr, var, val)
    assert be.query_covariance_plan_seconds() > 0.0
    _check(B3, queries, S, N, 1e-10, "pattern set again")
    be.close()


# ---------------------------------------------------------------- refusals and a singular JtJ
def test_refusals(gpu):
    prob = oa.BAProblem(5, 40, 300, seed=11)
    be, *_ = _sparse_backend(prob, 0.0)
    N, M = prob.N, prob.M
    ok = [[(0, 1.0), (7, 2.0)], [(3, 1.0)]]
    for bad in ([[(0, 1.0)]] * 17, [], [[(N, 1.0)]], [[(-1, 1.0)]]):
        with pytest.raises(capi.DlgError) as e:
            _call(be, [ok, bad])
        if len(bad) == 17:
            assert "dlg_solve_multi" in str(e.value)
    with pytest.raises(capi.DlgError):
        _call(be, [ok], nobs=M + 1)
    assert len(_call(be, [ok], nobs=M)) == 1
    z = np.zeros(2, dtype=np.int32)
    assert be.L.dlg_query_covariance(be.h, 0, 0, iptr(z), iptr(z), iptr(z), dptr(np.zeros(1)), -1, None) == 0   # nq == 0
    with pytest.raises(capi.DlgError):
        _call(be, [ok], slot=1)                                    # slot 1 holds no factor
    be.close()
    # a partitioned backend: refused as such
    prob = oa.BAProblem(49, 900, 10000, seed=5)
    Jp, Ji = prob.pattern()
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_partition(0, 2)
    be.set_pattern(Jp, Ji)
    with pytest.raises(capi.DlgError, match="sharded or partitioned"):
        _call(be, [ok])
    be.close()


def test_singular_like_covariance(gpu):
    """a singular JtJ: at lambda = 0 the query call does what dlg_covariance_blocks does; at lambda > 0 the zero columns
    give 1 / lambda"""
    prob = oa.BAProblem(12, 120, 720, seed=2, n_zero_cols=3)
    p = prob.p0()
    x, Jx = prob.eval(p)
    Jp, Ji = prob.pattern()
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_pattern(Jp, Ji)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    J = _dense_J(Jp, Ji, Jx, prob.M, prob.N)
    zero = np.where(~np.any(J != 0.0, axis=0))[0]
    assert len(zero) == 3
    ok0 = be.factorize(0, 0.0)

    def outcome(f):
        try:
            return ("ok", f())
        except capi.DlgError:
            return ("refused", None)
    a = outcome(lambda: be.covariance_blocks(0, np.array([zero[0]], np.int32), np.array([1], np.int32),
                                             np.array([zero[0]], np.int32), np.array([1], np.int32))[0])
    b = outcome(lambda: _call(be, [[[(int(zero[0]), 1.0)]]])[0])
    print(f"lambda = 0: factorisation ok={ok0}; covariance blocks {a[0]}, query {b[0]}")
    assert a[0] == b[0]
    if a[0] == "ok":
        assert np.array_equal(np.isfinite(a[1]), np.isfinite(b[1]))
    lam = 1e-6
    assert be.factorize(0, lam)
    B = _call(be, [[[(int(z), 1.0)] for z in zero]])[0]
    assert np.allclose(np.diag(B), 1.0 / lam, rtol=1e-9, atol=0)
    be.close()


# ---------------------------------------------------------------- the public API from C
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("qcov") / "query_harness")
    cmd = ["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "query_harness.c"), "-o", exe,
           "-L", os.path.join(ROOT, "libdogleg_amd"), "-ldogleg_amd",
           "-L", os.path.join(ROOT, "problems"), "-lproblems", "-lm",
           "-Wl,-rpath," + os.path.join(ROOT, "libdogleg_amd"), "-Wl,-rpath," + os.path.join(ROOT, "problems")]
    subprocess.run(cmd, check=True)
    return exe


def test_public_api_end_to_end(gpu, harness):
    r = subprocess.run([harness], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    out = {}
    for line in r.stdout.splitlines():
        if line.strip():
            k, *v = line.split()
            out[k] = v
    assert out.get("alive") == ["1"]
    assert out["rc"] == ["0", "0", "0"], out["rc"]
    pub = np.array([float.fromhex(v) for v in out["public"]])
    be_ = np.array([float.fromhex(v) for v in out["backend"]])
    obs = np.array([float.fromhex(v) for v in out["public_obs"]])
    assert len(pub) == len(be_) > 0 and np.array_equal(pub, be_)
    assert np.all(np.isfinite(obs)) and np.max(np.abs(obs)) > 0
