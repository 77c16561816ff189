"""The selected inverse: dlg_covariance_entries returns Sigma = inv(JtJ + lambda I) at entries of the structure of the
factor held on the device, all of them from one sweep over the supernodal tree.

Checked against numpy's inverse on small problems (every entry of the structure, fill included), against
dlg_covariance_blocks and dlg_marginal_variances on configs #3 and #4, on the whole structure of JtJ of config #4, on
supernodes wider than the chunk route takes, on a singular JtJ, on the dense and dense-products backends, for
reproducibility and independence of the other entries, for its refusals, across pattern changes and from C
(tests/c/selinv_harness.c) on the point dogleg_optimize2 left behind.  The tolerance is that of
test_covariance_gpu.py: 1e-9 scaled by sqrt(Sigma_ii Sigma_jj)."""
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
TOL = 1e-9


def _dense_J(Jp, Ji, Jx, M, N):
    J = np.zeros((M, N))
    for r in range(M):
        J[r, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
    return J


def _backend(N, M, Jp, Ji, p, x, Jx, lam):
    be = capi.Backend(capi.DLG_SPARSE, N, M, len(Ji))
    be.set_pattern(Jp, Ji)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    assert be.factorize(0, lam)
    return be


def _ba_backend(prob, lam):
    p = prob.p0()
    x, Jx = prob.eval(p)
    Jp, Ji = prob.pattern()
    return _backend(prob.N, prob.M, Jp, Ji, p, x, Jx, lam), Jp, Ji, Jx


def _structure(N, M, Jp, Ji):
    """every lower entry (i >= j) of the structure of the factor, by the host probe"""
    ii, jj = np.tril_indices(N)
    ins, st = capi.covariance_entries_probe(N, M, Jp, Ji, ii, jj)
    assert int(np.sum(ins)) == st["nnz"]
    return ii[ins].astype(np.int32), jj[ins].astype(np.int32)


def _jtj_lower(N, Jp, Ji):
    """the lower structure of JtJ: every pair of variables that share a measurement row"""
    pairs = set()
    for r in range(len(Jp) - 1):
        c = np.sort(Ji[Jp[r]:Jp[r + 1]])
        a, b = np.meshgrid(c, c, indexing="ij")
        m = a >= b
        pairs.update(zip(a[m].tolist(), b[m].tolist()))
    pairs = np.array(sorted(pairs), dtype=np.int32)
    return pairs[:, 0].copy(), pairs[:, 1].copy()


def _scaled_err(vals, ref, d, i, j):
    return float(np.max(np.abs(vals - ref) / np.sqrt(d[i] * d[j])))


def _check_numpy(be, N, M, Jp, Ji, Jx, lam):
    J = _dense_J(Jp, Ji, Jx, M, N)
    S = np.linalg.inv(J.T @ J + lam * np.eye(N))
    d = np.diag(S)
    i, j = _structure(N, M, Jp, Ji)
    vals = be.covariance_entries(0, i, j)
    err = _scaled_err(vals, S[i, j], d, i, j)
    return err, len(i), S, i, j, vals


# ---------------------------------------------------------------- small problems against numpy
@pytest.mark.parametrize("lam", [0.0, 1e-3])
@pytest.mark.parametrize("shape", [(12, 120, 720), (49, 900, 10000)], ids=["small", "medium"])
def test_structure_matches_numpy(gpu, shape, lam):
    prob = oa.BAProblem(*shape, seed=3)
    be, Jp, Ji, Jx = _ba_backend(prob, lam)
    err, n, S, i, j, vals = _check_numpy(be, prob.N, prob.M, Jp, Ji, Jx, lam)
    ti, tj = _jtj_lower(prob.N, Jp, Ji)
    print(f"{shape} lambda={lam}: {n} entries of the structure ({len(ti)} of JtJ), scaled error {err:.2e}")
    assert err <= TOL
    assert n > len(ti)                               # fill is part of it
    # the other order of every entry: the same bits
    assert np.array_equal(be.covariance_entries(0, j, i), vals)
    be.close()


# ---------------------------------------------------------------- large configs against the existing routes
def _blocks_values(be, i, j):
    """Sigma[i, j] through dlg_covariance_blocks, one 1 x 1 request per entry"""
    one = np.ones(len(i), dtype=np.int32)
    return np.array([B[0, 0] for B in be.covariance_blocks(0, i, one, j, one)])


def _sample_ba_entries(Nc, Np, Jp, Ji, rng, n):
    """global, camera, point and observed camera x point entries"""
    cam0, pt0 = G, G + BC * Nc
    out = []
    for _ in range(n // 4):
        a, b = rng.integers(0, G, 2)
        out.append((a, b))
        c = rng.integers(Nc)
        out.append((cam0 + BC * c + rng.integers(BC), cam0 + BC * c + rng.integers(BC)))
        p = rng.integers(Np)
        out.append((pt0 + BP * p + rng.integers(BP), pt0 + BP * p + rng.integers(BP)))
        r = 2 * rng.integers((len(Jp) - 1) // 2)
        cols = Ji[Jp[r]:Jp[r + 1]]
        out.append((int(cols[G + rng.integers(BC)]), int(cols[G + BC + rng.integers(BP)])))
    out += [(rng.integers(G), cam0 + rng.integers(BC * Nc)) for _ in range(n // 8)]
    out += [(rng.integers(G), pt0 + rng.integers(BP * Np)) for _ in range(n // 8)]
    a = np.array(out, dtype=np.int32)
    return a[:, 0].copy(), a[:, 1].copy()


@pytest.mark.parametrize("cfg", [3, 4])
def test_configs_against_blocks_and_variances(gpu, cfg):
    Nc, Np, Nobs = {3: (499, 9000, 100000), 4: (2499, 45000, 500000)}[cfg]
    prob = oa.BAProblem(Nc, Np, Nobs, seed=1)
    be, Jp, Ji, Jx = _ba_backend(prob, 0.0)
    var = be.marginal_variances(0)
    N = prob.N
    diag = be.covariance_entries(0, np.arange(N), np.arange(N))
    derr = float(np.max(np.abs(diag - var) / var))
    i, j = _sample_ba_entries(Nc, Np, Jp, Ji, np.random.default_rng(cfg), 4000)
    vals = be.covariance_entries(0, i, j)
    ref = _blocks_values(be, i, j)
    err = _scaled_err(vals, ref, var, i, j)
    print(f"config #{cfg}: diagonal against dlg_marginal_variances {derr:.2e}; {len(i)} entries against "
          f"dlg_covariance_blocks {err:.2e}")
    assert derr <= TOL and err <= TOL
    be.close()


def test_config4_whole_structure_of_jtj(gpu):
    Nc, Np = 2499, 45000
    prob = oa.BAProblem(Nc, Np, 500000, seed=1)
    be, Jp, Ji, Jx = _ba_backend(prob, 0.0)
    N = prob.N
    cam0, pt0 = G, G + BC * Nc
    # the lower structure of JtJ from the block layout: globals x everything, camera and point blocks, observed pairs
    rows, cols = [], []
    gi, gj = np.tril_indices(G)
    rows.append(gi); cols.append(gj)
    rows.append(np.repeat(np.arange(G, N), G)); cols.append(np.tile(np.arange(G), N - G))
    for base, nb, w in ((cam0, Nc, BC), (pt0, Np, BP)):
        a, b = np.tril_indices(w)
        off = base + w * np.arange(nb)
        rows.append((off[:, None] + a[None, :]).ravel()); cols.append((off[:, None] + b[None, :]).ravel())
    r = np.arange(0, prob.M, 2)
    cam = Ji[Jp[r] + G]
    pt = Ji[Jp[r] + G + BC]
    obs = np.unique(np.stack([(cam - cam0) // BC, (pt - pt0) // BP], 1), axis=0)
    a, b = np.meshgrid(np.arange(BP), np.arange(BC), indexing="ij")
    rows.append((pt0 + BP * obs[:, 1, None] + a.ravel()[None, :]).ravel())
    cols.append((cam0 + BC * obs[:, 0, None] + b.ravel()[None, :]).ravel())
    i = np.concatenate(rows).astype(np.int32)
    j = np.concatenate(cols).astype(np.int32)
    vals = be.covariance_entries(0, i, j)
    t, nsx, nfront = be.covariance_entries_stats()
    var = be.marginal_variances(0)
    assert np.all(np.isfinite(vals))
    # the diagonal among them, and a sample against dlg_covariance_blocks
    dm = i == j
    assert float(np.max(np.abs(vals[dm] - var[i[dm]]) / var[i[dm]])) <= TOL
    k = np.random.default_rng(0).choice(len(i), 3000, replace=False)
    err = _scaled_err(vals[k], _blocks_values(be, i[k], j[k]), var, i[k], j[k])
    print(f"config #4: {len(i)} entries of JtJ ({len(obs)} observed pairs) in one call; Sx {nsx} values, fronts "
          f"{nfront} doubles, plan {t:.3f} s; sample against the blocks {err:.2e}")
    assert err <= TOL
    be.close()


# ---------------------------------------------------------------- wide supernodes
def _wide_problem(wa, ws, rows_per, seed):
    """two dense groups of wa columns that share a dense separator of ws columns: every dense block is wider than the
    16-variable requests of dlg_covariance_blocks, and the separator is wider than the 128 columns its chunk route takes
    whole; the symbolic phase cuts such blocks into supernodes whose panels fit LDS (at most about 100 columns), whose
    fronts (up to wa + ws rows) do not fit LDS"""
    rng = np.random.default_rng(seed)
    N = 2 * wa + ws
    groups = [np.r_[0:wa, 2 * wa:N], np.r_[wa:2 * wa, 2 * wa:N]]
    Jp, Ji, Jx = [0], [], []
    for g in groups:
        for _ in range(rows_per):
            Ji.extend(g.tolist())
            Jx.extend(rng.standard_normal(len(g)).tolist())
            Jp.append(len(Ji))
    Jp, Ji, Jx = np.array(Jp, dtype=np.int32), np.array(Ji, dtype=np.int32), np.array(Jx)
    M = len(Jp) - 1
    return N, M, Jp, Ji, Jx, rng.standard_normal(M)


@pytest.mark.parametrize("wa,ws", [(140, 150), (60, 200)], ids=["wide-children", "wide-root"])
def test_wide_supernodes(gpu, wa, ws):
    N, M, Jp, Ji, Jx, x = _wide_problem(wa, ws, wa + ws + 40, 7)
    sym = capi.symbolic_probe(N, M, Jp, Ji)
    be = _backend(N, M, Jp, Ji, np.zeros(N), x, Jx, 1e-3)
    err, n, *_ = _check_numpy(be, N, M, Jp, Ji, Jx, 1e-3)
    _, nsx, nfront = be.covariance_entries_stats()
    _, st = capi.covariance_entries_probe(N, M, Jp, Ji, [0], [0])
    print(f"wa={wa} ws={ws}: {sym['supernodes']} supernodes (widest {st['wmax']}), {n} entries, front {nfront} doubles "
          f"(LDS holds {160 * 1024 // 8}), scaled error {err:.2e}")
    assert nfront * 8 > 160 * 1024                   # the fronts do not fit in LDS
    assert err <= TOL
    be.close()


# ---------------------------------------------------------------- singular JtJ
def test_singular_columns(gpu):
    lam = 1e-6
    prob = oa.BAProblem(12, 120, 720, seed=2, n_zero_cols=3)
    be, Jp, Ji, Jx = _ba_backend(prob, lam)
    J = _dense_J(Jp, Ji, Jx, prob.M, prob.N)
    zero = np.where(~np.any(J != 0.0, axis=0))[0]
    assert len(zero) == 3
    vals = be.covariance_entries(0, zero, zero)
    assert np.allclose(vals, 1.0 / lam, rtol=1e-9, atol=0)
    err, *_ = _check_numpy(be, prob.N, prob.M, Jp, Ji, Jx, lam)
    assert err <= TOL
    be.close()


# ---------------------------------------------------------------- dense and dense-products
@pytest.mark.parametrize("lam", [0.0, 1e-2])
@pytest.mark.parametrize("kind", ["dense", "products_packed_upper", "products_unpacked"])
def test_dense_matches_numpy(gpu, kind, lam):
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
    i, j = np.tril_indices(N)
    vals = be.covariance_entries(0, i, j)
    err = _scaled_err(vals, S[i, j], d, i, j)
    print(f"{kind} lambda={lam}: {len(i)} entries, scaled error {err:.2e}")
    assert err <= TOL
    assert np.array_equal(be.covariance_entries(0, j, i), vals)
    be.close()


# ---------------------------------------------------------------- reproducibility, independence
def test_reproducible_and_independent(gpu):
    prob = oa.BAProblem(49, 900, 10000, seed=5)
    be, Jp, Ji, Jx = _ba_backend(prob, 1e-3)
    i, j = _structure(prob.N, prob.M, Jp, Ji)
    v1 = be.covariance_entries(0, i, j)
    v2 = be.covariance_entries(0, i, j)
    assert np.array_equal(v1, v2), "two calls differ"
    perm = np.random.default_rng(2).permutation(len(i))
    v3 = be.covariance_entries(0, i[perm], j[perm])
    assert np.array_equal(v3, v1[perm]), "values changed with the order"
    for k in (0, 7, len(i) // 2, len(i) - 1):
        assert np.array_equal(be.covariance_entries(0, i[k:k + 1], j[k:k + 1]), v1[k:k + 1])
    be.close()


# ---------------------------------------------------------------- refusals
def test_refusals(gpu):
    prob = oa.BAProblem(5, 40, 300, seed=11)
    be, Jp, Ji, Jx = _ba_backend(prob, 0.0)
    N = prob.N
    ii, jj = np.tril_indices(N)
    ins, _ = capi.covariance_entries_probe(N, prob.M, Jp, Ji, ii, jj)
    assert not np.all(ins)
    off = (int(ii[~ins][0]), int(jj[~ins][0]))
    with pytest.raises(capi.DlgError, match="dlg_covariance_blocks"):
        be.covariance_entries(0, [0, off[0]], [0, off[1]])
    for bad in [(-1, 0), (0, N), (N, N)]:
        with pytest.raises(capi.DlgError):
            be.covariance_entries(0, [0, bad[0]], [0, bad[1]])
    z = np.zeros(1, dtype=np.int32)
    assert be.L.dlg_covariance_entries(be.h, 0, 0, None, None, None) == 0          # n == 0
    assert be.L.dlg_covariance_entries(be.h, 0, -1, iptr(z), iptr(z), dptr(np.zeros(1))) != 0
    assert be.L.dlg_covariance_entries(be.h, 0, 1, None, iptr(z), dptr(np.zeros(1))) != 0
    assert be.L.dlg_covariance_entries(be.h, 0, 1, iptr(z), iptr(z), None) != 0
    with pytest.raises(capi.DlgError, match="no factorization"):
        be.covariance_entries(1, [0], [0])                       # slot 1 holds no factor
    assert be.covariance_entries(0, [0], [0])[0] > 0             # (still fine after the refusals)
    be.close()
    # no pattern
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    with pytest.raises(capi.DlgError):
        be.covariance_entries(0, [0], [0])
    be.close()
    # a partitioned backend
    prob = oa.BAProblem(49, 900, 10000, seed=5)
    Jp, Ji = prob.pattern()
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_partition(0, 2)
    be.set_pattern(Jp, Ji)
    with pytest.raises(capi.DlgError, match="sharded or partitioned"):
        be.covariance_entries(0, [0], [0])
    be.close()


# ---------------------------------------------------------------- pattern changes
def test_pattern_dropped_and_set_again(gpu):
    Nc, Np, Nobs = 12, 120, 720
    prob = oa.BAProblem(Nc, Np, Nobs, seed=3)
    Jp, Ji = prob.pattern()
    pt0 = G + BC * Nc
    relabel = np.random.default_rng(6).permutation(Np)
    Ji2 = Ji.copy()
    pts = Ji >= pt0
    Ji2[pts] = pt0 + BP * relabel[(Ji[pts] - pt0) // BP] + (Ji[pts] - pt0) % BP
    pats = [(Jp, Ji), (Jp, Ji2)]
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    p = prob.p0()
    x, Jx = prob.eval(p)
    for k, s in enumerate([0, 1, 0, 1]):
        Jpk, Jik = pats[s]
        if k > 0:
            assert be.L.dlg_sparse_drop_pattern(be.h) == 0
            with pytest.raises(capi.DlgError):
                be.covariance_entries(0, [0], [0])
        be.set_pattern(Jpk, Jik)
        be.set_p(0, p)
        be.upload(0, x, Jx)
        be.eval(0)
        lam = 1e-3 * k
        assert be.factorize(0, lam)
        err, *_ = _check_numpy(be, prob.N, prob.M, Jpk, Jik, Jx, lam)
        assert err <= TOL, (k, s)
        if k == 1:
            # a reset forgets the factor and the inputs: upload them again
            assert be.L.dlg_backend_reset(be.h) == 0
            with pytest.raises(capi.DlgError):
                be.covariance_entries(0, [0], [0])
            be.set_p(0, p)
            be.upload(0, x, Jx)
            be.eval(0)
            assert be.factorize(0, lam)
            err, *_ = _check_numpy(be, prob.N, prob.M, Jpk, Jik, Jx, lam)
            assert err <= TOL
    be.close()


# ---------------------------------------------------------------- the public API from C
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("selinv") / "selinv_harness")
    cmd = ["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "selinv_harness.c"), "-o", exe,
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
    ent = np.array(out["ent"], dtype=int).reshape(-1, 2)
    for tag in ("before", "fresh"):
        assert out[f"{tag}_rc"] == ["0"], (tag, out[f"{tag}_rc"])
        J = _dense_J(np.array(out[f"{tag}_Jp"], dtype=np.int32), np.array(out[f"{tag}_Ji"], dtype=np.int32),
                     _f(out[f"{tag}_Jx"]), M, N)
        lam = _f(out[f"{tag}_lambda"])[0]
        S = np.linalg.inv(J.T @ J + lam * np.eye(N))
        d = np.diag(S)
        got = _f(out[f"{tag}_vals"])
        err = _scaled_err(got, S[ent[:, 0], ent[:, 1]], d, ent[:, 0], ent[:, 1])
        print(f"{tag}: lambda {lam:.3g}, {len(ent)} entries, scaled error {err:.2e}")
        assert err <= TOL
    assert out["refuse"] == ["-1", "-1"]
