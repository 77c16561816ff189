"""The users of the factor held on the device -- dlg_solve_with_factor, dlg_solve_multi, dlg_pseudoinverse_chunk,
dlg_feature_leverage, dlg_marginal_variances, dlg_covariance_blocks, dlg_covariance_entries, dlg_query_covariance --
beyond bundle adjustment, under every schedule and on a factor that has a history.

A  every user on every case of tests/factor_user_zoo.py (one supernode of 16 .. 128 columns with no rows below, merged
   leaves, chains, empty rows, untouched variables, fronts that do not fit LDS) against the extended-precision inverse,
   within max(16 u kappa, 64 N u) in the measures of that module; the full-sweep route (DOGLEG_AMD_LEVERAGE_SWEEP) too.
B  every user under every environment of test_sparse_gpu.FALLBACK_ENVS (they change which kernels write the panels and
   how the supernodes are cut) and two more, against numpy's float64 inverse within the ceilings the suite has for each
   entry point.
C  every user as the first call behind a displacement of the factor by the next point's factorisation (one backend per
   entry point), every user behind the driver's retry of a step (bit for bit as with DOGLEG_AMD_NO_PRESOLVE), and every
   user on panels that were cleared in part only (bit for bit as with DOGLEG_AMD_FULL_CLEAR)."""
import functools

import numpy as np
import pytest

from libdogleg_amd import capi
from tests import factor_user_zoo as zoo
from tests import oracle_api as oa
from tests.test_covariance_gpu import _ba_requests
from tests.test_query_covariance_gpu import _csr, _pixel_queries
from tests.test_selected_inverse_gpu import _structure
from tests.test_sparse_gpu import FALLBACK_ENVS, FALLBACK_IDS

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _backend(N, M, Jp, Ji, p, x, Jx, lam):
    be = capi.Backend(capi.DLG_SPARSE, N, M, len(Ji))
    be.set_pattern(Jp, Ji)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    assert be.factorize(0, lam)
    return be


def _blocks_of_packed(A, fs):
    """dlg_feature_leverage's packed upper triangles as (fs, fs) arrays"""
    if fs == 1:
        return [np.array([[a]]) for a in A]
    return [np.array([[a, b], [b, c]]) for a, b, c in A]


# ================================================================ A: every user on every case
def _zoo_block_requests(N, rng):
    """(r0, nr, c0, nc): every diagonal block of 16 consecutive variables (the last one shorter), the two corners, 40
    random 8 x 8 blocks off the diagonal (most of them between subtrees: entries outside the structure of the factor), one
    request whose row and column ranges overlap in part"""
    req = [(a, min(16, N - a), a, min(16, N - a)) for a in range(0, N, 16)]
    req += [(0, 1, 0, 1), (N - 1, 1, N - 1, 1)]
    while len(req) < N // 16 + (N % 16 > 0) + 2 + 40:
        r0 = int(rng.integers(0, N - 7))
        free = [c for c in range(0, N - 7) if abs(c - r0) >= 8]
        if free:                                             # (N = 16: only 0 and 8 have a block beside them)
            req.append((r0, 8, int(rng.choice(free)), 8))
    a = N // 2 - 6
    req.append((a, 8, a + 4, 8))
    return req


def _zoo_queries(N, rng):
    """queries of 1, 2, 5 and 16 rows with 1 - 6 random variables a row; a row that names a variable twice; rows whose
    values are all zero (alone, and beside a row that is not)"""
    def row():
        k = int(rng.integers(1, 7))
        return (rng.choice(N, size=min(k, N), replace=False).astype(np.int64), rng.standard_normal(min(k, N)))
    qs = [[row() for _ in range(fs)] for fs in (1, 2, 5, 16)]
    v, x = row()
    qs.append([(np.r_[v, v[0]], np.r_[x, 0.75])])
    v, x = row()
    qs.append([(v, np.zeros(len(v)))])
    v, x = row()
    qs.append([row(), (v, np.zeros(len(v)))])
    return qs


def _call_queries(be, qs, nobs):
    return be.query_covariance(0, *_csr([[list(zip(var, val)) for var, val in rows] for rows in qs]), nobs=nobs)


@pytest.mark.parametrize("name", zoo.NAMES)
def test_every_user_on(gpu, name, monkeypatch):
    N, M, Jp, Ji, Jx, x, lam = zoo.case(name)
    S, _ = zoo.truth(name)
    d = np.diag(S)
    bnd = zoo.bound(name)
    J = zoo.dense_J(name)
    rng = np.random.default_rng(7)
    be = _backend(N, M, Jp, Ji, np.zeros(N), x, Jx, lam)
    worst = {}

    def note(what, err):
        worst[what] = max(worst.get(what, 0.0), err)

    # ---- solves
    rhs = rng.standard_normal((33, N))
    want = rhs.astype(LD) @ S
    note("solve_with_factor", zoo.solve_error(be.solve_with_factor(0, rhs[:3]), want[:3]))
    for nrhs in (1, 16, 17, 33):
        note("solve_multi", zoo.solve_error(be.solve_multi(0, rhs[:nrhs]), want[:nrhs]))
    ranges = [(0, 1), (0, 16), (M - 17, M)]
    if name == "holes":
        assert Jp[35] == Jp[34]                              # an empty row inside the range
        ranges.append((30, 40))
    for r0, r1 in ranges:
        note("pseudoinverse_chunk", zoo.solve_error(be.pseudoinverse_chunk(0, r0, r1), J[r0:r1].astype(LD) @ S))

    # ---- leverage, covariance, queries: by the supernodes a chunk reaches, then by full solves
    rows = zoo.measurement_rows(name, 0, M)
    lev_want = {fs: zoo.exact_blocks(name, [rows[f * fs:(f + 1) * fs] for f in range(M // fs)]) for fs in (1, 2)}
    req = _zoo_block_requests(N, rng)
    r0, nr, c0, nc = (np.array(a, dtype=np.int32) for a in zip(*req))
    qs = _zoo_queries(N, rng)
    q_want = {-1: zoo.exact_blocks(name, qs)}
    for nobs in (M, M // 2):
        q_want[nobs] = zoo.exact_sandwich_blocks(name, qs, nobs)
    for route in ("", " (full sweep)"):
        if route:
            monkeypatch.setenv("DOGLEG_AMD_LEVERAGE_SWEEP", "1")
        for fs in (1, 2):
            got = _blocks_of_packed(be.feature_leverage(0, fs, 0, M // fs), fs)
            note("feature_leverage" + route, max(zoo.block_error(g, w) for g, w in zip(got, lev_want[fs])))
        var = be.marginal_variances(0)
        note("marginal_variances" + route, zoo.entry_error(var, d, d, d))
        blocks = be.covariance_blocks(0, r0, nr, c0, nc)
        for B, (a, na, c, ncol) in zip(blocks, req):
            note("covariance_blocks" + route,
                 zoo.entry_error(B, S[a:a + na, c:c + ncol], d[a:a + na, None], d[None, c:c + ncol]))
        for nobs in (-1, M, M // 2):
            got = _call_queries(be, qs, nobs)
            note("query_covariance" + route + (" sandwich" if nobs >= 0 else ""),
                 max(zoo.block_error(g, w) for g, w in zip(got, q_want[nobs])))
    monkeypatch.delenv("DOGLEG_AMD_LEVERAGE_SWEEP")

    # ---- the selected inverse: every lower entry of the structure of the factor
    i, j = _structure(N, M, Jp, Ji)
    note("covariance_entries", zoo.entry_error(be.covariance_entries(0, i, j), S[i, j], d[i], d[j]))
    if name == "holes":
        assert np.allclose(var[N - 5:], 1.0 / lam, rtol=bnd, atol=0)
    be.close()

    for what, err in worst.items():
        print(f"zoo {name:16s} {what:40s} {err:9.2e}   bound {bnd:.2e}")
    bad = {what: err for what, err in worst.items() if not err <= bnd}
    assert not bad, (name, bnd, bad)


# ================================================================ B: every user under every schedule
ENVS = [{}] + FALLBACK_ENVS + [{"DOGLEG_AMD_LDS_SPLIT": "0"}, {"DOGLEG_AMD_FULL_CLEAR": "1"}]
ENV_IDS = ["default"] + FALLBACK_IDS + ["lds-split-off", "full-clear"]
# dlg_sparse_schedule shows the levels and the one-launch region only, dlg_sparse_stats the supernodes.  These four knobs
# move one of them on this pattern (the host planner says so: capi.region_probe, capi.symbolic_probe), and the test
# asserts that they did.  The OTHER knobs (assembly and update kernels, workgroup sizes and replicas inside the region,
# a region that is as deep as it can go already, ...) leave all of that as it is: that they were read is NOT checked here.
SCHEDULE_DIFFERS = {"small-slices", "no-multifrontal", "no-persistent-top", "lds-split-off"}
BA_SHAPE = (49, 900, 10000)
BA_LAM = 1e-3


def _jtj_entries(Jp, Ji, rng, n):
    """n entries (i >= j) of the structure of JtJ: two variables of one measurement row"""
    out = np.zeros((n, 2), dtype=np.int32)
    for e in range(n):
        r = int(rng.integers(len(Jp) - 1))
        a, b = rng.choice(Ji[Jp[r]:Jp[r + 1]], 2)
        out[e] = (max(a, b), min(a, b))
    return out[:, 0].copy(), out[:, 1].copy()


@functools.lru_cache(maxsize=None)
def _ba():
    """the problem of part B, its requests and numpy's float64 inverse: computed once, left unchanged"""
    Nc, Np, Nobs = BA_SHAPE
    prob = oa.BAProblem(Nc, Np, Nobs, seed=5)
    p = prob.p0()
    x, Jx = prob.eval(p)
    Jp, Ji = prob.pattern()
    N, M = prob.N, prob.M
    A = BA_LAM * np.eye(N)
    for r in range(M):                                       # JtJ row by row: 15 variables a row
        idx = Ji[Jp[r]:Jp[r + 1]]
        A[np.ix_(idx, idx)] += np.outer(Jx[Jp[r]:Jp[r + 1]], Jx[Jp[r]:Jp[r + 1]])
    S = np.linalg.inv(A)
    rng = np.random.default_rng(12)
    K = dict(prob=prob, p=p, x=x, Jx=Jx, Jp=Jp, Ji=Ji, S=S, d=np.diag(S).copy())
    K["rhs"] = rng.standard_normal((17, N))
    K["feats"] = [(0, 512), (M // 2 - 100, 100)]
    K["req"] = _ba_requests(Nc, Np, Jp, Ji, rng, n_obs=200, n_unobs=50)
    K["ent"] = _jtj_entries(Jp, Ji, rng, 3000)
    K["queries"] = _pixel_queries(Nc, Np, rng, 200)
    Q = np.zeros((2 * len(K["queries"]), N))
    for k, rows in enumerate(K["queries"]):
        for a, row in enumerate(rows):
            for v, val in row:
                Q[2 * k + a, v] += val
    K["Q"] = Q
    return K


def _lev_ref(K, f0, nf):
    """{a00, a01, a11} of J_f Sigma J_f^T, features of 2 rows"""
    Jp, Ji, Jx, N = K["Jp"], K["Ji"], K["Jx"], K["prob"].N
    out = np.zeros((nf, 3))
    for k in range(nf):
        Jf = np.zeros((2, N))
        for a in range(2):
            r = 2 * (f0 + k) + a
            Jf[a, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
        A = Jf @ K["S"] @ Jf.T
        out[k] = (A[0, 0], A[0, 1], A[1, 1])
    return out


@functools.lru_cache(maxsize=None)
def _ba_refs():
    K = _ba()
    S, Q = K["S"], K["Q"]
    SQ = S @ Q.T
    return dict(solve=K["rhs"] @ S, lev=[_lev_ref(K, f0, nf) for f0, nf in K["feats"]],
                query=[Q[2 * k:2 * k + 2] @ SQ[:, 2 * k:2 * k + 2] for k in range(len(K["queries"]))])


def _schedule(be):
    return dict(be.schedule(), n_supernodes=be.stats()["n_supernodes"])


@functools.lru_cache(maxsize=None)
def _default_schedule():
    """the schedule of the pattern with no knob set (called with none set: the knobs are read when the pattern is set)"""
    K = _ba()
    prob = K["prob"]
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_pattern(K["Jp"], K["Ji"])
    sched = _schedule(be)
    be.close()
    assert sched["persist_level0"] >= 1                      # (what the knobs are measured against: a region is there)
    return sched


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_every_user_under(gpu, env, request, monkeypatch):
    default = _default_schedule()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    K, R = _ba(), _ba_refs()
    prob, S, d = K["prob"], K["S"], K["d"]
    be = _backend(prob.N, prob.M, K["Jp"], K["Ji"], K["p"], K["x"], K["Jx"], BA_LAM)
    sched = _schedule(be)
    eid = request.node.callspec.id
    print(f"schedule {eid}: {env} {sched}")
    # solves: the norm-wise relative error of test_multi_rhs_gpu.py
    u = be.solve_multi(0, K["rhs"])
    e_solve = float(np.max(np.linalg.norm(u - R["solve"], axis=1) / np.linalg.norm(R["solve"], axis=1)))
    # leverage: the absolute error of test_outliers_gpu.py
    e_lev = max(float(np.max(np.abs(be.feature_leverage(0, 2, f0, nf) - ref))) for (f0, nf), ref in zip(K["feats"], R["lev"]))
    # covariance: scaled by sqrt(Sigma_ii Sigma_jj), test_covariance_gpu.py and test_selected_inverse_gpu.py
    e_var = float(np.max(np.abs(be.marginal_variances(0) - d) / d))
    req = K["req"]
    blocks = be.covariance_blocks(0, *(np.array(a, dtype=np.int32) for a in zip(*req)))
    e_blk = max(float(np.max(np.abs(B - S[r0:r0 + nr, c0:c0 + nc]) / np.sqrt(np.outer(d[r0:r0 + nr], d[c0:c0 + nc]))))
                for B, (r0, nr, c0, nc) in zip(blocks, req))
    i, j = K["ent"]
    e_ent = float(np.max(np.abs(be.covariance_entries(0, i, j) - S[i, j]) / np.sqrt(d[i] * d[j])))
    # queries: scaled by the largest entry of the block, test_query_covariance_gpu.py
    got = be.query_covariance(0, *_csr(K["queries"]))
    e_qry = max(float(np.max(np.abs(B - ref))) / float(np.max(np.abs(ref))) for B, ref in zip(got, R["query"]))
    be.close()
    print(f"under {eid}: solve_multi {e_solve:.2e}, leverage {e_lev:.2e}, variances {e_var:.2e}, blocks {e_blk:.2e}, "
          f"entries {e_ent:.2e}, queries {e_qry:.2e}")
    assert e_solve <= 1e-10 and e_lev <= 1e-10 and e_qry <= 1e-10
    assert e_var <= 1e-9 and e_blk <= 1e-9 and e_ent <= 1e-9
    if not env:
        assert sched == default
    elif eid in SCHEDULE_DIFFERS:
        assert sched != default, f"{env} left the schedule as it is: the knob was not read"


# ================================================================ C: users of a factor that has a history
def _small_requests(prob):
    """a small request set for every entry point on the pattern of a problem of BA_SHAPE"""
    Nc, Np, _ = BA_SHAPE
    Jp, Ji = prob.pattern()
    rng = np.random.default_rng(21)
    allreq = _ba_requests(Nc, Np, Jp, Ji, rng, n_obs=40, n_unobs=20)
    req = [allreq[k] for k in rng.choice(len(allreq), 20, replace=False)]
    return dict(M=prob.M, rhs=np.cos(0.01 * np.arange(2 * prob.N)).reshape(2, prob.N),
                req=tuple(np.array(a, dtype=np.int32) for a in zip(*req)),
                ent=_jtj_entries(Jp, Ji, rng, 500), queries=_csr(_pixel_queries(Nc, Np, rng, 20)))


def _users(R):
    """(name, call) of every entry point with its small request set R; a call returns arrays"""
    M = R["M"]
    return [
        ("solve_with_factor", lambda be: [be.solve_with_factor(0, R["rhs"])]),
        ("solve_multi", lambda be: [be.solve_multi(0, R["rhs"])]),
        ("pseudoinverse_chunk", lambda be: [be.pseudoinverse_chunk(0, 4321, 4321 + 17)]),
        ("feature_leverage", lambda be: [be.feature_leverage(0, 2, 1000, 64), be.feature_leverage(0, 1, 0, 64)]),
        ("marginal_variances", lambda be: [be.marginal_variances(0)]),
        ("covariance_blocks", lambda be: be.covariance_blocks(0, *R["req"])),
        ("covariance_entries", lambda be: [be.covariance_entries(0, *R["ent"])]),
        ("query_covariance", lambda be: be.query_covariance(0, *R["queries"])),
        ("query_covariance sandwich", lambda be: be.query_covariance(0, *R["queries"], nobs=M - 37)),
    ]


def _all_users(be, R, tag):
    out = []
    for name, call in _users(R):
        vals = [np.array(v, copy=True) for v in call(be)]
        assert all(np.all(np.isfinite(v)) for v in vals) and any(np.any(v != 0) for v in vals), (tag, name)
        out.append((f"{tag}: {name}", vals))
    return out


def _same_bits(got, want):
    assert [t for t, _ in got] == [t for t, _ in want]
    for (tag, a), (_, b) in zip(got, want):
        assert len(a) == len(b), tag
        for k, (u, v) in enumerate(zip(a, b)):
            # (a value that is not a number -- the k of a step that interpolates nothing -- equals itself)
            assert np.array_equal(u, v, equal_nan=True), f"{tag} [{k}]: {int(np.sum(u != v))} of {u.size} values differ, " \
                                                         f"by up to {float(np.nanmax(np.abs(u - v))):.3e}"


def _displaced_script(after_displacement):
    """A backend with speculation on takes the step A -> B and evaluates B in slot 1: dlg_point_eval enqueues B's
    factorisation where A's factor was (step_prepare).  after_displacement(be, tr, xB, JB) goes on from there and returns
    [(tag, arrays)].  Run twice, as it is and with DOGLEG_AMD_NO_PRESOLVE=1 (nothing is enqueued ahead, A's factor stays
    where it is): (got, want)."""
    K = _ba()
    prob, Jp, Ji, pA, xA, JA = K["prob"], K["Jp"], K["Ji"], K["p"], K["x"], K["Jx"]

    def run():
        be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
        be.set_pattern(Jp, Ji)
        be.set_speculation(True)
        be.set_p(0, pA)
        be.upload(0, xA, JA)
        be.eval(0)
        lam, n2c, n2g = be.cauchy_gauss_newton(0, 0.0)
        tr = 0.7 * np.sqrt(n2g)
        be.upload(0, xA, JA)
        be.eval(0)
        lam, r, pB = be.take_step(0, 1, tr, 0.0)               # A -> B: a step from a fresh point, the next evaluation prepares
        pB = pB.copy()
        xB, JB = prob.eval(pB)
        be.upload(1, xB, JB)
        be.eval(1)                                             # B's factorisation enqueued in A's place
        res = [("step", [pB])] + after_displacement(be, tr, xB, JB)
        be.close()
        return res
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("DOGLEG_AMD_NO_PRESOLVE", raising=False)
        got = run()
        mp.setenv("DOGLEG_AMD_NO_PRESOLVE", "1")
        want = run()
    finally:
        mp.undo()
    return got, want


USER_NAMES = ["solve_with_factor", "solve_multi", "pseudoinverse_chunk", "feature_leverage", "marginal_variances",
              "covariance_blocks", "covariance_entries", "query_covariance", "query_covariance sandwich"]


@pytest.mark.parametrize("user", USER_NAMES, ids=[u.replace(" ", "-") for u in USER_NAMES])
def test_a_user_gets_a_displaced_factor_back(gpu, user):
    """the "held" situation of test_sparse_gpu.test_factor_and_solve_ahead_of_the_decision_change_no_bit, one backend per
    entry point: the entry point is the FIRST call behind the displacement, so it is the one that has to bring A's factor
    back (dlg_factor_user_begin -> dlg_step_unprepare) before it reads a panel.  A first user marks the trial point as
    rejected, and no later evaluation enqueues anything ahead until a step is taken from a fresh point: behind it A's
    factor is plainly held.  The other entry points are called there too (what the restore left behind is what they
    read), then the step from B is taken.  All bits as with DOGLEG_AMD_NO_PRESOLVE."""
    R = _small_requests(_ba()["prob"])
    calls = dict(_users(R))
    assert list(calls) == USER_NAMES

    def after(be, tr, xB, JB):
        vals = [np.array(v, copy=True) for v in calls[user](be)]
        assert all(np.all(np.isfinite(v)) for v in vals) and any(np.any(v != 0) for v in vals)
        res = [(f"first behind the displacement: {user}", vals)]
        res += _all_users(be, R, "held again")
        lam, r, pC = be.take_step(1, 0, tr, 0.0)               # B: factorised in line now
        res.append(("next step", [np.array([lam] + [v for _, v in sorted(r.items())]), pC.copy()]))
        return res
    _same_bits(*_displaced_script(after))


def test_every_user_behind_the_drivers_retry(gpu):
    """the "driver-retry" situation of the same test for every entry point: with B's factorisation enqueued in A's place
    the driver takes the step from A again out of A's cached vectors (dlg_step).  That step brings A's factor back and its
    tail clears the spare panel buffer; every entry point then reads the restored panels.  The trial point counts as
    rejected from there on, so the evaluation of the next trial point enqueues nothing ahead: the entry points behind it
    find A's factor held, as they must.  All bits as with DOGLEG_AMD_NO_PRESOLVE."""
    prob = _ba()["prob"]
    R = _small_requests(prob)

    def after(be, tr, xB, JB):
        n2, k, amax, ei, pB2 = be.step(0, 1, capi.KIND_GN, 0.25 * tr)
        pB2 = pB2.copy()
        res = [("retry", [np.array([n2, k, amax, ei]), pB2])]
        res += _all_users(be, R, "behind the retry")
        n2, k, amax, pB3 = be.make_step(0, 1, capi.KIND_CAUCHY, 0.125 * tr)
        res.append(("cauchy", [np.array([n2, k, amax]), pB3.copy()]))
        xB2, JB2 = prob.eval(pB2)
        be.upload(1, xB2, JB2)
        be.eval(1)                                             # (after a rejection: nothing is enqueued ahead)
        res += _all_users(be, R, "behind the next trial point")
        return res
    _same_bits(*_displaced_script(after))


def test_every_user_after_partial_clears(gpu, monkeypatch):
    """the eight steps over three inputs of test_sparse_gpu.test_partial_clears_change_no_bit, then every entry point on
    the last factor: the bits of the same steps with full clears (DOGLEG_AMD_FULL_CLEAR).  What a partial clear leaves in
    the part of a merged leaf's top block that no leaf owns, these calls would read."""
    Nc, Np, Nobs = BA_SHAPE
    prob = oa.BAProblem(Nc, Np, Nobs, seed=6, eps=0.4, p0_spread=0.6)
    Jp, Ji = prob.pattern()
    R = _small_requests(prob)
    rng = np.random.default_rng(2)
    pts = [prob.p0() + 0.05 * c * rng.standard_normal(prob.N) for c in range(3)]
    inputs = [prob.eval(pts[i % 3]) for i in range(8)]

    def run():
        be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
        be.set_pattern(Jp, Ji)
        be.set_speculation(True)
        be.set_p(0, prob.p0())
        res, tr = [], None
        for x, Jx in inputs:
            be.upload(0, x, Jx)
            be.eval(0)
            if tr is None:
                lam, n2c, n2g = be.cauchy_gauss_newton(0, 0.0)
                tr = 0.5 * (n2c ** 0.5 + n2g ** 0.5)
                be.upload(0, x, Jx)
                be.eval(0)
            lam, r, pnew = be.take_step(0, 1, tr, 0.0)
            res.append(("step", [pnew.copy(), be.download(0, capi.VEC_GN)]))
        res += _all_users(be, R, "after eight steps")
        be.close()
        return res

    monkeypatch.delenv("DOGLEG_AMD_FULL_CLEAR", raising=False)
    got = run()
    monkeypatch.setenv("DOGLEG_AMD_FULL_CLEAR", "1")
    want = run()
    _same_bits(got, want)
