"""The lean leaf launch of the sparse factorisation: a level of merged point
leaves stores the augmented row only and leaves the rows below the member blocks as the assembly wrote them (W); the
backward solve takes L_below' x = L_tt^-1 (W' x) from them, every other reader of the factor gets L_below formed first,
once (k_leaf_rows_materialize).  DOGLEG_AMD_LEAF_STORE_ROWS=1 is the write-back of every row and the old formula: the
"old mode" of these tests.

The patterns: BAProblem(49, 900, 10000) has 50 merged leaves that the lean instantiation k_factor_level<256, true>
factors.  A level of fewer than 100 supernodes pushes its updates from the panels in HBM (k_update_mfma reads the rows
below), and such a level never runs lean; DOGLEG_AMD_SYRK_MIN=1 -- a knob of test_sparse_gpu.FALLBACK_ENVS -- gives this
small level the update route of the flagship's leaf level (update matrices out of the leaf launch's LDS copy, then the
gather), and with it the lean mode; the tests on this pattern set it in BOTH modes.  That the lean mode ran is asserted
through dlg_sparse_leaf_rows_stats in every test that is about it.  The pattern's backward leaf level runs in
k_solve_bwd_level<512, false> (fewer than 512 supernodes).  BAProblem(599, 10800, 120000) has 600 of them (default knobs): the
backward leaf level runs in the lean k_solve_bwd_level<256, true>, as on the flagship workload.  BAProblem(20, 300, 3000,
seed=3) has merged leaves too, but of at most 128 rows: its leaf level runs in k_factor_level<128>, never lean -- there,
and on a pattern without merged leaves, the two modes must agree bit for bit."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import dptr, iptr
from tests import factor_user_zoo as zoo
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

STORE_ROWS = "DOGLEG_AMD_LEAF_STORE_ROWS"
_problems = {}


def _problem(shape, **kw):
    """a problem, its pattern and one operating point, built once and left unchanged"""
    key = (shape, tuple(sorted(kw.items())))
    if key not in _problems:
        prob = oa.BAProblem(*shape, **kw)
        Jp, Ji = prob.pattern()
        p = prob.p0()
        x, Jx = prob.eval(p)
        _problems[key] = dict(prob=prob, Jp=Jp, Ji=Ji, p=p, x=x, Jx=Jx, syrk_min=shape[0] < 100)
    return _problems[key]


def _mode(mp, old, syrk_min=True):
    if syrk_min:
        mp.setenv("DOGLEG_AMD_SYRK_MIN", "1")
    else:
        mp.delenv("DOGLEG_AMD_SYRK_MIN", raising=False)
    if old:
        mp.setenv(STORE_ROWS, "1")
    else:
        mp.delenv(STORE_ROWS, raising=False)


def _backend(K, speculation=False):
    prob = K["prob"]
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_pattern(K["Jp"], K["Ji"])
    if speculation:
        be.set_speculation(True)
    be.set_p(0, K["p"])
    be.upload(0, K["x"], K["Jx"])
    be.eval(0)
    return be


def _assert_lean_ran(be, old, at_least=1):
    st = be.leaf_rows_stats()
    if old:
        assert st["lean_levels"] == 0 and st["lean_launches"] == 0 and not st["raw"], st
    else:
        assert st["lean_levels"] >= 1 and st["lean_launches"] >= at_least, st
    return st


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


_oracle_refs = {}


def _oracle_step(K, lam):
    """Cauchy step, Gauss-Newton step, the interpolated step between them at the trust region 0.5 (|cauchy| + |gn|) and its
    expected improvement, from the CPU oracle's primitives; once per (problem, lambda)"""
    key = (id(K), lam)
    if key in _oracle_refs:
        return _oracle_refs[key]
    O = oa.oracle()
    prob, Jp, Ji, x, Jx = K["prob"], K["Jp"], K["Ji"], K["x"], K["Jx"]
    N, M = prob.N, prob.M
    g = np.zeros(N)
    O.orc_spmv_Jt_x(dptr(g), N, M, iptr(Jp), iptr(Ji), dptr(Jx), dptr(x))
    g2 = O.orc_norm2(dptr(g), N)
    Jg2 = O.orc_norm2_J_v(M, iptr(Jp), iptr(Ji), dptr(Jx), dptr(g))
    cauchy = (-g2 / Jg2) * g
    F = O.orc_sparse_analyze(N, M, iptr(Jp), iptr(Ji))
    assert O.orc_sparse_factorize(F, iptr(Jp), iptr(Ji), dptr(Jx), lam) == N
    gn = np.zeros(N)
    O.orc_sparse_solve(F, dptr(g), dptr(gn))
    O.orc_sparse_free(F)
    gn *= -1
    tr = 0.5 * (np.linalg.norm(cauchy) + np.linalg.norm(gn))
    d = gn - cauchy
    A, B, Cq = d @ d, 2 * (cauchy @ d), cauchy @ cauchy - tr * tr
    k = (-B + np.sqrt(B * B - 4 * A * Cq)) / (2 * A)
    step = np.ascontiguousarray(cauchy + k * d)
    ei = -2 * (g @ step) - O.orc_norm2_J_v(M, iptr(Jp), iptr(Ji), dptr(Jx), dptr(step))
    _oracle_refs[key] = dict(cauchy=cauchy, gn=gn, tr=tr, step=step, ei=ei)
    return _oracle_refs[key]


def _device_step(K, lam, old, mp):
    """the same four on the device: errors against the oracle, relative"""
    ref = _oracle_step(K, lam)
    _mode(mp, old, K["syrk_min"])
    be = _backend(K)
    be.cauchy(0)
    assert be.factorize(0, lam)
    be.solve_gn(0)
    st = _assert_lean_ran(be, old)
    assert old or st["raw"], "the backward solve of the new mode must have found the rows raw"
    out = dict(cauchy=be.download(0, capi.VEC_CAUCHY), gn=be.download(0, capi.VEC_GN))
    n2s, kk, amax, pnew = be.make_step(0, 1, capi.KIND_INTERP, ref["tr"])
    out["step"] = be.download(1, capi.VEC_STEP)
    out["ei"] = be.expected_improvement(0, 1)
    st = be.leaf_rows_stats()
    assert st["materialized"] == 0, "nothing inside a step reads L_below of the leaves"
    be.close()
    err = {k: _rel(out[k], ref[k]) for k in ("cauchy", "gn", "step")}
    err["ei"] = abs(out["ei"] - ref["ei"]) / abs(ref["ei"])
    return err, out


BA_SMALL = ((49, 900, 10000), dict(seed=3))
BA_600 = ((599, 10800, 120000), dict(seed=11))


# ---------------------------------------------------------------- 1: a full step, new mode against old mode
@pytest.mark.parametrize("lam", [0.0, 1e-3], ids=["lambda=0", "lambda=1e-3"])
@pytest.mark.parametrize("which", [BA_SMALL, BA_600], ids=["50-leaves-bwd512", "600-leaves-bwd256-lean"])
def test_step_matches_oracle_as_well_as_with_the_rows_stored(gpu, which, lam, monkeypatch):
    """Cauchy step, Gauss-Newton step, interpolated step and expected improvement against the CPU oracle at the
    project's parity tolerance (1e-10 relative) in both modes; the new mode's error is at most twice
    the old mode's, or 1e-13."""
    K = _problem(which[0], **which[1])
    e_old, _ = _device_step(K, lam, True, monkeypatch)
    e_new, _ = _device_step(K, lam, False, monkeypatch)
    for k in ("cauchy", "gn", "step", "ei"):
        print(f"{which[0]} lambda={lam:g} {k}: error against the oracle: rows stored {e_old[k]:.3e}, lean {e_new[k]:.3e}")
    for k in ("cauchy", "gn", "step", "ei"):
        assert e_old[k] <= 1e-10 and e_new[k] <= 1e-10, (k, e_old[k], e_new[k])
        assert e_new[k] <= max(2 * e_old[k], 1e-13), (k, e_old[k], e_new[k])


# ---------------------------------------------------------------- 2: the users of the held factor
def _users_twice(K, old, mp):
    prob = K["prob"]
    _mode(mp, old)
    be = _backend(K)
    lam, n2c, n2g = be.cauchy_gauss_newton(0, 0.0)
    be.step(0, 1, capi.KIND_INTERP, 0.5 * (n2c ** 0.5 + n2g ** 0.5))
    st = _assert_lean_ran(be, old)
    assert st["materialized"] == 0 and st["raw"] == (not old)
    rhs = np.random.default_rng(5).standard_normal((3, prob.N))
    c0 = 6 * 49                                  # the first point's block and the camera block it couples to
    calls = [lambda: be.covariance_blocks(0, [c0], [3], [0], [6])[0],
             lambda: be.solve_multi(0, rhs),
             lambda: be.feature_leverage(0, 1, 0, 8)]
    first = [np.array(c(), copy=True) for c in calls]
    st = be.leaf_rows_stats()
    assert st["materialized"] == (0 if old else 1) and not st["raw"], st
    second = [np.array(c(), copy=True) for c in calls]
    assert be.leaf_rows_stats()["materialized"] == st["materialized"], "the second call must not form the rows again"
    be.close()
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert all(np.all(np.isfinite(a)) and np.any(a != 0) for a in first)
    return first


def test_held_factor_users_get_the_bits_of_the_stored_rows(gpu, monkeypatch):
    """one covariance block, dlg_solve_multi with 3 right-hand sides and the leverages of 8 rows behind a step: the
    materialised rows are the arithmetic of the write-back, so every bit is that of the old mode; each call twice --
    the rows are formed once"""
    K = _problem(BA_SMALL[0], **BA_SMALL[1])
    new = _users_twice(K, False, monkeypatch)
    old = _users_twice(K, True, monkeypatch)
    for a, b in zip(new, old):
        assert np.array_equal(a, b), f"{int(np.sum(a != b))} of {a.size} values differ, by up to {np.max(np.abs(a - b)):.3e}"


# ---------------------------------------------------------------- 3: hold and restore
def _reject_and_retry(K, old, mp):
    prob = K["prob"]
    _mode(mp, old)
    be = _backend(K, speculation=True)
    lam, n2c, n2g = be.cauchy_gauss_newton(0, 0.0)
    tr = 0.7 * np.sqrt(n2g)
    be.upload(0, K["x"], K["Jx"])
    be.eval(0)
    lam, r, pB = be.take_step(0, 1, tr, 0.0)                   # A -> B from a fresh point: the next evaluation prepares
    pB = pB.copy()
    xB, JB = prob.eval(pB)
    be.upload(1, xB, JB)
    be.eval(1)                                                 # B's factorisation enqueued where A's factor was: A's is held
    n2, k, amax, ei, pB2 = be.step(0, 1, capi.KIND_GN, 0.25 * tr)      # B rejected: the step from A again, off the held factor
    pB2 = pB2.copy()
    _assert_lean_ran(be, old, at_least=2)                      # (A at least twice: the first point and the fresh one; B's where it was enqueued)
    # the factor in place is A's again, in the buffer it was held in: its rows are raw as the leaf launch left them (the
    # state followed the exchange of the buffers), nothing has been formed yet, and the first user forms them, once
    st = be.leaf_rows_stats()
    assert st["raw"] == (not old) and st["materialized"] == 0, st
    blk = np.array(be.covariance_blocks(0, [6 * 49], [3], [0], [6])[0], copy=True)
    st = be.leaf_rows_stats()
    assert not st["raw"] and st["materialized"] == (0 if old else 1), st
    lev = np.array(be.feature_leverage(0, 1, 0, 8), copy=True)
    assert be.leaf_rows_stats()["materialized"] == st["materialized"]
    be.close()
    return dict(pB=pB, retry=np.array([n2, amax, ei]), pB2=pB2, blk=blk, lev=lev)      # (k of a Gauss-Newton step is not a number)


def test_hold_reject_and_retry_from_the_held_factor(gpu, monkeypatch):
    """a step in the new mode, the trial point's factorisation enqueued in the held factor's place, the trial point
    rejected and the step taken again from the held factor, then the users of that factor: the old mode's values at 1e-10"""
    K = _problem((49, 900, 10000), seed=5, eps=0.4, p0_spread=0.6)
    new = _reject_and_retry(K, False, monkeypatch)
    old = _reject_and_retry(K, True, monkeypatch)
    for k in new:
        e = _rel(new[k], old[k])
        print(f"hold/restore {k}: lean against rows stored {e:.3e}")
        assert e <= 1e-10, (k, e)


# ---------------------------------------------------------------- 4: the breakdown path
def test_sticky_lambda_path_is_the_same_in_both_modes(gpu, monkeypatch, capfd):
    """numerically-zero columns (the problem of test_shard_gpu's lambda-loop test): the factorisation at lambda = 0
    breaks down, lambda becomes 1e-10 and sticks.  The failed attempts leave leaves whose rows were never touched; the
    retries must not trip over their state.  lambda of every trial is the same in both modes and no call fails
    (DLG_ERR_STATE would make the solve return -1).  The iterates: bit for bit they cannot agree (the backward leaves round
    differently in the two modes); they agree to 1e-10 relative, the bound of every other comparison of the two modes
    here (measured: 9.5e-18, profiles/r07_experiments.md)."""
    prob = oa.BAProblem(49, 900, 10000, seed=9, n_zero_cols=2)
    prm = oa.default_params()
    prm.max_iterations = 5
    prm.trustregion0 = 100.0
    res = {}
    for old in (False, True):
        _mode(monkeypatch, old)
        monkeypatch.setenv("DOGLEG_AMD_SYM_DEBUG", "1")
        capfd.readouterr()
        r, p, tr = capi.optimize("sparse", prob.p0(), prob.N, prob.M, prob.nnz, prob.cb, prob.cookie, prm)
        err = capfd.readouterr().err
        assert ("factor level 0: lean leaf rows 1" in err) == (not old), err[-2000:]
        assert "leaf instantiation 1" in err
        assert r >= 0
        res[old] = (p.copy(), [t["lambda_"] for t in tr.trials()])
    monkeypatch.delenv("DOGLEG_AMD_SYM_DEBUG")
    assert res[False][1] == res[True][1] and 1e-10 in res[False][1], (res[False][1], res[True][1])
    e = _rel(res[False][0], res[True][0])
    print(f"sticky lambda: lambdas {res[False][1]}, iterates lean against rows stored {e:.3e}")
    assert e <= 1e-10


# ---------------------------------------------------------------- 5: two logical ranks on one device
def _rank_partials(K, rank, old, mp):
    prob, Jp, x, Jx = K["prob"], K["Jp"], K["x"], K["Jx"]
    _mode(mp, old)
    be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
    be.set_noop_comm(True)
    be.set_partition(rank, 2)
    be.set_pattern(K["Jp"], K["Ji"])
    rows = be.partition_rows()
    be.set_p(0, K["p"])
    be.upload(0, x[rows], np.concatenate([Jx[Jp[r]:Jp[r+1]] for r in rows]))
    be.eval(0)
    be.cauchy(0)
    lam, n2g = be.gauss_newton(0, 1.0)          # (lambda 1: the rank's partial top of the tree must stay positive definite)
    assert lam == 1.0
    _assert_lean_ran(be, old)
    gn = be.download(0, capi.VEC_GN)
    be.close()
    return gn


@pytest.mark.parametrize("rank", [0, 1])
def test_a_logical_ranks_gauss_newton_partials(gpu, rank, monkeypatch):
    """rank 0 / 1 of a partition over two ranks on this one device, the sums over the ranks skipped
    (dlg_backend_set_noop_comm, as bench.py --logical-ranks): the rank's own leaf level runs lean too, and its
    Gauss-Newton partials are the old mode's at 1e-10"""
    K = _problem(BA_SMALL[0], **BA_SMALL[1])
    new = _rank_partials(K, rank, False, monkeypatch)
    old = _rank_partials(K, rank, True, monkeypatch)
    e = _rel(new, old)
    print(f"rank {rank} of 2: Gauss-Newton partials lean against rows stored {e:.3e}")
    assert np.any(new != 0) and e <= 1e-10


# ---------------------------------------------------------------- 6: where the path is not taken
def _plain_run(N, M, Jp, Ji, p, x, Jx, lam, old, mp):
    _mode(mp, old, syrk_min=False)
    be = capi.Backend(capi.DLG_SPARSE, N, M, len(Ji))
    be.set_pattern(Jp, Ji)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    be.cauchy(0)
    assert be.factorize(0, lam)
    be.solve_gn(0)
    st = be.leaf_rows_stats()
    assert st["lean_levels"] == 0 and st["lean_launches"] == 0 and not st["raw"], st
    out = [be.download(0, capi.VEC_GN), be.solve_multi(0, np.random.default_rng(1).standard_normal((3, N))),
           be.marginal_variances(0)]
    assert be.leaf_rows_stats()["materialized"] == 0
    be.close()
    return [np.array(a, copy=True) for a in out]


@pytest.mark.parametrize("name", ["banded", "ba-20-300-3000"])
def test_patterns_without_lean_leaves_are_bit_identical(gpu, name, monkeypatch):
    """a banded pattern (no merged leaves at all) and BAProblem(20, 300, 3000, seed=3) (merged leaves of at most 128 rows:
    k_factor_level<128>, not the lean instantiation): no level runs lean, and the switch changes no bit"""
    if name == "banded":
        N, M, Jp, Ji, Jx, x, lam = zoo.case(name)
        args = (N, M, Jp, Ji, np.zeros(N), x, Jx, lam)
    else:
        K = _problem((20, 300, 3000), seed=3)
        args = (K["prob"].N, K["prob"].M, K["Jp"], K["Ji"], K["p"], K["x"], K["Jx"], 0.0)
    new = _plain_run(*args, False, monkeypatch)
    old = _plain_run(*args, True, monkeypatch)
    for a, b in zip(new, old):
        assert np.array_equal(a, b)
