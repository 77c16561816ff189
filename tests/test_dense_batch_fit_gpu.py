"""The ..._fit forms of the batch uncertainty and query calls: the covariance, variances, outlierness factors and query
covariances of the REWEIGHTED problem on its FREE variables, at the optimum of a robust and / or bounded batch solve.

The reference is the NumPy / C-oracle reference of tests/batch_fit_oracle.py at the very p[b] handed to the call (tests/
test_dense_batch_fit_cpu.py holds its two routes against each other to 1e-12).  The tolerances are those of
tests/test_dense_batch_uncertainty_gpu.py and tests/test_dense_batch_query_gpu.py, imported: Sigma 1e-9 scaled (over the free
block; the held rows and columns are compared for exact +0.0), variances 1e-9 relative, factors rtol 1e-9 / atol 1e-12, a
computed scale 1e-12 relative, query blocks 1e-9 scaled.  Every figure is printed before it is asserted.

The cases: tests/batch_fit_oracle.py (one shape per size class, ragged last tiles, fs of the factors in {1, 2}, lfs of the
weights in {1, 2, 4}, six held patterns; batches of 5)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, BATCH_UNC_FAILED, BATCH_UNC_SKIPPED, BatchLoss, LOSS_TRIVIAL, LOSS_HUBER
from problems.batch import MODE_ZERO_COLUMN
from problems.batch_rowscale import RowScaleDeviceBatch
from tests import batch_fit_oracle as fo
from tests import batch_oracle as bo
from tests import batch_query_oracle as qo
from tests import test_dense_batch_bounds_gpu as tbd
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_robust_gpu as rt
from tests import test_dense_batch_uncertainty_gpu as tu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV_TOL, VAR_TOL, SCALE_TOL, FAC_RTOL, FAC_ATOL, QUERY_TOL = tu.COV_TOL, tu.VAR_TOL, tu.SCALE_TOL, tu.FAC_RTOL, tu.FAC_ATOL, qo.TOL
UNC_KEYS = ("cov", "var", "factors", "scale", "lam", "status")
QRY_KEYS = ("out", "lam", "status")
fit = capi.batch_fit


def planted_batch(N, M, lfs, nb=fo.B):
    return rt.device_batch(N, M, lfs, tuple(range(1, 1 + nb)), fo.SETNAME, planted=True)


def unc(db, p, lam, f, fs=1, scale=None, want=("cov", "var", "factors")):
    out = capi.dense_batch_uncertainty(p, db.N, db.M, db.cb, db.cookie, lam=lam, want=want, fs=fs, scale=scale, fit=f)
    assert out["rc"] == 0
    return out


def qry(db, p, lam, Jq, nobs, f):
    out = capi.dense_batch_query_covariance(p, db.N, db.M, db.cb, db.cookie, Jq, lam=lam, nobs=nobs, fit=f)
    assert out["rc"] == 0
    return out


def same_bits(a, b, keys, ia=None, ib=None):
    return tu.same_bits(a, b, keys=keys, idx_a=ia, idx_b=ib)


def check_unc(out, refs, held, what, computed_scale):
    """every problem of an uncertainty call against its reference; prints the figures, then asserts"""
    ecov = evar = efac = esc = 0.0
    ok = True
    for b, r in enumerate(refs):
        ecov = max(ecov, fo.cov_error(out["cov"][b], r["S"], held[b]))
        free = held[b] == 0
        ok = ok and bool(np.all(out["var"][b][~free] == 0.0)) and out["var"][b].tobytes() == np.diag(out["cov"][b]).copy().tobytes()
        if free.any():
            evar = max(evar, float(np.max(np.abs(out["var"][b] - r["var"])[free] / r["var"][free])))
        esc = max(esc, abs(out["scale"][b] - r["scale"]) / r["scale"])
        want, got = r["factors"], out["factors"][b]
        big = want == fo.DBL_MAX
        ok = ok and bool(np.all(got[big] == fo.DBL_MAX)) and bool(np.allclose(got[~big], want[~big], rtol=FAC_RTOL, atol=FAC_ATOL))
        if np.any(~big):
            efac = max(efac, float(np.max(np.abs(got - want)[~big] / np.maximum(np.abs(want[~big]), FAC_ATOL / FAC_RTOL))))
    print(f"{what}: Sigma scaled error {ecov:.3g} (held rows and columns exactly +0), variances rel {evar:.3g}, factors rel "
          f"{efac:.3g}, scale rel {esc:.3g} ({'computed' if computed_scale else 'given'})")
    assert np.all(out["status"] == BATCH_UNC_OK)
    assert ecov <= COV_TOL and evar <= VAR_TOL and ok and esc <= (SCALE_TOL if computed_scale else 0.0)


def check_qry(out, refs, what):
    e = max(qo.scaled_error(out["out"][b], r["blocks"]) for b, r in enumerate(refs))
    print(f"{what}: query blocks scaled error {e:.3g}")
    assert np.all(out["status"] == BATCH_UNC_OK) and e <= QUERY_TOL


def parity(N, M, fs, lfs, kind, pattern, mode, nb, what):
    """mode "loss": the loss alone, "held": the held pattern alone, "both"; every output of both calls"""
    seeds, p, lam, w = fo.points(N, M, lfs, kind, nb)
    held = fo.held_pattern(pattern if mode != "loss" else "none", nb, N)
    oloss, lloss = fo.loss_of(kind, lfs)
    f = fit(loss=lloss if mode != "held" else None, held=held if mode != "loss" else None)
    rl, rlfs = (oloss, lfs) if mode != "held" else (None, 1)
    Jq = fo.queries(nb, N)
    xJ = fo.evaluated(N, M, lfs, kind, nb)
    db = planted_batch(N, M, lfs, nb)
    out = unc(db, p, lam, f, fs=fs)
    refs = [fo.reference(x, J, lam[b], held[b], lfs=rlfs, loss=rl, fs=fs) for b, (x, J) in enumerate(xJ)]
    assert np.array_equal(out["lam"], lam)
    check_unc(out, refs, held, f"{what} {mode} {pattern}", True)
    given = unc(db, p, lam, f, fs=fs, scale=2.5)
    check_unc(given, [fo.reference(x, J, lam[b], held[b], lfs=rlfs, loss=rl, fs=fs, scale=2.5) for b, (x, J) in enumerate(xJ)],
              held, f"{what} {mode} {pattern}", False)
    assert same_bits(out, given, ("cov", "var", "lam", "status"))
    for nobs in (-1, 0, lfs, M):
        q = qry(db, p, lam, Jq, nobs, f)
        rq = [fo.reference(x, J, lam[b], held[b], lfs=rlfs, loss=rl, Jq=Jq[b], nobs=nobs) for b, (x, J) in enumerate(xJ)]
        check_qry(q, rq, f"{what} {mode} {pattern} Nobservations {nobs}")
        if pattern == "all" and mode != "loss":
            assert not q["out"].any()
    if pattern == "all" and mode != "loss":
        assert not out["cov"].any() and not out["var"].any() and np.array_equal(out["lam"], lam)
    db.close()


# ---------------------------------------------------------------- 1. parity with the host reference
@pytest.mark.parametrize("kind", sorted(rt.KINDS))
def test_parity_loss_only_on_the_planted_batch(kind):
    (N, M), lfs = fo.PLANTED_SHAPE, fo.PLANTED_LFS
    for fs in (1, 2):
        parity(N, M, fs, lfs, kind, "none", "loss", fo.PLANTED_B, f"planted {kind} fs {fs}")


@pytest.mark.parametrize("mode", ["loss", "held", "both"])
@pytest.mark.parametrize("case", fo.CASES, ids=str)
def test_parity_every_size_class(case, mode):
    N, M, fs, lfs, kind = case
    for pattern in (("none",) if mode == "loss" else fo.HELD_PATTERNS):
        parity(N, M, fs, lfs, kind, pattern, mode, fo.B, str(case))


# ---------------------------------------------------------------- 2. end to end behind the bounded solve
def test_end_to_end_behind_a_bounded_huber_solve():
    """p, lambda, weights and held as the bounded solve returns them, handed to the fit calls unchanged.  The bounded solve
    runs under tests/test_dense_batch_bounds_gpu.py's stopping thresholds (its docstring)"""
    N, M, lfs, nb = 6, 40, tbd.HUBER_FS, 16
    seeds = tuple(range(1, 1 + nb))
    _, lo, hi = tbd.oracle_batch(N, M, seeds, "diverse", LOSS_HUBER, lfs)
    lloss = tbd.loss_pair("diverse", LOSS_HUBER, lfs)[1]
    db = tb.device_batch(N, M, seeds, "diverse")
    p, res, held, w = tbd.run(db, tbd.params("diverse"), lo, hi, lloss)
    lam = np.ascontiguousarray(res["lambda_"])
    assert np.all(res["status"] > 0) and 2 * int(held.any(axis=1).sum()) >= nb and float(np.mean(w < 1.0)) >= 0.1
    f = fit(loss=lloss, weights=w, held=held)
    Jq = fo.queries(nb, N)
    eps, noise, spread, _ = tb.SETS["diverse"]
    xJ = []
    for b, s in enumerate(seeds):
        hp = bo.HostProblem(M, N, int(s), eps, noise, spread)
        xJ.append(hp.eval(np.ascontiguousarray(p[b])))
        hp.dp.close()
    for fs in (1, 2):
        out = unc(db, p, lam, f, fs=fs)
        check_unc(out, [fo.reference(x, J, lam[b], held[b], lfs=lfs, w=w[b], fs=fs) for b, (x, J) in enumerate(xJ)], held,
                  f"behind the bounded solve, fs {fs}", True)
    for nobs in (-1, lfs, M):
        q = qry(db, p, lam, Jq, nobs, f)
        check_qry(q, [fo.reference(x, J, lam[b], held[b], lfs=lfs, w=w[b], Jq=Jq[b], nobs=nobs) for b, (x, J) in enumerate(xJ)],
                  f"behind the bounded solve, Nobservations {nobs}")
    db.close()


# ---------------------------------------------------------------- 3. identities, bitwise
@pytest.mark.parametrize("case", [fo.CASES[1], fo.CASES[6], fo.CASES[7]], ids=str)
def test_identities(case):
    N, M, fs, lfs, kind = case
    nb = fo.B
    seeds, p, lam, _ = fo.points(N, M, lfs, kind)
    Jq = fo.queries(nb, N)
    db = planted_batch(N, M, lfs)
    plain, plain_q = unc(db, p, lam, None, fs=fs), [qry(db, p, lam, Jq, nobs, None) for nobs in (-1, lfs)]
    # fit == NULL, and a record whose members are all NULL: the call without _fit
    for f in (capi.NULL_FIT, fit()):
        assert same_bits(unc(db, p, lam, f, fs=fs), plain, UNC_KEYS)
        for k, nobs in enumerate((-1, lfs)):
            assert same_bits(qry(db, p, lam, Jq, nobs, f), plain_q[k], QRY_KEYS)
    # the TRIVIAL loss of size 1 with no variable held: the tiles of the plain sweep
    f = fit(loss=BatchLoss(LOSS_TRIVIAL, 0.0, 1), held=np.zeros((nb, N), dtype=np.uint8))
    assert same_bits(unc(db, p, lam, f, fs=fs), plain, UNC_KEYS)
    for k, nobs in enumerate((-1, lfs)):
        assert same_bits(qry(db, p, lam, Jq, nobs, f), plain_q[k], QRY_KEYS)
    # weights that are all exactly 1: the plain call on everything that does not sum x over tiles of another height
    f = fit(loss=BatchLoss(LOSS_TRIVIAL, 0.0, lfs), weights=np.ones((nb, M // lfs)))
    ones = unc(db, p, lam, f, fs=fs)
    assert same_bits(ones, plain, ("cov", "var", "lam", "status"))
    assert np.allclose(ones["scale"], plain["scale"], rtol=SCALE_TOL, atol=0)
    assert np.allclose(ones["factors"], plain["factors"], rtol=FAC_RTOL, atol=FAC_ATOL)
    for k, nobs in enumerate((-1, lfs)):
        assert same_bits(qry(db, p, lam, Jq, nobs, f), plain_q[k], QRY_KEYS)
    # the weights the robust solve returns at its optimum against the loss evaluated there: the same bits
    lloss = fo.loss_of(kind, lfs)[1]
    ps, rs, ws = rt.run(db, tb.params(fo.SETNAME, **dict(rt.PLANTED_OVER)), lloss)
    ls = np.ascontiguousarray(rs["lambda_"])
    assert np.all(rs["status"] > 0) and ws.min() < 0.1
    by_loss, by_w = unc(db, ps, ls, fit(loss=lloss), fs=fs), unc(db, ps, ls, fit(loss=lloss, weights=ws), fs=fs)
    assert same_bits(by_loss, by_w, UNC_KEYS) and not same_bits(by_loss, unc(db, ps, ls, None, fs=fs), ("cov",))
    for nobs in (-1, lfs):
        assert same_bits(qry(db, ps, ls, Jq, nobs, fit(loss=lloss)), qry(db, ps, ls, Jq, nobs, fit(loss=lloss, weights=ws)), QRY_KEYS)
    db.close()


def dev_unc(db, p, lam, f_dev, fs, mask=None, stream=None):
    """the device twin under prefilled guards: the dict of the host wrapper"""
    nb, N, M = len(p), db.N, db.M
    P, Lm, St = td.Buf(p), td.Buf(lam), td.Buf(np.full(nb, -1, dtype=np.int32))
    Cv, Vr = td.Buf(np.full((nb, N, N), td.GUARD)), td.Buf(np.full((nb, N), td.GUARD))
    Fc, Sc = td.Buf(np.full((nb, M // fs), td.GUARD)), td.Buf(np.full(nb, -1.0))
    A = td.mask_dev(mask)
    rc = capi.dense_batch_uncertainty_device(P.ptr, nb, N, M, db.cb, db.cookie, St.ptr, Lm.ptr, Cv.ptr, Vr.ptr, Fc.ptr, Sc.ptr, fs,
                                             A.ptr if A else None, stream, fit=f_dev)
    assert rc == 0 and P.get().tobytes() == np.ascontiguousarray(p).tobytes()
    return dict(cov=Cv.get(), var=Vr.get(), factors=Fc.get(), scale=Sc.get(), lam=Lm.get(), status=St.get())


def dev_qry(db, p, lam, Jq, nobs, f_dev, mask=None):
    nb, N = len(p), db.N
    P, Lm, St, Jd = td.Buf(p), td.Buf(lam), td.Buf(np.full(nb, -1, dtype=np.int32)), td.Buf(Jq)
    Od = td.Buf(np.full((nb, Jq.shape[1], Jq.shape[2], Jq.shape[2]), td.GUARD))
    A = td.mask_dev(mask)
    rc = capi.dense_batch_query_covariance_device(P.ptr, nb, N, db.M, db.cb, db.cookie, Jd.ptr, Jq.shape[1], Jq.shape[2], Od.ptr,
                                                  St.ptr, nobs, Lm.ptr, A.ptr if A else None, fit=f_dev)
    assert rc == 0
    return dict(out=Od.get(), lam=Lm.get(), status=St.get())


@pytest.mark.parametrize("case", [fo.CASES[3], fo.CASES[6]], ids=str)
def test_device_twin_mask_order_and_neighbours(case):
    """the device twin equals the host twin; a masked problem writes nothing but SKIPPED; an active problem's bits depend
    neither on the mask, nor on B, nor on its position: a batch of 5 against its problems run singly and permuted"""
    N, M, fs, lfs, kind = case
    nb = fo.B
    seeds, p, lam, w = fo.points(N, M, lfs, kind)
    held = fo.held_pattern("third", nb, N)
    Jq = np.ascontiguousarray(fo.queries(nb, N))
    lloss = fo.loss_of(kind, lfs)[1]
    db = planted_batch(N, M, lfs)
    W, H = td.Buf(w), td.Buf(held)
    host_u, host_q = unc(db, p, lam, fit(loss=lloss, weights=w, held=held), fs=fs), qry(db, p, lam, Jq, lfs, fit(loss=lloss, held=held))
    du = dev_unc(db, p, lam, fit(loss=lloss, weights=W.ptr, held=H.ptr), fs)
    dq = dev_qry(db, p, lam, Jq, lfs, fit(loss=lloss, held=H.ptr))
    assert same_bits(du, host_u, UNC_KEYS) and same_bits(dq, host_q, QRY_KEYS)
    assert W.get().tobytes() == w.tobytes() and H.get().tobytes() == held.tobytes()
    # the mask
    mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    on, off = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    mu = dev_unc(db, p, lam, fit(loss=lloss, weights=W.ptr, held=H.ptr), fs, mask=mask)
    mq = dev_qry(db, p, lam, Jq, lfs, fit(loss=lloss, held=H.ptr), mask=mask)
    assert np.all(mu["status"][off] == BATCH_UNC_SKIPPED) and np.all(mq["status"][off] == BATCH_UNC_SKIPPED)
    for k in ("cov", "var", "factors"):
        assert np.all(mu[k][off] == td.GUARD), k
    assert np.all(mu["scale"][off] == -1.0) and mu["lam"][off].tobytes() == lam[off].tobytes() and np.all(mq["out"][off] == td.GUARD)
    assert same_bits(mu, host_u, UNC_KEYS, on, on) and same_bits(mq, host_q, QRY_KEYS, on, on)
    db.close()
    # singly, and permuted: the offsets of a planted batch belong to the position, so the rows travel with the problem
    off_all = rt.offsets_of(nb, M, lfs, fo.SETNAME)
    perm = np.array([3, 0, 4, 2, 1])
    for idx in [perm] + [np.array([b]) for b in range(nb)]:
        from problems.batch_offsets import OffsetDeviceBatch
        dbi = OffsetDeviceBatch(tb.device_batch(N, M, [seeds[i] for i in idx], fo.SETNAME), off_all[idx])
        f = fit(loss=lloss, weights=np.ascontiguousarray(w[idx]), held=np.ascontiguousarray(held[idx]))
        assert same_bits(unc(dbi, p[idx], lam[idx], f, fs=fs), host_u, UNC_KEYS, None, idx)
        f = fit(loss=lloss, held=np.ascontiguousarray(held[idx]))
        assert same_bits(qry(dbi, p[idx], lam[idx], np.ascontiguousarray(Jq[idx]), lfs, f), host_q, QRY_KEYS, None, idx)
        dbi.close()


# ---------------------------------------------------------------- 4. against the row-scaling callback
@pytest.mark.parametrize("case", fo.CASES, ids=str)
def test_against_the_row_scaling_callback(case):
    """the loss form against the entry point without _fit behind problems/batch_rowscale.py: Sigma, the variances, the query
    blocks, lambda and status bit for bit; a computed scale and the factors to the tolerances (|x~|^2 is summed over tiles of
    another height)"""
    N, M, fs, lfs, kind = case
    seeds, p, lam, w = fo.points(N, M, lfs, kind)
    Jq = fo.queries(fo.B, N)
    lloss = fo.loss_of(kind, lfs)[1]
    db = planted_batch(N, M, lfs)
    got = unc(db, p, lam, fit(loss=lloss, weights=w), fs=fs)
    rs = RowScaleDeviceBatch(db, w, lfs)
    want = unc(rs, p, lam, None, fs=fs)
    assert same_bits(got, want, ("cov", "var", "lam", "status")) and np.all(got["status"] == BATCH_UNC_OK)
    esc = float(np.max(np.abs(got["scale"] - want["scale"]) / want["scale"]))
    efac = float(np.max(np.abs(got["factors"] - want["factors"]) / np.maximum(np.abs(want["factors"]), FAC_ATOL / FAC_RTOL)))
    print(f"{case}: against the row-scaling callback: scale rel {esc:.3g}, factors rel {efac:.3g}")
    assert esc <= SCALE_TOL and np.allclose(got["factors"], want["factors"], rtol=FAC_RTOL, atol=FAC_ATOL)
    for nobs in (-1, 0, lfs, M):
        assert same_bits(qry(db, p, lam, Jq, nobs, fit(loss=lloss, weights=w)), qry(rs, p, lam, Jq, nobs, None), QRY_KEYS), nobs
    rs.close()
    db.close()


# ---------------------------------------------------------------- 5. a singular column
def test_a_singular_column_held_and_not_held():
    N, M, fs, lfs, kind = fo.CASES[2]
    nb, c = fo.B, 4
    seeds, p, lam, w = fo.points(N, M, lfs, kind)
    assert np.all(lam == 0.0)
    db = planted_batch(N, M, lfs)
    db.set_mode(np.full(nb, MODE_ZERO_COLUMN, dtype=np.uint8), c)
    held = np.zeros((nb, N), dtype=np.uint8)
    held[:, c] = 1
    lloss = fo.loss_of(kind, lfs)[1]
    out = unc(db, p, lam, fit(loss=lloss, weights=w, held=held), fs=fs)
    assert np.all(out["lam"] == 0.0)
    refs = []
    for b, s in enumerate(seeds):
        hp = fo.host_problem(N, M, lfs, s, b, nb, zero_col=c)
        x, J = hp.eval(np.ascontiguousarray(p[b]))
        refs.append(fo.reference(x, J, 0.0, held[b], lfs=lfs, w=w[b], fs=fs))
        hp.close()
    check_unc(out, refs, held, "zero column, held", True)
    # not held: the lambda schedule moves, as in the call without _fit
    moved = unc(db, p, lam, fit(loss=lloss, weights=w), fs=fs)
    assert np.all(moved["status"] == BATCH_UNC_OK) and np.all(moved["lam"] == 1e-10)
    assert np.allclose(moved["var"][:, c], 1e10, rtol=1e-9, atol=0)
    db.close()


# ---------------------------------------------------------------- 6. weights 0 / 1
def test_dropping_the_planted_features_is_the_problem_without_their_rows():
    N, M, fs, lfs, kind = fo.CASES[3]
    nb = fo.B
    seeds, p, lam, _ = fo.points(N, M, lfs, kind)
    _, planted = rt.planted_offsets(nb, M, lfs, rt.OUTLIER_FRACTION, rt.OUTLIER_SIZE * tb.SETS[fo.SETNAME][1], rt.OUTLIER_SEED)
    w01 = np.where(planted, 0.0, 1.0)
    assert 0 < planted.sum() < planted.size
    held = fo.held_pattern("first", nb, N)
    Jq = fo.queries(nb, N)
    db = planted_batch(N, M, lfs)
    f = fit(loss=BatchLoss(LOSS_TRIVIAL, 0.0, lfs), weights=w01, held=held)
    out, q = unc(db, p, lam, f, fs=fs, want=("cov", "var")), qry(db, p, lam, Jq, -1, f)
    ecov = eq = 0.0
    for b, (x, J) in enumerate(fo.evaluated(N, M, lfs, kind)):
        rows = np.repeat(~planted[b], lfs)
        r = fo.reference(x[rows], J[rows], lam[b], held[b], Jq=Jq[b])
        ecov = max(ecov, fo.cov_error(out["cov"][b], r["S"], held[b]))
        eq = max(eq, qo.scaled_error(q["out"][b], r["blocks"]))
    print(f"weights 0 / 1 against the kept rows: Sigma scaled error {ecov:.3g}, query blocks {eq:.3g}")
    assert ecov <= COV_TOL and eq <= QUERY_TOL
    # and the factors, on the whole problem with those weights: a dropped feature has x~ = 0 and a factor of exactly 0
    full = unc(db, p, lam, f, fs=lfs if lfs <= 2 else 2)
    refs = [fo.reference(x, J, lam[b], held[b], lfs=lfs, w=w01[b], fs=lfs if lfs <= 2 else 2) for b, (x, J) in enumerate(fo.evaluated(N, M, lfs, kind))]
    check_unc(full, refs, held, "weights 0 / 1", True)
    db.close()


# ---------------------------------------------------------------- 7. failing alone
def test_a_bad_weight_fails_its_problem_alone():
    N, M, fs, lfs, kind = fo.CASES[1]
    nb = fo.B
    seeds, p, lam, w = fo.points(N, M, lfs, kind)
    Jq = fo.queries(nb, N)
    lloss = fo.loss_of(kind, lfs)[1]
    db = planted_batch(N, M, lfs)
    good_u, good_q = unc(db, p, lam, fit(loss=lloss, weights=w), fs=fs), qry(db, p, lam, Jq, lfs, fit(loss=lloss, weights=w))
    wb = np.array(w)
    wb[0, M // lfs - 1] = np.nan        # in the ragged last tile
    wb[2, 1] = -0.25
    wb[4, :] = np.nan                   # what a solve that FAILED returns
    bad, good = [0, 2, 4], [1, 3]
    for out, ref, keys, outs in ((unc(db, p, lam, fit(loss=lloss, weights=wb), fs=fs), good_u, UNC_KEYS, ("cov", "var", "factors")),
                                 (qry(db, p, lam, Jq, lfs, fit(loss=lloss, weights=wb)), good_q, QRY_KEYS, ("out",))):
        assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
        for k in outs:
            assert np.all(np.isnan(out[k][bad])), k
        assert same_bits(out, ref, keys, good, good)
    db.close()


# ---------------------------------------------------------------- 8. refusals with a device present
def test_refusals_on_the_gpu():
    N, M, fs, lfs, kind = fo.CASES[1]
    nb = fo.B
    seeds, p, lam, w = fo.points(N, M, lfs, kind)
    held = fo.held_pattern("third", nb, N)
    Jq = np.ascontiguousarray(fo.queries(nb, N))
    lloss = fo.loss_of(kind, lfs)[1]
    db = planted_batch(N, M, lfs)
    db.reset_counters()
    P, Lm, St, Cv = td.Buf(p), td.Buf(lam), td.Buf(np.full(nb, -1, dtype=np.int32)), td.Buf(np.full((nb, N, N), td.GUARD))
    Jd, Od = td.Buf(Jq), td.Buf(np.full((nb, fo.NQ, fo.Q, fo.Q), td.GUARD))
    W, H = td.Buf(w), td.Buf(held)
    short_w, short_h = capi.DeviceArray(nbytes=8 * (w.size - 1)), capi.DeviceArray(nbytes=held.size - 1)

    def u(f):
        return capi.dense_batch_uncertainty_device(P.ptr, nb, N, M, db.cb, db.cookie, St.ptr, Lm.ptr, Cv.ptr, fit=f)

    def q(f):
        return capi.dense_batch_query_covariance_device(P.ptr, nb, N, M, db.cb, db.cookie, Jd.ptr, fo.NQ, fo.Q, Od.ptr, St.ptr, -1,
                                                        Lm.ptr, fit=f)

    for call in (u, q):
        assert call(fit(loss=lloss, weights=w)) == -1                    # pageable host memory (a numpy array by its address)
        assert call(fit(held=held)) == -1
        assert call(fit(loss=lloss, weights=short_w.ptr)) == -1          # a device allocation that is too short
        assert call(fit(held=short_h.ptr)) == -1
        assert call(fit(weights=W.ptr)) == -1                            # weights without a loss
    assert db.ncalls() == 0
    assert np.all(St.get() == -1) and np.all(Cv.get() == td.GUARD) and np.all(Od.get() == td.GUARD)
    assert u(fit(loss=lloss, weights=W.ptr, held=H.ptr)) == 0 and np.all(St.get() == BATCH_UNC_OK)
    assert q(fit(loss=lloss, weights=W.ptr, held=H.ptr)) == 0 and db.ncalls() == 2
    s = capi.batch_uncertainty_last_stats()
    assert (s["launches"], s["syncs"]) == (1, 1)
    short_w.free()
    short_h.free()
    db.close()


# ---------------------------------------------------------------- the products form: held only
def test_products_form_takes_held():
    from problems.batch import DeviceProductsBatch
    N, M, nb = 13, 40, fo.B
    seeds = np.arange(1, 1 + nb)
    eps, noise, spread, _ = tb.SETS[fo.SETNAME]
    dp = DeviceProductsBatch(nb, M, N, seeds=seeds.astype(np.uint64), eps=eps, noise=noise, p0_spread=spread)
    prm = capi.default_parameters()
    prm.JtJ_packed, prm.JtJ_upper = True, True
    dp.set_params(prm)
    p, lam = dp.p0(), np.zeros(nb)
    Jq = fo.queries(nb, N)
    for pattern in fo.HELD_PATTERNS:
        held = fo.held_pattern(pattern, nb, N)
        out = capi.dense_products_batch_uncertainty(p, N, dp.cb, dp.cookie, prm, lam=lam, fit=fit(held=held))
        q = capi.dense_products_batch_query_covariance(p, N, dp.cb, dp.cookie, Jq, prm, lam=lam, fit=fit(held=held))
        assert out["rc"] == 0 and q["rc"] == 0 and np.all(out["status"] == BATCH_UNC_OK) and np.all(q["status"] == BATCH_UNC_OK)
        ecov = eq = 0.0
        for b, s in enumerate(seeds):
            hp = bo.HostProblem(M, N, int(s), eps, noise, spread)
            x, J = hp.eval(np.ascontiguousarray(p[b]))
            hp.dp.close()
            r = fo.reference(x, J, 0.0, held[b], Jq=Jq[b])
            ecov = max(ecov, fo.cov_error(out["cov"][b], r["S"], held[b]))
            eq = max(eq, qo.scaled_error(q["out"][b], r["blocks"]))
        print(f"products form, held {pattern}: Sigma scaled error {ecov:.3g}, query blocks {eq:.3g}")
        assert ecov <= COV_TOL and eq <= QUERY_TOL
    dp.close()


# ---------------------------------------------------------------- 9. the caller's stream
STREAM_CHILD = r'''
import sys
import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded
sys.path.insert(0, sys.argv[1])
from tests import batch_fit_oracle as fo
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_fit_gpu as tf
from libdogleg_amd import capi

N, M, fs, lfs, kind = fo.CASES[3]
B = fo.B
seeds, p, lam, w = fo.points(N, M, lfs, kind)
held = fo.held_pattern("third", B, N)
lloss = fo.loss_of(kind, lfs)[1]
db = tf.planted_batch(N, M, lfs)
want = tf.unc(db, p, lam, capi.batch_fit(loss=lloss, weights=w, held=held), fs=fs, want=("cov", "var"))
s = torch.cuda.Stream()
host = torch.from_numpy(np.array(p)).pin_memory()
dev = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
cov = torch.full((B * N * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
var = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
lmd = torch.from_numpy(np.array(lam)).cuda()
wd, hd = torch.from_numpy(np.array(w)).cuda(), torch.from_numpy(held.copy()).cuda()
st = torch.full((B,), -1, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(s):
    dev[:B * N].copy_(host.reshape(-1), non_blocking=True)      # asynchronous, on s; no synchronisation before the call
rc = capi.dense_batch_uncertainty_device(dev.data_ptr(), B, N, M, db.cb, db.cookie, st.data_ptr(), lmd.data_ptr(), cov.data_ptr(),
                                         var.data_ptr(), stream=s.cuda_stream,
                                         fit=capi.batch_fit(loss=lloss, weights=wd.data_ptr(), held=hd.data_ptr()))
assert rc == 0
torch.cuda.synchronize()
c, v = cov.cpu().numpy(), var.cpu().numpy()
assert np.all(c[B * N * N:] == td.GUARD) and np.all(v[B * N:] == td.GUARD)
assert c[:B * N * N].tobytes() == want["cov"].tobytes() and v[:B * N].tobytes() == want["var"].tobytes()
assert np.all(st.cpu().numpy() == 0) and lmd.cpu().numpy().tobytes() == want["lam"].tobytes()
db.close()
print("STREAM OK")
'''


def test_stream(tmp_path):
    """in a process of its own, as tests/test_dense_batch_device_gpu.py::test_stream: torch is loaded before the library there"""
    src = tmp_path / "stream_child.py"
    src.write_text(STREAM_CHILD)
    r = subprocess.run([sys.executable, str(src), ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "STREAM OK" in r.stdout, r.stdout + r.stderr
