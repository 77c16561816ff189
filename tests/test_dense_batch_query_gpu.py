"""dogleg_amd_dense_batch_query_covariance and its three twins: Jq Sigma_b Jq^T (and the observations-only form
Jq Sigma_b Jobs^T Jobs Sigma_b Jq^T) of caller-supplied query Jacobians for every problem of a batch, against values computed
on the host by tests/batch_query_oracle.py from HostProblem.eval(p[b]) at the very p[b] handed to the call: Sigma by the
recipe of tests/test_dense_batch_uncertainty_gpu.py::ref_sigma, the blocks by numpy.  Nothing of the library under test
computes what is checked, except where a test says so (the unit-vector queries against the uncertainty call's covariance,
the device twins against the host-pointer call, bytewise).

Tolerance: max |out - ref|_cd / sqrt(ref_cc ref_dd) <= 1e-9, the scaled tolerance of the covariance tests; an entry whose
expected row or column is exactly zero must be exactly zero.  Two independent host computations (the oracle's packed
Cholesky, LAPACK's general inverse) agree to 2.0e-15 on the plain cases and 2.2e-14 on the observations-only cases
(tests/test_dense_batch_query_cpu.py asserts 1e-12); cond(JtJ) <= 34, lambda is 0 at every point."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, BATCH_UNC_FAILED, BATCH_UNC_SKIPPED
from problems.batch import MODE_NAN, MODE_ZERO_COLUMN, LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED
from tests import batch_products_oracle as po
from tests import batch_query_oracle as qo
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_uncertainty_gpu as tu
from tests import test_dense_products_batch_uncertainty_gpu as tpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, NQ, TOL = qo.B, qo.NQ, qo.TOL
GUARD = td.GUARD


def query(db, p, Jq, lam=0.0, nobs=-1):
    """the host-pointer call; lam: a number for all, an array, or None (NULL)"""
    nb = len(p)
    lam = None if lam is None else np.array(np.broadcast_to(lam, (nb,)), dtype=np.float64)
    out = capi.dense_batch_query_covariance(p, db.N, db.M, db.cb, db.cookie, Jq, lam=lam, nobs=nobs)
    assert out["rc"] == 0
    return out


def query_products(db, p, Jq, lam=0.0):
    lam = None if lam is None else np.array(np.broadcast_to(lam, (len(p),)), dtype=np.float64)
    out = capi.dense_products_batch_query_covariance(p, db.N, db.cb, db.cookie, Jq, db.set_params(po.params(tpu.SET)), lam=lam)
    assert out["rc"] == 0
    return out


def check_structure(out, Jq):
    """every block bitwise symmetric, a zero row of Jq an exact zero row and column"""
    o = out["out"]
    assert o.tobytes() == np.ascontiguousarray(np.swapaxes(o, -1, -2)).tobytes(), "a block is not bitwise symmetric"
    for b, q, c in zip(*np.nonzero(~Jq.any(axis=-1))):
        assert not o[b, q, c, :].any() and not o[b, q, :, c].any(), (b, q, c)


def bits(a, idx=None):
    return np.ascontiguousarray(a if idx is None else a[idx]).tobytes()


# ---------------------------------------------------------------- 1. parity, plain form
@pytest.mark.parametrize("Q", qo.QROWS)
@pytest.mark.parametrize("shape", qo.PLAIN_SHAPES, ids=str)
def test_parity_plain(shape, Q):
    N, M = shape
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    db.reset_counters()
    out = query(db, p, Jq)
    assert db.ncalls() == 1 and db.nevals() == B
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK) and not out["lam"].any()
    err = qo.scaled_error(out["out"], qo.expected(N, M, Q))
    print(f"{shape} Q {Q}: {B} problems of {NQ} queries: scaled error {err:.3g}")
    assert err <= TOL
    check_structure(out, Jq)
    assert np.all(np.einsum("bqcc->bqc", out["out"]) >= 0.0)
    zb, zq = qo.ZERO_ROW
    assert not Jq[zb, zq, Q - 1].any() and not out["out"][zb, zq, Q - 1].any()


# ---------------------------------------------------------------- 2. parity, observations-only form
@pytest.mark.parametrize("case", qo.SANDWICH_CASES, ids=str)
def test_parity_sandwich(case):
    (N, M), nobs = case
    Q = 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    out = query(db, p, Jq, nobs=nobs)
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK) and not out["lam"].any()
    err = qo.scaled_error(out["out"], qo.expected(N, M, Q, nobs))
    print(f"{case}: scaled error {err:.3g}")
    assert err <= TOL
    check_structure(out, Jq)
    if nobs == 0:
        assert np.all(out["out"] == 0.0)
    if nobs == M:
        # J_obs = J and lambda = 0: Sigma JtJ Sigma = Sigma
        err = qo.scaled_error(out["out"], qo.expected(N, M, Q))
        print(f"{case}: against the plain form {err:.3g}")
        assert err <= TOL


# ---------------------------------------------------------------- 3. unit-vector queries are entries of Sigma
@pytest.mark.parametrize("shape", [(6, 40), (32, 64), (64, 130)], ids=str)
def test_unit_vectors_give_the_covariance(shape):
    N, M = shape
    Q = min(16, N)
    seeds, p, _ = qo.solved(N, M)
    Jq = np.zeros((B, 1, Q, N))
    Jq[:, 0, np.arange(Q), np.arange(Q)] = 1.0
    db = tu.device_batch(N, M, seeds)
    out = query(db, p, Jq)
    cov = tu.unc(db, p, np.zeros(B), want=("cov",))["cov"]
    db.close()
    err = qo.scaled_error(out["out"], cov[:, None, :Q, :Q])
    print(f"{shape}: unit vectors against the covariance of the uncertainty call: {err:.3g}")
    assert err <= TOL
    check_structure(out, Jq)


# ---------------------------------------------------------------- 4. position independence
@pytest.mark.parametrize("shape,nobs", [((6, 40), -1), ((6, 40), 17), ((48, 100), -1), ((64, 130), 71)], ids=str)
def test_position_neighbours_and_other_queries_do_not_matter(shape, nobs):
    N, M = shape
    Q = 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    base = query(db, p, Jq, nobs=nobs)["out"]
    # a subset of the queries
    part = query(db, p, Jq[:, 1:2], nobs=nobs)["out"]
    assert bits(part) == bits(base[:, 1:2])
    db.close()
    # every problem alone
    for b in range(B):
        db1 = tu.device_batch(N, M, seeds[b:b + 1])
        one = query(db1, p[b:b + 1], Jq[b:b + 1], nobs=nobs)["out"]
        db1.close()
        assert bits(one) == bits(base[b:b + 1]), b
    # at other indices, among other neighbours: 23 problems, ours scattered among copies of problem 0 at perturbed points
    nb = 23
    pos = np.random.default_rng(3).permutation(nb)[:B]
    s2, p2, Jq2 = np.full(nb, seeds[0]), np.tile(p[0] + 0.01, (nb, 1)), np.tile(Jq[0], (nb, 1, 1, 1))
    s2[pos], p2[pos], Jq2[pos] = seeds, p, Jq
    db2 = tu.device_batch(N, M, s2)
    big = query(db2, p2, Jq2, nobs=nobs)["out"]
    db2.close()
    assert bits(big, pos) == bits(base)


# ---------------------------------------------------------------- 5. the products form
@pytest.mark.parametrize("layout", [LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED])
@pytest.mark.parametrize("shape", [(6, 40), (24, 60), (48, 100), (64, 130)], ids=str)
def test_products_form(shape, layout):
    N, M = shape
    Q = 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tpu.device_batch(N, np.full(B, M), seeds, layout)
    db.reset_counters()
    out = query_products(db, p, Jq)
    assert db.ncalls() == 1 and db.nevals() == B
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK) and not out["lam"].any()
    err = qo.scaled_error(out["out"], qo.expected(N, M, Q))
    print(f"products {shape} layout {layout}: scaled error {err:.3g}")
    assert err <= TOL
    check_structure(out, Jq)


# ---------------------------------------------------------------- 6. the device twins
def query_dev(db, p, Jq, lam=0.0, nobs=-1, mask=None, products=False, stream=None):
    """the device-resident twin: the dict of the host-pointer call, `out` prefilled with the guard value"""
    nb, N = db.B, db.N
    _, Nq, Q, _ = Jq.shape
    P, JQ = td.Buf(p), td.Buf(Jq)
    Lm = None if lam is None else td.Buf(np.array(np.broadcast_to(lam, (nb,)), dtype=np.float64))
    S, O = td.Buf(np.full(nb, 42, dtype=np.int32)), td.Buf(np.full((nb, Nq, Q, Q), GUARD))
    A = td.mask_dev(mask)
    db.reset_counters()
    if products:
        rc = capi.dense_products_batch_query_covariance_device(P.ptr, nb, N, db.cb, db.cookie, db.set_params(po.params(tpu.SET)),
                                                               JQ.ptr, Nq, Q, O.ptr, S.ptr, Lm.ptr if Lm else None,
                                                               A.ptr if A else None, stream)
    else:
        rc = capi.dense_batch_query_covariance_device(P.ptr, nb, N, db.M, db.cb, db.cookie, JQ.ptr, Nq, Q, O.ptr, S.ptr, nobs,
                                                      Lm.ptr if Lm else None, A.ptr if A else None, stream)
    assert bits(P.get()) == bits(p) and bits(JQ.get()) == bits(Jq)
    return dict(rc=rc, status=S.get(), lam=Lm.get() if Lm else None, out=O.get(), ncalls=db.ncalls(),
                stats=capi.batch_uncertainty_last_stats())


def same_as_host(dev, host, what):
    assert dev["rc"] == 0 and dev["ncalls"] == 1, what
    for k in ("out", "lam", "status"):
        if host[k] is not None:
            assert bits(dev[k]) == bits(host[k]), f"{what}: {k}"
    s = dev["stats"]
    assert s["launches"] == 1 and s["syncs"] == 1 and s["copies"] <= 2, s


@pytest.mark.parametrize("shape,nobs", [((6, 40), -1), ((6, 40), 39), ((32, 64), -1), ((48, 100), 37), ((64, 130), -1)], ids=str)
def test_device_twin(shape, nobs):
    N, M = shape
    Q = 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    same_as_host(query_dev(db, p, Jq, nobs=nobs), query(db, p, Jq, nobs=nobs), f"{shape} nobs {nobs}")
    nolam = query_dev(db, p, Jq, lam=None, nobs=nobs)
    assert nolam["lam"] is None
    same_as_host(nolam, query(db, p, Jq, lam=None, nobs=nobs), "lambda NULL")
    db.close()
    if nobs < 0:
        dbp = tpu.device_batch(N, np.full(B, M), seeds)
        same_as_host(query_dev(dbp, p, Jq, products=True), query_products(dbp, p, Jq), f"products {shape}")
        dbp.close()


@pytest.mark.parametrize("shape", [(6, 40), (48, 100)], ids=str)
def test_device_twin_with_the_mask(shape):
    N, M = shape
    Q = 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    m = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0], dtype=np.uint8)         # (mixed workgroups, and b = 0 and b = B - 1 inactive)
    on, off = np.flatnonzero(m), np.flatnonzero(m == 0)
    lam = np.zeros(B)
    lam[off] = -5.0             # (a negative lambda would FAIL a problem that ran, and NaN its blocks)
    for products in (False, True):
        db = tpu.device_batch(N, np.full(B, M), seeds) if products else tu.device_batch(N, M, seeds)
        full = query_dev(db, p, Jq, products=products)
        out = query_dev(db, p, Jq, lam=lam, mask=m, products=products)
        assert out["rc"] == 0 and out["ncalls"] == 1
        assert np.all(out["status"][off] == BATCH_UNC_SKIPPED) and np.all(out["status"][on] == BATCH_UNC_OK)
        assert np.all(out["out"][off] == GUARD) and np.all(out["lam"][off] == -5.0)
        assert bits(out["out"], on) == bits(full["out"], on) and not out["lam"][on].any()
        none = query_dev(db, p, Jq, mask=np.zeros(B, dtype=np.uint8), products=products)
        assert none["rc"] == 0 and none["ncalls"] <= 1 and np.all(none["status"] == BATCH_UNC_SKIPPED)
        assert np.all(none["out"] == GUARD)
        db.close()


STREAM_CHILD = r'''
import sys
import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded
sys.path.insert(0, sys.argv[1])
from tests import batch_query_oracle as qo
from tests import test_dense_batch_query_gpu as tq
from tests import test_dense_batch_uncertainty_gpu as tu
from libdogleg_amd import capi

N, M, Q, B, NQ = 6, 40, 2, qo.B, qo.NQ
seeds, p, _ = qo.solved(N, M)
Jq = qo.queries(B, NQ, Q, N)
db = tu.device_batch(N, M, seeds)
want = tq.query(db, p, Jq, nobs=17)
s = torch.cuda.Stream()
sp, sq = torch.from_numpy(p.copy()).cuda().reshape(-1), torch.from_numpy(Jq.copy()).cuda().reshape(-1)
dp = torch.full((B * N + 64,), tq.GUARD, dtype=torch.float64, device="cuda")
dq = torch.full((Jq.size + 64,), tq.GUARD, dtype=torch.float64, device="cuda")
out = torch.full((B * NQ * Q * Q + 64,), tq.GUARD, dtype=torch.float64, device="cuda")
lam = torch.zeros(B, dtype=torch.float64, device="cuda")
status = torch.full((B,), 42, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(s):
    torch.mul(sp, 1.0, out=dp[:B * N])          # kernels on s that write p_dev and Jq_dev; no synchronisation before the call
    torch.mul(sq, 1.0, out=dq[:Jq.size])
rc = capi.dense_batch_query_covariance_device(dp.data_ptr(), B, N, M, db.cb, db.cookie, dq.data_ptr(), NQ, Q, out.data_ptr(),
                                              status.data_ptr(), 17, lam.data_ptr(), None, s.cuda_stream)
assert rc == 0
torch.cuda.synchronize()
o = out.cpu().numpy()
assert np.all(o[B * NQ * Q * Q:] == tq.GUARD)
assert o[:B * NQ * Q * Q].tobytes() == want["out"].tobytes()
assert status.cpu().numpy().tobytes() == want["status"].tobytes() and lam.cpu().numpy().tobytes() == want["lam"].tobytes()
db.close()
print("STREAM OK")
'''


def test_stream(tmp_path):
    """in a process of its own, torch loaded before the library (tests/test_dense_batch_device_gpu.py::test_stream): the kernels
    that write p_dev and Jq_dev are enqueued on the caller's stream and the call follows without a synchronisation"""
    src = tmp_path / "stream_child.py"
    src.write_text(STREAM_CHILD)
    r = subprocess.run([sys.executable, str(src), ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "STREAM OK" in r.stdout, r.stdout + r.stderr


def test_refusals_and_the_pointer_check():
    """with a device: -1, no invocation, nothing written; short and host arrays only through dlg_batch_device_span_ok"""
    N, M, Q = 6, 40, 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    db.reset_counters()
    P, JQ = td.Buf(p), td.Buf(Jq)
    S, O = td.Buf(np.full(B, 42, dtype=np.int32)), td.Buf(np.full((B, NQ, Q, Q), GUARD))

    def call(p_=P.ptr, jq=JQ.ptr, nq=NQ, q=Q, nobs=-1, o=O.ptr, s=S.ptr):
        return capi.dense_batch_query_covariance_device(p_, B, N, M, db.cb, db.cookie, jq, nq, q, o, s, nobs)

    assert call(p_=None) == -1 and call(jq=None) == -1 and call(o=None) == -1 and call(s=None) == -1
    assert call(nq=0) == -1 and call(q=0) == -1 and call(q=17) == -1 and call(nobs=M + 1) == -1
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    L = capi.lib()
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call() == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert db.ncalls() == 0 and np.all(O.get() == GUARD) and np.all(S.get() == 42)
    # the spans the entry points hand to the check: Jq_dev and out_dev in full
    assert capi.batch_device_span_ok(JQ.ptr, Jq.nbytes) and capi.batch_device_span_ok(O.ptr, 8 * B * NQ * Q * Q)
    d = capi.DeviceArray(nbytes=Jq.nbytes)
    assert capi.batch_device_span_ok(d, Jq.nbytes) and not capi.batch_device_span_ok(d, Jq.nbytes + 1)
    assert not capi.batch_device_span_ok(Jq.ctypes.data, Jq.nbytes)
    d.free()
    assert call() == 0 and db.ncalls() == 1
    db.close()


# ---------------------------------------------------------------- 7. one callback, constant launches
def test_one_callback_and_constant_launches():
    N, M, Q = 6, 40, 2
    stats = {}
    for nb in (1, 64):
        seeds, p, _ = qo.solved(N, M, nb)
        db = tu.device_batch(N, M, seeds)
        for Nq in (1, 8):
            Jq = qo.queries(nb, Nq, Q, N)
            db.reset_counters()
            out = query(db, p, Jq)
            assert db.ncalls() == 1 and db.nevals() == nb and np.all(out["status"] == BATCH_UNC_OK)
            s = capi.batch_uncertainty_last_stats()
            # the host-pointer call: the upload, the download and ONE fill (the live bytes)
            assert (s["launches"], s["syncs"], s["copies"]) == (1, 1, 3), s
            for kw in (dict(), dict(lam=None)):
                dev = query_dev(db, p, Jq, **kw)
                assert dev["rc"] == 0 and dev["ncalls"] == 1
                s = dev["stats"]
                stats[(nb, Nq, len(kw))] = (s["launches"], s["syncs"], s["copies"])
                assert s["launches"] == 1 and s["syncs"] == 1 and s["copies"] <= 2, s
        db.close()
    print(stats)
    for Nq in (1, 8):
        for k in (0, 1):
            assert stats[(1, Nq, k)] == stats[(64, Nq, k)] == stats[(1, 1, k)]


# ---------------------------------------------------------------- 8. lambda and failure
def test_lambda_loop_on_a_zero_column():
    """the batch of tests/test_dense_batch_uncertainty_gpu.py::test_lambda_loop_on_a_zero_column"""
    N, M, c, nb, chosen, Q = 6, 40, 2, 32, [3, 17, 30], 2
    seeds, p, _ = qo.solved(N, M, nb)
    Jq = qo.queries(nb, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    plain = query(db, p, Jq)
    mode = np.zeros(nb, dtype=np.uint8)
    mode[chosen] = MODE_ZERO_COLUMN
    db.set_mode(mode, c)
    out = query(db, p, Jq)
    unc = tu.unc(db, p, np.zeros(nb), want=("var",))
    db.close()
    assert np.all(out["status"] == BATCH_UNC_OK)
    assert bits(out["lam"]) == bits(unc["lam"]) and np.all(out["lam"][chosen] == 1e-10)
    others = [b for b in range(nb) if b not in chosen]
    assert not out["lam"][others].any() and bits(out["out"], others) == bits(plain["out"], others)
    for b in chosen:
        _, _, S = tu.reference(N, M, seeds[b], p[b], out["lam"][b], zero_col=c)
        err = qo.scaled_error(out["out"][b], qo.blocks(Jq[b], S))
        print(f"problem {b}: lambda {out['lam'][b]:g}, scaled error {err:.3g}")
        assert err <= TOL


def test_a_failing_problem_fails_alone():
    N, M, Q = 6, 40, 2
    seeds, p, _ = qo.solved(N, M)
    Jq = qo.queries(B, NQ, Q, N)
    db = tu.device_batch(N, M, seeds)
    plain = query(db, p, Jq, nobs=17)
    # a non-finite x in problem 4, a negative lambda[1], a NaN lambda[7]
    mode = np.zeros(B, dtype=np.uint8)
    mode[4] = MODE_NAN
    db.set_mode(mode)
    lam = np.zeros(B)
    lam[1], lam[7] = -1.0, np.nan
    out = query(db, p, Jq, lam=lam, nobs=17)           # (query asserts rc == 0)
    db.close()
    bad = [1, 4, 7]
    good = [b for b in range(B) if b not in bad]
    assert np.all(out["status"][bad] == BATCH_UNC_FAILED) and np.all(out["status"][good] == BATCH_UNC_OK)
    assert np.all(np.isnan(out["out"][bad]))
    assert out["lam"][1] == -1.0 and np.isnan(out["lam"][7])
    assert bits(out["out"], good) == bits(plain["out"], good) and not out["lam"][good].any()
