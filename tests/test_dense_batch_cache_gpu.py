"""The batch solver's cache between calls of different kinds: the solve, the uncertainty call and the query call share three
buffers (callback output, state, page-locked staging), each grown when a call needs more and otherwise reused as it is.  Here
five calls of four kinds run in one sequence behind dogleg_amd_release_cache(), consecutive calls of different shapes, so
that each finds the buffers as a larger or a smaller call of another kind left them:

  1. host uncertainty with covariance, variances and factors      (B, N, M) = (5, 3, 8)     class <8>, 4 per workgroup, partial
  2. bounded robust solve, host route, with held and weights                  (3, 33, 40)   class <48>, 2 per workgroup, partial
  3. query covariance, device route, with a mask                              (9, 6, 12)
  4. products-form solve                                                      (3, 33, .)
  5. call 1 again

Every output array of each call (status, lambda, p, results, held, weights, cov, var, factors and its scale, out) must be
BITWISE what the same call gives directly behind a dogleg_amd_release_cache(), on fresh buffers.  Bitwise is the bar because
one wavefront owns a problem and no kernel has a floating-point atomic (the only atomic is the integer live counter), and the
callbacks of problems/ sum without atomics too.  Nothing is compared with an oracle: what the calls compute is the business
of the tests of each kind."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_UNC_OK, BATCH_UNC_SKIPPED, BATCH_FAILED, LOSS_HUBER, BatchLoss
from problems.batch import DeviceBatch, DeviceProductsBatch
from problems.batch_linear import LinearDeviceBatch
from problems.batch_offsets import OffsetDeviceBatch, planted_offsets
from tests import batch_query_oracle as qo
from tests import test_dense_batch_query_gpu as tq

pytestmark = pytest.mark.gpu

SMALL, WIDE, MID = (5, 3, 8), (3, 33, 40), (9, 6, 12)


def uncertainty_host():
    B, N, M = SMALL
    db = DeviceBatch(B, M, N, seeds=11)
    out = capi.dense_batch_uncertainty(db.p0(), N, M, db.cb, db.cookie, lam=np.zeros(B), want=("cov", "var", "factors"))
    db.close()
    assert out.pop("rc") == 0 and np.all(out["status"] == BATCH_UNC_OK)
    return out


def bounded_robust_host():
    B, N, M = WIDE
    off, _ = planted_offsets(B, M, 2, 0.2, 5.0, seed=3)
    db = OffsetDeviceBatch(DeviceBatch(B, M, N, seeds=21), off)
    p0 = db.p0()
    prm = capi.default_parameters()
    prm.max_iterations = 12
    rc, p, res, held, w = capi.optimize_dense_batch_bounded(p0, N, M, db.cb, db.cookie, p0 - 0.05, p0 + 0.05,
                                                            loss=BatchLoss(LOSS_HUBER, 1.0, 2), params=prm)
    db.close()
    assert rc == 0 and np.all(res["status"] != BATCH_FAILED)
    assert held.max() <= 2 and held.any(), "no variable ended on a bound: the held array would be all zero"
    assert np.all(w >= 0.0) and np.any(w < 1.0), "no feature was down-weighted"
    return dict(p=p, results=res, held=held, weights=w)


def query_device_masked():
    B, N, M = MID
    rng = np.random.default_rng(5)
    db = LinearDeviceBatch(rng.standard_normal((B, M, N)), rng.standard_normal((B, M)), rng.standard_normal((B, N)))
    mask = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0], dtype=np.uint8)
    out = tq.query_dev(db, db.p0(), qo.queries(B, 3, 2, N), nobs=7, mask=mask)
    db.close()
    assert out["rc"] == 0 and out["ncalls"] == 1
    assert np.all(out["status"][mask == 1] == BATCH_UNC_OK) and np.all(out["status"][mask == 0] == BATCH_UNC_SKIPPED)
    return dict(status=out["status"], lam=out["lam"], out=out["out"])


def products_solve():
    B, N, M = WIDE
    db = DeviceProductsBatch(B, M, N, seeds=31)
    prm = db.set_params(capi.default_parameters())
    prm.max_iterations = 12
    rc, p, res = capi.optimize_dense_products_batch(db.p0(), N, db.cb, db.cookie, prm)
    db.close()
    assert rc == 0 and np.all(res["status"] != BATCH_FAILED)
    return dict(p=p, results=res)


def bits(a):
    """the bytes of an array; of a record array (results): of its fields, not of the padding between records, which a copy
    need not keep"""
    if a.dtype.names:
        return b"".join(np.ascontiguousarray(a[f]).tobytes() for f in a.dtype.names)
    return np.ascontiguousarray(a).tobytes()


SEQUENCE = [uncertainty_host, bounded_robust_host, query_device_masked, products_solve, uncertainty_host]


def test_calls_of_different_kinds_and_shapes_share_the_cache():
    release = capi.lib().dogleg_amd_release_cache
    release()
    shared = [call() for call in SEQUENCE]
    for k, (call, got) in enumerate(zip(SEQUENCE, shared)):
        release()
        fresh = call()
        assert set(got) == set(fresh)
        for name in fresh:
            if fresh[name] is None:
                assert got[name] is None
                continue
            assert bits(got[name]) == bits(fresh[name]), \
                f"call {k + 1} ({call.__name__}): {name} differs between shared and fresh buffers"
    release()
