"""The return codes of the entry points that use the factor held on the device (libdogleg_amd/csrc/factor_users.hip),
as a table of literals: entry point, condition, code.  The codes are part of the interface: a caller tells "factorise
first" (DLG_ERR_STATE) from "fix the call" (DLG_ERR_ARG), and a count of zero is either nothing to do (DLG_OK) or still a
question to the backend's state, per entry point.  Where a call breaks two rules at once (a null output AND no factor)
the row pins which of them answers.  Nothing here looks at a computed value; no kernel of interest runs.

dlg_feature_leverage with a null output is not in the table: it does not check that pointer."""
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import dptr, iptr
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu
OK, ARG, STATE = 0, 2, 3


# ---------------------------------------------------------------- the calls: valid on every backend of the fixture
# z: a count of zero; null: no output pointer
def _solve_with_factor(be, s, z, null):
    rhs, out = np.zeros(be.N), np.zeros(be.N)
    return be.L.dlg_solve_with_factor(be.h, s, dptr(rhs), None if null else dptr(out), 0 if z else 1)


def _solve_multi(be, s, z, null):
    rhs, out = np.zeros(be.N), np.zeros(be.N)
    return be.L.dlg_solve_multi(be.h, s, dptr(rhs), None if null else dptr(out), 0 if z else 1)


def _pseudoinverse_chunk(be, s, z, null):
    out = np.zeros(be.N)
    return be.L.dlg_pseudoinverse_chunk(be.h, s, 0, 0 if z else 1, None if null else dptr(out))


def _feature_leverage(be, s, z, null):
    assert not null
    out = np.zeros(1)
    return be.L.dlg_feature_leverage(be.h, s, 1, 0, 0 if z else 1, dptr(out))


def _outlierness_factors(be, s, z, null):
    out = np.zeros(1)
    return be.L.dlg_outlierness_factors(be.h, s, 1, 0 if z else 1, 1.0, None if null else dptr(out))


def _leverage_query(be, s, z, null):
    assert not z
    Jq, out = np.ones(1), np.zeros(1)
    return be.L.dlg_leverage_query(be.h, s, dptr(Jq), 0, 1, 1, None if null else dptr(out))


def _covariance_blocks(be, s, z, null):
    a, one, out = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1)
    return be.L.dlg_covariance_blocks(be.h, s, 0 if z else 1, iptr(a), iptr(one), iptr(a), iptr(one), None if null else dptr(out))


def _marginal_variances(be, s, z, null):
    assert not z
    out = np.zeros(be.N)
    return be.L.dlg_marginal_variances(be.h, s, None if null else dptr(out))


def _query(be, s, z, null, nobs):
    qrow, var, val, out = np.array([0, 1], dtype=np.int32), np.zeros(1, dtype=np.int32), np.ones(1), np.zeros(1)
    return be.L.dlg_query_covariance(be.h, s, 0 if z else 1, iptr(qrow), iptr(qrow), iptr(var), dptr(val), nobs,
                                     None if null else dptr(out))


def _query_covariance(be, s, z, null):
    return _query(be, s, z, null, -1)


def _query_covariance_obs(be, s, z, null):
    return _query(be, s, z, null, 1)


def _covariance_entries(be, s, z, null):
    a, out = np.zeros(1, dtype=np.int32), np.zeros(1)
    return be.L.dlg_covariance_entries(be.h, s, 0 if z else 1, iptr(a), iptr(a), None if null else dptr(out))


CALLS = {f.__name__[1:]: f for f in (
    _solve_with_factor, _solve_multi, _pseudoinverse_chunk, _feature_leverage, _outlierness_factors, _leverage_query,
    _covariance_blocks, _marginal_variances, _query_covariance, _query_covariance_obs, _covariance_entries)}

# ---------------------------------------------------------------- the conditions: (backend, slot, count of zero, null output)
CONDITIONS = {
    "no factor":             ("sparse_unfactored", 0, False, False),
    "factor of other slot":  ("sparse", 1, False, False),       # slot 1 has inputs, slot 0 the factor
    "sharded":               ("dense_sharded", 0, False, False),     # a factor is held
    "partitioned":           ("sparse_partitioned", 0, False, False),
    "dense-products":        ("products", 0, False, False),     # a factor is held
    "no inputs":             ("dense", 1, False, False),        # slot 0 has inputs and the factor
    "zero count":            ("sparse", 0, True, False),
    "zero count, no factor": ("sparse_unfactored", 0, True, False),
    "null output":           ("sparse", 0, False, True),
    "null output, no factor": ("sparse_unfactored", 0, False, True),
}

# ---------------------------------------------------------------- the table
TABLE = [
    ("solve_with_factor", "no factor", STATE),
    ("solve_with_factor", "factor of other slot", STATE),
    ("solve_with_factor", "sharded", OK),
    ("solve_with_factor", "partitioned", STATE),
    ("solve_with_factor", "dense-products", OK),
    ("solve_with_factor", "no inputs", STATE),
    ("solve_with_factor", "zero count", OK),
    ("solve_with_factor", "zero count, no factor", STATE),
    ("solve_with_factor", "null output", ARG),
    ("solve_with_factor", "null output, no factor", ARG),

    ("solve_multi", "no factor", STATE),
    ("solve_multi", "factor of other slot", STATE),
    ("solve_multi", "sharded", OK),                        # refuses a partitioned backend only
    ("solve_multi", "partitioned", STATE),
    ("solve_multi", "dense-products", OK),
    ("solve_multi", "no inputs", STATE),
    ("solve_multi", "zero count", OK),
    ("solve_multi", "zero count, no factor", STATE),
    ("solve_multi", "null output", ARG),
    ("solve_multi", "null output, no factor", ARG),

    ("pseudoinverse_chunk", "no factor", STATE),
    ("pseudoinverse_chunk", "factor of other slot", STATE),
    ("pseudoinverse_chunk", "sharded", STATE),
    ("pseudoinverse_chunk", "partitioned", STATE),
    ("pseudoinverse_chunk", "dense-products", STATE),
    ("pseudoinverse_chunk", "no inputs", STATE),
    ("pseudoinverse_chunk", "zero count", OK),
    ("pseudoinverse_chunk", "zero count, no factor", STATE),
    ("pseudoinverse_chunk", "null output", ARG),
    ("pseudoinverse_chunk", "null output, no factor", ARG),

    ("feature_leverage", "no factor", STATE),
    ("feature_leverage", "factor of other slot", STATE),
    ("feature_leverage", "sharded", STATE),
    ("feature_leverage", "partitioned", STATE),
    ("feature_leverage", "dense-products", STATE),
    ("feature_leverage", "no inputs", STATE),
    ("feature_leverage", "zero count", OK),
    ("feature_leverage", "zero count, no factor", STATE),       # nf == 0 still asks for the factor

    ("outlierness_factors", "no factor", STATE),
    ("outlierness_factors", "factor of other slot", STATE),
    ("outlierness_factors", "sharded", STATE),
    ("outlierness_factors", "partitioned", STATE),
    ("outlierness_factors", "dense-products", STATE),
    ("outlierness_factors", "no inputs", STATE),
    ("outlierness_factors", "zero count", OK),
    ("outlierness_factors", "zero count, no factor", STATE),
    ("outlierness_factors", "null output", ARG),
    ("outlierness_factors", "null output, no factor", STATE),   # the state is asked before the output is looked at

    ("leverage_query", "no factor", STATE),
    ("leverage_query", "factor of other slot", STATE),
    ("leverage_query", "sharded", STATE),
    ("leverage_query", "partitioned", STATE),
    ("leverage_query", "dense-products", STATE),
    ("leverage_query", "no inputs", STATE),
    ("leverage_query", "null output", ARG),
    ("leverage_query", "null output, no factor", STATE),

    ("covariance_blocks", "no factor", STATE),
    ("covariance_blocks", "factor of other slot", STATE),
    ("covariance_blocks", "sharded", STATE),
    ("covariance_blocks", "partitioned", STATE),
    ("covariance_blocks", "dense-products", OK),
    ("covariance_blocks", "no inputs", STATE),
    ("covariance_blocks", "zero count", OK),
    ("covariance_blocks", "zero count, no factor", OK),         # nreq == 0: nothing to do, whatever the state
    ("covariance_blocks", "null output", ARG),
    ("covariance_blocks", "null output, no factor", ARG),

    ("marginal_variances", "no factor", STATE),
    ("marginal_variances", "factor of other slot", STATE),
    ("marginal_variances", "sharded", STATE),
    ("marginal_variances", "partitioned", STATE),
    ("marginal_variances", "dense-products", OK),
    ("marginal_variances", "no inputs", STATE),
    ("marginal_variances", "null output", ARG),
    ("marginal_variances", "null output, no factor", ARG),

    ("query_covariance", "no factor", STATE),
    ("query_covariance", "factor of other slot", STATE),
    ("query_covariance", "sharded", STATE),
    ("query_covariance", "partitioned", STATE),
    ("query_covariance", "dense-products", OK),                 # the plain form reads no J
    ("query_covariance", "no inputs", STATE),
    ("query_covariance", "zero count", OK),
    ("query_covariance", "zero count, no factor", OK),
    ("query_covariance", "null output", ARG),
    ("query_covariance", "null output, no factor", ARG),

    ("query_covariance_obs", "no factor", STATE),
    ("query_covariance_obs", "factor of other slot", STATE),
    ("query_covariance_obs", "sharded", STATE),
    ("query_covariance_obs", "partitioned", STATE),
    ("query_covariance_obs", "dense-products", STATE),          # the observation form does
    ("query_covariance_obs", "no inputs", STATE),
    ("query_covariance_obs", "zero count", OK),
    ("query_covariance_obs", "zero count, no factor", OK),
    ("query_covariance_obs", "null output", ARG),
    ("query_covariance_obs", "null output, no factor", ARG),

    ("covariance_entries", "no factor", STATE),
    ("covariance_entries", "factor of other slot", STATE),
    ("covariance_entries", "sharded", STATE),
    ("covariance_entries", "partitioned", STATE),
    ("covariance_entries", "dense-products", OK),
    ("covariance_entries", "no inputs", STATE),
    ("covariance_entries", "zero count", OK),
    ("covariance_entries", "zero count, no factor", OK),
    ("covariance_entries", "null output", ARG),
    ("covariance_entries", "null output, no factor", ARG),
]

# what the messages of these refusals must keep saying (callers and other tests match on it)
MESSAGES = [
    ("covariance_entries", "no factor", "no factorization"),
    ("solve_multi", "no factor", "no factorization"),
    ("covariance_blocks", "partitioned", "sharded or partitioned"),
    ("marginal_variances", "sharded", "sharded or partitioned"),
    ("query_covariance", "partitioned", "sharded or partitioned"),
    ("covariance_entries", "sharded", "sharded or partitioned"),
    ("query_covariance_obs", "dense-products", "dense-products"),
    ("feature_leverage", "dense-products", "dense-products"),
]


# ---------------------------------------------------------------- the backends, made once
@pytest.fixture(scope="module")
def backends(gpu):
    B, keep = {}, []
    prob = oa.BAProblem(5, 40, 300, seed=11)
    Jp, Ji = prob.pattern()
    p = prob.p0()
    x, Jx = prob.eval(p)
    for name in ("sparse", "sparse_unfactored"):
        be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
        be.set_pattern(Jp, Ji)
        for s in ((1, 0) if name == "sparse" else (0,)):
            be.set_p(s, p)
            be.upload(s, x, Jx)
            be.eval(s)
        if name == "sparse":
            assert be.factorize(0, 0.0)
        B[name] = be
    big = oa.BAProblem(49, 900, 10000, seed=5)                 # (the pattern the other refusal tests partition)
    be = capi.Backend(capi.DLG_SPARSE, big.N, big.M, big.nnz)
    be.set_partition(0, 2)
    be.set_pattern(*big.pattern())
    B["sparse_partitioned"] = be
    dp = oa.DenseProblem(M=40, N=7, seed=2)
    p = dp.p0()
    x, J = dp.eval(p)
    for name in ("dense", "dense_sharded"):
        be = capi.Backend(capi.DLG_DENSE, dp.N, dp.M)
        if name == "dense_sharded":
            be.set_shard(0, dp.M, lambda buf, count, cookie: 0)     # one rank holding every row: the sum is what is there
        be.set_p(0, p)
        be.upload(0, x, J)
        be.eval(0)
        assert be.factorize(0, 0.0)
        B[name] = be
    be = capi.Backend(capi.DLG_DENSE_PRODUCTS, dp.N, dp.M)
    be.set_p(0, p)
    be.upload_products(0, float(x @ x), J.T @ x, J.T @ J)
    be.eval(0)
    assert be.factorize(0, 0.0)
    B["products"] = be
    keep += [prob, big, dp]
    yield B
    for be in B.values():
        be.close()


def _call(backends, entry, cond):
    name, s, z, null = CONDITIONS[cond]
    return CALLS[entry](backends[name], s, z, null)


@pytest.mark.parametrize("entry,cond,code", TABLE, ids=[f"{e}-{c.replace(' ', '_').replace(',', '')}" for e, c, _ in TABLE])
def test_return_code(backends, entry, cond, code):
    rc = _call(backends, entry, cond)
    print(f"dlg_{entry}, {cond}: {rc}" + (f" ({backends['sparse'].L.dlg_last_error().decode()})" if rc else ""))
    assert rc == code


@pytest.mark.parametrize("entry,cond,text", MESSAGES, ids=[f"{e}-{c.replace(' ', '_')}" for e, c, _ in MESSAGES])
def test_message(backends, entry, cond, text):
    assert _call(backends, entry, cond) == STATE
    msg = backends["sparse"].L.dlg_last_error().decode()
    assert text in msg, msg
    assert "dlg_" + entry.replace("_obs", "") in msg, msg          # every message names the entry point
