"""dogleg_amd_optimize_device2_robust on the GPU: the sparse and the dense device solve with a loss.

The reference is the NumPy oracle of tests/batch_robust_oracle.py on the host side of the same models (problems/device_robust.py's
OffsetHostModel).  The cases, their parameters and the seeds chosen by the oracle's decision margin are in
tests/device_robust_cases.py; every margin is asserted (floor 1e-6, the recorded value to 5 %) before anything is compared.
Limits, those of tests/test_dense_batch_robust_gpu.py: |p - p_oracle|_inf <= 1e-10, F and every weight to 1e-8 relative, the
number of accepted steps equal.  The figures are printed before they are asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_TRIVIAL, dptr
from problems.device_robust import OffsetDeviceModel, OffsetHostModel, TableDeviceModel
from tests import batch_robust_oracle as ro
from tests import device_robust_cases as dc
from tests import oracle_api as oa
from tests.parity import STEP_TOL, compare_traces

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_TOL = 1e-8


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/c/device_robust_abi.c as a shared library: the fields of a returned context through dogleg.h's own structs"""
    so = str(tmp_path_factory.mktemp("robust") / "libdevice_robust_abi.so")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "device_robust_abi.c"), "-o", so, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    S = C.CDLL(so)
    V = C.c_void_p
    S.robust_ctx_lambda.restype, S.robust_ctx_lambda.argtypes = C.c_double, [V]
    S.robust_ctx_before.restype, S.robust_ctx_before.argtypes = V, [V]
    S.robust_point_norm2x.restype, S.robust_point_norm2x.argtypes = C.c_double, [V]
    S.robust_point_x.restype, S.robust_point_x.argtypes = C.POINTER(C.c_double), [V]
    S.robust_point_p.restype, S.robust_point_p.argtypes = C.POINTER(C.c_double), [V]
    return S


class Model:
    """a case's problem behind the offsets wrapper: the device callback and the host side of the same function"""

    def __init__(self, name, fs):
        self.prob = dc.problem(name)
        self.off, self.planted = dc.offsets(name, fs)
        self.dev = OffsetDeviceModel(oa.DeviceTwin(self.prob), self.off)
        self.host = OffsetHostModel(self.prob, self.off)
        self.sparse = isinstance(self.prob, oa.BAProblem)
        self.Jp, self.Ji = self.prob.pattern() if self.sparse else (None, None)
        self.nnz = self.prob.nnz if self.sparse else 0

    def solve(self, loss, prm=None, **kw):
        p = self.prob
        return capi.optimize_device_robust(p.p0(), p.N, p.M, self.nnz, self.Jp, self.Ji, self.dev.cb, self.dev.cookie, loss,
                                           dc.params() if prm is None else prm, **kw)

    def close(self):
        self.dev.close()
        self.prob.close()


def compare(case, r, p, tr, w, o, neval):
    """a solve against the oracle's; prints the figures, then asserts.  The model is evaluated as often as the oracle evaluates
    it, or once more (the point behind a step that ends the solve, enqueued from inside that step: never counted, never used)"""
    dp = float(np.max(np.abs(p - o["p"])))
    dF = abs(r - o["norm2_x"]) / max(abs(o["norm2_x"]), 1e-300)
    dw = float(np.max(np.abs(w - o["weights"]) / o["weights"]))
    accepted = sum(1 for t in tr.trials() if t["accepted"] == 1)
    print(f"{case}: max |p - p_oracle| {dp:.3g}, F rel {dF:.3g}, weights rel {dw:.3g}, accepted steps {accepted} "
          f"(oracle {o['iterations']}), callbacks {tr.ncallbacks} / model evaluations {neval} (oracle {o['evaluations']})")
    assert r >= 0
    assert accepted == o["iterations"]
    assert tr.ncallbacks == o["evaluations"] and neval in (o["evaluations"], o["evaluations"] + 1)
    assert dp <= STEP_TOL and dF <= REL_TOL and dw <= REL_TOL
    assert np.all((w > 0) & (w <= 1))


def run_case(case):
    name, fs, kind = case
    o = dc.assert_margin(case)
    m = Model(name, fs)
    r, p, tr, w = m.solve(dc.loss_of(kind, fs))
    compare(case, r, p, tr, w, o, m.dev.neval())
    if kind == "cauchy" and fs >= 2:
        # the planted features end with the smallest weights.  (Not asked at featureSize 1 on the small problem: half an
        # observation displaced by 1.0 is taken up by its point, which only three observations hold -- the oracle's own solve ends
        # with one planted row at w = 0.985 and a clean one at 0.025.)
        print(f"largest weight of a planted feature {w[m.planted].max():.3g}, smallest of the others {w[~m.planted].min():.3g}")
        assert w[m.planted].max() < w[~m.planted].min()
    m.close()


# ---------------------------------------------------------------- 1. / 2. / 7. parity with the oracle, sparse and dense
@pytest.mark.parametrize("case", sorted(c for c in dc.MARGINS if c[0] in ("ba_small", "ba_medium")), ids=str)
def test_sparse_parity_with_the_oracle(gpu, case):
    run_case(case)


@pytest.mark.parametrize("case", sorted(c for c in dc.MARGINS if c[0] in ("dense_small", "dense_medium")), ids=str)
def test_dense_parity_with_the_oracle(gpu, case):
    run_case(case)


# ---------------------------------------------------------------- 3. TRIVIAL is the plain solve
def test_trivial_loss_is_the_plain_solve(gpu):
    """the limits of test_device_solve_same_iterates_as_host_callback_solve; F is summed in another order than norm2(x) (its
    last bits may differ: compare_traces holds the scalars to 1e-8), every weight is exactly 1"""
    m = Model("ba_medium", 2)
    pr = m.prob
    rp, pp, trp = capi.optimize_device(pr.p0(), pr.N, pr.M, pr.nnz, m.Jp, m.Ji, m.dev.cb, m.dev.cookie, dc.params())
    for fs in (1, 2, 3, 4):
        rr, p, tr, w = m.solve(BatchLoss(LOSS_TRIVIAL, 0.0, fs))
        compare_traces(tr, trp, step_tol=1e-12, what=("robust", "plain"))
        print(f"featureSize {fs}: max |p - p_plain| {np.max(np.abs(p - pp)):.3g}, F - norm2(x) {rr - rp:.3g}")
        assert np.max(np.abs(p - pp)) <= 1e-12 and abs(rr - rp) <= 1e-12 * rp
        assert w.shape == (pr.M // fs,) and np.all(w == 1.0)
    m.close()


# ---------------------------------------------------------------- 4. the prelude alone, on handcrafted patterns
CHUNK = 256                      # rows a workgroup of the sparse pass stages (libdogleg_amd/csrc/robust_prelude.hip: ROWS)
TABLE_M, TABLE_N = 600, 320


def handcrafted_pattern():
    """rows of 1, 2, 7, 300 and 0 entries; the 300-entry rows sit on both sides of the chunk boundaries (rows 255 | 256 and
    511 | 512) and at the end, so that the entry span of a chunk starts and ends inside long rows' neighbourhoods at odd and even
    offsets; rows 257 .. 259 are empty right behind a long row, and M = 600 is no multiple of the chunk"""
    rng = np.random.default_rng(11)
    lengths = np.array([1, 2, 7, 0, 2, 1, 7, 1] * (TABLE_M // 8))
    for r in (CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, TABLE_M - 1):
        lengths[r] = 300
    lengths[[CHUNK + 1, CHUNK + 2, CHUNK + 3]] = 0
    Jp = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    Ji = np.concatenate([np.sort(rng.choice(TABLE_N, size=k, replace=False)) for k in lengths]).astype(np.int32)
    assert TABLE_M % CHUNK != 0 and set(lengths) == {0, 1, 2, 7, 300} and Jp[CHUNK] % 2 != Jp[2 * CHUNK] % 2
    return Jp, Ji


def table_values(M, nJ, seed, fs):
    """x with a magnitude per feature over six decades around the loss scale, so that the weights run from 1 down below 1e-3"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(M) * np.repeat(10.0 ** rng.uniform(-3.5, 2.5, size=M // fs), fs)
    return x, rng.standard_normal(nJ)


def prelude_alone(shim, N, M, nnz, Jp, Ji, x, Jx, loss, row_of_entry):
    """one evaluation (max_iterations = 0) of the table model: (F, weights, x and J of the returned context)"""
    L = capi.lib()
    t = TableDeviceModel(x, Jx)
    ctx = C.c_void_p()
    F, p, tr, w = capi.optimize_device_robust(np.zeros(N), N, M, nnz, Jp, Ji, t.cb, t.cookie, loss, dc.params(max_iterations=0),
                                              ctx=ctx)
    assert F >= 0 and ctx.value and t.neval() == 1
    pt = shim.robust_ctx_before(ctx)
    assert shim.robust_point_norm2x(pt) == F
    xw = np.ctypeslib.as_array(shim.robust_point_x(pt), shape=(M,)).copy()
    Jw = np.zeros(len(Jx))
    assert L.dlg_point_download(L.dogleg_amd_backend(ctx), L.dogleg_amd_point_slot(ctx, pt), capi.VEC_J, dptr(Jw), len(Jx)) == 0
    L.dogleg_freeContext(C.byref(ctx))
    t.close()
    # NumPy's side
    lo = ro.Loss(loss.kind, loss.scale, loss.featureSize)
    rho, wr = lo.rho_w(lo.s(x))
    sq = np.sqrt(np.repeat(wr, lo.fs))
    for got, want, what in ((xw, sq * x, "x"), (Jw, sq[row_of_entry] * Jx, "J"), (w, wr, "weights")):
        err = float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))
        print(f"featureSize {lo.fs} kind {lo.kind}: {what} against NumPy {err:.3g}")
        assert err <= 1e-14, what
    Fref = float(rho.sum())
    print(f"featureSize {lo.fs} kind {lo.kind}: F {F!r} against NumPy {abs(F - Fref) / Fref:.3g}")
    assert abs(F - Fref) <= 1e-13 * Fref
    return F, w, xw, Jw


@pytest.mark.parametrize("fs", [1, 2, 3, 4])
def test_the_prelude_alone_on_a_handcrafted_sparse_pattern(gpu, shim, fs):
    Jp, Ji = handcrafted_pattern()
    nnz = int(Jp[-1])
    x, Jx = table_values(TABLE_M, nnz, 100 + fs, fs)
    rows = np.repeat(np.arange(TABLE_M), np.diff(Jp))
    for kind in ("cauchy", "huber", "soft_l1"):
        a = prelude_alone(shim, TABLE_N, TABLE_M, nnz, Jp, Ji, x, Jx, dc.loss_of(kind, fs), rows)
        b = prelude_alone(shim, TABLE_N, TABLE_M, nnz, Jp, Ji, x, Jx, dc.loss_of(kind, fs), rows)
        assert a[0] == b[0] and all(u.tobytes() == v.tobytes() for u, v in zip(a[1:], b[1:])), "two runs, other bits"
        assert a[1].min() < 1e-3 and a[1].max() > 0.5


@pytest.mark.parametrize("shape,fs", [((37, 5), 1), ((36, 5), 2), ((36, 5), 3), ((36, 5), 4), ((1500, 3), 2)], ids=str)
def test_the_prelude_alone_on_a_dense_table(gpu, shim, shape, fs):
    """37 x 5: an odd number of entries, pairs that straddle rows; 37 is prime, so the feature sizes above 1 run on 36 x 5;
    1500 x 3: 4500 entries, more than the 4096 a workgroup of the dense pass covers"""
    M, N = shape
    x, Jx = table_values(M, M * N, 200 + fs, fs)
    rows = np.repeat(np.arange(M), N)
    for kind in ("cauchy", "soft_l1"):
        a = prelude_alone(shim, N, M, 0, None, None, x, Jx, dc.loss_of(kind, fs), rows)
        b = prelude_alone(shim, N, M, 0, None, None, x, Jx, dc.loss_of(kind, fs), rows)
        assert a[0] == b[0] and all(u.tobytes() == v.tobytes() for u, v in zip(a[1:], b[1:])), "two runs, other bits"


# ---------------------------------------------------------------- 5. a parked backend with another pattern
@pytest.mark.parametrize("kind", ["cauchy", "huber"])
@pytest.mark.parametrize("overlap", [True, False], ids=["comparison beside the evaluation", "comparison first"])
def test_a_parked_backend_with_another_pattern(gpu, overlap, kind, monkeypatch):
    """patterns A, A, then B of equal N, M and nnz, as robust solves, each against the oracle: the second takes over the first's
    backend as it is, the third finds A's pattern there while its first evaluation runs -- the prelude scales J by B's row
    boundaries all the same (it reads the colptr of its own solve), and the evaluation made again uses that J.  With and without
    the work between a step and its wait: the same bits."""
    if overlap:
        monkeypatch.delenv("DOGLEG_AMD_NO_PATTERN_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("DOGLEG_AMD_NO_PATTERN_OVERLAP", "1")
    fs = 2
    bits = {}
    for between in (True, False):
        if between:
            monkeypatch.delenv("DOGLEG_AMD_NO_BETWEEN", raising=False)
        else:
            monkeypatch.setenv("DOGLEG_AMD_NO_BETWEEN", "1")
        capi.lib().dogleg_amd_release_cache()
        out = []
        for k, name in enumerate(("parked_a", "parked_a", "parked_b")):
            case = (name, fs, kind)
            o = dc.assert_margin(case)
            m = Model(name, fs)
            r, p, tr, w = m.solve(dc.loss_of(kind, fs))
            compare((k,) + case, r, p, tr, w, o, m.dev.neval())
            out.append((r, p.tobytes(), w.tobytes()))
            m.close()
        bits[between] = out
    assert bits[True] == bits[False]


# ---------------------------------------------------------------- 6. the held factor is the weighted one
def test_the_held_factor_is_the_weighted_one(gpu, shim):
    """dogleg_amd_marginal_variances on the context a robust solve returns: the diagonal of (J' W J + lambda I)^-1 with J of the
    model at the returned p, the returned weights and ctx->lambda; the tolerance of tests/test_covariance_gpu.py for the same
    call (1e-9 relative)"""
    L = capi.lib()
    L.dogleg_amd_marginal_variances.argtypes = [C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    fs = 2
    m = Model("ba_medium", fs)
    ctx = C.c_void_p()
    r, p, tr, w = m.solve(dc.loss_of("cauchy", fs), ctx=ctx)
    assert r >= 0 and ctx.value
    pt = shim.robust_ctx_before(ctx)
    lam = shim.robust_ctx_lambda(ctx)
    assert shim.robust_point_norm2x(pt) == r
    assert np.ctypeslib.as_array(shim.robust_point_p(pt), shape=(m.prob.N,)).tobytes() == p.tobytes()
    var = np.zeros(m.prob.N)
    assert L.dogleg_amd_marginal_variances(dptr(var), pt, ctx) == 0
    x, J = m.host.eval(p)
    wr = np.repeat(w, fs)
    d = np.diag(np.linalg.inv(J.T @ (wr[:, None] * J) + lam * np.eye(m.prob.N)))
    plain = np.diag(np.linalg.inv(J.T @ J + lam * np.eye(m.prob.N)))
    err = float(np.max(np.abs(var - d) / d))
    print(f"lambda {lam:.3g}: variances against (J'WJ + lambda I)^-1 {err:.3g}; against the unweighted inverse "
          f"{float(np.max(np.abs(var - plain) / plain)):.3g}")
    assert err <= 1e-9
    assert float(np.max(np.abs(var - plain) / plain)) > 1e-3          # (the unweighted factor would not pass)
    # x of the context is the weighted one
    xw = np.ctypeslib.as_array(shim.robust_point_x(pt), shape=(m.prob.M,))
    assert np.max(np.abs(xw - np.sqrt(wr) * x)) <= 1e-12 * max(1.0, np.max(np.abs(x)))
    L.dogleg_freeContext(C.byref(ctx))
    m.close()
