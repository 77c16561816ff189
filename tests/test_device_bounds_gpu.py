"""dogleg_amd_optimize_device2_bounded on the GPU: the sparse and the dense device solve under box bounds.

The reference is the NumPy oracle of tests/batch_bounds_oracle.py on the host side of the same models (problems/device_robust.py's
OffsetHostModel).  The cases, their bounds and parameters and the oracle's decision margin of each are in
tests/device_bounds_cases.py; every margin is asserted (floor 1e-6, the recorded value to 5 %) before anything is compared.
Limits, those of tests/test_device_robust_gpu.py: |p - p_oracle|_inf <= STEP_TOL = 1e-10, F and every weight to 1e-8 relative;
held equal byte for byte; accepted steps, callbacks and the four counts of dogleg_amd_bounded_last_stats equal to the oracle's.
The figures are printed before they are asserted."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_TRIVIAL, dptr
from problems.batch_linear import from_normal_equations
from problems.device_robust import OffsetDeviceModel, OffsetHostModel, TableDeviceModel, dense_of
from tests import batch_bounds_oracle as bb
from tests import batch_robust_oracle as ro
from tests import device_bounds_cases as bc
from tests import device_robust_cases as dc
from tests import oracle_api as oa
from tests.parity import STEP_TOL, compare_traces
from tests.test_device_robust_gpu import TABLE_M, TABLE_N, handcrafted_pattern

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_TOL = 1e-8
VAR_TOL = 1e-9                   # tests/test_covariance_gpu.py's, for dogleg_amd_marginal_variances


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    """tests/c/device_robust_abi.c as a shared library: the fields of a returned context through dogleg.h's own structs"""
    so = str(tmp_path_factory.mktemp("bounds") / "libdevice_robust_abi.so")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "device_robust_abi.c"), "-o", so, "-L", libdir, "-ldogleg_amd",
                    "-Wl,-rpath," + libdir], check=True)
    S = C.CDLL(so)
    V = C.c_void_p
    S.robust_ctx_lambda.restype, S.robust_ctx_lambda.argtypes = C.c_double, [V]
    S.robust_ctx_before.restype, S.robust_ctx_before.argtypes = V, [V]
    S.robust_point_norm2x.restype, S.robust_point_norm2x.argtypes = C.c_double, [V]
    S.robust_point_p.restype, S.robust_point_p.argtypes = C.POINTER(C.c_double), [V]
    return S


class Model:
    """a case's problem behind the offsets wrapper: the device callback and the host side of the same function"""

    def __init__(self, name):
        self.name = name
        self.prob = bc.problem(name)
        self.off = bc.offsets(name)
        self.dev = OffsetDeviceModel(oa.DeviceTwin(self.prob), self.off)
        self.host = OffsetHostModel(self.prob, self.off)
        self.sparse = isinstance(self.prob, oa.BAProblem)
        self.Jp, self.Ji = self.prob.pattern() if self.sparse else (None, None)
        self.nnz = self.prob.nnz if self.sparse else 0
        self.loss = bc.loss_pair(name)[1]

    def solve(self, lo, hi, prm=None, **kw):
        p = self.prob
        return capi.optimize_device_bounded(p.p0(), p.N, p.M, self.nnz, self.Jp, self.Ji, self.dev.cb, self.dev.cookie, lo, hi,
                                            self.loss, bc.params(self.name) if prm is None else prm, **kw)

    def close(self):
        self.dev.close()
        self.prob.close()


def compare(what, r, p, tr, w, held, o, stats):
    """a solve against the oracle's; prints the figures, then asserts"""
    dp = float(np.max(np.abs(p - o["p"])))
    dF = abs(r - o["norm2_x"]) / max(abs(o["norm2_x"]), 1e-300)
    accepted = sum(1 for t in tr.trials() if t["accepted"] == 1)
    want = {k: float(o[k]) for k in ("evaluations", "clipped", "fallbacks", "held_steps")}
    got = {k: stats[k] for k in want}
    print(f"{what}: max |p - p_oracle| {dp:.3g}, F rel {dF:.3g}, held {int(np.count_nonzero(held))} (oracle "
          f"{int(np.count_nonzero(o['held']))}, {int(np.count_nonzero(held != o['held']))} bytes differ), accepted steps {accepted} "
          f"(oracle {o['iterations']}), callbacks {tr.ncallbacks} (oracle {o['evaluations']}), stats {got} (oracle {want})")
    assert r >= 0
    assert accepted == o["iterations"] and tr.ncallbacks == o["evaluations"]
    assert got == want
    assert held.tobytes() == o["held"].tobytes()
    assert dp <= STEP_TOL and dF <= REL_TOL
    if w is not None:
        dw = float(np.max(np.abs(w - o["weights"]) / o["weights"]))
        print(f"{what}: weights rel {dw:.3g}, in [{w.min():.3g}, {w.max():.3g}]")
        assert dw <= REL_TOL and np.all((w > 0) & (w <= 1))


def run_case(name, what=None):
    o = bc.assert_margin(name)
    lo, hi = bc.oracle(name)[1:3]
    m = Model(name)
    r, p, tr, w, held = m.solve(lo, hi)
    compare(what or name, r, p, tr, w, held, o, capi.bounded_last_stats())
    assert np.all((p >= lo) & (p <= hi))
    m.close()
    return r, p, held


# ---------------------------------------------------------------- 1. / 7. parity with the oracle, sparse and dense; Huber and bounds
@pytest.mark.parametrize("name", bc.SPARSE)
def test_sparse_parity_with_the_oracle(gpu, name):
    """branch1's second step is a fallback whose alpha is set by variable 9 (p = 0.0238, far = lower = -0.0944): p + alpha d
    rounds onto the bound's bits in the oracle, and one ulp (1.4e-17) short of them where d differs in its last bit, as the
    GPU's Cauchy step does -- the library puts the component that sets alpha on its bound whichever way the sum rounds
    (libdogleg_amd/csrc/bounds_device.hip: k_bounds_fallback), so the variable is held at the next point as it is in the
    oracle"""
    run_case(name)


@pytest.mark.parametrize("name", bc.DENSE)
def test_dense_parity_with_the_oracle(gpu, name):
    run_case(name)


# ---------------------------------------------------------------- 2. bounds that clamp nothing
@pytest.mark.parametrize("name", ["ba_small", "dense_small", "ba_small_huber"])
def test_bounds_that_clamp_nothing_are_the_plain_solve(gpu, name):
    """NULL arrays, infinite entries and a box that is never met, against dogleg_optimize_device2 (with a loss: against _robust):
    the traces to STEP_TOL, held all 0.  Not bit for bit: the bounded solve takes the unfused route, which sums Jt x in another
    fixed order than the one-pass evaluation."""
    m = Model(name)
    pr = m.prob
    prm = bc.params(name)
    if m.loss is None:
        rp, pp, trp = capi.optimize_device(pr.p0(), pr.N, pr.M, m.nnz, m.Jp, m.Ji, m.dev.cb, m.dev.cookie, prm)
        wp = None
    else:
        rp, pp, trp, wp = capi.optimize_device_robust(pr.p0(), pr.N, pr.M, m.nnz, m.Jp, m.Ji, m.dev.cb, m.dev.cookie, m.loss, prm)
    assert rp >= 0
    far = 1e6 * (1.0 + np.abs(pr.p0()))
    for what, lo, hi in (("NULL", None, None), ("infinite", np.full(pr.N, -np.inf), np.full(pr.N, np.inf)),
                         ("one side NULL", None, np.full(pr.N, np.inf)), ("never met", pr.p0() - far, pr.p0() + far)):
        r, p, tr, w, held = m.solve(lo, hi)
        worst = compare_traces(tr, trp, step_tol=STEP_TOL, what=("bounded", "plain"))
        st = capi.bounded_last_stats()
        print(f"{name}, {what}: worst step difference {worst:.3g}, max |p - p_plain| {np.max(np.abs(p - pp)):.3g}, "
              f"F rel {abs(r - rp) / rp:.3g}, stats {st}")
        assert np.max(np.abs(p - pp)) <= STEP_TOL and abs(r - rp) <= REL_TOL * rp
        assert not held.any() and st["clipped"] == st["fallbacks"] == st["held_steps"] == 0 and st["evaluations"] == tr.ncallbacks
        if wp is not None:
            assert np.max(np.abs(w - wp) / wp) <= REL_TOL
    m.close()


# ---------------------------------------------------------------- 3. hold and mask alone
def table(M, nJ, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return scale * rng.standard_normal(M), rng.standard_normal(nJ)


def placed_bounds(p0, g, mode):
    """p0 on bounds with the sign of g prescribing what happens there.  mode "mixed", by i mod 5: 0 on a bound that g pushes
    against (held: lower where g > 0, upper where g < 0); 1 on a bound that g pushes away from (free); 2 strictly inside a box;
    3 lower = upper = p0 (held, on the side g says); 4 no bound.  "none": infinite bounds.  "all": lower = upper = p0 everywhere"""
    N = len(p0)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    for i in range(N):
        k = {"mixed": i % 5, "none": 4, "all": 3}[mode]
        if k == 0:
            (lo if g[i] > 0 else hi)[i] = p0[i]
        elif k == 1:
            (hi if g[i] > 0 else lo)[i] = p0[i]
        elif k == 2:
            lo[i], hi[i] = p0[i] - 1.0, p0[i] + 1.0
        elif k == 3:
            lo[i] = hi[i] = p0[i]
    return lo, hi


def hold_and_mask_alone(shim, N, M, nnz, Jp, Ji, x, Jx, col_of_entry, mode):
    """one evaluation (max_iterations = 0) of the table model under bounds placed on p0: the returned context's J and Jt_x
    against NumPy, the held bytes against the oracle's held_set"""
    L = capi.lib()
    Jd = dense_of(Jp, Ji, Jx, N) if nnz else Jx.reshape(M, N)
    g = Jd.T @ x
    assert np.all(g != 0.0) and np.min(np.abs(g)) > 1e-6 * np.max(np.abs(g))     # (no sign sits on a rounding edge)
    p0 = np.random.default_rng(5).standard_normal(N)
    lo, hi = placed_bounds(p0, g, mode)
    want = bb.held_set(p0, g, lo, hi)
    t = TableDeviceModel(x, Jx)
    ctx = C.c_void_p()
    F, p, tr, w, held = capi.optimize_device_bounded(p0, N, M, nnz, Jp, Ji, t.cb, t.cookie, lo, hi, None, dc.params(max_iterations=0),
                                                     ctx=ctx)
    assert F >= 0 and ctx.value and t.neval() == 1 and p.tobytes() == p0.tobytes()
    pt = shim.robust_ctx_before(ctx)
    be, slot = L.dogleg_amd_backend(ctx), L.dogleg_amd_point_slot(ctx, pt)
    Jm, gF = np.full(len(Jx), np.nan), np.full(N, np.nan)
    assert L.dlg_point_download(be, slot, capi.VEC_J, dptr(Jm), len(Jx)) == 0
    assert L.dlg_point_download(be, slot, capi.VEC_JTX, dptr(gF), N) == 0
    L.dogleg_freeContext(C.byref(ctx))
    t.close()
    st = capi.bounded_last_stats()
    h = want != 0
    print(f"{mode}: {int(h.sum())} of {N} held ({int((want == 1).sum())} at lower, {int((want == 2).sum())} at upper), "
          f"{int(h[col_of_entry].sum())} of {len(Jx)} entries of J in held columns, stats {st}")
    assert held.tobytes() == want.tobytes()
    assert {"none": not h.any(), "all": h.all(), "mixed": 0 < h.sum() < N and (N < 5 or set(want) == {0, 1, 2})}[mode]
    # J: exact zeros in the held columns (+0.0: the bits), every other entry with its input bits
    Jwant = np.where(h[col_of_entry], 0.0, Jx)
    assert Jm.tobytes() == Jwant.tobytes()
    # Jt_x: exact zeros where held, NumPy's g elsewhere
    err = float(np.max(np.abs(gF - np.where(h, 0.0, g)))) / float(np.max(np.abs(g)))
    print(f"{mode}: g_F against NumPy {err:.3g}")
    assert np.all(gF[h] == 0.0) and err <= 1e-13
    assert abs(F - float(x @ x)) <= 1e-13 * F and st["evaluations"] == 1 and st["clipped"] == st["fallbacks"] == st["held_steps"] == 0
    return F, held, Jm, gF


def test_hold_and_mask_alone_on_a_handcrafted_sparse_pattern(gpu, shim):
    """rows of 0, 1, 2, 7 and 300 entries, M = 600, N = 320 (two workgroups of the per-variable kernels, the second one partly
    filled; 3 061 entries: more than the 2 048 a workgroup of the mask pass covers, and no multiple of its lanes)"""
    Jp, Ji = handcrafted_pattern()
    nnz = int(Jp[-1])
    assert nnz > 2048 and TABLE_N > 256 and TABLE_N % 256 != 0
    x, Jx = table(TABLE_M, nnz, 301)
    for mode in ("mixed", "none", "all"):
        a = hold_and_mask_alone(shim, TABLE_N, TABLE_M, nnz, Jp, Ji, x, Jx, Ji, mode)
        b = hold_and_mask_alone(shim, TABLE_N, TABLE_M, nnz, Jp, Ji, x, Jx, Ji, mode)
        assert a[0] == b[0] and all(u.tobytes() == v.tobytes() for u, v in zip(a[1:], b[1:])), "two runs, other bits"


@pytest.mark.parametrize("shape", [(37, 5), (1500, 3)], ids=str)
def test_hold_and_mask_alone_on_a_dense_table(gpu, shim, shape):
    """37 x 5: an odd number of entries; 1500 x 3: 4500 entries, more than the 2 048 a workgroup of the mask pass covers, and a
    column count that does not divide the workgroup's stride"""
    M, N = shape
    x, Jx = table(M, M * N, 400 + N)
    cols = np.tile(np.arange(N), M)
    for mode in ("mixed", "none", "all"):
        a = hold_and_mask_alone(shim, N, M, 0, None, None, x, Jx, cols, mode)
        b = hold_and_mask_alone(shim, N, M, 0, None, None, x, Jx, cols, mode)
        assert a[0] == b[0] and all(u.tobytes() == v.tobytes() for u, v in zip(a[1:], b[1:])), "two runs, other bits"


# ---------------------------------------------------------------- 4. lambda > 0: a singular free block
class TableHostModel:
    """the host side of TableDeviceModel for the oracle: x and J do not depend on p"""

    def __init__(self, x, Jd, p0):
        self.x, self.J, self._p0 = x, Jd, p0
        self.M, self.N = Jd.shape

    def p0(self):
        return self._p0.copy()

    def eval(self, p):
        return self.x.copy(), self.J.copy()


def free_block_inverse_diagonal(Jd, held, lam):
    """diag of the inverse of the matrix of step 4: J_F' J_F + lambda I with the held rows and columns the identity's"""
    h = held != 0
    JF = np.where(h[None, :], 0.0, Jd)
    H = JF.T @ JF + lam * np.eye(len(h))
    H[h, h] = 1.0
    return np.diag(np.linalg.inv(H))


@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_a_singular_free_block_takes_the_lambda_schedule_and_the_held_diagonal_is_one(gpu, shim, kind):
    """a table model with an exactly-zero column that stays free (its g is 0: never held), as tests/test_dense_gpu.py makes JtJ
    singular, and a fifth of the variables held: the factorisation at lambda = 0 breaks down on the free block, lambda goes
    to 1e-10 as the oracle's does, and afterwards the held diagonal is exactly 1 -- the marginal variance of a held variable
    is 1.0, that of the zero column 1 / lambda"""
    L = capi.lib()
    L.dogleg_amd_marginal_variances.argtypes = [C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    if kind == "sparse":
        N, M = TABLE_N, TABLE_M
        Jp, Ji = handcrafted_pattern()
        nnz = int(Jp[-1])
        x, Jx = table(M, nnz, 501, scale=1e-2)
        zero = 7
        Jx[Ji == zero] = 0.0
        Jd = dense_of(Jp, Ji, Jx, N)
    else:
        N, M, nnz, Jp, Ji = 5, 37, 0, None, None
        x, Jx = table(M, M * N, 502, scale=1e-2)
        zero = 2
        Jx.reshape(M, N)[:, zero] = 0.0
        Jd = Jx.reshape(M, N)
    g = Jd.T @ x
    p0 = np.random.default_rng(6).standard_normal(N)
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    for i in range(N):
        if i % 5 == 0 and i != zero:
            (lo if g[i] > 0 else hi)[i] = p0[i]
    prm = dc.params()
    o = bb.solve_one(TableHostModel(x, Jd, p0), prm, ro.Loss(LOSS_TRIVIAL, 0.0, 1), lo, hi)
    t = TableDeviceModel(x, Jx)
    ctx = C.c_void_p()
    F, p, tr, w, held = capi.optimize_device_bounded(p0, N, M, nnz, Jp, Ji, t.cb, t.cookie, lo, hi, None, prm, ctx=ctx)
    st = capi.bounded_last_stats()
    assert F >= 0 and ctx.value
    lam = shim.robust_ctx_lambda(ctx)
    lambdas = [tt["lambda_"] for tt in tr.trials()]
    print(f"{kind}: lambda {lam:g} (oracle {o['lambda_']:g}), per trial {sorted(set(lambdas))}, {tr.ntrials} trials, callbacks "
          f"{tr.ncallbacks} (oracle {o['evaluations']}), held {int(np.count_nonzero(held))}, stats {st}")
    assert o["lambda_"] == 1e-10 and lam == o["lambda_"] and 1 in o["step_types"]
    assert held.tobytes() == o["held"].tobytes() and np.count_nonzero(held) == len(range(0, N, 5)) and held[zero] == 0
    assert tr.ncallbacks == o["evaluations"] and sum(1 for tt in tr.trials() if tt["accepted"] == 1) == o["iterations"]
    assert (st["evaluations"], st["clipped"], st["fallbacks"], st["held_steps"]) == \
           (o["evaluations"], o["clipped"], o["fallbacks"], o["held_steps"])
    pt = shim.robust_ctx_before(ctx)
    var = np.zeros(N)
    assert L.dogleg_amd_marginal_variances(dptr(var), pt, ctx) == 0
    L.dogleg_freeContext(C.byref(ctx))
    t.close()
    want = free_block_inverse_diagonal(Jd, held, lam)
    h = held != 0
    err = float(np.max(np.abs(var[~h] - want[~h]) / want[~h]))
    print(f"{kind}: variances of the held variables {sorted(set(var[h]))}, of the zero column {var[zero]:.6g}, free ones against "
          f"NumPy {err:.3g}")
    assert np.all(var[h] == 1.0)
    assert abs(var[zero] - 1.0 / lam) <= VAR_TOL / lam and err <= VAR_TOL


# ---------------------------------------------------------------- 5. the held factor
def test_the_held_factor_is_that_of_the_free_block(gpu, shim):
    """dogleg_amd_marginal_variances on the context a bounded solve returns: at the free variables the diagonal of
    (J_F' J_F + lambda I)^-1 with J of the model at the returned p, at the held ones exactly 1.0; the inverse of the unmasked
    matrix would not pass"""
    L = capi.lib()
    L.dogleg_amd_marginal_variances.argtypes = [C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    name = "ba_medium3"
    lo, hi = bc.oracle(name)[1:3]
    m = Model(name)
    ctx = C.c_void_p()
    r, p, tr, w, held = m.solve(lo, hi, ctx=ctx)
    assert r >= 0 and ctx.value
    pt = shim.robust_ctx_before(ctx)
    lam = shim.robust_ctx_lambda(ctx)
    assert shim.robust_point_norm2x(pt) == r
    assert np.ctypeslib.as_array(shim.robust_point_p(pt), shape=(m.prob.N,)).tobytes() == p.tobytes()
    N = m.prob.N
    var, gF, Jm = np.zeros(N), np.zeros(N), np.zeros(m.nnz)
    assert L.dogleg_amd_marginal_variances(dptr(var), pt, ctx) == 0
    be, slot = L.dogleg_amd_backend(ctx), L.dogleg_amd_point_slot(ctx, pt)
    assert L.dlg_point_download(be, slot, capi.VEC_JTX, dptr(gF), N) == 0
    assert L.dlg_point_download(be, slot, capi.VEC_J, dptr(Jm), m.nnz) == 0
    L.dogleg_freeContext(C.byref(ctx))
    x, J = m.host.eval(p)
    h = held != 0
    want = free_block_inverse_diagonal(J, held, lam)
    plain = np.diag(np.linalg.inv(J.T @ J + lam * np.eye(N)))
    err = float(np.max(np.abs(var[~h] - want[~h]) / want[~h]))
    unmasked = float(np.max(np.abs(var[~h] - plain[~h]) / plain[~h]))
    print(f"lambda {lam:.3g}, {int(h.sum())} of {N} held: variances of the free variables against (J_F'J_F + lambda I)^-1 {err:.3g}; "
          f"against the unmasked inverse {unmasked:.3g}; held ones {sorted(set(var[h]))}")
    assert h.sum() == bc.RECORDED[name]["held"]
    assert err <= VAR_TOL and np.all(var[h] == 1.0)
    assert unmasked > 1e-3                                  # (the unmasked factor would not pass)
    # the context holds the masked point
    assert np.all(gF[h] == 0.0) and np.max(np.abs(gF - np.where(h, 0.0, J.T @ x))) <= 1e-9 * max(1.0, np.max(np.abs(J.T @ x)))
    Jx = m.prob.eval(p)[1]
    assert np.all(Jm[h[m.Ji]] == 0.0) and np.max(np.abs(Jm - Jx)[~h[m.Ji]]) <= 1e-12 * np.max(np.abs(Jx))
    m.close()


# ---------------------------------------------------------------- 6. a parked backend with another pattern
def test_a_parked_backend_with_another_pattern(gpu):
    """patterns A, A, then B of equal N, M and nnz, as bounded solves, each against the oracle: the second takes over the first's
    backend as it is, the third finds A's pattern there -- a bounded solve finishes the comparison before its first evaluation,
    and masks J by the row indices of its own call"""
    capi.lib().dogleg_amd_release_cache()
    out = []
    for k, name in enumerate(("parked_a", "parked_a", "parked_b")):
        out.append(run_case(name, what=f"{k}: {name}"))
    assert out[0][0] == out[1][0] and out[0][1].tobytes() == out[1][1].tobytes() and out[0][2].tobytes() == out[1][2].tobytes()


# ---------------------------------------------------------------- 8. a failed solve
def test_a_failed_solve_leaves_p_weights_and_held_untouched(gpu, monkeypatch):
    """the fallback example of tests/test_dense_batch_bounds_cpu.py as a table: H = [[1, .95], [.95, 1]], g = (-.14, -.25), upper =
    (inf, 0.1), trustregion0 = 10.  The first step is the Gauss-Newton step (-1, 1.2); clipped it is (-1, 0.1), whose expected
    improvement is -1.05: the fallback.  Its value is the third the backend hands out (the step's, the clipped step's, the
    fallback's); the test hook DOGLEG_AMD_DEBUG_EI_FLIP=3 negates it, which step 6 answers by failing the solve."""
    monkeypatch.setenv("DOGLEG_AMD_NO_BACKEND_CACHE", "1")
    A, y = from_normal_equations([[1.0, 0.95], [0.95, 1.0]], [-0.14, -0.25])
    M, N = A.shape
    p0 = np.zeros(N)
    x = A @ p0 - y
    lo, hi = np.full(N, -np.inf), np.array([np.inf, 0.1])
    prm = dc.params(trustregion0=10.0, max_iterations=1)
    loss = BatchLoss(LOSS_TRIVIAL, 0.0, 1)
    t = TableDeviceModel(x, A)
    r, p, tr, w, held = capi.optimize_device_bounded(p0, N, M, 0, None, None, t.cb, t.cookie, lo, hi, loss, prm)
    st = capi.bounded_last_stats()
    first = tr.trials()[0]
    print(f"un-hooked: F {r:.6g}, first trial {first['step_type']} (0: Cauchy), expected improvement {first['expected_improvement']:.6g}, "
          f"stats {st}")
    assert r >= 0 and st["clipped"] >= 1 and st["fallbacks"] >= 1 and first["step_type"] == 0 and first["expected_improvement"] > 0
    assert np.all(w == 1.0) and np.all(held != 255)
    monkeypatch.setenv("DOGLEG_AMD_DEBUG_EI_FLIP", "3")
    r, p, tr, w, held = capi.optimize_device_bounded(p0, N, M, 0, None, None, t.cb, t.cookie, lo, hi, loss, prm)
    monkeypatch.delenv("DOGLEG_AMD_DEBUG_EI_FLIP")
    print(f"hooked: returned {r}")
    assert r == -1.0 and p.tobytes() == p0.tobytes() and np.all(w == -1.0) and np.all(held == 255)
    t.close()
