"""dogleg_amd_optimize_dense_products_batch_bounded and its device twin.

The reference is the NumPy oracle of tests/batch_bounds_oracle.py (solve_one, the trivial loss) on the host model of the same
problems, tests/batch_oracle.py::HostProblem(M[b], N, seed, ...): it is per problem, so a ragged batch needs nothing new.
Tolerances, the project's, as in tests/test_dense_batch_bounds_gpu.py: |p - p_oracle|_inf <= STEP_TOL = 1e-10, norm2_x and the
trust region to REL_SCALAR_TOL = 1e-8 relative; lambda, iterations, evaluations, status and held equal.  The figures are printed
before they are asserted (compare of that module, imported).

The batches, their bounds, their stopping thresholds and the margins recorded for them: tests/batch_products_bounds_cases.py;
tests/test_dense_products_batch_bounds_cpu.py holds the margins against the oracle without a GPU.  Every margin is asserted
again here, before anything is compared."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BATCH_FAILED, BATCH_JTX, BATCH_NOT_RUN, BATCH_TRUSTREGION, BATCH_UNC_OK, LOSS_TRIVIAL
from problems.batch import LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED_NAN_LOWER
from problems.batch_linear_products import LinearProductsBatch, exact_bounded_solution
from tests import batch_bounds_oracle as bb
from tests import batch_fit_oracle as fo
from tests import batch_oracle as bo
from tests import batch_products_bounds_cases as pc
from tests import batch_products_oracle as po
from tests import batch_query_oracle as qo
from tests import batch_robust_oracle as ro
from tests import test_dense_batch_bounds_gpu as tbd
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_fit_gpu as tf
from tests import test_dense_batch_gpu as tb
from tests import test_dense_products_batch_gpu as tp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MARGIN_FLOOR = pc.MARGIN_FLOOR
GUARD, HELD_GUARD = td.GUARD, tbd.HELD_GUARD
KKT_TOL = 1e-9
PARITY_KEY = (6, (20, 90), 65)


def run(db, prm, lo, hi, p0=None):
    """the host-pointer call in the layout the batch is set to: (p, results, held); one batched callback per round, live problems
    only"""
    db.reset_counters()
    rc, p, res, held = capi.optimize_dense_products_batch_bounded(db.p0() if p0 is None else p0, db.N, db.cb, db.cookie, lo, hi,
                                                                  db.set_params(prm))
    assert rc == 0
    assert db.ncalls() == int(res["evaluations"].max()) == capi.batch_last_stats()["rounds"]
    assert db.nevals() == int(res["evaluations"].sum())
    return p, res, held


def ragged_batch(N, ragged, B, every=False):
    """(the oracle's solves, lo, hi, M, seeds) of a batch of tests/batch_products_bounds_cases.py"""
    orc, lo, hi, Ms = pc.oracle_batch(N, ragged, B, every)
    return orc, lo, hi, Ms, tuple(range(1, 1 + B))


def parity_batch():
    N, ragged, B = PARITY_KEY
    return (N,) + ragged_batch(N, ragged, B) + (pc.PARITY[PARITY_KEY][1],)


# ---------------------------------------------------------------- 1. bounds that clamp nothing: the plain solve, bit for bit
@pytest.mark.parametrize("layout", [LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED_NAN_LOWER])
@pytest.mark.parametrize("shape", [(6, (20, 90)), (64, 128)], ids=str)
def test_bounds_that_clamp_nothing_are_the_plain_solve_bit_for_bit(shape, layout):
    N, M = shape
    nb = 9
    db = tp.device_batch(N, td.products_Ms(M, nb), range(1, 1 + nb), "diverse", layout=layout)
    prm = po.params("diverse")
    pp, rp = tp.run(db, prm)
    assert np.all(rp["status"] > 0) and np.all(rp["status"] != BATCH_FAILED)
    inf = np.full((nb, N), np.inf)
    for what, lo, hi in (("NULL", None, None), ("infinite", -inf, inf), ("a box 1e300 wide", np.full((nb, N), -5e299),
                                                                      np.full((nb, N), 5e299)), ("lower only", -inf, None)):
        p, res, held = run(db, prm, lo, hi)
        assert p.tobytes() == pp.tobytes() and tb.bitwise_equal(res, rp), what
        assert not held.any(), what
    db.close()


# ---------------------------------------------------------------- 2. parity over the ragged batch
def test_parity_over_the_ragged_batch():
    N, orc, lo, hi, Ms, seeds, recorded = parity_batch()
    types = set().union(*[o["step_types"] for o in orc])
    nclipped, nfallbacks = sum(o["clipped"] for o in orc), sum(o["fallbacks"] for o in orc)
    print(f"M {sorted(set(Ms.tolist()))[:3]} .. {int(Ms.max())}: {pc.held_problems(orc)} of {len(orc)} problems end with a held "
          f"variable, step types {sorted(types)}, {nclipped} clipped steps, {nfallbacks} fallbacks, evaluations "
          f"{sorted({o['evaluations'] for o in orc})}")
    assert types == {0, 1, 2} and nclipped > 0 and len({o["evaluations"] for o in orc}) > 1
    pc.assert_margin(orc, recorded, "ragged, bounded")
    db = tp.device_batch(N, Ms, seeds, "diverse")
    p, res, held = run(db, pc.params(), lo, hi)
    tbd.compare(p, res, held, None, orc, "ragged, bounded")
    assert np.all(p >= lo) and np.all(p <= hi)
    db.close()


# ---------------------------------------------------------------- 3. rejected trials with held variables
@pytest.mark.parametrize("threshold", [None, 100.0], ids=str)
def test_rejected_trials(threshold):
    """the batch of tests/test_dense_batch_bounds_gpu.py::test_rejected_trials (its comment: bounds at the start point, so the
    bounded variables are held from the first step on), with its oracle solves and its recorded margins, here through the
    products callback with one M for all"""
    N, M = 6, 40
    over = tbd.REJECT_OVER + (() if threshold is None else (("trustregion_threshold", threshold),))
    orc, lo, hi = tbd.oracle_batch(N, M, tbd.REJECT_SEEDS, "hard", over=over, frac=1.0)
    tbd.assert_margin(orc, tbd.REJECT_MARGIN[threshold], f"hard, bounded, threshold {threshold}")
    assert sum(o["rejected"] for o in orc) >= 2
    if threshold is None:
        assert sum(o["held_resteps"] for o in orc) >= 1
    else:
        stopped = [o for o in orc if o["status"] == BATCH_TRUSTREGION]
        assert len(stopped) >= 1 and all(o["rejected"] == 1 for o in stopped) and any(o["held"].any() for o in stopped)
    db = tp.device_batch(N, M, tbd.REJECT_SEEDS, "hard")
    p, res, held = run(db, tb.params("hard", **dict(over)), lo, hi)
    tbd.compare(p, res, held, None, orc, f"hard, bounded, products, threshold {threshold}")
    db.close()


# ---------------------------------------------------------------- 4. the branches, one per problem of a linear batch
def test_branches_on_the_linear_problem():
    A, y, p0, lo, hi, tr0 = tbd.branch_batch()
    nb, N = p0.shape
    prm = tb.params("default")
    prm.trustregion0 = tr0
    db = LinearProductsBatch(list(A), list(y), p0)
    orc = [bb.solve_one(db.host(b), prm, ro.Loss(LOSS_TRIVIAL), lo[b], hi[b]) for b in range(nb)]
    margin = min(o["margin"] for o in orc)
    print(f"the oracle: fallbacks {[o['fallbacks'] for o in orc]}, clipped {[o['clipped'] for o in orc]}, statuses "
          f"{[o['status'] for o in orc]}, smallest margin {margin:.3g}")
    assert orc[0]["fallbacks"] == 1 and margin > MARGIN_FLOOR
    p, res, held = run(db, prm, lo, hi)
    first = db.first_p()
    tbd.compare(p, res, held, None, orc, "branches, products")
    good = [0, 1, 2, 3, 6, 7]
    for b in good:
        assert float(np.max(np.abs(p[b] - exact_bounded_solution(A[b], y[b], lo[b], hi[b])))) <= KKT_TOL, b
        assert np.all(first[b] >= lo[b]) and np.all(first[b] <= hi[b]), b
    assert p[1][1] == 0.25
    # everything held at the start
    assert (res["status"][2], res["evaluations"][2], res["iterations"][2]) == (BATCH_JTX, 1, 0)
    assert p[2].tobytes() == p0[2].tobytes() and held[2].tolist() == [2, 2]
    # the infeasible start was clamped before the first evaluation
    assert first[3].tolist() == [0.5, -0.5]
    # bad bounds: FAILED alone, nothing evaluated, nothing written but the record
    for b in (4, 5):
        assert (res["status"][b], res["evaluations"][b], res["iterations"][b], res["norm2_x"][b]) == (BATCH_FAILED, 0, 0, -1.0)
        assert p[b].tobytes() == p0[b].tobytes() and not held[b].any()
    db.close()
    # the two ordinary problems alone: the same bits
    for b in (6, 7):
        d1 = LinearProductsBatch([A[b]], [y[b]], p0[b:b + 1])
        p1, r1, h1 = run(d1, prm, lo[b:b + 1], hi[b:b + 1])
        assert p1.tobytes() == p[b:b + 1].tobytes() and tb.bitwise_equal(r1, res[b:b + 1]) and h1.tobytes() == held[b:b + 1].tobytes()
        d1.close()


def test_ragged_linear_batch_in_every_layout():
    """the linear model with its own number of rows per problem: the exact bounded solution, and the same bits in the three
    layouts of JtJ (the NaN of the third lies where the library must not read)"""
    from problems.batch import LAYOUT_UNPACKED
    from problems.batch_linear_products import random_ragged
    N, nb = 3, 7
    A, y, p0, lo, hi = random_ragged(N, nb, seed=1)
    assert len({a.shape[0] for a in A}) > 1
    prm = tb.params("default")
    got = []
    for layout in (LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED, LAYOUT_UNPACKED_NAN_LOWER):
        db = LinearProductsBatch(A, y, p0, layout=layout)
        got.append(run(db, prm, lo, hi))
        first = db.first_p()
        db.close()
        assert np.all(first >= lo) and np.all(first <= hi)
    p, res, held = got[0]
    for p2, r2, h2 in got[1:]:
        assert p2.tobytes() == p.tobytes() and tb.bitwise_equal(r2, res) and h2.tobytes() == held.tobytes()
    err = max(float(np.max(np.abs(p[b] - exact_bounded_solution(A[b], y[b], lo[b], hi[b])))) for b in range(nb))
    print(f"ragged linear batch: rows {[a.shape[0] for a in A]}, worst |p - exact| {err:.3g}, held {held.tolist()}")
    assert err <= KKT_TOL and held.any() and np.all(res["status"] != BATCH_FAILED)


# ---------------------------------------------------------------- 5. every size class
@pytest.mark.parametrize("case", sorted(pc.CLASSES), ids=str)
def test_every_size_class(case):
    N, ragged = case
    every, recorded, nheld = pc.CLASSES[case]
    orc, lo, hi, Ms, seeds = ragged_batch(N, ragged, pc.CLASS_B, every)
    pc.assert_margin(orc, recorded, str(case))
    assert pc.held_problems(orc) == nheld
    if every:
        assert any(o["held"][N - 1] for o in orc), "no problem holds the last variable: the top bit of the mask is not exercised"
    db = tp.device_batch(N, Ms, seeds, "diverse")
    p, res, held = run(db, pc.params(), lo, hi)
    tbd.compare(p, res, held, None, orc, str(case))
    assert np.all(p >= lo) and np.all(p <= hi)
    db.close()


# ---------------------------------------------------------------- 6. both forms agree
def test_both_forms_agree():
    N, M, nb = 6, 40, 33
    seeds = tuple(range(1, 1 + nb))
    orc, lo, hi = tbd.oracle_batch(N, M, seeds, "diverse")
    prm = tbd.params("diverse")
    dj = tb.device_batch(N, M, seeds, "diverse")
    pj, rj, hj, _ = tbd.run(dj, prm, lo, hi)
    dj.close()
    dp = tp.device_batch(N, M, seeds, "diverse")
    pp, rp, hp = run(dp, tbd.params("diverse"), lo, hi)
    dp.close()
    print(f"J form against products form: max |p_J - p_products| {float(np.max(np.abs(pj - pp))):.3g}")
    for k in ("iterations", "evaluations", "status", "lambda_"):
        assert rj[k].tolist() == rp[k].tolist(), k
    assert hj.tobytes() == hp.tobytes() and hj.any()


# ---------------------------------------------------------------- 7. the device twin
def solve_dev(db, prm, lo, hi, mask=None, stream=None, want_held=True):
    """the device-resident bounded solve under prefilled sentinels: (p, results, lambda, held, counts); lo, hi: arrays or None"""
    nb, N = db.B, db.N
    P = td.Buf(db.p0())
    R = td.Buf(np.full(nb * td.RSIZE, td.PAD, dtype=np.uint8))
    Lm = td.Buf(np.full(nb, GUARD))
    Lo = None if lo is None else td.Buf(np.ascontiguousarray(lo, dtype=np.float64))
    Hi = None if hi is None else td.Buf(np.ascontiguousarray(hi, dtype=np.float64))
    H = td.Buf(np.full((nb, N), HELD_GUARD, dtype=np.uint8)) if want_held else None
    A = td.mask_dev(mask)
    db.reset_counters()
    rc = capi.optimize_dense_products_batch_bounded_device(P.ptr, nb, N, db.cb, db.cookie, db.set_params(prm),
                                                           Lo.ptr if Lo else None, Hi.ptr if Hi else None, H.ptr if H else None,
                                                           R.ptr, Lm.ptr, A.ptr if A else None, stream)
    assert rc == 0
    counts = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    if A is not None:
        assert np.array_equal(A.get(), np.asarray(mask, dtype=np.uint8))
    # (Buf.get checks the guard behind each array: the bounds are read only, held is written within its span)
    if Lo is not None:
        assert Lo.get().tobytes() == np.ascontiguousarray(lo, dtype=np.float64).tobytes()
    if Hi is not None:
        assert Hi.get().tobytes() == np.ascontiguousarray(hi, dtype=np.float64).tobytes()
    return P.get(), td.results_of(R, nb), Lm.get(), H.get() if H else None, counts


def test_device_twin_equals_host_twin():
    N, orc, lo, hi, Ms, seeds, _ = parity_batch()
    db = tp.device_batch(N, Ms, seeds, "diverse")
    prm = pc.params()
    ph, rh, hh = run(db, prm, lo, hi)
    ch = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    pd, rd, ld, hd, cd = solve_dev(db, prm, lo, hi)
    assert pd.tobytes() == ph.tobytes() and tb.bitwise_equal(rd, rh) and hd.tobytes() == hh.tobytes() and cd == ch
    assert ld.tobytes() == np.ascontiguousarray(rh["lambda_"]).tobytes() and hh.any()
    # no held asked for, one side of the box only: the same solves
    pn, rn, _, hn, _ = solve_dev(db, prm, lo, hi, want_held=False)
    assert pn.tobytes() == ph.tobytes() and tb.bitwise_equal(rn, rh) and hn is None
    p1, r1, h1 = run(db, prm, lo, None)
    pd1, rd1, _, hd1, _ = solve_dev(db, prm, lo, None)
    assert pd1.tobytes() == p1.tobytes() and tb.bitwise_equal(rd1, r1) and hd1.tobytes() == h1.tobytes()
    db.close()


@pytest.mark.parametrize("case", [(6, (20, 90), td.B, False), (64, (128, 160), 9, True)], ids=str)
def test_mask(case):
    """a problem that is not run: the NOT_RUN record (lambda_dev 0 there, as the plain twin's contract has it), its p and its held
    row not written, the guards behind every array intact (Buf.get); an active problem's bits do not depend on the mask"""
    N, ragged, nb, every = case
    orc, lo, hi, Ms, seeds = ragged_batch(N, ragged, nb, every)
    db = tp.device_batch(N, Ms, seeds, "diverse")
    prm = pc.params()
    p0 = db.p0()
    pf, rf, lf, hf, _ = solve_dev(db, prm, lo, hi)
    m = td.the_mask(N, nb)
    on, off = np.flatnonzero(m), np.flatnonzero(m == 0)
    # a problem that is not run is not checked either: bad bounds in one of them
    lo2 = lo.copy()
    lo2[off[0], 0] = np.nan
    pm, rm, lm, hm, cm = solve_dev(db, prm, lo2, hi, mask=m)
    assert pm[on].tobytes() == pf[on].tobytes() and tb.bitwise_equal(rm[on], rf[on]) and lm[on].tobytes() == lf[on].tobytes()
    assert hm[on].tobytes() == hf[on].tobytes() and hf.any()
    assert pm[off].tobytes() == p0[off].tobytes() and np.all(hm[off] == HELD_GUARD)
    assert np.all(rm["norm2_x"][off] == -1.0) and np.all(rm["status"][off] == BATCH_NOT_RUN)
    for k in ("trustregion", "lambda_", "iterations", "evaluations"):
        assert not rm[k][off].any(), k
    assert not lm[off].any()
    assert cm["nevals"] == int(rm["evaluations"].sum()) and cm["ncalls"] == int(rm["evaluations"].max()) == cm["rounds"]
    db.close()


STREAM_CHILD = r'''
import sys
import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded
sys.path.insert(0, sys.argv[1])
from tests import batch_products_bounds_cases as pc
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_bounds_gpu as tbb
from tests import test_dense_products_batch_bounds_gpu as tpb
from tests import test_dense_products_batch_gpu as tp
from tests import test_dense_batch_gpu as tb
from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchResult

N, ragged, B = 6, (20, 90), 33
orc, lo, hi, Ms, seeds = tpb.ragged_batch(N, ragged, B)
db = tp.device_batch(N, Ms, seeds, "diverse")
prm = db.set_params(pc.params())
p0 = db.p0()
pn, rn, ln, hn, cn = tpb.solve_dev(db, prm, lo, hi)             # hip_stream NULL
s = torch.cuda.Stream()
host = torch.from_numpy(p0.copy()).pin_memory()
hlo, hhi = torch.from_numpy(lo.copy()).pin_memory(), torch.from_numpy(hi.copy()).pin_memory()
dev = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
dlo = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
dhi = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
held = torch.full((B * N + 64,), tbb.HELD_GUARD, dtype=torch.uint8, device="cuda")
res = torch.full((B * td.RSIZE + 512,), td.PAD, dtype=torch.uint8, device="cuda")
lam = torch.full((B + 64,), td.GUARD, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(s):
    # asynchronous, on s; no synchronisation before the call
    dev[:B * N].copy_(host.reshape(-1), non_blocking=True)
    dlo[:B * N].copy_(hlo.reshape(-1), non_blocking=True)
    dhi[:B * N].copy_(hhi.reshape(-1), non_blocking=True)
rc = capi.optimize_dense_products_batch_bounded_device(dev.data_ptr(), B, N, db.cb, db.cookie, prm, dlo.data_ptr(), dhi.data_ptr(),
                                                       held.data_ptr(), res.data_ptr(), lam.data_ptr(), None, s.cuda_stream)
assert rc == 0
torch.cuda.synchronize()
ps, ls, hs, raw = dev.cpu().numpy(), lam.cpu().numpy(), held.cpu().numpy(), res.cpu().numpy()
assert np.all(ps[B * N:] == td.GUARD) and np.all(ls[B:] == td.GUARD) and np.all(raw[B * td.RSIZE:] == td.PAD)
assert np.all(hs[B * N:] == tbb.HELD_GUARD) and np.all(dlo.cpu().numpy()[B * N:] == td.GUARD)
rs = capi._batch_results((BatchResult * B).from_buffer_copy(raw[:B * td.RSIZE].tobytes()), B)
assert ps[:B * N].tobytes() == pn.tobytes() and ls[:B].tobytes() == ln.tobytes() and tb.bitwise_equal(rs, rn)
assert hs[:B * N].tobytes() == hn.tobytes() and hn.any()
assert np.all(rs["status"] > 0)
db.close()
print("STREAM OK")
'''


def test_stream(tmp_path):
    """in a process of its own, as tests/test_dense_batch_device_gpu.py::test_stream: torch is loaded before the library there"""
    src = tmp_path / "stream_child.py"
    src.write_text(STREAM_CHILD)
    r = subprocess.run([sys.executable, str(src), ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "STREAM OK" in r.stdout, r.stdout + r.stderr


def test_refusals_on_the_gpu():
    N, nb = 6, 4
    db = tp.device_batch(N, po.ragged_M(nb, 20, 90), range(1, 1 + nb), "default")
    db.reset_counters()
    P = td.Buf(db.p0())
    R = td.Buf(np.full(nb * td.RSIZE, td.PAD, dtype=np.uint8))
    Lm = td.Buf(np.full(nb, GUARD))
    Lo, Hi = td.Buf(np.full((nb, N), -50.0)), td.Buf(np.full((nb, N), 50.0))
    H = td.Buf(np.full((nb, N), HELD_GUARD, dtype=np.uint8))
    short = capi.DeviceArray(nbytes=nb * N - 1)
    short8 = capi.DeviceArray(nbytes=8 * nb * N - 8)
    pageable = np.full((nb, N), -50.0)
    prm = db.set_params(po.params("default"))

    def dev(lo=Lo.ptr, hi=Hi.ptr, h=H.ptr, p=P.ptr, r=R.ptr):
        return capi.optimize_dense_products_batch_bounded_device(p, nb, N, db.cb, db.cookie, prm, lo, hi, h, r, Lm.ptr)

    assert capi.batch_device_span_ok(H.ptr, nb * N) and not capi.batch_device_span_ok(short.ptr, nb * N)
    assert not capi.batch_device_span_ok(short8.ptr, 8 * nb * N)
    assert not capi.batch_device_span_ok(pageable.ctypes.data, 8 * nb * N)
    assert dev(lo=pageable.ctypes.data) == -1                   # a pageable-host lower
    assert dev(hi=pageable.ctypes.data) == -1
    assert dev(lo=short8.ptr) == -1 and dev(hi=short8.ptr) == -1        # a bounds array one double short
    assert dev(h=short.ptr) == -1                               # a held one byte short
    assert dev(h=np.zeros((nb, N), dtype=np.uint8).ctypes.data) == -1   # a held in pageable host memory
    assert dev(p=None) == -1 and dev(r=None) == -1
    L = capi.lib()
    assert L.dogleg_amd_optimize_dense_products_batch_bounded_device(P.ptr, nb, N, db.cb, db.cookie, None, None, R.ptr, Lm.ptr,
                                                                     None, None) == -1      # a NULL bounds
    assert db.ncalls() == 0
    assert np.all(R.get() == td.PAD) and np.all(Lm.get() == GUARD) and np.all(H.get() == HELD_GUARD)
    assert P.get().tobytes() == db.p0().tobytes()
    # and the valid call behind them
    assert dev() == 0 and np.all(td.results_of(R, nb)["status"] > 0) and not H.get().any()
    short.free()
    short8.free()
    db.close()


# ---------------------------------------------------------------- 8. independence
def test_order_size_and_neighbours_do_not_matter():
    """the same problem in three batches -- the batch, the batch reversed with its neighbours' bounds gone, and alone -- gives
    the same bits"""
    N, orc, lo, hi, Ms, seeds, _ = parity_batch()
    nb = len(seeds)
    prm = pc.params()
    db = tp.device_batch(N, Ms, seeds, "diverse")
    p, res, held = run(db, prm, lo, hi)
    db.close()
    db = tp.device_batch(N, Ms[::-1], tuple(reversed(seeds)), "diverse")
    pr, rr, hr = run(db, prm, lo[::-1], hi[::-1])
    db.close()
    assert pr[::-1].tobytes() == p.tobytes() and tb.bitwise_equal(rr[::-1], res) and hr[::-1].tobytes() == held.tobytes()
    for b in (0, 31, nb - 1):
        # the neighbours' bounds changed (none at all), one problem's kept
        lo2, hi2 = np.full_like(lo, -np.inf), np.full_like(hi, np.inf)
        lo2[b], hi2[b] = lo[b], hi[b]
        db = tp.device_batch(N, Ms, seeds, "diverse")
        p2, r2, h2 = run(db, prm, lo2, hi2)
        db.close()
        assert p2[b].tobytes() == p[b].tobytes() and tb.bitwise_equal(r2[b:b + 1], res[b:b + 1]) and h2[b].tobytes() == held[b].tobytes()
        # alone
        db = tp.device_batch(N, Ms[b:b + 1], seeds[b:b + 1], "diverse")
        p1, r1, h1 = run(db, prm, lo[b:b + 1], hi[b:b + 1])
        db.close()
        assert p1[0].tobytes() == p[b].tobytes() and tb.bitwise_equal(r1, res[b:b + 1]) and h1[0].tobytes() == held[b].tobytes()


# ---------------------------------------------------------------- 9. round accounting
def test_round_accounting():
    """run() asserts, for every batch above, one callback per round and live problems only; here also against the oracle's
    counts and with problems that never start"""
    N, orc, lo, hi, Ms, seeds, _ = parity_batch()
    db = tp.device_batch(N, Ms, seeds, "diverse")
    lo2 = lo.copy()
    lo2[[0, 17]] = np.nan
    p, res, held = run(db, pc.params(), lo2, hi)
    want = [0 if b in (0, 17) else o["evaluations"] for b, o in enumerate(orc)]
    assert res["evaluations"].tolist() == want and db.ncalls() == max(want) and db.nevals() == sum(want)
    assert capi.batch_last_stats()["rounds"] == max(want)
    assert res["status"][0] == res["status"][17] == BATCH_FAILED and not held[[0, 17]].any()
    db.close()


# ---------------------------------------------------------------- 10. end to end with the fit calls
def test_end_to_end_with_the_fit_calls():
    """p, results.lambda and held of the ragged parity batch's first 9 problems, handed unchanged to the products fit calls;
    the reference and the tolerances of tests/test_dense_batch_fit_gpu.py"""
    N, orc, lo, hi, Ms, seeds, _ = parity_batch()
    nb = 9
    db = tp.device_batch(N, Ms[:nb], seeds[:nb], "diverse")
    prm = db.set_params(pc.params())
    p, res, held = run(db, prm, lo[:nb], hi[:nb])
    lam = np.ascontiguousarray(res["lambda_"])
    assert np.all(res["status"] > 0) and np.all(res["status"] != BATCH_FAILED) and held.any(axis=1).all()
    f = capi.batch_fit(held=held)
    Jq = np.ascontiguousarray(fo.queries(nb, N)[:, :2, :2, :])              # Nq = 2 queries of 2 rows
    out = capi.dense_products_batch_uncertainty(p, N, db.cb, db.cookie, prm, lam=lam, fit=f)
    q = capi.dense_products_batch_query_covariance(p, N, db.cb, db.cookie, Jq, prm, lam=lam, fit=f)
    assert out["rc"] == 0 and q["rc"] == 0 and np.all(out["status"] == BATCH_UNC_OK) and np.all(q["status"] == BATCH_UNC_OK)
    eps, noise, spread, _ = tb.SETS["diverse"]
    ecov = evar = eq = 0.0
    for b in range(nb):
        hp = bo.HostProblem(int(Ms[b]), N, seeds[b], eps, noise, spread)
        x, J = hp.eval(np.ascontiguousarray(p[b]))
        hp.dp.close()
        r = fo.reference(x, J, lam[b], held[b], Jq=Jq[b])
        ecov = max(ecov, fo.cov_error(out["cov"][b], r["S"], held[b]))           # inf unless held rows and columns are +0.0
        free = held[b] == 0
        assert np.all(out["var"][b][~free] == 0.0) and not np.any(np.signbit(out["var"][b][~free]))
        assert out["var"][b].tobytes() == np.diag(out["cov"][b]).copy().tobytes()
        evar = max(evar, float(np.max(np.abs(out["var"][b] - r["var"])[free] / r["var"][free])))
        eq = max(eq, qo.scaled_error(q["out"][b], r["blocks"]))
    print(f"behind the bounded products solve: held {held.tolist()}, Sigma scaled error {ecov:.3g} (held rows and columns exactly "
          f"+0), variances rel {evar:.3g}, query blocks scaled error {eq:.3g}")
    assert ecov <= tf.COV_TOL and evar <= tf.VAR_TOL and eq <= tf.QUERY_TOL
    db.close()
