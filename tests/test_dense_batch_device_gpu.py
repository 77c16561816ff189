"""The device-resident batch entry points (dogleg_amd_optimize_dense_batch_device, ..._products_batch_device,
dogleg_amd_dense_batch_uncertainty_device, ..._products_batch_uncertainty_device) and their active mask.

The reference of every comparison is the host-pointer entry point on the same inputs: the kernels and their order of
operations are the same and a problem's bits do not depend on its position, so the tolerance is zero and bytes are
compared.  The host entry points are themselves held to the CPU oracle by the files the helpers here come from.

B = 65 unless said: a last workgroup with one problem in the size classes up to <32> (four problems a workgroup), a
half-empty 33rd workgroup in <48> (two), 65 workgroups in <64>.  Every device array a call writes lies in an allocation with
64 doubles of guard behind the payload (class Buf), checked when the array is read back."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (BATCH_FAILED, BATCH_NOT_RUN, BATCH_UNC_OK, BATCH_UNC_SKIPPED, BATCH_MAX_NSTATE,
                                       BatchResult)
from problems.batch import MODE_NAN, LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED
from tests import batch_products_oracle as po
from tests import dense_batch_shapes as ds
from tests import dense_batch_wide_shapes as ws
from tests import oracle_api as oa
from tests import test_dense_batch_gpu as tb
from tests import test_dense_batch_uncertainty_gpu as tu
from tests import test_dense_products_batch_gpu as tp
from tests import test_dense_products_batch_uncertainty_gpu as tpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B = 65
SHAPES = [(1, 5), (6, 40), (16, 50), (24, 73), (32, 70), (33, 70), (48, 100), (64, 128)]
# (N, M or (Mmin, Mmax))
PRODUCTS_SHAPES = [(6, (20, 90)), (33, 70), (64, 128)]
LAYOUTS = [LAYOUT_PACKED_UPPER, LAYOUT_UNPACKED]
MASK_SHAPES = [(6, 40), (48, 100), (64, 128)]
GUARD = -7.5
GUARD_BYTES = np.full(64, GUARD).view(np.uint8)
PAD = 0xA5                      # what the result structs are prefilled with: their 4 bytes of padding keep it
RSIZE = C.sizeof(BatchResult)


class Buf:
    """a device array with 64 guard doubles behind it"""

    def __init__(self, payload):
        payload = np.ascontiguousarray(payload)
        self.dtype, self.shape = payload.dtype, payload.shape
        raw = payload.reshape(-1).view(np.uint8)
        self.n = raw.size
        self.d = capi.DeviceArray(np.concatenate([raw, GUARD_BYTES]))
        self.ptr = self.d.ptr

    def get(self):
        raw = self.d.numpy()
        assert raw[self.n:].tobytes() == GUARD_BYTES.tobytes(), "written behind the end of the array"
        return raw[:self.n].copy().view(self.dtype).reshape(self.shape)


def mask_dev(mask):
    return None if mask is None else Buf(np.asarray(mask, dtype=np.uint8))


def results_of(R, nb):
    raw = R.get().reshape(nb, RSIZE)
    assert np.all(raw[:, 36:] == PAD), "the padding of dogleg_amd_batch_result_t was written"
    return capi._batch_results((BatchResult * nb).from_buffer_copy(raw.tobytes()), nb)


def solve_dev(db, prm, products=False, p0=None, mask=None, stream=None):
    """the device-resident solve of the batch: (p, results, lambda, dict(rounds, ncalls, nevals))"""
    nb, N = db.B, db.N
    P = Buf(db.p0() if p0 is None else p0)
    R = Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8))
    Lm = Buf(np.full(nb, GUARD))
    A = mask_dev(mask)
    db.reset_counters()
    if products:
        rc = capi.optimize_dense_products_batch_device(P.ptr, nb, N, db.cb, db.cookie, db.set_params(prm), R.ptr, Lm.ptr,
                                                       A.ptr if A else None, stream)
    else:
        rc = capi.optimize_dense_batch_device(P.ptr, nb, N, db.M, db.cb, db.cookie, prm, R.ptr, Lm.ptr, A.ptr if A else None,
                                              stream)
    assert rc == 0
    counts = dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())
    if A is not None:
        assert np.array_equal(A.get(), np.asarray(mask, dtype=np.uint8))
    return P.get(), results_of(R, nb), Lm.get(), counts


def solve_host(db, prm, products=False):
    p, res = (tp.run if products else tb.run)(db, prm)
    return p, res, dict(rounds=capi.batch_last_stats()["rounds"], ncalls=db.ncalls(), nevals=db.nevals())


def same_solve(db, prm, what, products=False):
    ph, rh, ch = solve_host(db, prm, products)
    pd, rd, ld, cd = solve_dev(db, prm, products)
    print(f"{what}: rounds {ch['rounds']}, evaluations {ch['nevals']}, statuses {sorted(set(rh['status'].tolist()))}")
    assert pd.tobytes() == ph.tobytes(), what
    assert tb.bitwise_equal(rd, rh), what
    assert ld.tobytes() == np.ascontiguousarray(rh["lambda_"]).tobytes(), what
    assert cd == ch, (cd, ch)
    return ph, rh


# ---------------------------------------------------------------- 1. the solve, J form
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_solve(shape):
    N, M = shape
    db = tb.device_batch(N, M, range(1, 1 + B), "diverse")
    same_solve(db, tb.params("diverse"), f"{shape} diverse")
    db.close()


HARD = [(s, ds.RETRY[s][0], ds.RETRY[s][1]) for s in sorted(ds.RETRY)] + [(s, ws.SEED0, ws.B) for s in sorted(ws.RETRY)]


@pytest.mark.parametrize("shape,seed0,nb", HARD, ids=str)
def test_solve_with_rejected_trials(shape, seed0, nb):
    """the "hard" batches of the two shape tables: rejected trials, so the reload of JtJ"""
    N, M = shape
    db = tb.device_batch(N, M, range(seed0, seed0 + nb), "hard")
    p, res = same_solve(db, tb.params("hard"), f"{shape} hard")
    # (a rejected trial: an evaluation that is neither the first nor an accepted step's)
    assert np.any(res["evaluations"] > res["iterations"] + 1)
    db.close()


# ---------------------------------------------------------------- 2. the solve, products form
def products_Ms(M, nb=B):
    return po.ragged_M(nb, *M) if isinstance(M, tuple) else np.full(nb, M)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", PRODUCTS_SHAPES, ids=str)
def test_solve_products(shape, layout):
    N, M = shape
    db = tp.device_batch(N, products_Ms(M), range(1, 1 + B), "diverse", layout=layout)
    same_solve(db, po.params("diverse"), f"products {shape} layout {layout}", products=True)
    db.close()


# ---------------------------------------------------------------- 3. a failing problem fails alone
def test_a_failing_problem_fails_alone():
    N, M = 6, 40
    bad = [0, 31, B - 1]
    db = tb.device_batch(N, M, range(1, 1 + B), "diverse")
    mode = np.zeros(B, dtype=np.uint8)
    mode[bad] = MODE_NAN
    db.set_mode(mode)
    p0 = db.p0()
    ph, rh = same_solve(db, tb.params("diverse"), "three problems of NaN")
    pd, rd, ld, _ = solve_dev(db, tb.params("diverse"))
    assert pd[bad].tobytes() == p0[bad].tobytes()
    assert np.all(rd["norm2_x"][bad] == -1.0) and np.all(rd["status"][bad] == BATCH_FAILED)
    good = np.setdiff1d(np.arange(B), bad)
    assert np.all(rd["status"][good] != BATCH_FAILED) and np.all(rd["norm2_x"][good] >= 0)
    db.close()


# ---------------------------------------------------------------- 4. the mask
def the_mask(N, nb=B):
    """about half zeros, seeded; one whole workgroup of zeros, b = 0 and b = B - 1 inactive, b = 1 active (so that in the
    classes of several problems a workgroup the first workgroup is a mixed one)"""
    wpb = ws.problems_per_workgroup(N)
    m = (np.random.default_rng(5).random(nb) < 0.5).astype(np.uint8)
    m[3 * wpb:4 * wpb] = 0
    m[0] = m[nb - 1] = 0
    m[1] = 1
    assert 0.3 * nb < m.sum() < 0.7 * nb
    return m


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_mask(shape):
    N, M = shape
    db = tb.device_batch(N, M, range(1, 1 + B), "diverse")
    prm = tb.params("diverse")
    p0 = db.p0()
    pf, rf, lf, _ = solve_dev(db, prm)
    m = the_mask(N)
    on, off = np.flatnonzero(m), np.flatnonzero(m == 0)
    pm, rm, lm, cm = solve_dev(db, prm, mask=m)
    assert pm[on].tobytes() == pf[on].tobytes() and tb.bitwise_equal(rm[on], rf[on]) and lm[on].tobytes() == lf[on].tobytes()
    assert pm[off].tobytes() == p0[off].tobytes()
    assert np.all(rm["norm2_x"][off] == -1.0) and np.all(rm["status"][off] == BATCH_NOT_RUN)
    for k in ("trustregion", "lambda_", "iterations", "evaluations"):
        assert not rm[k][off].any(), k
    assert not lm[off].any()
    assert cm["nevals"] == int(rm["evaluations"].sum()) and cm["ncalls"] == int(rm["evaluations"].max()) == cm["rounds"]
    # nothing active: 0, at most one invocation of the callback, p as it was
    pz, rz, lz, cz = solve_dev(db, prm, mask=np.zeros(B, dtype=np.uint8))
    assert pz.tobytes() == p0.tobytes() and cz["ncalls"] <= 1 and cz["nevals"] == 0
    assert np.all(rz["status"] == BATCH_NOT_RUN) and np.all(rz["norm2_x"] == -1.0) and not lz.any()
    db.close()


# ---------------------------------------------------------------- 5. - 7. the uncertainty call
def unc_dev(db, p, lam, want=("cov", "var", "factors"), fs=1, scale=None, mask=None, products=False, prm=None, p_dev=None,
            lam_dev=None, stream=None):
    """the device-resident twin of capi.dense_batch_uncertainty / dense_products_batch_uncertainty: the same dict, every
    output prefilled with the guard value.  p_dev, lam_dev: addresses to use in place of uploads of p and lam."""
    nb, N = db.B, db.N
    P = None if p_dev is not None else Buf(p)
    Lm = None if lam_dev is not None or lam is None else Buf(np.array(lam, dtype=np.float64))
    S = Buf(np.full(nb, 42, dtype=np.int32))
    O = {}
    if "cov" in want:
        O["cov"] = Buf(np.full((nb, N, N), GUARD))
    if "var" in want:
        O["var"] = Buf(np.full((nb, N), GUARD))
    if "factors" in want:
        O["factors"] = Buf(np.full((nb, db.M // max(fs, 1)), GUARD))
        O["scale"] = Buf(np.full(nb, -1.0) if scale is None else np.array(np.broadcast_to(scale, (nb,)), dtype=np.float64))
    A = mask_dev(mask)
    ptr = lambda k: O[k].ptr if k in O else None
    p_ptr = p_dev if p_dev is not None else P.ptr
    lam_ptr = lam_dev if lam_dev is not None else (Lm.ptr if Lm else None)
    db.reset_counters()
    if products:
        rc = capi.dense_products_batch_uncertainty_device(p_ptr, nb, N, db.cb, db.cookie, db.set_params(prm), S.ptr, lam_ptr,
                                                          ptr("cov"), ptr("var"), A.ptr if A else None, stream)
    else:
        rc = capi.dense_batch_uncertainty_device(p_ptr, nb, N, db.M, db.cb, db.cookie, S.ptr, lam_ptr, ptr("cov"), ptr("var"),
                                                 ptr("factors"), ptr("scale"), fs, A.ptr if A else None, stream)
    out = dict(rc=rc, status=S.get(), lam=Lm.get() if Lm else None, ncalls=db.ncalls())
    out.update({k: b.get() for k, b in O.items()})
    if P is not None:
        assert P.get().tobytes() == np.ascontiguousarray(p).tobytes()
    out["stats"] = capi.batch_uncertainty_last_stats()
    return out


def same_outputs(dev, host, what, idx=None):
    """every array the host call returned, bytewise"""
    assert dev["rc"] == 0 and dev["ncalls"] == 1, what
    for k, v in host.items():
        if k == "rc" or v is None:
            continue
        a, b = (dev[k], v) if idx is None else (dev[k][idx], v[idx])
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what}: {k}"
    s = dev["stats"]
    assert s["launches"] == 1 and s["syncs"] == 1 and s["copies"] <= 2, s


@pytest.mark.parametrize("fs", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_uncertainty(shape, fs):
    N, M = shape
    assert M > N + 1
    db, p, lam = tu.solved(N, M, np.arange(1, 1 + B))
    # everything, the scale to be computed (<= 0, written back)
    host = tu.unc(db, p, lam, fs=fs)
    dev = unc_dev(db, p, lam, fs=fs)
    assert np.all(dev["status"] == BATCH_UNC_OK) and np.all(dev["scale"] > 0)
    same_outputs(dev, host, f"{shape} fs {fs} all")
    # the scale given
    same_outputs(unc_dev(db, p, lam, fs=fs, scale=2.5), tu.unc(db, p, lam, fs=fs, scale=2.5), "scale given")
    # one output alone, and no lambda
    same_outputs(unc_dev(db, p, lam, fs=fs, want=("var",)), tu.unc(db, p, lam, fs=fs, want=("var",)), "variances alone")
    same_outputs(unc_dev(db, p, lam, fs=fs, want=("factors",)), tu.unc(db, p, lam, fs=fs, want=("factors",)), "factors alone")
    nolam = unc_dev(db, p, None, fs=fs)
    assert nolam["lam"] is None
    same_outputs(nolam, tu.unc(db, p, None, fs=fs), "lambda NULL")
    db.close()


def test_uncertainty_stats_do_not_depend_on_the_batch_size():
    N, M = 6, 40
    stats = {}
    for nb in (1, B):
        db, p, lam = tu.solved(N, M, np.arange(1, 1 + nb))
        for name, kw in (("all", dict(lam=lam)), ("no lambda", dict(lam=None))):
            out = unc_dev(db, p, fs=2, **kw)
            assert out["rc"] == 0 and out["ncalls"] == 1
            s = out["stats"]
            stats[(nb, name)] = (s["launches"], s["syncs"], s["copies"])
        db.close()
    print(stats)
    for name in ("all", "no lambda"):
        assert stats[(1, name)] == stats[(B, name)] and stats[(1, name)][:2] == (1, 1) and stats[(1, name)][2] <= 2


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", PRODUCTS_SHAPES, ids=str)
def test_uncertainty_products(shape, layout):
    N, M = shape
    db, p, lam = tpu.solved(N, products_Ms(M), np.arange(1, 1 + B), layout)
    prm = po.params(tpu.SET)
    same_outputs(unc_dev(db, p, lam, want=("cov", "var"), products=True, prm=prm), tpu.unc(db, p, lam), f"products {shape} all")
    same_outputs(unc_dev(db, p, lam, want=("var",), products=True, prm=prm), tpu.unc(db, p, lam, want=("var",)), "variances alone")
    same_outputs(unc_dev(db, p, None, want=("cov",), products=True, prm=prm), tpu.unc(db, p, None, want=("cov",)), "lambda NULL")
    db.close()


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_uncertainty_with_the_mask(shape):
    N, M = shape
    db, p, lam = tu.solved(N, M, np.arange(1, 1 + B))
    full = unc_dev(db, p, lam, fs=2)
    m = the_mask(N)
    on, off = np.flatnonzero(m), np.flatnonzero(m == 0)
    lam_in = lam.copy()
    lam_in[off] = -5.0          # (a negative lambda would FAIL a problem that ran, and NaN its outputs)
    out = unc_dev(db, p, lam_in, fs=2, mask=m)
    assert out["rc"] == 0 and out["ncalls"] == 1
    assert np.all(out["status"][off] == BATCH_UNC_SKIPPED) and np.all(out["status"][on] == BATCH_UNC_OK)
    for k in ("cov", "var", "factors"):
        assert np.all(out[k][off] == GUARD), k
        assert out[k][on].tobytes() == full[k][on].tobytes(), k
    assert np.all(out["scale"][off] == -1.0) and np.all(out["lam"][off] == -5.0)
    assert out["scale"][on].tobytes() == full["scale"][on].tobytes() and out["lam"][on].tobytes() == full["lam"][on].tobytes()
    # products form, and nothing active
    dbp, pp, lamp = tpu.solved(N, np.full(B, M), np.arange(1, 1 + B))
    prm = po.params(tpu.SET)
    fullp = unc_dev(dbp, pp, lamp, want=("cov", "var"), products=True, prm=prm)
    outp = unc_dev(dbp, pp, lamp, want=("cov", "var"), products=True, prm=prm, mask=m)
    assert outp["rc"] == 0 and np.all(outp["status"][off] == BATCH_UNC_SKIPPED)
    for k in ("cov", "var"):
        assert np.all(outp[k][off] == GUARD) and outp[k][on].tobytes() == fullp[k][on].tobytes(), k
    none = unc_dev(db, p, lam, fs=2, mask=np.zeros(B, dtype=np.uint8))
    assert none["rc"] == 0 and none["ncalls"] <= 1 and np.all(none["status"] == BATCH_UNC_SKIPPED)
    assert all(np.all(none[k] == GUARD) for k in ("cov", "var", "factors")) and np.all(none["scale"] == -1.0)
    db.close()
    dbp.close()


# ---------------------------------------------------------------- 8. solve, then uncertainty, nothing downloaded in between
@pytest.mark.parametrize("shape", [(6, 40), (48, 100)], ids=str)
def test_chain_without_the_host(shape):
    N, M = shape
    seeds = np.arange(1, 1 + B)
    dbh, p, lam = tu.solved(N, M, seeds)
    host = tu.unc(dbh, p, lam, fs=2)
    dbh.close()
    db = tu.device_batch(N, M, seeds)
    P = Buf(db.p0())
    R = Buf(np.full(B * RSIZE, PAD, dtype=np.uint8))
    Lm = Buf(np.full(B, GUARD))
    assert capi.optimize_dense_batch_device(P.ptr, B, N, M, db.cb, db.cookie, oa.default_params(), R.ptr, Lm.ptr) == 0
    dev = unc_dev(db, None, None, fs=2, p_dev=P.ptr, lam_dev=Lm.ptr)
    dev["lam"] = Lm.get()
    same_outputs(dev, host, f"chain {shape}")
    assert P.get().tobytes() == p.tobytes()
    db.close()


# ---------------------------------------------------------------- 9. the caller's stream
STREAM_CHILD = r'''
import sys
import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded
sys.path.insert(0, sys.argv[1])
from tests import test_dense_batch_device_gpu as td
from tests import test_dense_batch_gpu as tb
from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import BatchResult

N, M, B = 6, 40, td.B
db = tb.device_batch(N, M, range(1, 1 + B), "diverse")
prm = tb.params("diverse")
p0 = db.p0()
pn, rn, ln, cn = td.solve_dev(db, prm)          # hip_stream NULL
s = torch.cuda.Stream()
host = torch.from_numpy(p0.copy()).pin_memory()
dev = torch.full((B * N + 64,), td.GUARD, dtype=torch.float64, device="cuda")
res = torch.full((B * td.RSIZE + 512,), td.PAD, dtype=torch.uint8, device="cuda")
lam = torch.full((B + 64,), td.GUARD, dtype=torch.float64, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(s):
    dev[:B * N].copy_(host.reshape(-1), non_blocking=True)      # asynchronous, on s; no synchronisation before the call
rc = capi.optimize_dense_batch_device(dev.data_ptr(), B, N, M, db.cb, db.cookie, prm, res.data_ptr(), lam.data_ptr(), None,
                                      s.cuda_stream)
assert rc == 0
torch.cuda.synchronize()
ps, ls, raw = dev.cpu().numpy(), lam.cpu().numpy(), res.cpu().numpy()
assert np.all(ps[B * N:] == td.GUARD) and np.all(ls[B:] == td.GUARD) and np.all(raw[B * td.RSIZE:] == td.PAD)
rs = capi._batch_results((BatchResult * B).from_buffer_copy(raw[:B * td.RSIZE].tobytes()), B)
assert ps[:B * N].tobytes() == pn.tobytes() and ls[:B].tobytes() == ln.tobytes() and tb.bitwise_equal(rs, rn)
assert np.all(rs["status"] > 0)
db.close()
print("STREAM OK")
'''


def test_stream(tmp_path):
    """in a process of its own: torch is loaded before the library there, as bench.py does it, so that both use one HIP
    runtime and the stream torch made is a stream of the library's runtime"""
    src = tmp_path / "stream_child.py"
    src.write_text(STREAM_CHILD)
    r = subprocess.run([sys.executable, str(src), ROOT], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "STREAM OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- 10. refusals: -1, no invocation, nothing written
def test_refusals():
    N, M = 6, 40
    nb = 4
    db = tu.device_batch(N, M, np.arange(1, 1 + nb))
    db.reset_counters()
    P = Buf(db.p0())
    R = Buf(np.full(nb * RSIZE, PAD, dtype=np.uint8))
    Lm = Buf(np.full(nb, GUARD))
    S = Buf(np.full(nb, 42, dtype=np.int32))
    cov, var = Buf(np.full((nb, N, N), GUARD)), Buf(np.full((nb, N), GUARD))
    fac, scale = Buf(np.full((nb, M), GUARD)), Buf(np.full(nb, 1.0))
    big = Buf(np.zeros((1, BATCH_MAX_NSTATE + 1)))
    prm = tb.params("default")
    L = capi.lib()

    def solve(p=P.ptr, b=nb, n=N, m=M, f=db.cb, r=R.ptr):
        return capi.optimize_dense_batch_device(p, b, n, m, f, db.cookie, prm, r, Lm.ptr)

    def solve_p(p=P.ptr, b=nb, n=N, f=db.cb, r=R.ptr, packed=True, upper=True):
        q = po.params("default")
        q.JtJ_packed, q.JtJ_upper = packed, upper
        return capi.optimize_dense_products_batch_device(p, b, n, f, db.cookie, q, r, Lm.ptr)

    def unc(p=P.ptr, b=nb, n=N, m=M, f=db.cb, s=S.ptr, c=cov.ptr, v=var.ptr, fa=fac.ptr, sc=scale.ptr, fs=1):
        return capi.dense_batch_uncertainty_device(p, b, n, m, f, db.cookie, s, Lm.ptr, c, v, fa, sc, fs)

    def unc_p(p=P.ptr, b=nb, n=N, f=db.cb, s=S.ptr, c=cov.ptr, v=var.ptr, packed=True, upper=True):
        q = po.params("default")
        q.JtJ_packed, q.JtJ_upper = packed, upper
        return capi.dense_products_batch_uncertainty_device(p, b, n, f, db.cookie, q, s, Lm.ptr, c, v)

    # (the callback of a J-form batch is never invoked here, so the products entry points may be handed it)
    assert solve(p=None) == -1 and solve(r=None) == -1 and solve(f=None) == -1
    assert solve_p(p=None) == -1 and solve_p(r=None) == -1 and solve_p(f=None) == -1
    assert unc(p=None) == -1 and unc(s=None) == -1 and unc(f=None) == -1
    assert unc_p(p=None) == -1 and unc_p(s=None) == -1 and unc_p(f=None) == -1
    assert solve(b=0) == -1 and solve_p(b=0) == -1 and unc(b=0) == -1 and unc_p(b=0) == -1
    n65 = BATCH_MAX_NSTATE + 1
    assert solve(p=big.ptr, b=1, n=n65) == -1 and solve_p(p=big.ptr, b=1, n=n65) == -1
    assert unc(p=big.ptr, b=1, n=n65, m=200) == -1 and unc_p(p=big.ptr, b=1, n=n65) == -1
    assert unc(fs=3) == -1
    assert unc(sc=None) == -1                                   # factors without scale
    assert unc(m=N + 1) == -1 and unc(m=N) == -1                # factors with Nmeas <= Nstate + 1
    assert unc(c=None, v=None, fa=None, sc=None) == -1 and unc_p(c=None, v=None) == -1
    assert solve_p(packed=True, upper=False) == -1 and unc_p(packed=True, upper=False) == -1
    fn = capi.ALLREDUCE_FN(lambda buf, n, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert solve() == -1 and solve_p() == -1 and unc() == -1 and unc_p() == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert db.ncalls() == 0
    assert np.all(R.get() == PAD) and np.all(Lm.get() == GUARD) and np.all(S.get() == 42)
    assert all(np.all(b.get() == GUARD) for b in (cov, var, fac)) and np.all(scale.get() == 1.0)
    assert P.get().tobytes() == db.p0().tobytes()
    db.close()


def test_the_pointer_checks_through_the_hook():
    """host pointers and short buffers go to dlg_batch_device_span_ok only, never to an entry point"""
    host = np.zeros(128)
    assert not capi.batch_device_span_ok(host.ctypes.data, host.nbytes)
    assert not capi.batch_device_span_ok(None, 8)
    need = 8 * 65 * 6
    d = capi.DeviceArray(nbytes=need)
    assert capi.batch_device_span_ok(d, need)
    assert not capi.batch_device_span_ok(d, need + 1)
    assert capi.batch_device_span_ok(d.ptr + 8 * 6, need - 8 * 6)           # an interior pointer whose span still fits
    assert not capi.batch_device_span_ok(d.ptr + 8 * 6, need - 8 * 6 + 1)
    d.free()
