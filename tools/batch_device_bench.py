#!/usr/bin/env python3
"""tools/batch_device_bench.py -- the device-resident batch entry points against the host-pointer ones.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96) and B = 1024, 16384 and 131072 problems of the dense device test
problem (problems/batch.py, the default generator settings): the solve, and the uncertainty call with all three outputs at
feature size 2 at the points the solve returned.  The quantity is the wall time of the call, a host clock around it (every
call ends in a synchronisation).  Both legs get their arrays allocated and touched beforehand: the host leg numpy arrays, the
device leg device arrays that hold the same inputs; what is timed is the library call alone.

Protocol: the two entry points on the same problems in one process, alternated -- host, device, host again per repeat, after
warm-up calls of both.  The two host legs are an A/A pair: their medians differ by nothing but the spread of the
measurement, which is the yardstick for the device leg ("slower" in the table: the device median above the first host median
by more than that spread).  The outputs of the timed calls are compared bytewise, every repeat.  The time on the stream
(the callback's kernels, the library's; events, DOGLEG_AMD_BATCH_TIMING=1) comes from calls of their own after the timed
ones.  Nothing is gated.

    python tools/batch_device_bench.py [--out profiles/batch_device.md] [--reps 7] [--max-b 131072]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                  # noqa: E402
from libdogleg_amd.ctypes_defs import BatchResult, dptr, iptr   # noqa: E402
from problems.batch import DeviceBatch                          # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
FS = 2


def clock(fn):
    t = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t
    assert rc == 0
    return dt


def with_timing(fn, stats):
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    try:
        assert fn() == 0
    finally:
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    s = stats()
    return s["ms_callback"], s["ms_library"]


def upload(dev, arr):
    capi._ck(capi.lib().dlg_mem_upload(dev.ptr, arr.ctypes.data, arr.nbytes), "upload")


class Solve:
    """the two legs of the solve on one batch"""
    stats = staticmethod(capi.batch_last_stats)

    def __init__(self, db):
        self.db, self.L, self.prm = db, capi.lib(), capi.default_parameters()
        B, N = db.B, db.N
        self.p0 = db.p0()
        self.p = self.p0.copy()
        self.res = (BatchResult * B)()
        self.p_dev = capi.DeviceArray(self.p0)
        self.res_dev = capi.DeviceArray(nbytes=C.sizeof(BatchResult) * B, dtype=np.uint8)
        self.lam_dev = capi.DeviceArray(nbytes=8 * B)

    def reset(self):
        self.p[...] = self.p0
        upload(self.p_dev, self.p0)

    def host(self):
        db = self.db
        return self.L.dogleg_amd_optimize_dense_batch(dptr(self.p), db.B, db.N, db.M, db.cb, db.cookie, C.byref(self.prm), self.res)

    def device(self):
        db = self.db
        return capi.optimize_dense_batch_device(self.p_dev, db.B, db.N, db.M, db.cb, db.cookie, self.prm, self.res_dev, self.lam_dev)

    def same(self):
        B = self.db.B
        rh = capi._batch_results(self.res, B)
        rd = capi.batch_results_from_device(self.res_dev, B)
        return (self.p_dev.numpy().tobytes() == self.p.tobytes()
                and all(rh[f].tobytes() == rd[f].tobytes() for f in rh.dtype.names)
                and self.lam_dev.numpy().tobytes() == np.ascontiguousarray(rh["lambda_"]).tobytes())


class Uncertainty:
    """the two legs of the uncertainty call at the solved points of one batch"""
    stats = staticmethod(capi.batch_uncertainty_last_stats)

    def __init__(self, db, p, lam):
        self.db, self.L = db, capi.lib()
        B, N, M = db.B, db.N, db.M
        self.p, self.lam0 = np.ascontiguousarray(p), np.ascontiguousarray(lam)
        self.h = dict(lam=self.lam0.copy(), cov=np.zeros((B, N, N)), var=np.zeros((B, N)), fac=np.zeros((B, M // FS)),
                      scale=np.full(B, -1.0), status=np.zeros(B, dtype=np.int32))
        self.d = {k: capi.DeviceArray(v) for k, v in self.h.items()}
        self.p_dev = capi.DeviceArray(self.p)
        self.minus = np.full(B, -1.0)

    def reset(self):
        self.h["lam"][...] = self.lam0
        self.h["scale"][...] = -1.0
        upload(self.d["lam"], self.lam0)
        upload(self.d["scale"], self.minus)

    def host(self):
        db, h = self.db, self.h
        return self.L.dogleg_amd_dense_batch_uncertainty(dptr(self.p), db.B, db.N, db.M, db.cb, db.cookie, dptr(h["lam"]),
                                                         dptr(h["cov"]), dptr(h["var"]), dptr(h["fac"]), dptr(h["scale"]), FS,
                                                         iptr(h["status"]))

    def device(self):
        db, d = self.db, self.d
        return capi.dense_batch_uncertainty_device(self.p_dev, db.B, db.N, db.M, db.cb, db.cookie, d["status"], d["lam"], d["cov"],
                                                   d["var"], d["fac"], d["scale"], FS)

    def same(self):
        return all(self.d[k].numpy().tobytes() == self.h[k].tobytes() for k in self.h) and not self.h["status"].any()


def measure(leg, reps, warm=2):
    for _ in range(warm):
        leg.reset()
        leg.host()
        leg.reset()
        leg.device()
    h1, dv, h2 = [], [], []
    same = True
    for _ in range(reps):
        leg.reset()
        h1.append(clock(leg.host))
        dv.append(clock(leg.device))
        same = same and leg.same()
        leg.reset()
        h2.append(clock(leg.host))
    leg.reset()
    host_st = with_timing(leg.host, leg.stats)
    leg.reset()
    dev_st = with_timing(leg.device, leg.stats)
    return dict(h1=h1, dv=dv, h2=h2, same=same, host_st=host_st, dev_st=dev_st)


def ms(ts):
    return f"{np.median(ts) * 1e3:.3f} ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def row(N, M, B, r):
    a, b, d = np.median(r["h1"]), np.median(r["h2"]), np.median(r["dv"])
    spread = abs(b / a - 1.0)
    verdict = "slower" if d > a * (1.0 + spread) else "not slower"
    return (f"| {N} | {M} | {B} | {ms(r['h1'])} | {ms(r['h2'])} | {100 * spread:.1f} % | {ms(r['dv'])} | {a / d:.2f} x | {verdict} | "
            f"{'yes' if r['same'] else 'NO'} | {r['host_st'][0]:.3f} / {r['host_st'][1]:.3f} | {r['dev_st'][0]:.3f} / {r['dev_st'][1]:.3f} |")


HEAD = ["| N | M | B | host ms | host again ms | A/A spread | device ms | host / device | device leg | bytes equal | "
        "host leg: callback / library ms on the stream | device leg: callback / library ms |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    solve_rows, unc_rows = [], []
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            reps = a.reps if B < 100000 else max(3, a.reps // 2 + 1)
            db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            s = Solve(db)
            solve_rows.append(row(N, M, B, measure(s, reps)))
            print("solve", solve_rows[-1], flush=True)
            s.reset()
            assert s.host() == 0
            lam = np.ascontiguousarray(capi._batch_results(s.res, B)["lambda_"])
            u = Uncertainty(db, s.p, lam)
            del s
            unc_rows.append(row(N, M, B, measure(u, reps)))
            print("uncertainty", unc_rows[-1], flush=True)
            del u
            db.close()
    out = ["# Device-resident batches: dogleg_amd_*_batch_device against the host-pointer entry points", "",
           f"Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1), the default parameters. "
           "Wall time of the library call alone, a host clock around it: median (min .. max) of the repeats "
           f"({a.reps}; at B = 131072 fewer) after 2 warm-up calls of each leg; per repeat host, device, host again, in one process. "
           "Both legs' arrays exist and are touched before the clock starts (the host leg's numpy arrays, the device leg's device "
           "arrays).  A/A spread: |median(host again) / median(host) - 1|.  device leg: \"slower\" where its median is above the "
           "host median by more than the A/A spread of its row.  bytes equal: every output of the timed device call against the "
           "timed host call's, every repeat.  Stream times: events (DOGLEG_AMD_BATCH_TIMING=1) in calls of their own.", "",
           "## The solve", ""] + HEAD + solve_rows + ["", f"## The uncertainty call: covariance, variances and factors, feature size {FS}",
                                                       ""] + HEAD + unc_rows
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
