#!/usr/bin/env python3
"""tools/batch_bench.py -- dogleg_amd_optimize_dense_batch on batches of the dense device test problem.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96) and B = 1 ... 131072 problems, and for (48, 160) and (64, 200) -- the
size classes above 32 variables -- at B = 1, 1024 and 16384 (problems/batch.py, the default generator settings): wall time of the call (median and range of the repeats after warm-up calls), rounds, the time of a
round split into the callback's kernels and the library's (events on the stream, DOGLEG_AMD_BATCH_TIMING=1, in a call
of its own), problems per second, and for the library's part the bytes it must move -- 8 Nmeas Nstate per evaluated
problem, read once -- over its time, beside the 6.29 TB/s copy ceiling of the MI355X.

The comparison: the same B = 1024 problems solved by a loop over dogleg_optimize_device2 (dense, one problem per call, no
trace, the library's cache warm: what the library offered for this job before), the two legs alternated; and, not gated,
the CPU oracle on the same problems on one host core (a single-thread baseline, as bench.py labels its cpu_baseline).

    python tools/batch_bench.py [--out profiles/batch.md] [--reps 7] [--max-b 131072]
    python tools/batch_bench.py --one 16384        # one warm call and one measured one, for a profiler
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                      # noqa: E402
from problems import DenseProblem, DeviceTwin       # noqa: E402
from problems.batch import DeviceBatch              # noqa: E402

BATCHES = [1, 64, 1024, 16384, 131072]
WIDE_BATCHES = [1, 1024, 16384]
SHAPES = [((6, 40), BATCHES), ((16, 96), BATCHES), ((48, 160), WIDE_BATCHES), ((64, 200), WIDE_BATCHES)]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
HBM_COPY_TBS = 6.29


def batch_call(db, p0, timing=False):
    if timing:
        os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    t = time.perf_counter()
    rc, p, res = capi.optimize_dense_batch(p0, db.N, db.M, db.cb, db.cookie)
    dt = time.perf_counter() - t
    os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert rc == 0 and np.all(res["status"] > 0)
    return dt, res, capi.batch_last_stats()


def measure(N, M, B, reps, warm=2):
    db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    p0 = db.p0()
    for _ in range(warm):
        batch_call(db, p0)
    ts = []
    for _ in range(reps):
        dt, res, st = batch_call(db, p0)
        ts.append(dt)
    _, res, st = batch_call(db, p0, timing=True)
    db.close()
    nev = int(res["evaluations"].sum())
    return dict(N=N, M=M, B=B, t=np.median(ts), tmin=min(ts), tmax=max(ts), rounds=st["rounds"], nev=nev,
                ms_cb=st["ms_callback"], ms_lib=st["ms_library"], bytes=8.0 * M * N * nev)


def loop_leg(probs, twins):
    t = time.perf_counter()
    for prob, twin in zip(probs, twins):
        r, p, _ = capi.optimize_device(prob.p0(), prob.N, prob.M, 0, None, None, twin.cb, twin.cookie, None, trace=False)
        assert r >= 0
    return time.perf_counter() - t


def comparison(N, M, B, reps):
    db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    p0 = db.p0()
    probs = [DenseProblem(M, N, seed=1 + b, eps=EPS, noise=NOISE, p0_spread=SPREAD) for b in range(B)]
    twins = [DeviceTwin(pr) for pr in probs]
    batch_call(db, p0)
    loop_leg(probs[:32], twins[:32])
    tb, tl = [], []
    for _ in range(reps):
        tb.append(batch_call(db, p0)[0])
        tl.append(loop_leg(probs, twins))
    from tests import oracle_api as oa
    t = time.perf_counter()
    for pr in probs:
        oa.oracle_solve("dense", pr.p0(), N, M, 0, pr.cb, pr.cookie, None, capacity=64)
    t_orc = time.perf_counter() - t
    for tw in twins:
        tw.close()
    db.close()
    return dict(N=N, M=M, B=B, batch=np.median(tb), batch_rng=(min(tb), max(tb)), loop=np.median(tl), loop_rng=(min(tl), max(tl)),
                oracle=t_orc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--one", type=int, default=0)
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    if a.one:
        db = DeviceBatch(a.one, 96, 16, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
        p0 = db.p0()
        batch_call(db, p0)
        dt, res, st = batch_call(db, p0)
        print(f"B = {a.one} (16, 96): {dt * 1e3:.2f} ms, {st['rounds']} rounds")
        db.close()
        return
    out = ["# Batches of small dense problems: dogleg_amd_optimize_dense_batch", "",
           f"Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1), default parameters; "
           f"wall time: median (min .. max) of {a.reps} calls after 2 warm-up calls; callback / library: events on the stream, "
           "per round, in a call of their own; GB/s: 8 Nmeas Nstate bytes per evaluated problem over the library's time "
           f"(copy ceiling of the MI355X: {HBM_COPY_TBS} TB/s).", "",
           "| N | M | B | wall ms | rounds | callback us/round | library us/round | problems/s | library GB/s | of ceiling |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for (N, M), batches in SHAPES:
        for B in batches:
            if B > a.max_b:
                continue
            r = measure(N, M, B, a.reps if B < 100000 else max(3, a.reps // 2))
            gbs = r["bytes"] / (r["ms_lib"] * 1e-3) / 1e9 if r["ms_lib"] > 0 else float("nan")
            line = (f"| {N} | {M} | {B} | {r['t'] * 1e3:.3f} ({r['tmin'] * 1e3:.3f} .. {r['tmax'] * 1e3:.3f}) | {r['rounds']} | "
                    f"{r['ms_cb'] * 1e3 / r['rounds']:.1f} | {r['ms_lib'] * 1e3 / r['rounds']:.1f} | {B / r['t']:.3g} | {gbs:.1f} | "
                    f"{100 * gbs / (HBM_COPY_TBS * 1e3):.2f} % |")
            print(line, flush=True)
            out.append(line)
    out += ["", "## The same 1024 problems: one batch call against a loop of single-problem solves", "",
            "Loop: dogleg_optimize_device2 (dense path, device callback, no trace), one problem per call, cache warm; the two legs "
            "alternated; oracle: the CPU restatement of the reference on one host core (single-thread baseline, not gated).", "",
            "| N | M | B | batch ms | loop ms | loop / batch | oracle, 1 core, ms |", "|---|---|---|---|---|---|---|"]
    for (N, M), _ in SHAPES:
        c = comparison(N, M, 1024, 3)
        line = (f"| {N} | {M} | {c['B']} | {c['batch'] * 1e3:.2f} ({c['batch_rng'][0] * 1e3:.2f} .. {c['batch_rng'][1] * 1e3:.2f}) | "
                f"{c['loop'] * 1e3:.0f} ({c['loop_rng'][0] * 1e3:.0f} .. {c['loop_rng'][1] * 1e3:.0f}) | {c['loop'] / c['batch']:.0f} x | "
                f"{c['oracle'] * 1e3:.0f} |")
        print(line, flush=True)
        out.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
