#!/usr/bin/env python3
"""tools/batch_numeric_bench.py -- the numeric-Jacobian adapter of the dense batch (dogleg_amd_batch_numeric_*) on the values-only
device test problem (problems/batch_values.py, the default generator settings).  Nothing is gated.

(a) The adapter's two kernels.  One invocation at the start points, every problem live: the time of k_numeric_perturb and
    k_numeric_jacobian together (events on the stream, DOGLEG_AMD_BATCH_TIMING=1) against a device-to-device copy that moves the
    bytes the Jacobian kernel MUST move: K B Nmeas doubles read, B Nmeas (Nstate + 1) written.  The two legs alternate in one
    process; the adapter is measured in two interleaved series, and the relative difference of their medians is the A/A spread.
(b) Whole solves with the default parameters: the values model through the adapter against the analytic DeviceBatch callback on
    the same problems, the legs alternated, the analytic leg twice for the A/A spread: wall time, rounds, ms per round on the
    stream split into the callback (for the adapter: the model's kernel and the adapter's two) and the library's round kernel
    (events, in a call of its own), and the largest distance of the end points.

    python tools/batch_numeric_bench.py [--out profiles/batch_numeric.md] [--reps 15] [--max-b 131072]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                              # noqa: E402
from libdogleg_amd.ctypes_defs import NUMERIC_FORWARD, NUMERIC_CENTRAL      # noqa: E402
from problems.batch import DeviceBatch                                      # noqa: E402
from problems.batch_values import DeviceValuesBatch, DeviceCopy             # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1024, 16384, 131072]
SCHEMES = [(NUMERIC_FORWARD, "forward"), (NUMERIC_CENTRAL, "central")]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5


NOTES = [
    "(a) The share is the copy's time over the kernels': 100 % would be the copy's rate.  The kernels' time also holds "
    "k_numeric_perturb, whose K B Nstate doubles written (and B Nstate read) are not among the bytes counted -- 7 to 11 % more "
    "bytes on these shapes --, so the Jacobian kernel alone is somewhat closer to the copy than the share says.",
    "Where the share is low (40 x 6 at every B, and every shape at B = 1024) the cause has been reasoned, not measured with "
    "counters.  At B = 1024 both legs are a few microseconds of work behind two launches: the figure is launch overhead.  At "
    "large B the Jacobian kernel waits on memory latency with too few bytes in flight: a block has ONE tile in flight at a time "
    "-- at 40 x 6 that is 32 x 7 doubles read, each thread at most one load pair, then a barrier, 1.5 KB stored, a barrier -- so "
    "8 resident blocks keep about 14 KB of loads in flight per CU, several times less than the latency-bandwidth product of "
    "HBM per CU; and 40 rows are a tile of 32 and a tile of 8, whose segments are 64 bytes, half a cache line, with a quarter of "
    "the lanes busy.  96 x 16 has 2.4 times the bytes per tile and only full tiles, and comes to 61 - 96 % of the copy at "
    "B >= 16384.  What would be tried next, in a pull request of its own and against these numbers: two tiles (or all tiles of "
    "a problem) in flight per block before the first barrier, and tiles that follow Nmeas (40 = 2 x 20) instead of a fixed 32.",
    "(b) The numeric solve's rounds and end points are the analytic solve's (the distance is the accuracy of the difference "
    "quotient carried through the stopping test).  Its time is the model's: a round evaluates the model at K points instead of "
    "one, and this test model is expensive per value (it draws every coefficient from a hash instead of loading it), so its K "
    "evaluations take 4 to 42 times the adapter's own two kernels.  The adapter's kernels cost 0.5 to 1.0 of the library's "
    "round kernel.  Against the analytic callback, which gets J for the price of about one evaluation, the whole solve is 1.25 to "
    "10 times slower: the price of not writing the Jacobian kernel, paid in evaluations of the model, not in the adapter.",
]


def med(v):
    return float(np.median(v))


def kernels(N, M, B, scheme, reps):
    vb = DeviceValuesBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    ad = capi.BatchNumeric(B, N, M, vb.cb, vb.cookie, scheme=scheme)
    K = ad.K
    moved = 8.0 * B * M * (K + N + 1)
    cp = DeviceCopy(moved)
    dp, dlive = capi.DeviceArray(vb.p0()), capi.DeviceArray(np.ones(B, dtype=np.uint8))
    dx, dJ = capi.DeviceArray(nbytes=8 * B * M), capi.DeviceArray(nbytes=8 * B * M * N)
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"

    def adapter_leg():
        a = ad.stats()
        ad.invoke(dp, dx, dJ, dlive)
        b = ad.stats()
        return b["ms_library"] - a["ms_library"], b["ms_f"] - a["ms_f"]

    for _ in range(3):
        adapter_leg()
        cp.run()
    a1, a2, c, f = [], [], [], []
    for _ in range(reps):
        t, tf = adapter_leg()
        a1.append(t)
        f.append(tf)
        c.append(cp.run())
        a2.append(adapter_leg()[0])
    os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    for a in (dp, dlive, dx, dJ):
        a.free()
    for o in (cp, ad, vb):
        o.close()
    both = a1 + a2
    return dict(K=K, moved=moved, lib=med(both), lib_rng=(min(both), max(both)), aa=abs(med(a1) - med(a2)) / med(both),
                copy=med(c), copy_rng=(min(c), max(c)), f=med(f))


def solve(cb, cookie, p0, N, M, timing=False):
    if timing:
        os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    t = time.perf_counter()
    rc, p, res = capi.optimize_dense_batch(p0, N, M, cb, cookie)
    dt = time.perf_counter() - t
    os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert rc == 0 and np.all(res["status"] > 0) and not np.any(res["norm2_x"] < 0)
    return dt, p, capi.batch_last_stats()


def solves(N, M, B, scheme, reps):
    vb = DeviceValuesBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    ad = capi.BatchNumeric(B, N, M, vb.cb, vb.cookie, scheme=scheme)
    p0 = vb.p0()
    assert np.array_equal(p0, db.p0())
    for _ in range(2):
        solve(ad.cb, ad.cookie, p0, N, M)
        solve(db.cb, db.cookie, p0, N, M)
    tn, ta1, ta2 = [], [], []
    for _ in range(reps):
        ta1.append(solve(db.cb, db.cookie, p0, N, M)[0])
        tn.append(solve(ad.cb, ad.cookie, p0, N, M)[0])
        ta2.append(solve(db.cb, db.cookie, p0, N, M)[0])
    _, pa, sa = solve(db.cb, db.cookie, p0, N, M, timing=True)
    before = ad.stats()
    _, pn, sn = solve(ad.cb, ad.cookie, p0, N, M, timing=True)
    after = ad.stats()
    inv = after["invocations"] - before["invocations"]
    out = dict(num=med(tn), num_rng=(min(tn), max(tn)), ana=med(ta1 + ta2), ana_rng=(min(ta1 + ta2), max(ta1 + ta2)),
               aa=abs(med(ta1) - med(ta2)) / med(ta1 + ta2), rounds_n=sn["rounds"], rounds_a=sa["rounds"],
               cb_n=sn["ms_callback"] / sn["rounds"], lib_n=sn["ms_library"] / sn["rounds"],
               cb_a=sa["ms_callback"] / sa["rounds"], lib_a=sa["ms_library"] / sa["rounds"],
               f_n=(after["ms_f"] - before["ms_f"]) / inv, own_n=(after["ms_library"] - before["ms_library"]) / inv,
               dist=float(np.max(np.abs(pn - pa))))
    for o in (ad, db, vb):
        o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    out = ["# Numeric Jacobians for values-only batch callbacks: dogleg_amd_batch_numeric_*", "",
           f"Values-only device test problem (problems/batch_values.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1); default "
           "deltas.  Written by tools/batch_numeric_bench.py; nothing here is gated.", "",
           "## (a) The adapter's two kernels against a copy of the bytes they must move", "",
           "One invocation at the start points, every problem live.  kernels: k_numeric_perturb + k_numeric_jacobian (events on the "
           f"stream), median (min .. max) of 2 x {a.reps} invocations in two interleaved series; A/A: the relative difference of the two "
           "series' medians.  copy: a device-to-device copy that moves 8 B Nmeas (K + Nstate + 1) bytes -- the K B Nmeas doubles "
           f"k_numeric_jacobian reads and the B Nmeas (Nstate + 1) it writes --, alternated with the invocations, median of {a.reps}.  "
           "share: copy / kernels.  model: the values kernel's time in the same invocations, for scale.", "",
           "| N | M | B | scheme | K | MB moved | kernels us | A/A | copy us | share | model us |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            for scheme, name in SCHEMES:
                r = kernels(N, M, B, scheme, a.reps)
                line = (f"| {N} | {M} | {B} | {name} | {r['K']} | {r['moved'] / 1e6:.1f} | {r['lib'] * 1e3:.1f} ({r['lib_rng'][0] * 1e3:.1f} .. "
                        f"{r['lib_rng'][1] * 1e3:.1f}) | {100 * r['aa']:.1f} % | {r['copy'] * 1e3:.1f} ({r['copy_rng'][0] * 1e3:.1f} .. "
                        f"{r['copy_rng'][1] * 1e3:.1f}) | {100 * r['copy'] / r['lib']:.0f} % | {r['f'] * 1e3:.1f} |")
                print(line, flush=True)
                out.append(line)
    out += ["", "## (b) Whole solves: the values model through the adapter against the analytic callback", "",
            "dogleg_amd_optimize_dense_batch with the default parameters on the same problems from the same start points.  wall: "
            f"median (min .. max) of {a.reps} solves (the analytic leg: 2 x {a.reps}, A/A: the relative difference of its two series' "
            "medians), the legs alternated.  Per round, from a call of its own with events on the stream: callback (numeric: the "
            "adapter's two kernels + the model's, given apart as own + model) and library (the round kernel).  distance: the largest "
            "|p_numeric - p_analytic| over all problems and variables.", "",
            "| N | M | B | scheme | numeric ms | analytic ms | A/A | numeric / analytic | rounds n / a | numeric callback us (own + model) "
            "| numeric library us | analytic callback us | analytic library us | distance |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            for scheme, name in SCHEMES:
                r = solves(N, M, B, scheme, a.reps)
                line = (f"| {N} | {M} | {B} | {name} | {r['num'] * 1e3:.2f} ({r['num_rng'][0] * 1e3:.2f} .. {r['num_rng'][1] * 1e3:.2f}) | "
                        f"{r['ana'] * 1e3:.2f} ({r['ana_rng'][0] * 1e3:.2f} .. {r['ana_rng'][1] * 1e3:.2f}) | {100 * r['aa']:.1f} % | "
                        f"{r['num'] / r['ana']:.2f} x | {r['rounds_n']:.0f} / {r['rounds_a']:.0f} | {r['cb_n'] * 1e3:.1f} "
                        f"({r['own_n'] * 1e3:.1f} + {r['f_n'] * 1e3:.1f}) | {r['lib_n'] * 1e3:.1f} | {r['cb_a'] * 1e3:.1f} | "
                        f"{r['lib_a'] * 1e3:.1f} | {r['dist']:.1e} |")
                print(line, flush=True)
                out.append(line)
    out += ["", "## Reading the tables", ""] + NOTES
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
