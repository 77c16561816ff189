#!/usr/bin/env python3
"""tools/bounded_device_bench.py -- what box bounds cost on dogleg_optimize_device2 (dogleg_amd_optimize_device2_bounded).

For each configuration (the shapes tools/robust_device_bench.py uses for configs #3 and #4), in one process:
  * the bounds of the "bounded" leg are those of the tests (tests/test_dense_batch_bounds_gpu.py: bounds_between): with p* the
    point the plain solve returns from p0, every third variable gets a bound half way between p*_i and p0_i on the side of p0,
    so the solve runs into them and ends with about a third of the variables on a bound;
  * the solves alternate, round after round, in the order plain, plain again (the A/A leg: the spread of the measurement),
    bounded with infinite bounds, bounded; the first --warmup rounds are not counted; a solve is timed by the host clock around
    the call, which returns synchronised; no trace is attached (as a user calls it);
  * evaluations and steps (trials) of a leg come from a traced solve each, which is not timed;
  * one more round with DOGLEG_AMD_TIMING=1 gives the time in the feature's own kernels and, of that, in the mask pass, from the
    library's own events (dogleg_amd_bounded_last_stats) -- that round is not part of the wall times;
  * a device-to-device copy of a buffer as large as the values of J, timed by events in the same process: the mask pass reads 5
    bytes an entry and writes 8 only where the variable is held, the copy reads and writes 8.
Prints a markdown report (--out: also written to that file).

    python tools/bounded_device_bench.py [--configs 3,4] [--rounds 5] [--warmup 2] [--iterations 10] [--out profiles/bounded_device.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                              # noqa: E402
from problems import BAProblem, DeviceTwin                                  # noqa: E402
from problems import device_robust                                          # noqa: E402

CONFIGS = {3: dict(Nc=499, Np=9000, Nobs=100000), 4: dict(Nc=2499, Np=45000, Nobs=500000)}
LEGS = ("plain", "plain again", "infinite bounds", "bounded")


def bounds_between(p0, pstar, frac=0.5):
    """every third variable: a bound between the optimum (0) and the start (1), on the side of the start"""
    lo, hi = np.full(len(p0), -np.inf), np.full(len(p0), np.inf)
    i = np.arange(0, len(p0), 3)
    mid = pstar[i] + frac * (p0[i] - pstar[i])
    above = p0[i] > pstar[i]
    lo[i[above]] = mid[above]
    hi[i[~above]] = mid[~above]
    return lo, hi


def run(cfg, rounds, warmup, iterations):
    c = CONFIGS[cfg]
    prob = BAProblem(c["Nc"], c["Np"], c["Nobs"], seed=1)
    Jp, Ji = prob.pattern()
    twin = DeviceTwin(prob)
    prm = capi.default_parameters()
    prm.max_iterations = iterations
    p0 = prob.p0()
    N = prob.N
    pstar = capi.optimize_device(p0, N, prob.M, prob.nnz, Jp, Ji, twin.cb, twin.cookie, prm, trace=False)[1]
    box = {"infinite bounds": (np.full(N, -np.inf), np.full(N, np.inf)), "bounded": bounds_between(p0, pstar)}
    held_end = {}

    def solve(leg, trace=False):
        if leg in box:
            r, p, tr, w, held = capi.optimize_device_bounded(p0, N, prob.M, prob.nnz, Jp, Ji, twin.cb, twin.cookie, box[leg][0],
                                                             box[leg][1], None, prm, trace=trace)
            held_end[leg] = int(np.count_nonzero(held))
        else:
            r, p, tr = capi.optimize_device(p0, N, prob.M, prob.nnz, Jp, Ji, twin.cb, twin.cookie, prm, trace=trace)
        assert r >= 0, leg
        return r, tr

    counts = {}
    for leg in LEGS:
        tr = solve(leg, trace=True)[1]
        counts[leg] = (tr.ncallbacks, tr.ntrials)
    times = {leg: [] for leg in LEGS}
    for k in range(warmup + rounds):
        for leg in LEGS:
            t = time.perf_counter()
            solve(leg)
            dt = time.perf_counter() - t
            if k >= warmup:
                times[leg].append(dt * 1e3)
    own = {}
    os.environ["DOGLEG_AMD_TIMING"] = "1"
    try:
        for leg in box:
            solve(leg)          # (a backend made under other DOGLEG_AMD_* knobs is not taken over: this one makes its own)
            solve(leg)
            own[leg] = capi.bounded_last_stats()
    finally:
        del os.environ["DOGLEG_AMD_TIMING"]
    copy_ms = device_robust.lib().robust_copy_ms(prob.nnz, 20)
    assert copy_ms > 0
    row = dict(cfg=cfg, N=N, M=prob.M, nnz=prob.nnz, counts=counts, own=own, copy_ms=copy_ms, held=held_end,
               ms={leg: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for leg, v in times.items()})
    twin.close()
    prob.close()
    capi.lib().dogleg_amd_release_cache()
    return row


def report(rows, a):
    lines = ["# The cost of box bounds on the device solve (dogleg_amd_optimize_device2_bounded)", "",
             f"`python tools/bounded_device_bench.py` on one MI355X: {a.rounds} rounds behind {a.warmup} that are not counted, every "
             f"round the four solves in turn, max_iterations = {a.iterations}.  The bounded leg has a bound on every third variable, "
             "half way between the start and the point the plain solve returns.  Wall times are the host clock around a call "
             "(median, min .. max over the rounds); the time in the feature's kernels is the library's own (events around its "
             "launches, DOGLEG_AMD_TIMING=1, in a round of its own); the copy is a device-to-device hipMemcpyAsync of a buffer as "
             "large as the values of J, by events.  The legs with bounds that bind minimise another problem, so they take other "
             "numbers of evaluations: compare them per evaluation and per step.  A bounded solve gives up the fused step, the "
             "assembly at evaluation time and the work between a step and its wait: the leg with infinite bounds shows what "
             "that costs by itself.", ""]
    lines += ["| config | leg | evaluations | steps | held at the end | solve ms (median, min .. max) | ms per evaluation | ms per step |",
              "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for leg in LEGS:
            med, lo, hi = r["ms"][leg]
            ne, ns = r["counts"][leg]
            lines.append(f"| #{r['cfg']} (N {r['N']}, M {r['M']}, nnz {r['nnz']}) | {leg} | {ne} | {ns} | {r['held'].get(leg, '-')} | "
                         f"{med:.2f} ({lo:.2f} .. {hi:.2f}) | {med / max(ne, 1):.3f} | {med / max(ns, 1):.3f} |")
    lines += ["", "| config | leg | ms in the feature's kernels a solve | per evaluation | of that the mask pass, per evaluation | copy of J ms | "
              "mask / copy | clipped steps | fallbacks | steps with a held variable |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for leg, st in r["own"].items():
            ne = max(st["evaluations"], 1.0)
            lines.append(f"| #{r['cfg']} | {leg} | {st['kernels_ms']:.4f} | {st['kernels_ms'] / ne:.4f} | {st['mask_ms'] / ne:.4f} | "
                         f"{r['copy_ms']:.4f} | {st['mask_ms'] / ne / r['copy_ms']:.2f} | {st['clipped']:.0f} | {st['fallbacks']:.0f} | "
                         f"{st['held_steps']:.0f} |")
    aa = max(abs(r["ms"]["plain"][0] - r["ms"]["plain again"][0]) / r["ms"]["plain"][0] for r in rows)
    lines += ["", f"A/A: the two plain legs differ by at most {100 * aa:.1f} % in their medians; differences between legs below "
              "that are not measured."]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU: nothing here is measured without one"
    rows = []
    for c in [int(v) for v in a.configs.split(",")]:
        rows.append(run(c, a.rounds, a.warmup, a.iterations))
        print(rows[-1], flush=True)
    txt = report(rows, a)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
