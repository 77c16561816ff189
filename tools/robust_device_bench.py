#!/usr/bin/env python3
"""tools/robust_device_bench.py -- what a loss costs on dogleg_optimize_device2 (dogleg_amd_optimize_device2_robust).

For each configuration (the shapes tools/outlier_bench.py uses for configs #3 and #4), in one process, with 5 % of the features
displaced by +-1.0 (problems/batch_offsets.py: planted_offsets) and features of two rows:
  * the solves alternate, round after round, in the order plain, plain again (the A/A leg: the spread of the measurement),
    robust TRIVIAL, robust Cauchy; the first --warmup rounds are not counted; a solve is timed by the host clock around the
    call, which returns synchronised; no trace is attached (as a user calls it);
  * one more round with DOGLEG_AMD_TIMING=1 gives the prelude's time per evaluation from the library's own events
    (dogleg_amd_robust_last_stats) -- that round is not part of the wall times;
  * a device-to-device copy of a buffer as large as the values of J, timed by events in the same process: the copy reads and
    writes the same 16 bytes per entry as the prelude's pass over J;
  * the prelude's share of the plain solve's time per evaluation.
Prints a markdown report (--out: also written to that file).

    python tools/robust_device_bench.py [--configs 3,4] [--rounds 5] [--warmup 2] [--iterations 10] [--out profiles/robust_device.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                              # noqa: E402
from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_TRIVIAL, LOSS_CAUCHY  # noqa: E402
from problems import BAProblem, DeviceTwin                                  # noqa: E402
from problems import device_robust                                          # noqa: E402
from problems.batch_offsets import planted_offsets                          # noqa: E402

CONFIGS = {3: dict(Nc=499, Np=9000, Nobs=100000), 4: dict(Nc=2499, Np=45000, Nobs=500000)}
FS, SCALE, FRACTION, SIZE = 2, 0.05, 0.05, 1.0
LEGS = ("plain", "plain again", "TRIVIAL", "Cauchy")


def run(cfg, rounds, warmup, iterations):
    c = CONFIGS[cfg]
    prob = BAProblem(c["Nc"], c["Np"], c["Nobs"], seed=1)
    Jp, Ji = prob.pattern()
    off = planted_offsets(1, prob.M, FS, FRACTION, SIZE, 1)[0][0]
    model = device_robust.OffsetDeviceModel(DeviceTwin(prob), off)
    prm = capi.default_parameters()
    prm.max_iterations = iterations
    p0 = prob.p0()
    losses = {"TRIVIAL": BatchLoss(LOSS_TRIVIAL, 0.0, FS), "Cauchy": BatchLoss(LOSS_CAUCHY, SCALE, FS)}

    def solve(leg, trace=False):
        if leg in losses:
            r, p, tr, w = capi.optimize_device_robust(p0, prob.N, prob.M, prob.nnz, Jp, Ji, model.cb, model.cookie, losses[leg], prm,
                                                      trace=trace)
        else:
            r, p, tr = capi.optimize_device(p0, prob.N, prob.M, prob.nnz, Jp, Ji, model.cb, model.cookie, prm, trace=trace)
        assert r >= 0, leg
        return r, tr

    # evaluations a solve: from a traced solve each (not timed)
    evals = {leg: solve(leg, trace=True)[1].ncallbacks for leg in LEGS}
    times = {leg: [] for leg in LEGS}
    for k in range(warmup + rounds):
        for leg in LEGS:
            t = time.perf_counter()
            solve(leg)
            dt = time.perf_counter() - t
            if k >= warmup:
                times[leg].append(dt * 1e3)
    # the prelude's own time, from the library's events
    prelude = {}
    os.environ["DOGLEG_AMD_TIMING"] = "1"
    try:
        for leg in losses:
            solve(leg)          # (a backend made under other DOGLEG_AMD_* knobs is not taken over: this one makes its own)
            solve(leg)
            st = capi.robust_last_stats()
            prelude[leg] = st["prelude_ms"] / st["evaluations"]
    finally:
        del os.environ["DOGLEG_AMD_TIMING"]
    copy_ms = device_robust.lib().robust_copy_ms(prob.nnz, 20)
    assert copy_ms > 0
    row = dict(cfg=cfg, N=prob.N, M=prob.M, nnz=prob.nnz, evals=evals, prelude=prelude, copy_ms=copy_ms,
               ms={leg: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for leg, v in times.items()})
    model.close()
    prob.close()
    capi.lib().dogleg_amd_release_cache()
    return row


def report(rows, a):
    lines = ["# The cost of a loss on the device solve (dogleg_amd_optimize_device2_robust)", "",
             f"`python tools/robust_device_bench.py` on one MI355X: {a.rounds} rounds behind {a.warmup} that are not counted, every "
             f"round the four solves in turn, max_iterations = {a.iterations}, 5 % of the features (two rows each) displaced by "
             "+-1.0, Cauchy scale 0.05.  Wall times are the host clock around a call (median, min .. max over the rounds); the "
             "prelude's time is the library's own (events around its launches, DOGLEG_AMD_TIMING=1, in a round of its "
             "own); the copy is a device-to-device hipMemcpyAsync of a buffer as large as the values of J, by events.  The "
             "legs minimise different functions (the plain and the TRIVIAL solve the same one), so they take different "
             "numbers of evaluations: compare them per evaluation.", ""]
    lines += ["| config | leg | evaluations | solve ms (median, min .. max) | ms per evaluation |", "|---|---|---|---|---|"]
    for r in rows:
        for leg in LEGS:
            med, lo, hi = r["ms"][leg]
            lines.append(f"| #{r['cfg']} (N {r['N']}, M {r['M']}, nnz {r['nnz']}) | {leg} | {r['evals'][leg]} | {med:.2f} ({lo:.2f} .. {hi:.2f}) | "
                         f"{med / r['evals'][leg]:.3f} |")
    lines += ["", "| config | values of J | prelude ms per evaluation (TRIVIAL / Cauchy) | copy of J ms | prelude / copy | bytes per s of the "
              "prelude's pass (16 B per entry) | share of the plain solve's time per evaluation |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        per_eval = r["ms"]["plain"][0] / r["evals"]["plain"]
        pt, pc = r["prelude"]["TRIVIAL"], r["prelude"]["Cauchy"]
        lines.append(f"| #{r['cfg']} | {8e-6 * r['nnz']:.1f} MB | {pt:.4f} / {pc:.4f} | {r['copy_ms']:.4f} | {pt / r['copy_ms']:.2f} / "
                     f"{pc / r['copy_ms']:.2f} | {16e-9 * r['nnz'] / (pc * 1e-3):.0f} GB/s | {100 * pc / per_eval:.1f} % |")
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
