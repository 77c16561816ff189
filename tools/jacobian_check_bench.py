#!/usr/bin/env python3
"""tools/jacobian_check_bench.py -- dogleg_amd_check_jacobian_device on the sparse benchmark configurations.

For configs #3 and #4 (problems.BAProblem with its GPU-resident twin, problems/device_problems.hip), at the starting
point: the wall time of the whole check (planner, uploads, 2 x ncolours evaluations, compare kernels, the one download;
median and range of the repeats after a warm-up call), its evaluations, and the time on the stream split into the
callback's kernels and the library's compare kernels (events, DOGLEG_AMD_CHECK_TIMING=1, in a call of its own).

For comparison, what checking one variable at a time costs: 32 sampled variables through
dogleg_amd_testGradient_device (two evaluations, one compare of the single column, one download and the print each;
stdout sent to /dev/null), the mean EXTRAPOLATED to all Nstate.  Nothing is gated.

    python tools/jacobian_check_bench.py [--configs 3,4] [--reps 5] [--out profiles/jacobian_check.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                      # noqa: E402
from libdogleg_amd.ctypes_defs import dptr, iptr    # noqa: E402
from problems import BAProblem, DeviceTwin          # noqa: E402

CONFIGS = {
    3: dict(Nc=499, Np=9000, Nobs=100000),
    4: dict(Nc=2499, Np=45000, Nobs=500000),
}
RTOL, ATOL = 0.0, 1e-7
SAMPLE = 32


def check(prob, twin, Jp, Ji, p0, timing=False):
    if timing:
        os.environ["DOGLEG_AMD_CHECK_TIMING"] = "1"
    t = time.perf_counter()
    out = capi.check_jacobian_device(p0, prob.N, prob.M, prob.nnz, Jp, Ji, twin.cb, twin.cookie, rtol=RTOL, atol=ATOL,
                                     want_var_error=False)
    dt = time.perf_counter() - t
    os.environ.pop("DOGLEG_AMD_CHECK_TIMING", None)
    assert out["rc"] >= 0, "the check failed"
    return dt, out["report"], capi.check_jacobian_last_stats()


def one_at_a_time(prob, twin, Jp, Ji, p0):
    """seconds per variable of the two-evaluation check, over SAMPLE variables; the table goes to /dev/null"""
    L = capi.lib()
    rng = np.random.default_rng(1)
    vs = rng.choice(prob.N, size=SAMPLE, replace=False)
    sys.stdout.flush()
    keep = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        L.dogleg_amd_testGradient_device(int(vs[0]), dptr(p0), prob.N, prob.M, prob.nnz, iptr(Jp), iptr(Ji), twin.cb, twin.cookie)
        t = time.perf_counter()
        for v in vs:
            L.dogleg_amd_testGradient_device(int(v), dptr(p0), prob.N, prob.M, prob.nnz, iptr(Jp), iptr(Ji), twin.cb, twin.cookie)
        dt = time.perf_counter() - t
    finally:
        os.dup2(keep, 1)
        os.close(null)
        os.close(keep)
    return dt / SAMPLE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    out = ["# The Jacobian of a device callback against central differences: dogleg_amd_check_jacobian_device", "",
           f"Block-arrowhead benchmark problems with their GPU-resident twin at the starting point; rtol {RTOL}, atol {ATOL}, the "
           f"reference's delta; wall: median (min .. max) of {a.reps} calls after a warm-up call, the host planner, the uploads and "
           "the download included; callback / library: events on the stream in a call of their own; one at a time: the mean of "
           f"{SAMPLE} sampled variables through dogleg_amd_testGradient_device (two evaluations, one compare, one download and the "
           "print, each) times Nstate -- an extrapolation, not a measurement.", "",
           "| config | Nstate | Nmeas | nnz | colours | evaluations | wall ms | callback ms | library ms | library share | "
           "max error | bad | one at a time: ms / variable | extrapolated s | ratio |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for cfg in [int(c) for c in a.configs.split(",")]:
        prm = CONFIGS[cfg]
        prob = BAProblem(prm["Nc"], prm["Np"], prm["Nobs"], seed=1)
        twin = DeviceTwin(prob)
        Jp, Ji = prob.pattern()
        p0 = prob.p0()
        check(prob, twin, Jp, Ji, p0)
        ts = [check(prob, twin, Jp, Ji, p0)[0] for _ in range(a.reps)]
        _, rep, st = check(prob, twin, Jp, Ji, p0, timing=True)
        per_var = one_at_a_time(prob, twin, Jp, Ji, p0)
        t = float(np.median(ts))
        share = st["ms_library"] / (st["ms_library"] + st["ms_callback"]) if st["ms_library"] + st["ms_callback"] > 0 else float("nan")
        line = (f"| #{cfg} | {prob.N} | {prob.M} | {prob.nnz} | {rep['ncolours']} | {rep['evaluations']} | "
                f"{t * 1e3:.2f} ({min(ts) * 1e3:.2f} .. {max(ts) * 1e3:.2f}) | {st['ms_callback']:.3f} | {st['ms_library']:.3f} | "
                f"{100 * share:.1f} % | {rep['max_error']:.2e} | {rep['nbad'] + rep['noutside']} | {per_var * 1e3:.3f} | "
                f"{per_var * prob.N:.1f} | {per_var * prob.N / t:.0f} x |")
        print(line, flush=True)
        out.append(line)
        twin.close()
        prob.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
