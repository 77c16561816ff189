#!/usr/bin/env python3
"""tools/numeric_device_bench.py -- the numeric-Jacobian adapter of a single problem (dogleg_amd_numeric_*) on the patterns of
the benchmark configs #3 (sparse-200k) and #4 (sparse-1m) with the values-only test model (problems/values.py).  Nothing is
gated.

(1) The adapter's two launches (events on the stream, DOGLEG_AMD_NUMERIC_TIMING=1) against a device-to-device copy that moves the
    bytes they MUST move: K Nmeas doubles read, nnz + Nmeas and K Nstate doubles written, 8 bytes of index per entry read.  The
    legs alternate in one process; the adapter is measured in two interleaved series, and the relative difference of their
    medians is the A/A spread.
(2) One invocation of the adapter (the model's K evaluations included) against one invocation of the analytic callback of the
    same model (problems/gradcheck.py): n calls back to back and one synchronisation, wall time over n, the legs alternated, the
    analytic leg twice for the A/A spread.
(3) A whole dogleg_optimize_device2 through the adapter against the analytic one from the same start: wall time, evaluations, ms
    an evaluation, the distance of the end points.

    python tools/numeric_device_bench.py [--out profiles/numeric_device.md] [--reps 9] [--configs sparse-200k,sparse-1m]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                              # noqa: E402
from libdogleg_amd.ctypes_defs import NUMERIC_FORWARD, NUMERIC_CENTRAL      # noqa: E402
from problems import BAProblem                                              # noqa: E402
from problems import gradcheck as gp                                        # noqa: E402
from problems.batch_values import DeviceCopy                                # noqa: E402
from problems.values import ValuesModel                                     # noqa: E402

CONFIGS = {"sparse-200k": dict(Nc=499, Np=9000, Nobs=100000), "sparse-1m": dict(Nc=2499, Np=45000, Nobs=500000),
           "sparse-tiny": dict(Nc=49, Np=900, Nobs=10000)}
SCHEMES = [(NUMERIC_FORWARD, "forward"), (NUMERIC_CENTRAL, "central")]
EPS, SPREAD, SEED = 0.4, 0.5, 5

NOTES = [
    "(1) The share is the copy's time over the kernels': 100 % would be the copy's rate.  The kernels' time holds both launches; "
    "k_numeric_perturb_coloured's K Nstate doubles are among the bytes counted.  The two launches come to 51 - 62 % of the copy.  "
    "Why not more has been reasoned, not measured with counters: a workgroup of k_numeric_jacobian_sparse has ONE tile in flight "
    "-- it stages 16 or 31 segments of 512 bytes, waits at a barrier, and then every lane does a six-step bisection in LDS before "
    "its gather of the divisor and its store --, so the loads of the next tile do not start under the entry walk of this one, and "
    "each entry reads two index words (colour, variable) where one packed word would do.  What would be tried next, in a pull "
    "request of its own and against these numbers: staging the next tile's segments while this tile's entries are walked (two "
    "LDS images, still four workgroups a CU on these patterns), one packed index word per entry, and a row found once per run of "
    "lanes instead of per lane.  Tuning is not part of this work.",
    "(2) An invocation costs 9 to 23 times the analytic callback's: the model is evaluated at K = 16 or 31 points instead of one, "
    "and this test model gathers 15 variables a row at every point.  The adapter's own two launches are 1.3 to 2.5 % of the "
    "invocation: the price of not writing the Jacobian kernel is paid in evaluations of the model, not in the adapter.",
    "(3) The numeric solve makes the analytic solve's number of evaluations and ends on its end point (to 2.5e-14; the model has a "
    "zero-residual optimum, which both reach).  It is 3.4 to 9.3 times slower, the ratio of (2) diluted by the solver's own work.",
    "The test of the central differences against the CPU oracle (tests/test_device_numeric_gpu.py, block-arrowhead pattern 7 x 50 "
    "x 400, eps 0.4, spread 0.5, seed 5, trustregion0 0.3): the oracle against the oracle with every x moved by up to one ulp "
    "differs by 3.59e-11 in its worst step (ulp seed 7; seed 8: 1.41e-11), so the step tolerance is 3.59e-10; the adapter's worst "
    "step difference from the oracle was 1.29e-11 over the six trials.",
]


def med(v):
    return float(np.median(v))


def problem(name):
    prob = BAProblem(**CONFIGS[name], seed=11)
    Jp, Ji = prob.pattern()
    N, M = prob.N, prob.M
    prob.close()
    rng = np.random.default_rng(SEED)
    a = rng.uniform(0.1, 1.0, len(Ji)) * rng.choice([-1.0, 1.0], len(Ji))
    pstar = rng.uniform(-1.0, 1.0, N)
    p0 = pstar + SPREAD * rng.uniform(-1.0, 1.0, N)
    return N, M, Jp, Ji, a, pstar, p0


def kernels(P, scheme, reps):
    N, M, Jp, Ji, a, pstar, p0 = P
    nnz = len(Ji)
    model = ValuesModel(N, M, Jp, Ji, a, pstar, EPS)
    ad = capi.DeviceNumeric(N, M, nnz, Jp, Ji, model.cb, model.cookie, scheme=scheme)
    K = ad.K
    moved = 8.0 * (K * M + nnz + M + K * N) + 8.0 * nnz
    cp = DeviceCopy(moved)
    dp, dx, dJ = capi.DeviceArray(p0), capi.DeviceArray(nbytes=8 * M), capi.DeviceArray(nbytes=8 * nnz)
    os.environ["DOGLEG_AMD_NUMERIC_TIMING"] = "1"

    def leg():
        s0 = ad.stats()
        ad.invoke(dp, dx, dJ)
        s1 = ad.stats()
        return s1["ms_library"] - s0["ms_library"], s1["ms_f"] - s0["ms_f"]

    for _ in range(3):
        leg()
        cp.run()
    a1, a2, c, f = [], [], [], []
    for _ in range(reps):
        t, tf = leg()
        a1.append(t)
        f.append(tf)
        c.append(cp.run())
        a2.append(leg()[0])
    os.environ.pop("DOGLEG_AMD_NUMERIC_TIMING", None)
    for d in (dp, dx, dJ):
        d.free()
    for o in (cp, ad, model):
        o.close()
    both = a1 + a2
    return dict(K=K, C=ad.C, moved=moved, lib=med(both), rng=(min(both), max(both)), aa=abs(med(a1) - med(a2)) / med(both),
                copy=med(c), copy_rng=(min(c), max(c)), f=med(f))


def invocations(P, scheme, reps, n=20):
    N, M, Jp, Ji, a, pstar, p0 = P
    nnz = len(Ji)
    L = capi.lib()
    model = ValuesModel(N, M, Jp, Ji, a, pstar, EPS)
    analytic = gp.SparseModel(N, M, Jp, Ji, a, pstar, EPS)
    ad = capi.DeviceNumeric(N, M, nnz, Jp, Ji, model.cb, model.cookie, scheme=scheme)
    dp, dx, dJ = capi.DeviceArray(p0), capi.DeviceArray(nbytes=8 * M), capi.DeviceArray(nbytes=8 * nnz)
    cb = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(analytic.cb.value)

    def timed(call):
        L.dlg_device_sync()
        t = time.perf_counter()
        for _ in range(n):
            call()
        L.dlg_device_sync()
        return (time.perf_counter() - t) / n * 1e3

    numeric = lambda: ad.invoke(dp, dx, dJ)
    ana = lambda: cb(dp.ptr, dx.ptr, dJ.ptr, None, analytic.cookie)
    for _ in range(2):
        timed(numeric)
        timed(ana)
    tn, t1, t2 = [], [], []
    for _ in range(reps):
        t1.append(timed(ana))
        tn.append(timed(numeric))
        t2.append(timed(ana))
    for d in (dp, dx, dJ):
        d.free()
    for o in (ad, model, analytic):
        o.close()
    return dict(K=ad.K, num=med(tn), num_rng=(min(tn), max(tn)), ana=med(t1 + t2), ana_rng=(min(t1 + t2), max(t1 + t2)),
                aa=abs(med(t1) - med(t2)) / med(t1 + t2))


def solves(P, scheme, reps):
    N, M, Jp, Ji, a, pstar, p0 = P
    nnz = len(Ji)
    model = ValuesModel(N, M, Jp, Ji, a, pstar, EPS)
    analytic = gp.SparseModel(N, M, Jp, Ji, a, pstar, EPS)
    ad = capi.DeviceNumeric(N, M, nnz, Jp, Ji, model.cb, model.cookie, scheme=scheme)

    def solve(cb, cookie):
        t = time.perf_counter()
        r, p, _ = capi.optimize_device(p0, N, M, nnz, Jp, Ji, cb, cookie, trace=False)
        dt = time.perf_counter() - t
        assert r >= 0
        return dt * 1e3, p

    solve(ad.cb, ad.cookie)
    solve(analytic.cb, analytic.cookie)
    tn, t1, t2 = [], [], []
    for _ in range(reps):
        t1.append(solve(analytic.cb, analytic.cookie)[0])
        tn.append(solve(ad.cb, ad.cookie)[0])
        t2.append(solve(analytic.cb, analytic.cookie)[0])
    model.reset()
    analytic.reset()
    _, pn = solve(ad.cb, ad.cookie)
    _, pa = solve(analytic.cb, analytic.cookie)
    out = dict(num=med(tn), num_rng=(min(tn), max(tn)), ana=med(t1 + t2), ana_rng=(min(t1 + t2), max(t1 + t2)),
               aa=abs(med(t1) - med(t2)) / med(t1 + t2), ev_n=model.ncalls(), ev_a=analytic.ncalls(), points=model.ncopies(),
               dist=float(np.max(np.abs(pn - pa))), off=float(np.max(np.abs(pn - pstar))))
    for o in (ad, model, analytic):
        o.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--configs", default="sparse-200k,sparse-1m")
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    names = a.configs.split(",")
    sreps = max(3, a.reps // 3)
    probs = {n: problem(n) for n in names}
    out = ["# Numeric Jacobians for values-only device callbacks, sparse: dogleg_amd_numeric_*", "",
           f"Values-only device test model (problems/values.py: eps {EPS}, spread {SPREAD}, coefficient seed {SEED}) on the patterns of "
           "the benchmark configs; default deltas.  Written by tools/numeric_device_bench.py; nothing here is gated.", "",
           "## (1) The adapter's two launches against a copy of the bytes they must move", "",
           "One invocation at the start point.  kernels: k_numeric_perturb_coloured + k_numeric_jacobian_sparse (events on the "
           f"stream), median (min .. max) of 2 x {a.reps} invocations in two interleaved series; A/A: the relative difference of the "
           "two series' medians.  copy: a device-to-device copy that moves 8 (K Nmeas + nnz + Nmeas + K Nstate) + 8 nnz bytes, "
           f"alternated with the invocations, median of {a.reps}.  share: copy / kernels.  model: the values kernel's time in the same "
           "invocations, for scale.", "",
           "| config | N | M | nnz | scheme | C | K | MB moved | kernels us | A/A | copy us | share | model us |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in names:
        N, M, Jp, Ji = probs[n][:4]
        for scheme, sname in SCHEMES:
            r = kernels(probs[n], scheme, a.reps)
            line = (f"| {n} | {N} | {M} | {len(Ji)} | {sname} | {r['C']} | {r['K']} | {r['moved'] / 1e6:.1f} | {r['lib'] * 1e3:.1f} "
                    f"({r['rng'][0] * 1e3:.1f} .. {r['rng'][1] * 1e3:.1f}) | {100 * r['aa']:.1f} % | {r['copy'] * 1e3:.1f} "
                    f"({r['copy_rng'][0] * 1e3:.1f} .. {r['copy_rng'][1] * 1e3:.1f}) | {100 * r['copy'] / r['lib']:.0f} % | {r['f'] * 1e3:.1f} |")
            print(line, flush=True)
            out.append(line)
    out += ["", "## (2) One invocation against the analytic callback of the same model", "",
            "20 calls back to back and one synchronisation, wall time over 20; numeric: the adapter with the model's K evaluations, "
            f"median (min .. max) of {a.reps}; analytic: problems/gradcheck.py's kernel (x and J in one pass), 2 x {a.reps}, A/A: the "
            "relative difference of its two series' medians; the legs alternated.", "",
            "| config | scheme | K | numeric us | analytic us | A/A | numeric / analytic |", "|---|---|---|---|---|---|---|"]
    for n in names:
        for scheme, sname in SCHEMES:
            r = invocations(probs[n], scheme, a.reps)
            line = (f"| {n} | {sname} | {r['K']} | {r['num'] * 1e3:.1f} ({r['num_rng'][0] * 1e3:.1f} .. {r['num_rng'][1] * 1e3:.1f}) | "
                    f"{r['ana'] * 1e3:.1f} ({r['ana_rng'][0] * 1e3:.1f} .. {r['ana_rng'][1] * 1e3:.1f}) | {100 * r['aa']:.1f} % | "
                    f"{r['num'] / r['ana']:.1f} x |")
            print(line, flush=True)
            out.append(line)
    out += ["", "## (3) Whole solves: dogleg_optimize_device2 through the adapter against the analytic callback", "",
            f"Default parameters, the same start.  wall: median (min .. max) of {sreps} solves (the analytic leg: 2 x {sreps}, A/A: "
            "the relative difference of its two series' medians), the legs alternated.  evaluations: invocations of the callback in "
            "one solve (numeric: each is K points of the model).  distance: the largest |p_numeric - p_analytic|; off: the largest "
            "|p_numeric - p*| (the model has a zero-residual optimum at p*).", "",
            "| config | scheme | numeric ms | analytic ms | A/A | numeric / analytic | evaluations n / a | points | ms an evaluation n / a "
            "| distance | off |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in names:
        for scheme, sname in SCHEMES:
            r = solves(probs[n], scheme, sreps)
            line = (f"| {n} | {sname} | {r['num']:.1f} ({r['num_rng'][0]:.1f} .. {r['num_rng'][1]:.1f}) | {r['ana']:.1f} "
                    f"({r['ana_rng'][0]:.1f} .. {r['ana_rng'][1]:.1f}) | {100 * r['aa']:.1f} % | {r['num'] / r['ana']:.2f} x | "
                    f"{r['ev_n']} / {r['ev_a']} | {r['points']} | {r['num'] / r['ev_n']:.2f} / {r['ana'] / r['ev_a']:.2f} | {r['dist']:.1e} | "
                    f"{r['off']:.1e} |")
            print(line, flush=True)
            out.append(line)
    out += ["", "## Reading the tables (the figures quoted are those of the run this file was first written from)", ""] + NOTES
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
