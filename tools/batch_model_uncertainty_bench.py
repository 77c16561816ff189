#!/usr/bin/env python3
"""tools/batch_model_uncertainty_bench.py -- what the fused uncertainty and query calls of a built-in model cost against the same
calls through the model's callback.

For GAUSS2D on a 7 x 7 window and EXPDECAY with M = 40, B = 1024, 16384 and 131072 problems (the data of tests/batch_models_np.py
for least squares and of tests/batch_poisson_oracle.py, level "high", for the Poisson likelihood: the problems of seeds 1 .. 1024,
repeated to B), at the optimum of the fused solve, every array in device memory (the _device twins): the time on the stream
(events, DOGLEG_AMD_BATCH_TIMING=1) of

  uncertainty       covariance + variances                       dogleg_amd_dense_batch_model_uncertainty_device
  + factors         the same with the outlierness factors, featureSize 1, the scale given
  query             Nq = 3 queries of 4 rows, the plain form     dogleg_amd_dense_batch_model_query_covariance_device
  query, obs.       the same, the observations-only form over all Nmeas rows

against dogleg_amd_dense_batch_uncertainty_device / _query_covariance_device through dogleg_amd_batch_model_callback (GAUSS) or
dogleg_amd_batch_model_fisher_callback (POISSON): for that route the callback's launch PLUS k_batch_uncertainty / k_batch_query, for
the fused call its one launch.  The legs of a repeat, call by call in one process: fused, callback route, fused again (the A/A pair
of the first leg: the yardstick for the ratio beside it).  Beside them the device memory each route allocates for the call: the
x / J buffer of the callback route, 8 B Nmeas (Nstate + 1) bytes, which the fused call does not have.  Nothing is gated and no
ratio is fixed in advance.  A "## Reading" section written by hand behind the resources is replaced with them: write it again after
--resources.

    python tools/batch_model_uncertainty_bench.py [--out profiles/batch_model_uncertainty.md] [--reps 5] [--max-b 131072]

Every (case, likelihood, B) is a step: a child process of its own (--step KIND LIKELIHOOD B) under `timeout` (--step-timeout
seconds), one behind the other; the first step that fails, is killed or runs out of time ends the run, and no further step is
started.  The process that starts them never opens the device.

The part of --out from the line "## Kernel resources" on is kept as it is; it is written by
    python tools/batch_model_uncertainty_bench.py --resources NEW_REMARKS PARENT_REMARKS --asm NEW_S PARENT_S --out ...
from two compilations of libdogleg_amd/csrc/dense_batch_kernels.hip with --offload-device-only -S
-Rpass-analysis=kernel-resource-usage (the build's flags otherwise), of this tree and of its parent commit.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libdogleg_amd import capi                                                          # noqa: E402
from libdogleg_amd.ctypes_defs import (LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON, MODEL_EXPDECAY, MODEL_GAUSS2D,      # noqa: E402
                                       MODEL_NSTATE)
from batch_products_bounds_bench import asm_functions                                   # noqa: E402
from batch_robust_bench import KEYS, parse_remarks                                      # noqa: E402

CASES = {"gauss2d": (MODEL_GAUSS2D, (7, 7)), "expdecay": (MODEL_EXPDECAY, 40)}
LIKELIHOODS = {"gauss": LIKELIHOOD_GAUSS, "poisson": LIKELIHOOD_POISSON}
BATCHES = [1024, 16384, 131072]
DISTINCT = 1024
NQ, QROWS = 3, 4
MARK = "## Kernel resources"
TITLE = "# Built-in models: the fused uncertainty and query calls against the callback route"


def timed(fn):
    """(ms in the callback's kernels, ms in the library's kernel) of one call"""
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    try:
        rc = fn()
    finally:
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert rc == 0
    s = capi.batch_uncertainty_last_stats()
    return s["ms_callback"], s["ms_library"]


def measure(fused, route, reps, warm=2):
    for _ in range(warm):
        assert fused() == 0 and route() == 0
    t = dict(fused=[], route=[], again=[])
    for _ in range(reps):
        t["fused"].append(timed(fused))
        t["route"].append(timed(route))
        t["again"].append(timed(fused))
    assert all(x[0] == 0.0 for x in t["fused"] + t["again"]), "the fused call reports 0 ms of callback"
    med = lambda xs, k: float(np.median([x[k] for x in xs]))
    return dict(fused=med(t["fused"], 1), again=med(t["again"], 1), cb=med(t["route"], 0), lib=med(t["route"], 1))


def cells(m):
    route = m["cb"] + m["lib"]
    spread = abs(m["again"] / m["fused"] - 1.0)
    return (f"{m['fused']:.4f} | {m['again']:.4f} | {100 * spread:.1f} % | {m['cb']:.4f} | {m['lib']:.4f} | {route:.4f} | "
            f"{route / m['fused']:.2f} x | {m['lib'] / m['fused']:.2f} x")


def step(name, lkname, B, reps):
    """one (case, likelihood, B) on the device: its rows of the table, as a JSON line"""
    from tests import batch_models_np as mz
    from tests import batch_poisson_oracle as po
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    case, lk = CASES[name], LIKELIHOODS[lkname]
    nd = min(B, DISTINCT)
    bt = mz.batch(case, seed0=1, nb=nd) if lk == LIKELIHOOD_GAUSS else po.batch((case, "high"), seed0=1, nb=nd)
    tile = lambda a: np.ascontiguousarray(np.tile(a, ((B + len(a) - 1) // len(a), 1))[:B])
    y, p0 = tile(bt["y"]), tile(bt["p0"])
    N, M = MODEL_NSTATE[bt["kind"]], bt["M"]
    yd = capi.DeviceArray(y)
    rec = capi.batch_model(bt["kind"], yd, M, bt["width"], bt["height"])
    cb, cookie, _, _ = capi.batch_model_callback(rec) if lk == LIKELIHOOD_GAUSS else capi.batch_model_fisher_callback(rec)
    rc, p, res, _ = capi.optimize_dense_batch_model_mle(p0, rec, lk, params=mz.params() if lk == LIKELIHOOD_GAUSS else po.params())
    assert rc == 0
    P, Lm, S = capi.DeviceArray(p), capi.DeviceArray(np.ascontiguousarray(res["lambda_"])), capi.DeviceArray(np.zeros(B, dtype=np.int32))
    cov, var = capi.DeviceArray(nbytes=8 * B * N * N), capi.DeviceArray(nbytes=8 * B * N)
    fac, scale = capi.DeviceArray(nbytes=8 * B * M), capi.DeviceArray(np.full(B, 2.5))
    Jq = capi.DeviceArray(np.random.default_rng(3).standard_normal((B, NQ, QROWS, N)))
    out = capi.DeviceArray(nbytes=8 * B * NQ * QROWS * QROWS)
    legs = {
        "uncertainty": (
            lambda: capi.dense_batch_model_uncertainty_device(P, B, rec, lk, S, Lm, cov, var),
            lambda: capi.dense_batch_uncertainty_device(P, B, N, M, cb, cookie, S, Lm, cov, var)),
        "+ factors": (
            lambda: capi.dense_batch_model_uncertainty_device(P, B, rec, lk, S, Lm, cov, var, fac, scale, 1),
            lambda: capi.dense_batch_uncertainty_device(P, B, N, M, cb, cookie, S, Lm, cov, var, fac, scale, 1)),
        "query": (
            lambda: capi.dense_batch_model_query_covariance_device(P, B, rec, lk, Jq, NQ, QROWS, out, S, -1, Lm),
            lambda: capi.dense_batch_query_covariance_device(P, B, N, M, cb, cookie, Jq, NQ, QROWS, out, S, -1, Lm)),
        "query, obs.": (
            lambda: capi.dense_batch_model_query_covariance_device(P, B, rec, lk, Jq, NQ, QROWS, out, S, M, Lm),
            lambda: capi.dense_batch_query_covariance_device(P, B, N, M, cb, cookie, Jq, NQ, QROWS, out, S, M, Lm)),
    }
    # what each route allocates for the call (device twins, lambda given): the callback route its x / J buffer and the live bytes
    # its callback reads, the fused call nothing
    route_mb, fused_mb = (8 * B * M * (N + 1) + B) / 1e6, 0.0
    rows = []
    for what, (fused, route) in legs.items():
        m = measure(fused, route, reps)
        assert np.count_nonzero(S.numpy()) <= B // 100, "(nearly) every problem ends DOGLEG_AMD_BATCH_UNC_OK"
        rows.append(f"| {name} | {lkname} | {N} | {M} | {B} | {what} | {cells(m)} | {route_mb:.1f} | {fused_mb:.1f} |")
    print(json.dumps(dict(rows=rows)), flush=True)


def bench(a):
    rows = []
    for name in CASES:
        for lkname in LIKELIHOODS:
            for B in BATCHES:
                if B > a.max_b:
                    continue
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, lkname,
                       str(B), "--reps", str(a.reps)]
                r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout + r.stderr)
                    sys.exit(f"step {name}, {lkname}, B = {B} ended with {r.returncode}: no further step is started")
                new = json.loads(r.stdout.strip().splitlines()[-1])["rows"]
                rows += new
                print("\n".join(new), flush=True)
    return [TITLE, "",
            "GAUSS2D on a 7 x 7 window and EXPDECAY with M = 40 (tests/batch_models_np.py; Poisson: tests/batch_poisson_oracle.py, level "
            "\"high\"; the problems of seeds 1 .. 1024 repeated to B, no scale, t_i = i), at the optimum of the fused solve, every array "
            "in device memory.  ms on the stream (events, DOGLEG_AMD_BATCH_TIMING=1): the median over "
            f"{a.reps} repeats, after 2 warm-up calls of each leg; per repeat fused, callback route, fused again, call by call in one "
            "process per (model, likelihood, B).  A/A spread: |fused again / fused - 1|.  The callback route is the callback's launch "
            "plus k_batch_uncertainty<8, FORM_J> or k_batch_query<8, FORM_J>; \"route / fused\" above 1 means the fused call is faster.  "
            f"query: Nq = {NQ} queries of {QROWS} rows; obs.: the observations-only form over all Nmeas rows.  Device memory allocated "
            "for the call: the callback route's x / J buffer and live bytes, 8 B Nmeas (Nstate + 1) + B bytes, against the fused call's "
            "(nothing: lambda_dev is given).  The figures are those of this run, on the MI355X it ran on, and nowhere else.", "",
            "| model | likelihood | N | M | B | call | fused ms | fused again | A/A spread | route: callback ms | route: kernel ms | route ms | "
            "route / fused | kernel alone / fused | route allocates MB | fused allocates MB |",
            "|---|---|---|---|---|---|" + "---|" * 10] + rows


def unsuffixed(fns):
    """asm_functions with the kernels' names as they were before the model argument joined their parameter lists"""
    return {k.replace("12ModelEvalDev", ""): v for k, v in fns.items()}


def resources(new_path, parent_path, asm):
    new, old = parse_remarks(new_path), parse_remarks(parent_path)
    fmt = lambda d: " | ".join(str(d[k]) for k in KEYS)
    names = ["k_batch_uncertainty<8, 0, false>", "k_batch_uncertainty<8, 0, true>", "k_batch_uncertainty<8, 2, true>",
             "k_batch_uncertainty<8, 3, true>", "k_batch_query<8, 0, false>", "k_batch_query<8, 0, true>", "k_batch_query<8, 2, true>",
             "k_batch_query<8, 3, true>"]
    moved = [k for k, v in old.items() if k not in new or any(new[k][x] != v[x] for x in KEYS)]
    out = [MARK, "", "From the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags).", "",
           "### The new instantiations, k_batch_uncertainty / k_batch_query<8, FORM_MODEL = 2 or FORM_POISSON = 3, FIT = true>, each "
           "under its J-form twins", "", "| kernel | " + " | ".join(KEYS) + " |", "|---|" + "---|" * len(KEYS)]
    out += [f"| {k} | {fmt(new[k])} |" for k in names]
    out += ["", f"Existing kernels of dense_batch_kernels.hip whose figures moved against the parent commit: {len(moved)} of {len(old)}"
            + (": " + ", ".join(moved) if moved else "") + "."]
    if asm:
        n, o = unsuffixed(asm_functions(asm[0])), asm_functions(asm[1])
        ks = [k for k in o if re.search(r"k_batch_(round|uncertainty|query)", k)]
        differ = [k for k in ks if n.get(k) != o[k]]
        others = [k for k in o if k not in ks and n.get(k) != o[k]]
        added = [k for k in n if k not in o and "k_batch_" in k]
        out += ["", f"Instruction streams (hipcc --offload-device-only -S of both trees, block labels unnumbered): {len(ks)} existing "
                f"instantiations of k_batch_round, k_batch_uncertainty and k_batch_query compared, {len(ks) - len(differ)} are the same "
                f"stream, {len(differ)} differ.  Kernels this tree adds: {len(added)}.  Other kernels of the file that differ: "
                f"{len(others)}.  UncDev, QueryDev and FitDev did not grow: the model record and the points are a third kernel argument "
                "of k_batch_uncertainty and k_batch_query behind FitDev, which the existing instantiations do not read, so no "
                "argument offset moved."]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a (case, likelihood, B) step may take")
    ap.add_argument("--step", nargs=3, metavar=("KIND", "LIKELIHOOD", "B"), help="run one step on the device and print its rows")
    ap.add_argument("--resources", nargs=2, metavar=("NEW_REMARKS", "PARENT_REMARKS"))
    ap.add_argument("--asm", nargs=2, metavar=("NEW_S", "PARENT_S"), help="with --resources: compare the kernels' instructions too")
    a = ap.parse_args()
    if a.step:
        step(a.step[0], a.step[1], int(a.step[2]), a.reps)
        return
    kept, tail = [], []
    if a.out and os.path.exists(a.out):
        lines = open(a.out).read().splitlines()
        cut = lines.index(MARK) if MARK in lines else len(lines)
        kept, tail = lines[:cut], lines[cut:]
    if a.resources:
        tail = resources(*a.resources, a.asm)
        kept = kept or [TITLE, "", "not measured", ""]
    else:
        kept = bench(a) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(kept + tail) + "\n")


if __name__ == "__main__":
    main()
