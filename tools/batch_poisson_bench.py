#!/usr/bin/env python3
"""tools/batch_poisson_bench.py -- what a round of the Poisson fused solve costs against the least-squares fused solve on the same data.

For GAUSS2D on a 7 x 7 window and EXPDECAY with M = 40 on count data (tests/batch_poisson_oracle.py: the high-count problems of
seeds 1 .. 1024, repeated to B), B = 1024, 16384 and 131072: dogleg_amd_optimize_dense_batch_model_mle with
DOGLEG_AMD_LIKELIHOOD_POISSON against the same entry point with DOGLEG_AMD_LIKELIHOOD_GAUSS on the same y in device memory.  The
quantity is the time on the stream per round (events, DOGLEG_AMD_BATCH_TIMING=1): one launch of k_batch_round either way.  The
legs of a repeat, call by call in one process:

  poisson           likelihood POISSON
  gauss             likelihood GAUSS
  poisson again     the A/A pair of the first leg: the yardstick for the ratio beside it

in two settings: max_iterations = 1 (every problem is evaluated twice, so both rounds take all B problems) and the whole solve
under the default parameters with the tables' stopping thresholds (the two estimators take their own numbers of rounds there: ms
per round is the figure, the rounds are beside it).  Nothing is gated and no ratio is fixed in advance.

    python tools/batch_poisson_bench.py [--out profiles/batch_poisson.md] [--reps 5] [--max-b 131072]

Every (case, B) is a step: a child process of its own (--step KIND B) under `timeout` (--step-timeout seconds), one behind the
other; the first step that fails, is killed or runs out of time ends the run, and no further step is started.  The process that
starts them never opens the device.

The part of --out from the line "## Kernel resources" on is kept as it is; it is written by
    python tools/batch_poisson_bench.py --resources NEW_REMARKS PARENT_REMARKS --asm NEW_S PARENT_S --out ...
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

from libdogleg_amd import capi                                                                          # noqa: E402
from libdogleg_amd.ctypes_defs import (MODEL_EXPDECAY, MODEL_GAUSS2D, MODEL_NSTATE, LIKELIHOOD_GAUSS,   # noqa: E402
                                       LIKELIHOOD_POISSON)
from batch_products_bounds_bench import asm_functions                                                   # noqa: E402
from batch_robust_bench import KEYS, parse_remarks                                                      # noqa: E402

CASES = {"gauss2d": (MODEL_GAUSS2D, (7, 7)), "expdecay": (MODEL_EXPDECAY, 40)}
BATCHES = [1024, 16384, 131072]
DISTINCT = 1024
MARK = "## Kernel resources"
TITLE = "# Poisson maximum-likelihood fits in the batch solve: a round against the least-squares round on the same counts"


def timed(fn):
    """(ms in the library's kernels, rounds) of one call"""
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    try:
        rc = fn()
    finally:
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert rc == 0
    s = capi.batch_last_stats()
    return s["ms_library"], s["rounds"]


def params(**over):
    prm = capi.default_parameters()
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def measure(rec, p0, prm, reps, warm=2):
    def leg(likelihood):
        return lambda: capi.optimize_dense_batch_model_mle(p0, rec, likelihood, params=prm)[0]

    poisson, gauss = leg(LIKELIHOOD_POISSON), leg(LIKELIHOOD_GAUSS)
    for _ in range(warm):
        assert poisson() == 0 and gauss() == 0
    t = dict(poisson=[], gauss=[], again=[])
    for _ in range(reps):
        t["poisson"].append(timed(poisson))
        t["gauss"].append(timed(gauss))
        t["again"].append(timed(poisson))
    med = lambda xs: float(np.median([x[0] / x[1] for x in xs]))
    return dict(poisson=med(t["poisson"]), gauss=med(t["gauss"]), again=med(t["again"]),
                rounds=(t["poisson"][0][1], t["gauss"][0][1]))


def cells(m):
    spread = abs(m["again"] / m["poisson"] - 1.0)
    diff = abs(m["poisson"] / m["gauss"] - 1.0)
    return (f"{m['rounds'][0]:.0f} / {m['rounds'][1]:.0f} | {m['poisson']:.4f} | {m['again']:.4f} | {100 * spread:.1f} % | {m['gauss']:.4f} | "
            f"{m['poisson'] / m['gauss']:.2f} x | {'inside' if diff <= spread else 'outside'}")


def step(name, B, reps):
    """one (case, B) on the device: its row of the table, as a JSON line"""
    from tests import batch_poisson_oracle as po
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    bt = po.batch((CASES[name], "high"), seed0=1, nb=min(B, DISTINCT))
    tile = lambda a: np.ascontiguousarray(np.tile(a, ((B + len(a) - 1) // len(a), 1))[:B])
    y, p0 = tile(bt["y"]), tile(bt["p0"])
    N, M = MODEL_NSTATE[bt["kind"]], bt["M"]
    yd = capi.DeviceArray(y)
    rec = capi.batch_model(bt["kind"], yd, M, bt["width"], bt["height"])
    stop = dict(po.STOP_OVER)
    live = measure(rec, p0, params(max_iterations=1, **stop), reps)
    whole = measure(rec, p0, params(**stop), reps)
    print(json.dumps(dict(row=f"| {name} | {N} | {M} | {B} | {cells(live)} | {cells(whole)} |")), flush=True)


def bench(a):
    rows = []
    for name in CASES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, str(B),
                   "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"step {name}, B = {B} ended with {r.returncode}: no further step is started")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1])["row"])
            print(rows[-1], flush=True)
    half = ("rounds Poisson / Gauss | Poisson ms/round | Poisson again | A/A spread | Gauss ms/round | Poisson / Gauss | the difference "
            "lies ... the A/A spread")
    return [TITLE, "",
            "GAUSS2D on a 7 x 7 window and EXPDECAY with M = 40 on Poisson-drawn counts (tests/batch_poisson_oracle.py, the high-count "
            "problems of seeds 1 .. 1024 repeated to B).  ms per round on the stream (events, DOGLEG_AMD_BATCH_TIMING=1): the median "
            f"over {a.reps} repeats of (ms of the call / its rounds), after 2 warm-up calls of each leg; per repeat Poisson, Gauss, "
            "Poisson again, call by call in one process per row.  A/A spread: |Poisson again / Poisson - 1|.  Both legs are one launch "
            "of k_batch_round<8, ...> a round: FORM_POISSON against FORM_MODEL.  In the whole solve the two estimators take their own "
            "numbers of rounds, and the later rounds hold few live problems.  The figures are those of this run, on the MI355X it ran "
            "on, and nowhere else.", "",
            "| model | N | M | B | every problem live (max_iterations 1): " + half + " | whole solve: " + half + " |",
            "|---|---|---|---|" + "---|" * 14] + rows


def resources(new_path, parent_path, asm):
    new, old = parse_remarks(new_path), parse_remarks(parent_path)
    fmt = lambda d: " | ".join(str(d[k]) for k in KEYS)
    names = ["k_batch_round<8, 2, false, false>", "k_batch_round<8, 3, false, false>", "k_batch_round<8, 2, false, true>",
             "k_batch_round<8, 3, false, true>"]
    moved = [k for k, v in old.items() if k not in new or any(new[k][x] != v[x] for x in KEYS)]
    out = [MARK, "", "From the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags).", "",
           "### The new instantiations, k_batch_round<8, FORM_POISSON = 3, ROBUST = false, BOUNDED>, each under its model-form twin "
           "(FORM_MODEL = 2)", "", "| kernel | " + " | ".join(KEYS) + " |", "|---|" + "---|" * len(KEYS)]
    out += [f"| {k} | {fmt(new[k])} |" for k in names]
    out += ["", f"Existing kernels of dense_batch_kernels.hip whose figures moved against the parent commit: {len(moved)} of {len(old)}"
            + (": " + ", ".join(moved) if moved else "") + "."]
    if asm:
        n, o = asm_functions(asm[0]), asm_functions(asm[1])
        ks = [k for k in o if re.search(r"k_batch_(round|uncertainty|query)", k)]
        differ = [k for k in ks if n.get(k) != o[k]]
        others = [k for k in o if k not in ks and n.get(k) != o[k]]
        added = [k for k in n if k not in o and "k_batch_" in k]
        out += ["", f"Instruction streams (hipcc --offload-device-only -S of both trees, block labels unnumbered): {len(ks)} existing "
                f"instantiations of k_batch_round, k_batch_uncertainty and k_batch_query compared, {len(ks) - len(differ)} are the same "
                f"stream, {len(differ)} differ.  Kernels this tree adds: {len(added)}.  Other kernels of the file (k_batch_init, "
                f"k_batch_clamp, k_batch_finish) that differ: {len(others)}."]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a (case, B) step may take")
    ap.add_argument("--step", nargs=2, metavar=("KIND", "B"), help="run one step on the device and print its row")
    ap.add_argument("--resources", nargs=2, metavar=("NEW_REMARKS", "PARENT_REMARKS"))
    ap.add_argument("--asm", nargs=2, metavar=("NEW_S", "PARENT_S"), help="with --resources: compare the kernels' instructions too")
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), a.reps)
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
