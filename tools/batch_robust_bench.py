#!/usr/bin/env python3
"""tools/batch_robust_bench.py -- what the robust sweep costs over the plain one.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96), B = 1024, 16384 and 131072 problems of the dense device test problem
(problems/batch.py, the default generator settings) and every loss (TRIVIAL, HUBER, SOFT_L1, CAUCHY; scale = the noise
sqrt(featureSize), featureSize 2): dogleg_amd_optimize_dense_batch_robust against dogleg_amd_optimize_dense_batch on the same
problems.  The quantity is the time on the stream inside the library's kernels (events, DOGLEG_AMD_BATCH_TIMING=1) per round,
in two settings:

  every problem live  max_iterations = 1: a problem is evaluated twice (three times where its first trial is rejected), so
                      the rounds run the sweep of all B problems (and the first one the step behind it) whatever the loss
  the whole solve     the default parameters; the losses stop after different numbers of rounds, with different shares of
                      the batch live in them, so this column is what a user sees, not a kernel comparison

Protocol: plain, robust, plain again per repeat in one process, after warm-up calls of both.  The two plain legs are an A/A
pair: their medians differ by nothing but the spread of the measurement, the yardstick for the ratio beside them.  Nothing is
gated and no ratio is fixed in advance.

    python tools/batch_robust_bench.py [--out profiles/batch_robust.md] [--reps 5] [--max-b 131072]

The part of --out from the line "## Kernel resources" on is kept as it is; it is written by
    python tools/batch_robust_bench.py --resources NEW_REMARKS PARENT_REMARKS [--asm NEW_S PARENT_S] --out profiles/batch_robust.md
from two compilations of libdogleg_amd/csrc/dense_batch.hip with -Rpass-analysis=kernel-resource-usage (the build's flags
otherwise), of this tree and of its parent commit.
"""
import argparse
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                                          # noqa: E402
from libdogleg_amd.ctypes_defs import (BatchLoss, LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY)     # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
FS = 2
LOSSES = [("TRIVIAL", LOSS_TRIVIAL), ("HUBER", LOSS_HUBER), ("SOFT_L1", LOSS_SOFT_L1), ("CAUCHY", LOSS_CAUCHY)]
MARK = "## Kernel resources"


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


def legs(db, loss, prm):
    p0 = db.p0()

    def plain():
        return capi.optimize_dense_batch(p0, db.N, db.M, db.cb, db.cookie, prm)[0]

    def robust():
        return capi.optimize_dense_batch_robust(p0, db.N, db.M, db.cb, db.cookie, loss, prm)[0]

    return plain, robust


def measure(db, loss, prm, reps, warm=2):
    plain, robust = legs(db, loss, prm)
    for _ in range(warm):
        assert plain() == 0 and robust() == 0
    a, r, b = [], [], []
    for _ in range(reps):
        a.append(timed(plain))
        r.append(timed(robust))
        b.append(timed(plain))
    per = lambda xs: float(np.median([ms / n for ms, n in xs]))
    return dict(plain=per(a), robust=per(r), again=per(b), rounds_plain=a[0][1], rounds_robust=r[0][1])


def cells(m):
    spread = abs(m["again"] / m["plain"] - 1.0)
    return (f"{m['plain']:.4f} | {m['again']:.4f} | {100 * spread:.1f} % | {m['robust']:.4f} | {m['robust'] / m['plain']:.2f} x")


def bench(a):
    from problems.batch import DeviceBatch
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    rows = []
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            for name, kind in LOSSES:
                loss = BatchLoss(kind, NOISE * float(np.sqrt(FS)), FS)
                one = capi.default_parameters()
                one.max_iterations = 1
                live = measure(db, loss, one, a.reps)
                whole = measure(db, loss, capi.default_parameters(), a.reps)
                rows.append(f"| {N} | {M} | {B} | {name} | {live['rounds_plain']} / {live['rounds_robust']} | {cells(live)} | "
                            f"{whole['rounds_plain']} / {whole['rounds_robust']} | "
                            f"{cells(whole)} |")
                print(rows[-1], flush=True)
            db.close()
    return ["# Robust losses in the batch solve: the robust sweep against the plain one", "",
            f"Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1); loss scale = noise "
            f"sqrt({FS}), featureSize {FS}.  ms per round on the stream inside the library's kernels (events, "
            f"DOGLEG_AMD_BATCH_TIMING=1): the median over {a.reps} repeats of (ms of the call / its rounds), after 2 warm-up calls of "
            "each leg; per repeat plain, robust, plain again, in one process.  A/A spread: |plain again / plain - 1|.  The plain "
            "leg's kernels are those of the parent commit (the same instructions), so robust / plain is the cost of the robust sweep "
            "over the parent's plain kernel as measured in this run, on the MI355X it ran on, and nowhere else.", "",
            "| N | M | B | loss | every problem live: rounds plain / robust | plain ms/round | plain again | A/A spread | robust ms/round | robust / plain | "
            "whole solve: rounds plain / robust | plain ms/round | plain again | A/A spread | robust ms/round | robust / plain |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows


KEYS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def parse_remarks(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = cur.replace("(anonymous namespace)::", "").replace("void ", "")
            cur = re.sub(r"\(.*\)$", "", cur)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass", ln)
        if m and cur and m.group(1) in KEYS:
            out[cur][m.group(1)] = int(m.group(2))
    return out


def resources(new_path, parent_path):
    new, old = parse_remarks(new_path), parse_remarks(parent_path)
    head = "| kernel | " + " | ".join(KEYS) + " |"
    sep = "|---|" + "---|" * len(KEYS)
    fmt = lambda d: " | ".join(str(d[k]) for k in KEYS)
    robust = [f"| {k} | {fmt(v)} |" for k, v in new.items() if k.endswith(", true>")]
    both, moved = [], 0
    for k, v in old.items():
        if k.startswith("k_batch_finish"):
            continue                         # (its argument list grew: the robust form's weights)
        n = new.get(k.replace(">", ", false>") if k.startswith("k_batch_round") else k)
        same = n is not None and all(n[x] == v[x] for x in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"))
        moved += not same
        both.append(f"| {k} | {fmt(v)} | {fmt(n) if n else 'gone'} | {'equal' if same else 'MOVED'} |")
    return [MARK, "",
            "From the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags).", "",
            "### The new instantiations, k_batch_round<NMAX, FORM_J, ROBUST = true>: no scratch", ""] + [head, sep] + robust + [
            "", f"### The existing kernels of dense_batch.hip, parent commit against this tree: {moved} moved", "",
            "(k_batch_round<NMAX, FORM> is k_batch_round<NMAX, FORM, false> now; VGPRs, scratch and LDS decide \"equal\")", "",
            "| kernel | parent: " + " | ".join(KEYS) + " | this tree: " + " | ".join(KEYS) + " | |",
            "|---|" + "---|" * (2 * len(KEYS) + 1)] + both


def asm_functions(path):
    """{kernel: its instructions} of a device assembly listing (hipcc --offload-device-only -S), block labels unnumbered"""
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1).replace("Lb0EEEvNS_8BatchDevE", "EEvNS_8BatchDevE"), [])
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip())
            if t and not t.startswith("."):
                cur.append(t)
    return out


def same_instructions(new_path, parent_path):
    new, old = asm_functions(new_path), asm_functions(parent_path)
    names = [k for k in old if re.search(r"k_batch_(round|uncertainty|query)", k)]
    differ = [k for k in names if new.get(k) != old[k]]
    return ["", f"Instruction streams (hipcc --offload-device-only -S of both trees, block labels unnumbered): {len(names)} existing "
            f"instantiations of k_batch_round, k_batch_uncertainty and k_batch_query compared, {len(differ)} differ"
            + (": " + ", ".join(differ) if differ else ".")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--resources", nargs=2, metavar=("NEW_REMARKS", "PARENT_REMARKS"))
    ap.add_argument("--asm", nargs=2, metavar=("NEW_S", "PARENT_S"), help="with --resources: compare the kernels' instructions too")
    a = ap.parse_args()
    kept, tail = [], []
    if a.out and os.path.exists(a.out):
        lines = open(a.out).read().splitlines()
        cut = lines.index(MARK) if MARK in lines else len(lines)
        kept, tail = lines[:cut], lines[cut:]
    if a.resources:
        tail = resources(*a.resources) + (same_instructions(*a.asm) if a.asm else [])
    else:
        kept = bench(a) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(kept + tail) + "\n")


if __name__ == "__main__":
    main()
