#!/usr/bin/env python3
"""tools/batch_products_bounds_bench.py -- what a round of the bounded products batch solve costs over the plain products one.

For the shapes (Nstate, Nmeas) = (6, ragged 20 .. 90: M[b] = 20 + 7 b mod 71) and (16, 96), B = 1024, 16384 and 131072 problems
of the products device test problem (problems/batch.py: DeviceProductsBatch, the default generator settings, packed upper):
dogleg_amd_optimize_dense_products_batch_bounded against dogleg_amd_optimize_dense_products_batch on the same problems.  The
quantity is the time on the stream inside the library's kernels (events, DOGLEG_AMD_BATCH_TIMING=1) per round; the callback's
time is not in it.  The legs of a repeat, call by call in one process:

  plain             dogleg_amd_optimize_dense_products_batch
  infinite bounds   the bounded solve with lower = -inf, upper = +inf everywhere: the bounded kernel where nothing is ever held
                    or clamped (the same rounds and results as the plain leg)
  a third active    the bounded solve with a bound on the variables i = b mod 3 of problem b, half way between the start point and
                    the optimum of the plain solve (a lower bound where the start lies above the optimum, an upper bound where
                    below): those variables end on their bounds, held
  plain again       the A/A pair of the first leg: their medians differ by nothing but the spread of the measurement, the
                    yardstick for the ratios beside them

in two settings: max_iterations = 1 (every problem is evaluated twice, so both rounds take all B problems) and the whole solve
under the default parameters (the bounded solve converges linearly where it ends on a bound, so it runs more rounds with fewer
problems live in them: what a user sees, not a kernel comparison).  Nothing is gated and no ratio is fixed in advance.

    python tools/batch_products_bounds_bench.py [--out profiles/batch_products_bounds.md] [--reps 5] [--max-b 131072]

Every (shape, B) is a step: a child process of its own (--step N M B, M a number or MIN:MAX) under `timeout` (--step-timeout
seconds), one behind the other; the first step that fails, is killed or runs out of time ends the run, and no further step is
started.  The process that starts them never opens the device.

The part of --out from the line "## Kernel resources" on is kept as it is; it is written by
    python tools/batch_products_bounds_bench.py --resources NEW_REMARKS PARENT_REMARKS --asm NEW_S PARENT_S --out ...
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
from batch_bounds_bench import third_active                                             # noqa: E402
from batch_robust_bench import KEYS, parse_remarks, timed                               # noqa: E402

SHAPES = [(6, (20, 90)), (16, 96)]
BATCHES = [1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
MARK = "## Kernel resources"
CLASSES = (8, 16, 24, 32, 48, 64)


def rows_of(M, B):
    """M[b]: one number for all, or (Mmin, Mmax): Mmin + 7 b mod (Mmax - Mmin + 1)"""
    return np.full(B, M) if not isinstance(M, tuple) else M[0] + (7 * np.arange(B)) % (M[1] - M[0] + 1)


def params(**over):
    prm = capi.default_parameters()
    prm.JtJ_packed = prm.JtJ_upper = True
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def measure(db, prm, lo, hi, reps, warm=2):
    p0 = db.p0()
    inf = np.full_like(p0, np.inf)
    held_share = []

    def plain():
        return capi.optimize_dense_products_batch(p0, db.N, db.cb, db.cookie, prm)[0]

    def infinite():
        return capi.optimize_dense_products_batch_bounded(p0, db.N, db.cb, db.cookie, -inf, inf, prm)[0]

    def active():
        rc, _, _, held = capi.optimize_dense_products_batch_bounded(p0, db.N, db.cb, db.cookie, lo, hi, prm)
        held_share.append(float(np.mean(held != 0)))
        return rc

    for _ in range(warm):
        assert plain() == 0 and infinite() == 0 and active() == 0
    t = dict(plain=[], infinite=[], active=[], again=[])
    for _ in range(reps):
        t["plain"].append(timed(plain))
        t["infinite"].append(timed(infinite))
        t["active"].append(timed(active))
        t["again"].append(timed(plain))
    per = lambda xs: float(np.median([ms / n for ms, n in xs]))
    out = {k: per(v) for k, v in t.items()}
    out.update(rounds={k: v[0][1] for k, v in t.items()}, held=held_share[-1])
    return out


def cells(m):
    spread = abs(m["again"] / m["plain"] - 1.0)
    r = m["rounds"]
    return (f"{r['plain']} / {r['infinite']} / {r['active']} | {m['plain']:.4f} | {m['again']:.4f} | {100 * spread:.1f} % | "
            f"{m['infinite']:.4f} | {m['infinite'] / m['plain']:.2f} x | {m['active']:.4f} | {m['active'] / m['plain']:.2f} x | "
            f"{100 * m['held']:.0f} %")


def shape_name(M):
    return f"{M[0]}..{M[1]}" if isinstance(M, tuple) else str(M)


def step(N, M, B, reps):
    """one (shape, B) on the device: its row of the table, as a JSON line"""
    from problems.batch import DeviceProductsBatch
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    db = DeviceProductsBatch(B, rows_of(M, B), N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    p0 = db.p0()
    rc, pstar, _ = capi.optimize_dense_products_batch(p0, N, db.cb, db.cookie, params())
    assert rc == 0
    lo, hi = third_active(p0, pstar)
    live = measure(db, params(max_iterations=1), lo, hi, reps)
    whole = measure(db, params(), lo, hi, reps)
    db.close()
    print(json.dumps(dict(row=f"| {N} | {shape_name(M)} | {B} | {cells(live)} | {cells(whole)} |")), flush=True)


def bench(a):
    rows = []
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(N),
                   shape_name(M).replace("..", ":"), str(B), "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"step N = {N}, M = {shape_name(M)}, B = {B} ended with {r.returncode}: no further step is started")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1])["row"])
            print(rows[-1], flush=True)
    half = ("rounds plain / infinite / a third | plain ms/round | plain again | A/A spread | infinite bounds ms/round | infinite / plain | "
            "a third active ms/round | a third / plain | held at the end")
    return ["# Box bounds in the products batch solve: a round of the bounded solve against the plain products one", "",
            f"Products device test problem (problems/batch.py: DeviceProductsBatch, eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, "
            "seed0 1, packed upper; M 20..90: M[b] = 20 + 7 b mod 71).  ms per round on the stream inside the library's kernels "
            f"(events, DOGLEG_AMD_BATCH_TIMING=1; the callback is not in it): the median over {a.reps} repeats of (ms of the call / "
            "its rounds), after 2 warm-up calls of each leg; per repeat plain, infinite bounds, a third active, plain again, call "
            "by call in one process per row.  A/A spread: |plain again / plain - 1|.  Infinite bounds: the bounded kernel with "
            "nothing held or clamped.  A third active: a bound on the variables i = b mod 3 of problem b half way between the "
            "start and the plain solve's optimum; \"held at the end\" is the share of all variables held at the returned points.  "
            "The yardstick is the plain products round, whose instruction stream is the parent commit's (below).  The ratios are "
            "those of this run, on the MI355X it ran on, and nowhere else.", "",
            "| N | M | B | every problem live (max_iterations 1): " + half + " | whole solve: " + half + " |",
            "|---|---|---|" + "---|" * 18] + rows


def asm_functions(path):
    """{kernel: its instructions} of a device assembly listing (hipcc --offload-device-only -S), block labels unnumbered"""
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
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
    reordered = [k for k in differ if k in new and sorted(new[k]) == sorted(old[k])]
    added = [k for k in new if k not in old and "k_batch_" in k]
    return ["", f"Instruction streams (hipcc --offload-device-only -S of both trees, block labels unnumbered): {len(names)} existing "
            f"instantiations of k_batch_round, k_batch_uncertainty and k_batch_query compared, {len(names) - len(differ)} are the "
            f"same stream, {len(reordered)} hold the same instructions in another order, {len(differ) - len(reordered)} differ "
            f"otherwise.  Kernels this tree adds: {len(added)}."]


def resources(new_path, parent_path):
    new, old = parse_remarks(new_path), parse_remarks(parent_path)
    head = "| kernel | " + " | ".join(KEYS) + " |"
    sep = "|---|" + "---|" * len(KEYS)
    fmt = lambda d: " | ".join(str(d[k]) for k in KEYS)
    pairs, ok = [], True
    for c in CLASSES:
        for flag in ("false", "true"):
            k = f"k_batch_round<{c}, 1, false, {flag}>"
            pairs.append(f"| {k} | {fmt(new[k])} |")
        b, u = new[f"k_batch_round<{c}, 1, false, true>"], new[f"k_batch_round<{c}, 1, false, false>"]
        ok = ok and b["ScratchSize [bytes/lane]"] == 0 and b["LDS Size [bytes/block]"] == u["LDS Size [bytes/block]"]
    both, moved = [], 0
    for k, v in old.items():
        n = new.get(k)
        same = n is not None and all(n[x] == v[x] for x in KEYS)
        moved += not same
        both.append(f"| {k} | {fmt(v)} | {fmt(n) if n else 'gone'} | {'equal' if same else 'MOVED'} |")
    return [MARK, "",
            "From the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags).", "",
            "### The new instantiations, k_batch_round<NMAX, FORM_PRODUCTS = 1, ROBUST = false, BOUNDED = true>, each under its "
            "unbounded twin: " + ("no scratch, the LDS of the twin" if ok else "SCRATCH OR LDS DIFFER"), ""]\
        + [head, sep] + pairs + [
            "", f"### The existing kernels of dense_batch_kernels.hip, parent commit against this tree: {moved} moved", "",
            "(every figure of the table decides \"equal\")",
            "", "| kernel | parent: " + " | ".join(KEYS) + " | this tree: " + " | ".join(KEYS) + " | |",
            "|---|" + "---|" * (2 * len(KEYS) + 1)] + both


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a (shape, B) step may take")
    ap.add_argument("--step", nargs=3, metavar=("N", "M", "B"), help="run one step on the device and print its row (M: a number or MIN:MAX)")
    ap.add_argument("--resources", nargs=2, metavar=("NEW_REMARKS", "PARENT_REMARKS"))
    ap.add_argument("--asm", nargs=2, metavar=("NEW_S", "PARENT_S"), help="with --resources: compare the kernels' instructions too")
    a = ap.parse_args()
    if a.step:
        M = tuple(int(v) for v in a.step[1].split(":")) if ":" in a.step[1] else int(a.step[1])
        step(int(a.step[0]), M, int(a.step[2]), a.reps)
        return
    kept, tail = [], []
    if a.out and os.path.exists(a.out):
        lines = open(a.out).read().splitlines()
        cut = lines.index(MARK) if MARK in lines else len(lines)
        kept, tail = lines[:cut], lines[cut:]
    if a.resources:
        tail = resources(*a.resources) + (same_instructions(*a.asm) if a.asm else [])
        kept = kept or ["# Box bounds in the products batch solve: a round of the bounded solve against the plain products one", "",
                        "not measured", ""]
    else:
        kept = bench(a) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(kept + tail) + "\n")


if __name__ == "__main__":
    main()
