#!/usr/bin/env python3
"""tools/batch_bounds_bench.py -- what a round of the bounded batch solve costs over the plain one.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96), B = 1024, 16384 and 131072 problems of the dense device test problem
(problems/batch.py, the default generator settings): dogleg_amd_optimize_dense_batch_bounded against
dogleg_amd_optimize_dense_batch on the same problems.  The quantity is the time on the stream inside the library's kernels
(events, DOGLEG_AMD_BATCH_TIMING=1) per round.  The legs of a repeat, in one process:

  plain             dogleg_amd_optimize_dense_batch
  infinite bounds   the bounded solve with lower = -inf, upper = +inf everywhere: the bounded kernel where nothing is ever held
                    or clamped (the same rounds and results as the plain leg)
  a third active    the bounded solve with a bound on the variables i = b mod 3 of problem b, half way between the start point and
                    the optimum of the plain solve (a lower bound where the start lies above the optimum, an upper bound where
                    below): those variables end on their bounds, held
  plain again       the A/A pair of the first leg: their medians differ by nothing but the spread of the measurement, the
                    yardstick for the ratios beside them

in two settings: max_iterations = 1 (every problem is evaluated twice, so both rounds sweep all B problems) and the whole solve
under the default parameters (the bounded solve converges linearly where it ends on a bound, so it runs more rounds with fewer
problems live in them: what a user sees, not a kernel comparison).  Nothing is gated and no ratio is fixed in advance.

    python tools/batch_bounds_bench.py [--out profiles/batch_bounds.md] [--reps 5] [--max-b 131072]

The part of --out from the line "## Kernel resources" on is kept as it is; it is written by
    python tools/batch_bounds_bench.py --resources NEW_REMARKS PARENT_REMARKS [--asm NEW_S PARENT_S] --out profiles/batch_bounds.md
from two compilations of libdogleg_amd/csrc/dense_batch.hip with -Rpass-analysis=kernel-resource-usage (the build's flags
otherwise), of this tree and of its parent commit.
"""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libdogleg_amd import capi                                                          # noqa: E402
from batch_robust_bench import KEYS, parse_remarks, timed                               # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
MARK = "## Kernel resources"


def third_active(p0, pstar):
    """(lower, upper) (B, N): the module's docstring"""
    B, N = p0.shape
    lo, hi = np.full((B, N), -np.inf), np.full((B, N), np.inf)
    on = (np.arange(N)[None, :] % 3) == (np.arange(B)[:, None] % 3)
    mid = pstar + 0.5 * (p0 - pstar)
    above = p0 > pstar
    lo[on & above] = mid[on & above]
    hi[on & ~above] = mid[on & ~above]
    return lo, hi


def measure(db, prm, lo, hi, reps, warm=2):
    p0 = db.p0()
    inf = np.full_like(p0, np.inf)
    held_share = []

    def plain():
        return capi.optimize_dense_batch(p0, db.N, db.M, db.cb, db.cookie, prm)[0]

    def infinite():
        return capi.optimize_dense_batch_bounded(p0, db.N, db.M, db.cb, db.cookie, -inf, inf, None, prm)[0]

    def active():
        rc, _, _, held, _ = capi.optimize_dense_batch_bounded(p0, db.N, db.M, db.cb, db.cookie, lo, hi, None, prm)
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


def bench(a):
    from problems.batch import DeviceBatch
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    rows = []
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            p0 = db.p0()
            rc, pstar, _ = capi.optimize_dense_batch(p0, N, M, db.cb, db.cookie, capi.default_parameters())
            assert rc == 0
            lo, hi = third_active(p0, pstar)
            one = capi.default_parameters()
            one.max_iterations = 1
            live = measure(db, one, lo, hi, a.reps)
            whole = measure(db, capi.default_parameters(), lo, hi, a.reps)
            rows.append(f"| {N} | {M} | {B} | {cells(live)} | {cells(whole)} |")
            print(rows[-1], flush=True)
            db.close()
    half = ("rounds plain / infinite / a third | plain ms/round | plain again | A/A spread | infinite bounds ms/round | infinite / plain | "
            "a third active ms/round | a third / plain | held at the end")
    return ["# Box bounds in the batch solve: a round of the bounded solve against the plain one", "",
            f"Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1).  ms per round on the "
            f"stream inside the library's kernels (events, DOGLEG_AMD_BATCH_TIMING=1): the median over {a.reps} repeats of (ms of "
            "the call / its rounds), after 2 warm-up calls of each leg; per repeat plain, infinite bounds, a third active, plain "
            "again, in one process.  A/A spread: |plain again / plain - 1|.  Infinite bounds: the bounded kernel with nothing "
            "held or clamped.  A third active: a bound on the variables i = b mod 3 of problem b half way between the start and "
            "the plain solve's optimum; \"held at the end\" is the share of all variables held at the returned points.  The "
            "ratios are those of this run, on the MI355X it ran on, and nowhere else.", "",
            "| N | M | B | every problem live (max_iterations 1): " + half + " | whole solve: " + half + " |",
            "|---|---|---|" + "---|" * 18] + rows


def asm_functions(path, strip):
    """{kernel: its instructions} of a device assembly listing (hipcc --offload-device-only -S), block labels unnumbered; strip:
    the last template flag of k_batch_round (BOUNDED = false) dropped from the name, so that both trees name a kernel alike"""
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            cur = out.setdefault(name.replace("Lb0EEEvNS_8BatchDevE", "EEvNS_8BatchDevE") if strip else name, [])
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
    new, old = asm_functions(new_path, True), asm_functions(parent_path, False)
    names = [k for k in old if re.search(r"k_batch_(round|uncertainty|query)", k)]
    differ = [k for k in names if new.get(k) != old[k]]
    reordered = [k for k in differ if k in new and sorted(new[k]) == sorted(old[k])]
    return ["", f"Instruction streams (hipcc --offload-device-only -S of both trees, block labels unnumbered): {len(names)} existing "
            f"instantiations of k_batch_round, k_batch_uncertainty and k_batch_query compared, {len(names) - len(differ)} are the "
            f"same stream, {len(reordered)} hold the same instructions in another order, {len(differ) - len(reordered)} differ "
            "otherwise."]


def resources(new_path, parent_path):
    new, old = parse_remarks(new_path), parse_remarks(parent_path)
    head = "| kernel | " + " | ".join(KEYS) + " |"
    sep = "|---|" + "---|" * len(KEYS)
    fmt = lambda d: " | ".join(str(d[k]) for k in KEYS)
    bounded = [f"| {k} | {fmt(v)} |" for k, v in new.items() if k.startswith("k_batch_round") and k.endswith(", true>")]
    both, moved = [], 0
    for k, v in old.items():
        if k.startswith("k_batch_finish"):
            continue                         # (it writes held now)
        n = new.get(k.replace(">", ", false>") if k.startswith("k_batch_round") else k)
        same = n is not None and all(n[x] == v[x] for x in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"))
        moved += not same
        both.append(f"| {k} | {fmt(v)} | {fmt(n) if n else 'gone'} | {'equal' if same else 'MOVED'} |")
    return [MARK, "",
            "From the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags).", "",
            "### The new instantiations, k_batch_round<NMAX, FORM_J, ROBUST, BOUNDED = true>: no scratch, no LDS of their own", ""]\
        + [head, sep] + bounded + [
            "", f"### The existing kernels of dense_batch.hip, parent commit against this tree: {moved} moved", "",
            "(k_batch_round<NMAX, FORM, ROBUST> is k_batch_round<NMAX, FORM, ROBUST, false> now; VGPRs, scratch and LDS decide \"equal\")",
            "", "| kernel | parent: " + " | ".join(KEYS) + " | this tree: " + " | ".join(KEYS) + " | |",
            "|---|" + "---|" * (2 * len(KEYS) + 1)] + both


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
