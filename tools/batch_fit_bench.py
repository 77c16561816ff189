#!/usr/bin/env python3
"""tools/batch_fit_bench.py -- what the fit forms of the batch uncertainty and query calls cost.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96), B = 1024, 16384 and 131072 problems of the dense device test problem
(problems/batch.py, the default generator settings) at the points, with the lambda and with the weights a robust batch solve
returned (HUBER, scale = the noise sqrt(featureSize), featureSize 2), every third variable held (i mod 3 == b mod 3), for
dogleg_amd_dense_batch_uncertainty (covariance, variances and factors of feature size 2 asked for) and
dogleg_amd_dense_batch_query_covariance (8 queries of 2 rows, the plain form):

  plain    the call without _fit
  loss     ..._fit with the loss and the weights
  held     ..._fit with the held set
  both     ..._fit with all three
  recipe   the call without _fit behind problems/batch_rowscale.py, which multiplies the rows of x and J by sqrt(w) in a kernel
           of its own: how the uncertainty of a reweighted fit was had before the fit forms

The quantity is the time on the stream inside the library's launch (events, DOGLEG_AMD_BATCH_TIMING=1); for the comparison of
loss against recipe, the callback's kernels are added on both sides (the recipe's extra pass over x and J runs there).
Protocol: per repeat plain, loss, held, both, recipe, plain again, in one process, after warm-up calls of every leg; medians.
The two plain legs are an A/A pair: their medians differ by nothing but the spread of the measurement, the yardstick for the
ratios beside them.  Nothing is gated and no ratio is fixed in advance.

    python tools/batch_fit_bench.py [--out profiles/batch_fit.md] [--reps 7] [--max-b 131072]

--out: the tables replace everything up to the line "## Kernel resources" in that file, which is kept from there on.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                                          # noqa: E402
from libdogleg_amd.ctypes_defs import BatchLoss, LOSS_HUBER                             # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
FS, LFS, NQ, Q = 2, 2, 8, 2
MARK = "## Kernel resources"


def timed(fn):
    """(ms in the callback's kernels, ms in the library's launch) of one call"""
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    try:
        out = fn()
    finally:
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert out["rc"] == 0 and not out["status"].any()
    s = capi.batch_uncertainty_last_stats()
    return s["ms_callback"], s["ms_library"]


def measure(legs, reps, warm=2):
    """{leg: (median ms callback, median ms library)}; legs in the order they are called, the first once more at the end"""
    names = list(legs) + ["again"]
    fns = list(legs.values()) + [next(iter(legs.values()))]
    for _ in range(warm):
        for fn in fns[:-1]:
            assert fn()["rc"] == 0
    t = {n: [] for n in names}
    for _ in range(reps):
        for n, fn in zip(names, fns):
            t[n].append(timed(fn))
    return {n: tuple(float(np.median([v[k] for v in t[n]])) for k in (0, 1)) for n in names}


def row(N, M, B, call, m):
    lib = lambda n: m[n][1]
    tot = lambda n: m[n][0] + m[n][1]
    spread = abs(lib("again") / lib("plain") - 1.0)
    return (f"| {N} | {M} | {B} | {call} | {lib('plain'):.4f} | {lib('again'):.4f} | {100 * spread:.1f} % | "
            f"{lib('loss'):.4f} ({lib('loss') / lib('plain'):.2f} x) | {lib('held'):.4f} ({lib('held') / lib('plain'):.2f} x) | "
            f"{lib('both'):.4f} ({lib('both') / lib('plain'):.2f} x) | {tot('loss'):.4f} | {tot('recipe'):.4f} | "
            f"{tot('loss') / tot('recipe'):.2f} x |")


def bench(a):
    from problems.batch import DeviceBatch
    from problems.batch_rowscale import RowScaleDeviceBatch
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    rows = []
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            loss = BatchLoss(LOSS_HUBER, NOISE * float(np.sqrt(LFS)), LFS)
            rc, p, res, w = capi.optimize_dense_batch_robust(db.p0(), N, M, db.cb, db.cookie, loss, capi.default_parameters())
            assert rc == 0 and np.all(res["norm2_x"] >= 0)
            lam = np.ascontiguousarray(res["lambda_"])
            held = (np.arange(N)[None, :] % 3 == np.arange(B)[:, None] % 3).astype(np.uint8)
            Jq = np.random.default_rng(7).standard_normal((B, NQ, Q, N))
            rs = RowScaleDeviceBatch(db, w, LFS)
            fits = dict(plain=None, loss=capi.batch_fit(loss=loss, weights=w), held=capi.batch_fit(held=held),
                        both=capi.batch_fit(loss=loss, weights=w, held=held))
            unc = {n: (lambda f=f: capi.dense_batch_uncertainty(p, N, M, db.cb, db.cookie, lam=lam, fs=FS, fit=f)) for n, f in fits.items()}
            unc["recipe"] = lambda: capi.dense_batch_uncertainty(p, N, M, rs.cb, rs.cookie, lam=lam, fs=FS)
            qry = {n: (lambda f=f: capi.dense_batch_query_covariance(p, N, M, db.cb, db.cookie, Jq, lam=lam, fit=f)) for n, f in fits.items()}
            qry["recipe"] = lambda: capi.dense_batch_query_covariance(p, N, M, rs.cb, rs.cookie, Jq, lam=lam)
            # the legs agree before they are timed: loss against recipe bit for bit on Sigma and the query blocks
            assert unc["loss"]()["cov"].tobytes() == unc["recipe"]()["cov"].tobytes()
            assert qry["loss"]()["out"].tobytes() == qry["recipe"]()["out"].tobytes()
            for call, legs in (("uncertainty", unc), ("query", qry)):
                rows.append(row(N, M, B, call, measure(legs, a.reps)))
                print(rows[-1], flush=True)
            rs.close()
            db.close()
    return ["# The fit forms of the batch uncertainty and query calls against the calls without a fit, and against row scaling", "",
            f"Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1) at the points, lambda and "
            f"weights of a robust batch solve (HUBER, scale = noise sqrt({LFS}), featureSize {LFS}); held: the variables i with i mod 3 == "
            f"b mod 3.  uncertainty: covariance, variances and factors (feature size {FS}); query: {NQ} queries of {Q} rows, the plain "
            f"form.  ms on the stream (events, DOGLEG_AMD_BATCH_TIMING=1): the median over {a.reps} repeats after 2 warm-up calls of "
            "every leg; per repeat plain, loss, held, both, recipe, plain again, in one process.  A/A spread: |plain again / plain - 1| "
            "of the library's launch.  The plain leg's kernels have the instructions of the parent commit's (below).  loss + callback "
            "and recipe + callback: the callback's kernels and the library's launch together; the recipe's callback is the model's "
            "plus the pass that scales the rows.  Measured on the MI355X this ran on, and nowhere else.", "",
            "| N | M | B | call | plain ms | plain again | A/A spread | loss ms (/ plain) | held ms (/ plain) | both ms (/ plain) | "
            "loss + callback ms | recipe + callback ms | loss / recipe |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    a = ap.parse_args()
    tail = []
    if a.out and os.path.exists(a.out):
        lines = open(a.out).read().splitlines()
        tail = lines[lines.index(MARK):] if MARK in lines else []
    body = bench(a) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(body + tail) + "\n")


if __name__ == "__main__":
    main()
