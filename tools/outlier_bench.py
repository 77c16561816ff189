#!/usr/bin/env python3
"""tools/outlier_bench.py -- the leverage blocks of the outlier API on the benchmark configurations.

For each configuration, in one process: the factor at the starting point (lambda loop as the driver runs it), then
  * all features through dlg_outlierness_factors (the path of dogleg_getOutliernessFactors): the first call (it builds
    the sparse reach plan) and the mean of the next ones;
  * a sample of chunks of 16 measurement rows through dlg_pseudoinverse_chunk (a full forward and backward solve per
    chunk, the reference's route) -- the solve alone, its Gram product not counted --, extrapolated to all features;
  * sparse: the supernodes a chunk visits (its reach) against the supernodes of the factor.
Prints a markdown table (--out: also written to that file).

    python tools/outlier_bench.py [--configs 3,4,2] [--sample 64] [--reps 3] [--out profiles/outliers.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                      # noqa: E402
from problems import BAProblem, DenseProblem        # noqa: E402

CONFIGS = {
    3: ("sparse", dict(Nc=499, Np=9000, Nobs=100000), 2),
    4: ("sparse", dict(Nc=2499, Np=45000, Nobs=500000), 2),
    2: ("dense", dict(M=50000, N=2000), 1),
}


def setup(cfg):
    kind, prm, fs = CONFIGS[cfg]
    if kind == "sparse":
        prob = BAProblem(prm["Nc"], prm["Np"], prm["Nobs"], seed=1)
        p = prob.p0()
        x, Jx = prob.eval(p)
        Jp, Ji = prob.pattern()
        be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
        be.set_pattern(Jp, Ji)
    else:
        prob = DenseProblem(prm["M"], prm["N"], seed=1)
        p = prob.p0()
        x, Jx = prob.eval(p)
        be = capi.Backend(capi.DLG_DENSE, prob.N, prob.M)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    n2x, _ = be.eval(0)
    lam, _ = be.gauss_newton(0, 0.0)
    return kind, fs, prob, be, n2x, lam


def run(cfg, sample, reps):
    kind, fs, prob, be, n2x, lam = setup(cfg)
    nf = prob.M // fs
    scale = 1.0
    t = time.perf_counter()
    f_first = be.outlierness_factors(0, fs, nf, scale)
    t_first = time.perf_counter() - t
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f = be.outlierness_factors(0, fs, nf, scale)
        ts.append(time.perf_counter() - t)
    assert np.array_equal(f, f_first)
    t_new = float(np.mean(ts))
    # the reference's route: a full solve per chunk of 16 rows
    nch = (nf * fs + 15) // 16
    chunks = np.random.default_rng(0).choice(nch, min(sample, nch), replace=False)
    be.pseudoinverse_chunk(0, 0, 16)                  # (its scratch)
    t = time.perf_counter()
    for c in chunks:
        be.pseudoinverse_chunk(0, int(c) * 16, min(int(c) * 16 + 16, nf * fs))
    t_pi = (time.perf_counter() - t) / len(chunks) * nch
    row = dict(cfg=cfg, kind=kind, fs=fs, N=prob.N, M=prob.M, nf=nf, lam=lam, t_first=t_first, t_new=t_new,
               t_pi=t_pi, sample=len(chunks), nch=nch)
    if kind == "sparse":
        nchunks, visits, nsn = be.leverage_stats(fs)
        row.update(reach=visits / nchunks, nsn=nsn, nnzL=be.stats()["nnz_L"])
    be.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4,2")
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for c in [int(v) for v in a.configs.split(",")]:
        r = run(c, a.sample, a.reps)
        rows.append(r)
        print(r, flush=True)
    lines = ["# Outlierness factors of every feature (dogleg_getOutliernessFactors' device path)", "",
             "`python tools/outlier_bench.py` on one MI355X: the factor at the starting point, then all features through "
             "`dlg_outlierness_factors`; the reference's route is a full forward and backward solve per chunk of 16 rows "
             f"(`dlg_pseudoinverse_chunk`, the solve alone), timed on {a.sample} random chunks and extrapolated.", "",
             "| config | features (size) | N | first call s | next calls s | pseudo-inverse route s (extrap.) | speed-up | "
             "reach: supernodes per chunk / all |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        reach = f"{r['reach']:.1f} / {r['nsn']} ({100.0 * r['reach'] / r['nsn']:.3f} %)" if "reach" in r else "-"
        lines.append(f"| #{r['cfg']} {r['kind']} | {r['nf']} ({r['fs']}) | {r['N']} | {r['t_first']:.3f} | {r['t_new']:.3f} | "
                     f"{r['t_pi']:.2f} | {r['t_pi'] / r['t_new']:.1f}x | {reach} |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
