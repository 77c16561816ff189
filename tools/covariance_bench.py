#!/usr/bin/env python3
"""tools/covariance_bench.py -- covariance blocks and marginal variances on the benchmark configurations.

For each configuration, in one process: the factor at the starting point (lambda loop as the driver runs it), then
  * all N marginal variances (dlg_marginal_variances);
  * every camera and point diagonal block (sparse; dense: every 6 x 6 diagonal block);
  * the camera x point blocks of 10 000 random observations (sparse; dense: 10 000 random 6 x 3 blocks);
each timed on the first call (it builds the plan; the host part of that is shown on its own) and as the mean of the
cached calls; the chunks of 16 variables and the supernodes each one visits; and the route the reference's users take
(dlg_solve_multi on unit columns, 16 per pass: a full forward and backward solve), timed on a sample of passes and
EXTRAPOLATED to the passes a workload needs (its distinct requested columns / 16).  Prints a markdown table (--out:
also written to that file).

    python tools/covariance_bench.py [--configs 3,4,2] [--sample 16] [--reps 3] [--out profiles/covariance.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                      # noqa: E402
from libdogleg_amd.ctypes_defs import dptr          # noqa: E402
from problems import BAProblem, DenseProblem        # noqa: E402

CONFIGS = {
    3: ("sparse", dict(Nc=499, Np=9000, Nobs=100000)),
    4: ("sparse", dict(Nc=2499, Np=45000, Nobs=500000)),
    2: ("dense", dict(M=50000, N=2000)),
}
G, BC, BP = 6, 6, 3


def setup(cfg):
    kind, prm = CONFIGS[cfg]
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
        Jp = Ji = None
        be = capi.Backend(capi.DLG_DENSE, prob.N, prob.M)
    be.set_p(0, p)
    be.upload(0, x, Jx)
    be.eval(0)
    lam, _ = be.gauss_newton(0, 0.0)
    return kind, prm, prob, be, Jp, Ji, lam


def workloads(kind, prm, prob, Jp, Ji):
    rng = np.random.default_rng(0)
    if kind == "sparse":
        Nc, Np = prm["Nc"], prm["Np"]
        cam0, pt0 = G, G + BC * Nc
        diag = [(cam0 + BC * c, BC, cam0 + BC * c, BC) for c in range(Nc)] + \
               [(pt0 + BP * q, BP, pt0 + BP * q, BP) for q in range(Np)]
        rows = 2 * rng.choice(prob.M // 2, 10000, replace=False)
        cross = []
        for r in rows:
            cols = Ji[Jp[r]:Jp[r + 1]]
            cross.append((int(cols[G]), BC, int(cols[G + BC]), BP))
    else:
        N = prob.N
        diag = [(v, 6, v, 6) for v in range(0, N - 5, 6)]
        a, b = rng.integers(0, N - 6, 10000), rng.integers(0, N - 3, 10000)
        cross = [(int(i), 6, int(j), 3) for i, j in zip(a, b)]
    return {"diagonal blocks": diag, "observed camera x point": cross}


def timed(fn, reps):
    t = time.perf_counter()
    first = fn()
    t_first = time.perf_counter() - t
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        again = fn()
        ts.append(time.perf_counter() - t)
    return first, again, t_first, float(np.mean(ts))


def run(cfg, sample, reps):
    kind, prm, prob, be, Jp, Ji, lam = setup(cfg)
    N = prob.N
    rows = []
    jobs = [("marginal variances", None)] + list(workloads(kind, prm, prob, Jp, Ji).items())
    for name, req in jobs:
        if req is None:
            fn = lambda: be.marginal_variances(0)              # noqa: E731
        else:
            r0, nr, c0, nc = (np.array(a, dtype=np.int32) for a in zip(*req))
            fn = lambda: np.concatenate([B.ravel() for B in be.covariance_blocks(0, r0, nr, c0, nc)])  # noqa: E731
        first, again, t_first, t_next = timed(fn, reps)
        assert np.array_equal(first, again)
        t_plan = be.covariance_plan_seconds()
        nch, visits, nsn = be.covariance_stats()
        # the unit-column route needs one pass per 16 distinct requested columns
        ncols = N if req is None else len({c0 + j for (_, _, c0, nc) in req for j in range(nc)})
        rows.append(dict(cfg=cfg, kind=kind, N=N, lam=lam, what=name, nreq=N if req is None else len(req), t_first=t_first,
                         t_plan=t_plan, t_next=t_next, nch=nch, reach=(visits / nch if kind == "sparse" else None), nsn=nsn,
                         npass=(ncols + 15) // 16))
        print(rows[-1], flush=True)
    # the unit-column route: dlg_solve_multi on 16 unit columns per pass, a sample of passes, extrapolated to the passes
    # each workload needs (its distinct requested columns / 16)
    ncols = 16 * sample
    cols = np.random.default_rng(1).choice(N, ncols, replace=False)
    E = np.zeros((16, N))
    X = np.zeros((16, N))
    be.L.dlg_solve_multi(be.h, 0, dptr(E), dptr(X), 16)   # (its scratch)
    t = time.perf_counter()
    for i in range(sample):
        E[:] = 0.0
        E[np.arange(16), cols[16 * i:16 * i + 16]] = 1.0
        assert be.L.dlg_solve_multi(be.h, 0, dptr(E), dptr(X), 16) == 0
    t_pass = (time.perf_counter() - t) / sample
    for r in rows:
        r["t_unit"] = t_pass * r["npass"]
        r["sample"] = sample
    be.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4,2")
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for c in [int(v) for v in a.configs.split(",")]:
        rows += run(c, a.sample, a.reps)
    lines = ["# Covariance blocks and marginal variances (dlg_covariance_blocks / dlg_marginal_variances)", "",
             "`python tools/covariance_bench.py` on one MI355X: the factor at the starting point, then each workload twice "
             "or more: the first call builds the plan (its host part in its own column), the next calls reuse it. "
             "The unit-column route is `dlg_solve_multi` with 16 unit right-hand sides per pass (a full forward and "
             f"backward solve), timed on {a.sample} passes and **extrapolated** to the passes of the row (its distinct "
             "requested columns / 16).", "",
             "| config | workload | requests | chunks | reach: supernodes per chunk / all | first call s (plan s) | "
             "next calls s | unit-column passes | unit-column route s (extrap.) | speed-up |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        reach = f"{r['reach']:.1f} / {r['nsn']}" if r["reach"] is not None else "-"
        lines.append(f"| #{r['cfg']} {r['kind']} N={r['N']} | {r['what']} | {r['nreq']} | {r['nch']} | {reach} | "
                     f"{r['t_first']:.4f} ({r['t_plan']:.4f}) | {r['t_next']:.4f} | {r['npass']} | {r['t_unit']:.2f} | "
                     f"{r['t_unit'] / r['t_next']:.0f}x |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
