#!/usr/bin/env python3
"""tools/query_covariance_bench.py -- query covariance (dlg_query_covariance) on the benchmark configurations.

For each configuration, in one process: the factor at the starting point (lambda loop as the driver runs it), then
  * 10 000 two-row queries on (globals, camera, point): half on observed camera x point pairs, half on random pairs
    (mostly unobserved); dense: two rows over 15 random variables each;
  * 1 000 sixteen-row queries of the same kind;
each timed on the first call (it builds the plan; the host part of that is shown on its own) and as the mean of the
cached calls, with the chunks of 16 rows and the supernodes each one visits; and the general route a caller has without
this call: dlg_solve_multi on the columns of Jq^T (16 per pass, a full forward and backward solve) plus the products
Jq X on the host, timed on a sample of passes and EXTRAPOLATED to the passes the workload needs (its rows / 16).
The observation form (nobs = all measurements) is timed on its own on the first 64 chunks of the two-row batch.

    python tools/query_covariance_bench.py [--configs 3,4,2] [--sample 16] [--reps 3] [--out profiles/query_covariance.md]
    python tools/query_covariance_bench.py --obs-only 4            (the observation form alone, for a kernel trace)
    python tools/query_covariance_bench.py --dump-existing FILE    (the outputs of the existing leverage and covariance
                                                                    calls, for a bitwise comparison of two libraries
                                                                    selected with DLG_TEST_LIB)
    python tools/query_covariance_bench.py --compare A B
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
    return kind, prm, prob, be, Jp, Ji, Jx, lam


def batch(kind, prm, prob, Jp, Ji, nq, fs, rng):
    """(qrow, rowptr, var, val) of nq queries of fs rows, 15 variables a row"""
    vs = []
    if kind == "sparse":
        cam0, pt0 = G, G + BC * prm["Nc"]
        rows = 2 * rng.choice(prob.M // 2, nq // 2, replace=False)
        pairs = [((int(Ji[Jp[r] + G]) - cam0) // BC, (int(Ji[Jp[r] + G + BC]) - pt0) // BP) for r in rows]
        pairs += [(int(c), int(q)) for c, q in zip(rng.integers(prm["Nc"], size=nq - len(pairs)),
                                                    rng.integers(prm["Np"], size=nq - len(pairs)))]
        for c, q in pairs:
            vs.append(np.r_[np.arange(G), cam0 + BC * c + np.arange(BC), pt0 + BP * q + np.arange(BP)])
    else:
        for _ in range(nq):
            vs.append(rng.choice(prob.N, 15, replace=False))
    var = np.concatenate([np.tile(v, fs) for v in vs]).astype(np.int32)
    rowptr = (15 * np.arange(nq * fs + 1)).astype(np.int32)
    qrow = (fs * np.arange(nq + 1)).astype(np.int32)
    val = rng.standard_normal(len(var))
    return qrow, rowptr, var, val


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


def solve_multi_pass_seconds(be, N, rowptr, var, val, sample):
    """dlg_solve_multi on 16 columns of Jq^T and the host product of those rows with the solved columns, per pass"""
    X = np.zeros((16, N))
    E = np.zeros((16, N))
    be.L.dlg_solve_multi(be.h, 0, dptr(E), dptr(X), 16)   # (its scratch)
    t = time.perf_counter()
    for i in range(sample):
        E[:] = 0.0
        for c in range(16):
            r = 16 * i + c
            np.add.at(E[c], var[rowptr[r]:rowptr[r + 1]], val[rowptr[r]:rowptr[r + 1]])
        assert be.L.dlg_solve_multi(be.h, 0, dptr(E), dptr(X), 16) == 0
        _ = E @ X.T
    return (time.perf_counter() - t) / sample


def run(cfg, sample, reps):
    kind, prm, prob, be, Jp, Ji, Jx, lam = setup(cfg)
    N = prob.N
    rng = np.random.default_rng(0)
    out = []
    for name, nq, fs in (("two-row queries", 10000, 2), ("16-row queries", 1000, 16)):
        qrow, rowptr, var, val = batch(kind, prm, prob, Jp, Ji, nq, fs, rng)
        fn = lambda: np.concatenate([B.ravel() for B in be.query_covariance(0, qrow, rowptr, var, val)])   # noqa: E731
        first, again, t_first, t_next = timed(fn, reps)
        assert np.array_equal(first, again)
        be.query_covariance(0, qrow, rowptr, var, val)
        nch, visits, nsn = be.query_covariance_stats()
        t_plan = 0.0
        # (the plan time of the first call: a fresh plan for the same arrays after another batch)
        be.query_covariance(0, qrow[:2], rowptr[:fs + 1], var[:15 * fs], val[:15 * fs])
        be.query_covariance(0, qrow, rowptr, var, val)
        t_plan = be.query_covariance_plan_seconds()
        t_pass = solve_multi_pass_seconds(be, N, rowptr, var, val, sample)
        npass = (nq * fs + 15) // 16
        r = dict(cfg=cfg, kind=kind, N=N, lam=lam, what=name, nq=nq, t_first=t_first, t_plan=t_plan, t_next=t_next,
                 nch=nch, reach=(visits / nch if visits else None), nsn=nsn, npass=npass, t_multi=t_pass * npass,
                 sample=sample)
        if fs == 2:
            # the observation form on the first 64 chunks (512 queries)
            k = 512
            q2 = (qrow[:k + 1], rowptr[:2 * k + 1], var[:rowptr[2 * k]], val[:rowptr[2 * k]])
            _, _, _, t_obs = timed(lambda: be.query_covariance(0, *q2, nobs=prob.M), reps)
            r["t_obs_chunk"] = t_obs / 64
        out.append(r)
        print(r, flush=True)
    be.close()
    return out


def obs_only(cfg, reps):
    kind, prm, prob, be, Jp, Ji, Jx, lam = setup(cfg)
    qrow, rowptr, var, val = batch(kind, prm, prob, Jp, Ji, 512, 2, np.random.default_rng(0))
    for _ in range(reps):
        be.query_covariance(0, qrow, rowptr, var, val, nobs=prob.M)
    print(f"config #{cfg}: {reps} calls of 64 chunks in the observation form")
    be.close()


def dump_existing(path):
    """the outputs of the existing leverage and covariance calls on config #3 and a dense problem"""
    res = {}
    kind, prm, prob, be, Jp, Ji, Jx, lam = setup(3)
    rng = np.random.default_rng(3)
    res["s_lev1"] = be.feature_leverage(0, 1, 0, 20000)
    res["s_lev2"] = be.feature_leverage(0, 2, 0, 20000)
    res["s_out2"] = be.outlierness_factors(0, 2, 20000, 1.0)
    res["s_out1"] = be.outlierness_factors(0, 1, 20000, 1.0)
    Nc, Np = prm["Nc"], prm["Np"]
    cam0, pt0 = G, G + BC * Nc
    req = [(cam0 + BC * c, BC, pt0 + BP * q, BP) for c, q in zip(rng.integers(Nc, size=2000), rng.integers(Np, size=2000))]
    req += [(pt0 + BP * q, BP, pt0 + BP * q, BP) for q in range(0, Np, 7)]
    r0, nr, c0, nc = (np.array(a, dtype=np.int32) for a in zip(*req))
    res["s_blocks"] = np.concatenate([B.ravel() for B in be.covariance_blocks(0, r0, nr, c0, nc)])
    res["s_var"] = be.marginal_variances(0)
    rows = 2 * rng.choice(prob.M // 2, 5000, replace=False)
    ii = np.array([Ji[Jp[r] + G] for r in rows], dtype=np.int32)
    jj = np.array([Ji[Jp[r] + G + BC] for r in rows], dtype=np.int32)
    res["s_entries"] = be.covariance_entries(0, ii, jj)
    be.close()
    dp = DenseProblem(4000, 300, seed=2)
    p = dp.p0()
    x, J = dp.eval(p)
    be = capi.Backend(capi.DLG_DENSE, dp.N, dp.M)
    be.set_p(0, p)
    be.upload(0, x, J)
    be.eval(0)
    assert be.factorize(0, 1e-3)
    res["d_lev2"] = be.feature_leverage(0, 2, 0, 2000)
    req = [(int(a), 6, int(b), 3) for a, b in zip(rng.integers(0, dp.N - 6, 500), rng.integers(0, dp.N - 3, 500))]
    r0, nr, c0, nc = (np.array(a, dtype=np.int32) for a in zip(*req))
    res["d_blocks"] = np.concatenate([B.ravel() for B in be.covariance_blocks(0, r0, nr, c0, nc)])
    res["d_var"] = be.marginal_variances(0)
    res["d_entries"] = be.covariance_entries(0, rng.integers(0, dp.N, 3000).astype(np.int32),
                                             rng.integers(0, dp.N, 3000).astype(np.int32))
    be.close()
    np.savez(path, **res)
    print(f"{path}: {', '.join(f'{k} ({len(v)})' for k, v in res.items())}")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in A.files:
        same = A[k].shape == B[k].shape and np.array_equal(A[k].view(np.uint64), B[k].view(np.uint64))
        print(f"{k}: {A[k].size} values, {'bitwise equal' if same else 'DIFFERENT'}")
        bad += not same
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="3,4,2")
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--obs-only", type=int, default=None)
    ap.add_argument("--dump-existing", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    a = ap.parse_args()
    if a.obs_only is not None:
        return obs_only(a.obs_only, a.reps)
    if a.dump_existing:
        return dump_existing(a.dump_existing)
    if a.compare:
        sys.exit(1 if compare(*a.compare) else 0)
    rows = []
    for c in [int(v) for v in a.configs.split(",")]:
        rows += run(c, a.sample, a.reps)
    lines = ["| config | workload | queries | chunks | reach: supernodes per chunk / all | first call s (plan s) | "
             "next calls s | solve_multi passes | solve_multi + host product s (extrap.) | speed-up | "
             "observation form s per chunk |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        reach = f"{r['reach']:.1f} / {r['nsn']}" if r["reach"] is not None else "-"
        obs = f"{r['t_obs_chunk'] * 1e3:.3f} ms" if "t_obs_chunk" in r else "-"
        lines.append(f"| #{r['cfg']} {r['kind']} N={r['N']} | {r['what']} | {r['nq']} | {r['nch']} | {reach} | "
                     f"{r['t_first']:.4f} ({r['t_plan']:.4f}) | {r['t_next']:.4f} | {r['npass']} | {r['t_multi']:.2f} | "
                     f"{r['t_multi'] / r['t_next']:.0f}x | {obs} |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
