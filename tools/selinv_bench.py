#!/usr/bin/env python3
"""tools/selinv_bench.py -- the selected inverse (dlg_covariance_entries) on the benchmark configurations.

For each configuration, in one process: the factor at the starting point (lambda loop as the driver runs it), then
  * the whole structure of JtJ: sparse, every global, camera and point block, the globals against every camera and point
    and every observed camera x point block (lower triangle); dense, the whole lower triangle;
  * all diagonal blocks (global, camera and point blocks; dense: 6 x 6), lower triangle;
each timed on the first call (it builds the sweep's plan and the entry lookup; their host part is shown on its own) and
as the mean of the cached calls; and the same values from dlg_covariance_blocks, one request per block, timed on all of
its requests or on a random sample of them and then EXTRAPOLATED by request count (marked).  The two routes' values are
compared.  Prints a markdown table (--out: also written to that file).

    python tools/selinv_bench.py [--configs 2,3,4] [--sample 20000] [--reps 3] [--out profiles/selinv_table.md]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.covariance_bench import G, BC, BP, setup, timed      # noqa: E402


def _blocks(kind, prm, prob, Jp, Ji):
    """block requests (r0, nr, c0, nc) of each workload, as arrays"""
    if kind == "dense":
        N = prob.N
        v = np.arange(0, N - 5, 6)
        diag = np.stack([v, np.full_like(v, 6), v, np.full_like(v, 6)], 1)
        a, b = np.tril_indices(len(v))
        whole = np.stack([v[a], np.full_like(a, 6), v[b], np.full_like(a, 6)], 1)
        return {"whole structure": whole, "diagonal blocks": diag}
    Nc, Np = prm["Nc"], prm["Np"]
    cam0, pt0 = G, G + BC * Nc
    cams, pts = cam0 + BC * np.arange(Nc), pt0 + BP * np.arange(Np)
    diag = np.concatenate([[[0, G, 0, G]],
                           np.stack([cams, np.full(Nc, BC), cams, np.full(Nc, BC)], 1),
                           np.stack([pts, np.full(Np, BP), pts, np.full(Np, BP)], 1)])
    r = np.arange(0, prob.M, 2)
    obs = np.unique(np.stack([Ji[Jp[r] + G], Ji[Jp[r] + G + BC]], 1), axis=0)
    cross = np.concatenate([np.stack([cams, np.full(Nc, BC), np.zeros(Nc, int), np.full(Nc, G)], 1),
                            np.stack([pts, np.full(Np, BP), np.zeros(Np, int), np.full(Np, G)], 1),
                            np.stack([obs[:, 1], np.full(len(obs), BP), obs[:, 0], np.full(len(obs), BC)], 1)])
    return {"whole structure": np.concatenate([diag, cross]), "diagonal blocks": diag}


def _entries(req):
    """the lower entries (i >= j) of a list of blocks, in block order"""
    rows, cols = [], []
    for shape in np.unique(req[:, [1, 3]], axis=0):
        q = req[(req[:, 1] == shape[0]) & (req[:, 3] == shape[1])]
        a, b = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
        i = (q[:, 0, None] + a.ravel()[None, :]).ravel()
        j = (q[:, 2, None] + b.ravel()[None, :]).ravel()
        m = i >= j
        rows.append(i[m]); cols.append(j[m])
    return np.concatenate(rows).astype(np.int32), np.concatenate(cols).astype(np.int32)


def run(cfg, sample, reps):
    kind, prm, prob, be, Jp, Ji, lam = setup(cfg)
    rows = []
    rng = np.random.default_rng(0)
    for name, req in _blocks(kind, prm, prob, Jp, Ji).items():
        i, j = _entries(req)
        t = time.perf_counter()
        first = be.covariance_entries(0, i, j)
        t_first = time.perf_counter() - t
        t_plan, nsx, nfront = be.covariance_entries_stats()          # (of the first call: it built the plans)
        _, again, _, t_next = timed(lambda: be.covariance_entries(0, i, j), reps)
        assert np.array_equal(first, again)
        # the blocks route on the same values: all requests, or a sample extrapolated by request count
        extrap = len(req) > sample
        sub = req[rng.choice(len(req), sample, replace=False)] if extrap else req
        r0, nr, c0, nc = (np.ascontiguousarray(sub[:, k], dtype=np.int32) for k in range(4))
        _, _, _, t_blk = timed(lambda: be.covariance_blocks(0, r0, nr, c0, nc), max(1, reps // 2))
        blocks = be.covariance_blocks(0, r0, nr, c0, nc)
        bi, bj, bv = [], [], []
        for B, q in zip(blocks, sub):
            a, b = np.meshgrid(np.arange(q[1]) + q[0], np.arange(q[3]) + q[2], indexing="ij")
            m = a >= b
            bi.append(a[m]); bj.append(b[m]); bv.append(B[m])
        bi, bj, bv = (np.concatenate(v) for v in (bi, bj, bv))
        ev = be.covariance_entries(0, bi.astype(np.int32), bj.astype(np.int32))
        d = be.marginal_variances(0)
        diff = float(np.max(np.abs(ev - bv) / np.sqrt(d[bi] * d[bj])))
        t_blk_all = t_blk * len(req) / len(sub)
        rows.append(dict(cfg=cfg, kind=kind, N=prob.N, what=name, nval=len(i), nreq=len(req), t_first=t_first, t_plan=t_plan,
                         t_next=t_next, nsx=nsx, nfront=nfront, t_blk=t_blk_all, extrap=extrap, nsub=len(sub), diff=diff))
        print(rows[-1], flush=True)
    be.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3,4")
    ap.add_argument("--sample", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for c in [int(v) for v in a.configs.split(",")]:
        rows += run(c, a.sample, a.reps)
    lines = [f"`python tools/selinv_bench.py --configs {a.configs} --sample {a.sample} --reps {a.reps}`; largest scaled "
             f"difference between the two routes: {max(r['diff'] for r in rows):.1e}", "",
             "| config | workload | values | first call s (plan s) | next calls s | Sx values | front doubles | "
             "dlg_covariance_blocks: requests | blocks route s | speed-up |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        blk = f"{r['t_blk']:.3f}" + (f" (extrap. from {r['nsub']})" if r["extrap"] else "")
        lines.append(f"| #{r['cfg']} {r['kind']} N={r['N']} | {r['what']} | {r['nval']} | {r['t_first']:.4f} "
                     f"({r['t_plan']:.4f}) | {r['t_next']:.4f} | {r['nsx']} | {r['nfront']} | {r['nreq']} | {blk} | "
                     f"{r['t_blk'] / r['t_next']:.1f}x |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
