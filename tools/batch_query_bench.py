#!/usr/bin/env python3
"""tools/batch_query_bench.py -- dogleg_amd_dense_batch_query_covariance_device against the route that existed before it.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96), B = 1024, 16384 and 131072 problems of the dense device test problem
(problems/batch.py, the default generator settings) at the points a batch solve returned, Nq = 1 and 8 queries of Qrows = 2
rows per problem (seeded normal entries), the plain form Jq Sigma Jq^T:

  query   one call of dogleg_amd_dense_batch_query_covariance_device
  before  dogleg_amd_dense_batch_uncertainty_device with covariance [B][N][N] requested, then Jq Sigma Jq^T on the device with
          two torch.bmm and a synchronisation

Both legs are device-resident; their arrays are allocated and touched beforehand.  The quantity is the wall time of the leg, a
host clock around it (each leg ends synchronised).  Protocol: both legs on the same problems in one process, alternated --
query, before, query again per repeat, after warm-up calls of both.  The two query legs are an A/A pair: their medians differ
by nothing but the spread of the measurement, the yardstick for the verdict.  The time on the stream (the callback's kernels,
the library's; events, DOGLEG_AMD_BATCH_TIMING=1) comes from calls of their own after the timed ones.  The two legs' results
are compared (scaled as the tests scale their error).  Nothing is gated; the table is reported whichever way it falls.

    python tools/batch_query_bench.py [--out profiles/batch_query.md] [--reps 7] [--max-b 131072]

--out: the table replaces everything from the line "## Measured" on in that file (or is appended to it).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch                                    # before the library, which then binds to the HIP runtime torch loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                  # noqa: E402
from problems.batch import DeviceBatch                          # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1024, 16384, 131072]
NQS = [1, 8]
Q = 2
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
MARK = "## Measured"


class Legs:
    def __init__(self, db, p, lam, Nq):
        self.db, self.Nq = db, Nq
        B, N = db.B, db.N
        dev = dict(dtype=torch.float64, device="cuda")
        self.p = torch.from_numpy(np.ascontiguousarray(p)).cuda()
        self.lam0 = torch.from_numpy(np.ascontiguousarray(lam)).cuda()
        self.lam = self.lam0.clone()
        self.Jq = torch.from_numpy(np.random.default_rng([7, B, Nq, N]).standard_normal((B, Nq, Q, N))).cuda()
        self.out = torch.zeros((B, Nq, Q, Q), **dev)
        self.cov = torch.zeros((B, N, N), **dev)
        self.status = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.ref = None
        torch.cuda.synchronize()

    def reset(self):
        self.lam.copy_(self.lam0)
        torch.cuda.synchronize()

    def query(self):
        db = self.db
        return capi.dense_batch_query_covariance_device(self.p.data_ptr(), db.B, db.N, db.M, db.cb, db.cookie, self.Jq.data_ptr(),
                                                        self.Nq, Q, self.out.data_ptr(), self.status.data_ptr(), -1,
                                                        self.lam.data_ptr())

    def uncertainty(self):
        db = self.db
        return capi.dense_batch_uncertainty_device(self.p.data_ptr(), db.B, db.N, db.M, db.cb, db.cookie, self.status.data_ptr(),
                                                   self.lam.data_ptr(), self.cov.data_ptr())

    def before(self):
        db = self.db
        rc = self.uncertainty()
        T = torch.bmm(self.Jq.reshape(db.B, self.Nq * Q, db.N), self.cov).reshape(db.B * self.Nq, Q, db.N)
        self.ref = torch.bmm(T, self.Jq.reshape(db.B * self.Nq, Q, db.N).transpose(1, 2))
        torch.cuda.synchronize()
        return rc

    def difference(self):
        a, r = self.out.reshape(-1, Q, Q), self.ref
        d = torch.sqrt(torch.diagonal(r, dim1=1, dim2=2))
        return float(torch.max(torch.abs(a - r) / (d[:, :, None] * d[:, None, :])))


def clock(fn):
    t = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t
    assert rc == 0
    return dt


def with_timing(fn):
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    try:
        assert fn() == 0
    finally:
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    s = capi.batch_uncertainty_last_stats()
    return s["ms_callback"], s["ms_library"]


def measure(leg, reps, warm=2):
    for _ in range(warm):
        leg.reset()
        leg.query()
        leg.reset()
        leg.before()
    q1, bf, q2 = [], [], []
    diff = 0.0
    for _ in range(reps):
        leg.reset()
        q1.append(clock(leg.query))
        leg.reset()
        bf.append(clock(leg.before))
        diff = max(diff, leg.difference())
        leg.reset()
        q2.append(clock(leg.query))
    leg.reset()
    q_st = with_timing(leg.query)
    leg.reset()
    u_st = with_timing(leg.uncertainty)
    torch.cuda.synchronize()
    return dict(q1=q1, bf=bf, q2=q2, diff=diff, q_st=q_st, u_st=u_st)


def ms(ts):
    return f"{np.median(ts) * 1e3:.3f} ({min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f})"


def row(N, M, B, Nq, r):
    a, b, o = np.median(r["q1"]), np.median(r["q2"]), np.median(r["bf"])
    spread = abs(b / a - 1.0)
    verdict = "slower" if a > o * (1.0 + spread) else "faster" if o > a * (1.0 + spread) else "within the spread"
    return (f"| {N} | {M} | {B} | {Nq} | {ms(r['q1'])} | {ms(r['q2'])} | {100 * spread:.1f} % | {ms(r['bf'])} | {o / a:.2f} x | {verdict} | "
            f"{r['diff']:.1e} | {r['q_st'][0]:.3f} / {r['q_st'][1]:.3f} | {r['u_st'][0]:.3f} / {r['u_st'][1]:.3f} |")


HEAD = ["| N | M | B | Nq | query ms | query again ms | A/A spread | before ms | before / query | query leg | largest scaled difference | "
        "query: callback / library ms on the stream | before, its uncertainty call: callback / library ms |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    rows = []
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            reps = a.reps if B < 100000 else max(3, a.reps // 2 + 1)
            db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            rc, p, res = capi.optimize_dense_batch(db.p0(), N, M, db.cb, db.cookie, capi.default_parameters())
            assert rc == 0 and np.all(res["norm2_x"] >= 0)
            for Nq in NQS:
                leg = Legs(db, p, res["lambda_"], Nq)
                rows.append(row(N, M, B, Nq, measure(leg, reps)))
                print(rows[-1], flush=True)
                del leg
            db.close()
    out = [MARK, "",
           f"`tools/batch_query_bench.py`, one MI355X.  Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread "
           f"{SPREAD}, seed0 1) at the points a batch solve with the default parameters returned; Nq queries of {Q} rows, the plain "
           "form.  query: one call of `dogleg_amd_dense_batch_query_covariance_device`.  before: "
           "`dogleg_amd_dense_batch_uncertainty_device` with `covariance` requested, then Jq Sigma Jq^T by two `torch.bmm` and a "
           "synchronisation.  Wall time of the leg, a host clock around it: median (min .. max) of the repeats "
           f"({a.reps}; at B = 131072 fewer) after 2 warm-up calls of each leg; per repeat query, before, query again, in one "
           "process; every array exists and is touched before the clock starts.  A/A spread: |median(query again) / median(query) "
           "- 1|; the verdict on the query leg holds where the two medians differ by more than that.  Stream times: events "
           "(DOGLEG_AMD_BATCH_TIMING=1) in calls of their own.", ""] + HEAD + rows
    if a.out:
        old = open(a.out).read() if os.path.exists(a.out) else ""
        keep = old.split(MARK)[0]
        with open(a.out, "w") as f:
            f.write(keep + "\n".join(out) + "\n")


if __name__ == "__main__":
    main()
