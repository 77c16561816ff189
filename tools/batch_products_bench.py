#!/usr/bin/env python3
"""tools/batch_products_bench.py -- the products form of a batch solve (dogleg_amd_optimize_dense_products_batch with the
fused callback of problems/device_batch_products.hip, packed upper) against the J form (dogleg_amd_optimize_dense_batch
with problems/device_batch_problems.hip) on the same problems, the two legs alternated in one process.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96) and B = 1 ... 131072: wall time of the call (median and range of the
repeats after warm-up calls), rounds, the time of a round split into the callback's kernels and the library's (events on
the stream, DOGLEG_AMD_BATCH_TIMING=1, in a call of its own), and the bytes each form moves per evaluated problem between
the callback and the library (written once, read once): 16 Nmeas (Nstate + 1) for the J form, 16 (1 + Nstate + Nstate
(Nstate + 1) / 2) for the products form.  Then a ragged row (Nstate 16, every problem its own Nmeas, 20 + 7 b mod 77: the
J form cannot run it) and a tall row (Nstate 6, Nmeas 4096, the largest power of two B whose x, J buffer stays under
--tall-gib).

    python tools/batch_products_bench.py [--out profiles/batch_products.md] [--reps 7] [--max-b 131072]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                                          # noqa: E402
from problems.batch import DeviceBatch, DeviceProductsBatch             # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1, 64, 1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
WARM = 2


def bytes_j(N, M):
    return 16.0 * M * (N + 1)


def bytes_products(N):
    return 16.0 * (1 + N + N * (N + 1) // 2)


class Leg:
    """one form on one batch"""

    def __init__(self, form, B, M, N):
        self.form, self.N = form, N
        if form == "products":
            self.db = DeviceProductsBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            self.prm = self.db.set_params(capi.default_parameters())
        else:
            self.db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
            self.prm = capi.default_parameters()
        self.p0 = self.db.p0()

    def call(self, timing=False):
        if timing:
            os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
        t = time.perf_counter()
        if self.form == "products":
            rc, p, res = capi.optimize_dense_products_batch(self.p0, self.N, self.db.cb, self.db.cookie, self.prm)
        else:
            rc, p, res = capi.optimize_dense_batch(self.p0, self.N, self.db.M, self.db.cb, self.db.cookie, self.prm)
        dt = time.perf_counter() - t          # (the call ends in a stream synchronisation and the read-back of the results)
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
        assert rc == 0 and np.all(res["status"] > 0) and np.all(res["norm2_x"] >= 0)
        return dt, p, res, capi.batch_last_stats()


def measure(legs, reps):
    """the legs alternated: WARM calls each, reps timed calls each, one call each with the stream events"""
    for _ in range(WARM):
        for leg in legs:
            leg.call()
    ts = {leg.form: [] for leg in legs}
    for _ in range(reps):
        for leg in legs:
            ts[leg.form].append(leg.call()[0])
    out = {}
    for leg in legs:
        _, p, res, st = leg.call(timing=True)
        t = ts[leg.form]
        out[leg.form] = dict(t=float(np.median(t)), tmin=min(t), tmax=max(t), rounds=st["rounds"], nev=int(res["evaluations"].sum()),
                             us_cb=st["ms_callback"] * 1e3 / st["rounds"], us_lib=st["ms_library"] * 1e3 / st["rounds"], p=p, res=res)
    return out


def row(N, Mtxt, B, form, r, nbytes):
    return (f"| {N} | {Mtxt} | {B} | {form} | {r['t'] * 1e3:.3f} ({r['tmin'] * 1e3:.3f} .. {r['tmax'] * 1e3:.3f}) | {r['rounds']} | "
            f"{r['us_cb']:.1f} | {r['us_lib']:.1f} | {nbytes:.0f} |")


def agree(r):
    """did the two forms solve the same problems the same way: (problems whose iterations, evaluations, status or lambda
    differ -- a decision on a rounding edge can fall either way in a large batch --, max |dp| over the others)"""
    a, b = r["products"], r["J"]
    same = np.ones(len(a["p"]), dtype=bool)
    for f in ("iterations", "evaluations", "status", "lambda_"):
        same &= a["res"][f] == b["res"][f]
    return int((~same).sum()), float(np.max(np.abs(a["p"][same] - b["p"][same])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--ragged-b", type=int, default=16384)
    ap.add_argument("--tall-gib", type=float, default=16.0)
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    head = ["| N | M | B | form | wall ms | rounds | callback us/round | library us/round | bytes / evaluated problem |",
            "|---|---|---|---|---|---|---|---|---|"]
    out = ["# The products form of a batch against the J form", "",
           f"Device test problems (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1), default parameters, "
           "packed upper JtJ; the two forms on the same problems, alternated call by call in one process; wall time: median "
           f"(min .. max) of {a.reps} calls after {WARM} warm-up calls, a host clock around the call (it ends in a stream "
           "synchronisation); callback / library: events on the stream, per round, in a call of their own; bytes: what passes "
           "between the callback and the library per evaluated problem, written once and read once (the state of "
           "Nstate (Nstate + 11) / 2 + 8 doubles a problem, the same in both forms, is not counted).", ""] + head
    worst, differ = 0.0, 0
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            legs = [Leg("products", B, M, N), Leg("J", B, M, N)]
            r = measure(legs, a.reps)
            nd, dp = agree(r)
            differ += nd
            worst = max(worst, dp)
            for form, nb in (("products", bytes_products(N)), ("J", bytes_j(N, M))):
                line = row(N, M, B, form, r[form], nb)
                print(line, flush=True)
                out.append(line)
            for leg in legs:
                leg.db.close()
    out += ["", f"Over all rows {differ} problems took different iterations, evaluations, status or lambda in the two forms; the end "
            f"points of all the others differ by at most {worst:.3g}.", "",
            "## A ragged batch: every problem its own number of measurements", "",
            "Nstate 16, M[b] = 20 + 7 b mod 77 (20 ... 90).  The J form takes one Nmeas for the whole batch and cannot run this.", ""] + head
    B = min(a.ragged_b, a.max_b)
    Ms = 20 + (7 * np.arange(B)) % 77
    leg = Leg("products", B, Ms, 16)
    r = measure([leg], a.reps)
    line = row(16, "20 .. 90", B, "products", r["products"], bytes_products(16))
    print(line, flush=True)
    out.append(line)
    leg.db.close()
    N, M = 6, 4096
    B = 1
    while 2 * B * 8.0 * M * (N + 1) <= a.tall_gib * 2 ** 30 and 2 * B <= a.max_b:
        B *= 2
    out += ["", "## A tall problem: Nstate 6, Nmeas 4096", "",
            f"B = {B}: the largest power of two at which the J form's x, J buffer (8 B Nmeas (Nstate + 1) = "
            f"{8.0 * B * M * (N + 1) / 2 ** 30:.1f} GiB) stays under {a.tall_gib:g} GiB; the products form's callback output at that B "
            f"is {8.0 * B * (1 + N + N * (N + 1) // 2) / 2 ** 20:.1f} MiB.", ""] + head
    legs = [Leg("products", B, M, N), Leg("J", B, M, N)]
    r = measure(legs, a.reps)
    nd, dp = agree(r)
    for form, nb in (("products", bytes_products(N)), ("J", bytes_j(N, M))):
        line = row(N, M, B, form, r[form], nb)
        print(line, flush=True)
        out.append(line)
    for leg in legs:
        leg.db.close()
    out += ["", f"{nd} problems differ in their decisions between the two forms; the end points of the others differ by at most {dp:.3g}."]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
