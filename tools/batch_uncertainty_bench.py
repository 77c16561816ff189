#!/usr/bin/env python3
"""tools/batch_uncertainty_bench.py -- dogleg_amd_dense_batch_uncertainty on batches of the dense device test problem.

For the shapes (Nstate, Nmeas) = (6, 40) and (16, 96) and B = 1 ... 131072 problems (problems/batch.py, the default
generator settings), at the points a batch solve returned and with all three outputs asked for (feature size 2): wall time
of the call (median and range of the repeats after warm-up calls), and the time on the stream split into the callback's
kernels and the library's one launch (events, DOGLEG_AMD_BATCH_TIMING=1, in a call of its own), with the bytes the
launch must move -- J and x twice (both sweeps read them), the outputs once -- over its time.

The comparison: for the same B = 1024 problems, alternated in one process, the route that exists without this call
(tools/c/batch_uncertainty_route.c): per problem dogleg_optimize_dense2 from p[b] with a returnContext (parameters
under which the solve stays at p[b]: one evaluation, one step computed and not applied), then dogleg_amd_covariance_blocks and
dogleg_getOutliernessFactors.  Nothing is gated.

    python tools/batch_uncertainty_bench.py [--out profiles/batch_uncertainty.md] [--reps 7] [--max-b 131072]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from libdogleg_amd import capi                      # noqa: E402
from libdogleg_amd.ctypes_defs import dptr          # noqa: E402
from problems.batch import DeviceBatch              # noqa: E402

SHAPES = [(6, 40), (16, 96)]
BATCHES = [1, 64, 1024, 16384, 131072]
EPS, NOISE, SPREAD = 0.3, 0.01, 0.5
FS = 2
HBM_COPY_TBS = 6.29


def unc_call(db, p, lam, timing=False):
    if timing:
        os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    t = time.perf_counter()
    out = capi.dense_batch_uncertainty(p, db.N, db.M, db.cb, db.cookie, lam=lam, fs=FS)
    dt = time.perf_counter() - t
    os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert out["rc"] == 0 and not out["status"].any()
    return dt, out, capi.batch_uncertainty_last_stats()


def solved(N, M, B):
    db = DeviceBatch(B, M, N, seeds=1, eps=EPS, noise=NOISE, p0_spread=SPREAD)
    rc, p, res = capi.optimize_dense_batch(db.p0(), N, M, db.cb, db.cookie)
    assert rc == 0
    return db, p, np.ascontiguousarray(res["lambda_"])


def measure(N, M, B, reps, warm=2):
    db, p, lam = solved(N, M, B)
    for _ in range(warm):
        unc_call(db, p, lam)
    ts = [unc_call(db, p, lam)[0] for _ in range(reps)]
    _, _, st = unc_call(db, p, lam, timing=True)
    db.close()
    return dict(N=N, M=M, B=B, t=np.median(ts), tmin=min(ts), tmax=max(ts), ms_cb=st["ms_callback"], ms_lib=st["ms_library"],
                bytes=8.0 * B * (2 * M * N + 2 * M + N * N + N + M // FS + 3))


def route_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="bunc"), "libroute.so")
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "c", "batch_uncertainty_route.c"), "-o", so,
                    "-L", os.path.join(ROOT, "libdogleg_amd"), "-ldogleg_amd", "-L", os.path.join(ROOT, "problems"), "-lproblems",
                    "-lm", "-Wl,-rpath," + os.path.join(ROOT, "libdogleg_amd"), "-Wl,-rpath," + os.path.join(ROOT, "problems")],
                   check=True)
    capi.lib()                                       # (the same libdogleg_amd.so, loaded first)
    R = C.CDLL(so)
    D = C.POINTER(C.c_double)
    R.route_create.restype = C.c_void_p
    R.route_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_double]
    R.route_free.argtypes = [C.c_void_p]
    R.route_free.restype = None
    R.route_run.argtypes = [C.c_void_p, D, C.c_int, D, D]
    return R


def comparison(R, N, M, B, reps):
    db, p, lam = solved(N, M, B)
    h = R.route_create(M, N, B, 1, EPS, NOISE, SPREAD)
    cov, fac = np.zeros((B, N, N)), np.zeros((B, M // FS))

    def loop_leg(n=B):
        t = time.perf_counter()
        done = R.route_run(h, dptr(p), FS, dptr(cov), dptr(fac))
        dt = time.perf_counter() - t
        assert done == B
        return dt

    unc_call(db, p, lam)
    loop_leg()
    tb, tl = [], []
    for _ in range(reps):
        dt, out, _ = unc_call(db, p, lam)
        tb.append(dt)
        tl.append(loop_leg())
    d = np.sqrt(np.einsum("bii->bi", cov))
    ecov = float(np.max(np.abs(out["cov"] - cov) / (d[:, :, None] * d[:, None, :])))
    efac = float(np.max(np.abs(out["factors"] - fac) / np.maximum(np.abs(fac), 1e-3)))
    R.route_free(h)
    db.close()
    return dict(N=N, M=M, B=B, batch=np.median(tb), batch_rng=(min(tb), max(tb)), loop=np.median(tl), loop_rng=(min(tl), max(tl)),
                ecov=ecov, efac=efac)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    a = ap.parse_args()
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    out = ["# Per-problem covariance and outlierness factors of a batch: dogleg_amd_dense_batch_uncertainty", "",
           f"Device test problem (problems/batch.py: eps {EPS}, noise {NOISE}, p0_spread {SPREAD}, seed0 1) at the points a batch "
           f"solve with the default parameters returned; covariance, variances and factors (feature size {FS}) all asked for; wall "
           f"time: median (min .. max) of {a.reps} calls after 2 warm-up calls, with the staging of the inputs and the copies of the "
           "outputs to the caller's arrays; callback / library: events on the stream, in a call of their own; GB/s: "
           "8 (2 Nmeas (Nstate + 1) + Nstate^2 + Nstate + Nmeas / 2 + 3) bytes per problem over the library's time (copy ceiling of "
           f"the MI355X: {HBM_COPY_TBS} TB/s).", "",
           "| N | M | B | wall ms | callback us | library us | problems/s | library GB/s | of ceiling |",
           "|---|---|---|---|---|---|---|---|---|"]
    for N, M in SHAPES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            r = measure(N, M, B, a.reps if B < 100000 else max(3, a.reps // 2))
            gbs = r["bytes"] / (r["ms_lib"] * 1e-3) / 1e9 if r["ms_lib"] > 0 else float("nan")
            line = (f"| {N} | {M} | {B} | {r['t'] * 1e3:.3f} ({r['tmin'] * 1e3:.3f} .. {r['tmax'] * 1e3:.3f}) | {r['ms_cb'] * 1e3:.1f} | "
                    f"{r['ms_lib'] * 1e3:.1f} | {B / r['t']:.3g} | {gbs:.1f} | {100 * gbs / (HBM_COPY_TBS * 1e3):.2f} % |")
            print(line, flush=True)
            out.append(line)
    out += ["", "## The same 1024 problems: one call against the single-problem route", "",
            "Route: per problem dogleg_optimize_dense2 from p[b] with a returnContext (host callback, cache warm; max_iterations 1 "
            "and update_threshold 1e300, so that the solve stays at p[b]: both legs work at the same points), dogleg_amd_covariance_blocks for the full Sigma, dogleg_getOutliernessFactors; the two legs alternated in one "
            "process; the last two columns: the largest difference of the two legs' results (Sigma scaled by sqrt(S_ii S_jj), "
            "factors relative).", "",
            "| N | M | B | batch ms | route ms | route / batch | Sigma diff | factors diff |", "|---|---|---|---|---|---|---|---|"]
    R = route_lib()
    for N, M in SHAPES:
        c = comparison(R, N, M, 1024, 3)
        line = (f"| {N} | {M} | {c['B']} | {c['batch'] * 1e3:.2f} ({c['batch_rng'][0] * 1e3:.2f} .. {c['batch_rng'][1] * 1e3:.2f}) | "
                f"{c['loop'] * 1e3:.0f} ({c['loop_rng'][0] * 1e3:.0f} .. {c['loop_rng'][1] * 1e3:.0f}) | {c['loop'] / c['batch']:.0f} x | "
                f"{c['ecov']:.1e} | {c['efac']:.1e} |")
        print(line, flush=True)
        out.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
