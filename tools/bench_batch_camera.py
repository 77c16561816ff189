#!/usr/bin/env python3
"""Raw camera frames in the fused Poisson fit against pre-expanded doubles: B = 100 000 GAUSS2D 7 x 7 problems, POISSON.

  (a) dogleg_amd_optimize_dense_batch_model_mle_device on f64 data that were expanded beforehand, plus the time of that expansion
      (tools/micro/expand_u16.hip, one element a thread, timed apart by events: the plain kernel a caller would have to write)
  (b) dogleg_amd_optimize_dense_batch_camera_device on the uint16 readings, no calibration
  (c) the same with offset, gain and read-noise maps of a 2048 x 2048 sensor and random origins

Each leg: the whole solve (wall time around the call, which ends with its last synchronisation) and ms per round from
dogleg_amd_batch_last_stats (ms in the library's kernels / rounds).  WARMUP untimed solves, then REPEATS timed ones per leg, the
legs interleaved so that a drift of the machine hits all of them; reported: median, minimum and maximum.  (a) is also what shows
that the new template parameters left the existing form alone: run this file on the parent commit with --only-a and compare the
two medians against the spread.  Writes a markdown report with --out.  Needs a GPU."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

os.environ.setdefault("DOGLEG_AMD_BATCH_TIMING", "1")     # the library's own events around its kernels: ms per round comes from them
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libdogleg_amd import capi                                                      # noqa: E402
from libdogleg_amd.ctypes_defs import BatchResult, MODEL_GAUSS2D, LIKELIHOOD_POISSON  # noqa: E402
import ctypes as C                                                                   # noqa: E402

W = H = 7
M = W * H
N = 5
SENSOR = (2048, 2048)


def data(B, seed=1):
    rng = np.random.default_rng(seed)
    truth = np.stack([rng.uniform(200.0, 400.0, B), 3.0 + rng.uniform(-0.7, 0.7, B), 3.0 + rng.uniform(-0.7, 0.7, B),
                      rng.uniform(1.0, 1.6, B), rng.uniform(5.0, 15.0, B)], axis=1)
    ix, iy = np.tile(np.arange(W), H), np.repeat(np.arange(H), W)
    f = (truth[:, :1] * np.exp(-((ix - truth[:, 1:2]) ** 2 + (iy - truth[:, 2:3]) ** 2) / (2.0 * truth[:, 3:4] ** 2)) + truth[:, 4:5])
    counts = rng.poisson(f)
    p0 = truth * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, size=truth.shape))
    p0[:, 1:3] = truth[:, 1:3] + 0.3 * rng.uniform(-1.0, 1.0, size=(B, 2))
    return counts, p0, rng


def expand_lib():
    """tools/micro/expand_u16.hip as a shared library beside its source, built for gfx950 where it is missing or older"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "micro")
    src, so = os.path.join(here, "expand_u16.hip"), os.path.join(here, "libexpand_u16.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", so],
                       check=True)
    L = C.CDLL(so)
    L.expand_u16_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_float)]
    return L


def stats(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-B", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--only-a", action="store_true", help="the existing fused solve alone (runs on the parent commit too)")
    ap.add_argument("--out")
    a = ap.parse_args()
    B = a.B
    counts, p0, rng = data(B)
    legs = {}
    keep = []

    y64 = capi.DeviceArray(counts.astype(np.float64))
    model = capi.batch_model(MODEL_GAUSS2D, y64, M, W, H)
    legs["a"] = (lambda P, R: capi.optimize_dense_batch_model_mle_device(P.ptr, B, model, LIKELIHOOD_POISSON, None, R.ptr),
                 8 * B * M)
    if not a.only_a:
        from libdogleg_amd.ctypes_defs import DATA_U16
        raw = capi.DeviceArray(counts.astype(np.uint16))
        none = capi.batch_model(MODEL_GAUSS2D, None, M, W, H)
        cam_b = capi.batch_camera(none, DATA_U16, raw)
        legs["b"] = (lambda P, R: capi.optimize_dense_batch_camera_device(P.ptr, B, cam_b, LIKELIHOOD_POISSON, None, R.ptr), 2 * B * M)
        Ws, Hs = SENSOR
        off = (100.0 + 5.0 * rng.uniform(-1.0, 1.0, size=(Hs, Ws))).astype(np.float32)
        gi = rng.uniform(0.4, 2.5, size=(Hs, Ws)).astype(np.float32)
        rv = rng.uniform(0.5, 4.0, size=(Hs, Ws)).astype(np.float32)
        org = np.stack([rng.integers(0, Ws - W + 1, B), rng.integers(0, Hs - H + 1, B)], axis=1).astype(np.int32)
        win = lambda m: np.stack([m[oy:oy + H, ox:ox + W].reshape(-1) for ox, oy in org])
        adu = np.rint(counts / win(gi).astype(np.float64) + win(off).astype(np.float64)).astype(np.uint16)
        keep += [capi.DeviceArray(x) for x in (adu, off, gi, rv, org)]
        cam_c = capi.batch_camera(none, DATA_U16, keep[0], SENSOR, keep[1], keep[2], keep[3], keep[4])
        legs["c"] = (lambda P, R: capi.optimize_dense_batch_camera_device(P.ptr, B, cam_c, LIKELIHOOD_POISSON, None, R.ptr),
                     2 * B * M + 3 * 4 * Ws * Hs + 8 * B)

    R = capi.DeviceArray(nbytes=B * C.sizeof(BatchResult), dtype=np.uint8)
    wall = {k: [] for k in legs}
    per_round = {k: [] for k in legs}
    rounds = {}
    for it in range(a.warmup + a.repeats):
        for k, (call, _) in legs.items():
            P = capi.DeviceArray(p0)
            t0 = time.perf_counter()
            rc = call(P, R)
            t1 = time.perf_counter()
            assert rc == 0, (k, rc)
            st = capi.batch_last_stats()
            rounds[k] = st["rounds"]
            if it >= a.warmup:
                wall[k].append(1e3 * (t1 - t0))
                per_round[k].append(st["ms_library"] / max(st["rounds"], 1))
            P.free()
    # the expansion (a) needs on top: uint16 -> float64, B M values, the plain kernel of tools/micro/expand_u16.hip
    X = expand_lib()
    src, dst = capi.DeviceArray(counts.astype(np.uint16)), capi.DeviceArray(nbytes=8 * B * M)
    ms = (C.c_float * a.repeats)()
    rc = X.expand_u16_ms(src.ptr, dst.ptr, B * M, a.warmup, a.repeats, ms)
    if rc != 0:
        raise RuntimeError(f"expand_u16_ms: HIP error {rc}")
    assert np.array_equal(dst.numpy(), counts.astype(np.float64).reshape(-1))
    expand = stats(list(ms))

    lines = [f"# Raw camera frames: B = {B} GAUSS2D {W} x {H}, POISSON, {a.repeats} repeats after {a.warmup} warm-up solves", "",
             "median (min .. max), ms", "",
             "| leg | whole solve | ms per round | rounds | device bytes of data |", "|---|---|---|---|---|"]
    names = {"a": "(a) model_mle on pre-expanded f64", "b": "(b) camera, u16", "c": "(c) camera, u16 + maps + read noise"}
    for k in legs:
        lines.append(f"| {names[k]} | {stats(wall[k])} | {stats(per_round[k])} | {rounds[k]} | {legs[k][1]} |")
    lines += ["", f"expansion u16 -> f64 that (a) needs first, ms: {expand}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
