#!/usr/bin/env python3
"""tools/batch_model_bench.py -- what a round of the fused model solve costs against the same solve through the adapter callback.

For GAUSS2D on a 7 x 7 window and EXPDECAY with M = 40, B = 1024, 16384 and 131072 problems (the data of
tests/batch_models_np.py: the problems of seeds 1 .. 1024, repeated to B): dogleg_amd_optimize_dense_batch_model against
dogleg_amd_optimize_dense_batch with dogleg_amd_batch_model_callback on the same data in device memory.  The quantity is the time
on the stream per round (events, DOGLEG_AMD_BATCH_TIMING=1): for the adapter route the callback's launch PLUS k_batch_round, for
the fused solve its one launch.  The legs of a repeat, call by call in one process:

  fused             dogleg_amd_optimize_dense_batch_model
  adapter           dogleg_amd_optimize_dense_batch through dogleg_amd_batch_model_callback (callback ms and library ms apart)
  fused again       the A/A pair of the first leg: the yardstick for the ratio beside it

in two settings: max_iterations = 1 (every problem is evaluated twice, so both rounds take all B problems) and the whole solve
under the default parameters.  Beside them: the bytes a fused round must move at the least (y, 8 B M, and the state it reads and
writes, 2 * 8 B (N (N + 11) / 2 + 8) at the most) against a device-to-device copy of y (hipMemcpyAsync between two events, the
median of the same number of repeats), which reads and writes 8 B M bytes each.  Nothing is gated and no ratio is fixed in
advance.  A "## Reading" section written by hand behind the resources is replaced with them: write it again after --resources.

    python tools/batch_model_bench.py [--out profiles/batch_model.md] [--reps 5] [--max-b 131072]

Every (case, B) is a step: a child process of its own (--step KIND B) under `timeout` (--step-timeout seconds), one behind the
other; the first step that fails, is killed or runs out of time ends the run, and no further step is started.  The process that
starts them never opens the device.

The part of --out from the line "## Kernel resources" on is kept as it is; it is written by
    python tools/batch_model_bench.py --resources NEW_REMARKS PARENT_REMARKS --asm NEW_S PARENT_S --out ...
from two compilations of libdogleg_amd/csrc/dense_batch_kernels.hip with --offload-device-only -S
-Rpass-analysis=kernel-resource-usage (the build's flags otherwise), of this tree and of its parent commit.
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from libdogleg_amd import capi                                                          # noqa: E402
from libdogleg_amd.ctypes_defs import MODEL_EXPDECAY, MODEL_GAUSS2D, MODEL_NSTATE       # noqa: E402
from batch_products_bounds_bench import asm_functions                                   # noqa: E402
from batch_robust_bench import KEYS, parse_remarks                                      # noqa: E402

CASES = {"gauss2d": (MODEL_GAUSS2D, (7, 7)), "expdecay": (MODEL_EXPDECAY, 40)}
BATCHES = [1024, 16384, 131072]
DISTINCT = 1024
MARK = "## Kernel resources"
TITLE = "# Built-in models in the batch solve: a round of the fused solve against the adapter route"


def timed(fn):
    """(ms in the callback's kernels, ms in the library's kernels, rounds) of one call"""
    os.environ["DOGLEG_AMD_BATCH_TIMING"] = "1"
    try:
        rc = fn()
    finally:
        os.environ.pop("DOGLEG_AMD_BATCH_TIMING", None)
    assert rc == 0
    s = capi.batch_last_stats()
    return s["ms_callback"], s["ms_library"], s["rounds"]


def params(**over):
    prm = capi.default_parameters()
    for k, v in over.items():
        setattr(prm, k, v)
    return prm


def measure(rec, cb, cookie, N, M, p0, prm, reps, warm=2):
    def fused():
        return capi.optimize_dense_batch_model(p0, rec, params=prm)[0]

    def adapter():
        return capi.optimize_dense_batch(p0, N, M, cb, cookie, prm)[0]

    for _ in range(warm):
        assert fused() == 0 and adapter() == 0
    t = dict(fused=[], adapter=[], again=[])
    for _ in range(reps):
        t["fused"].append(timed(fused))
        t["adapter"].append(timed(adapter))
        t["again"].append(timed(fused))
    med = lambda xs, f: float(np.median([f(x) for x in xs]))
    return dict(fused=med(t["fused"], lambda x: x[1] / x[2]), again=med(t["again"], lambda x: x[1] / x[2]),
                adapter_cb=med(t["adapter"], lambda x: x[0] / x[2]), adapter_lib=med(t["adapter"], lambda x: x[1] / x[2]),
                rounds=(t["fused"][0][2], t["adapter"][0][2]))


def cells(m):
    route = m["adapter_cb"] + m["adapter_lib"]
    spread = abs(m["again"] / m["fused"] - 1.0)
    return (f"{m['rounds'][0]} / {m['rounds'][1]} | {m['fused']:.4f} | {m['again']:.4f} | {100 * spread:.1f} % | {m['adapter_cb']:.4f} | "
            f"{m['adapter_lib']:.4f} | {route:.4f} | {route / m['fused']:.2f} x | {m['adapter_lib'] / m['fused']:.2f} x")


def copy_ms(nbytes, reps):
    """the median ms of a device-to-device copy of nbytes (reads and writes that much)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    V = C.c_void_p
    hip.hipMemcpyAsync.argtypes = [V, V, C.c_size_t, C.c_int, V]
    hip.hipEventRecord.argtypes = [V, V]
    hip.hipEventSynchronize.argtypes = [V]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), V, V]
    src, dst = capi.DeviceArray(nbytes=nbytes), capi.DeviceArray(nbytes=nbytes)
    a, b = V(), V()
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    ms = []
    for k in range(reps + 2):
        assert hip.hipEventRecord(a, None) == 0
        assert hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None) == 0            # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(b, None) == 0 and hip.hipEventSynchronize(b) == 0
        t = C.c_float(0.0)
        assert hip.hipEventElapsedTime(C.byref(t), a, b) == 0
        if k >= 2:
            ms.append(t.value)
    hip.hipEventDestroy(a)
    hip.hipEventDestroy(b)
    return float(np.median(ms))


def step(name, B, reps):
    """one (case, B) on the device: its row of the table, as a JSON line"""
    from tests import batch_models_np as mz
    assert capi.lib().dlg_device_count() > 0, "needs a GPU"
    case = CASES[name]
    bt = mz.batch(case, seed0=1, nb=min(B, DISTINCT))
    tile = lambda a: np.ascontiguousarray(np.tile(a, ((B + len(a) - 1) // len(a), 1))[:B])
    y, p0 = tile(bt["y"]), tile(bt["p0"])
    N, M = MODEL_NSTATE[bt["kind"]], bt["M"]
    yd = capi.DeviceArray(y)
    rec = capi.batch_model(bt["kind"], yd, M, bt["width"], bt["height"])
    cb, cookie, _, _ = capi.batch_model_callback(rec)
    live = measure(rec, cb, cookie, N, M, p0, params(max_iterations=1), reps)
    whole = measure(rec, cb, cookie, N, M, p0, params(), reps)
    ybytes, state = 8 * B * M, 8 * B * (N * (N + 11) // 2 + 8)
    cms = copy_ms(ybytes, reps)
    mem = (f"{ybytes / 1e6:.1f} | {2 * state / 1e6:.1f} | {8 * B * M * (N + 1) / 1e6:.1f} | {cms:.4f} | {2 * ybytes / cms / 1e6:.0f} | "
           f"{live['fused'] / cms:.1f} x")
    print(json.dumps(dict(row=f"| {name} | {N} | {M} | {B} | {cells(live)} | {cells(whole)} | {mem} |")), flush=True)


def bench(a):
    rows = []
    for name in CASES:
        for B in BATCHES:
            if B > a.max_b:
                continue
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, str(B),
                   "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"step {name}, B = {B} ended with {r.returncode}: no further step is started")
            rows.append(json.loads(r.stdout.strip().splitlines()[-1])["row"])
            print(rows[-1], flush=True)
    half = ("rounds fused / adapter | fused ms/round | fused again | A/A spread | adapter: callback ms/round | adapter: k_batch_round "
            "ms/round | adapter route ms/round | route / fused | k_batch_round alone / fused")
    return [TITLE, "",
            "GAUSS2D on a 7 x 7 window and EXPDECAY with M = 40 (tests/batch_models_np.py, the problems of seeds 1 .. 1024 repeated to "
            "B, no scale, t_i = i).  ms per round on the stream (events, DOGLEG_AMD_BATCH_TIMING=1): the median over "
            f"{a.reps} repeats of (ms of the call / its rounds), after 2 warm-up calls of each leg; per repeat fused, adapter, fused "
            "again, call by call in one process per row.  A/A spread: |fused again / fused - 1|.  The adapter route is the "
            "callback's launch plus k_batch_round<8, FORM_J>; \"route / fused\" above 1 means the fused round is faster.  Memory: the "
            "bytes of y, the most a round reads and writes of the state, the x / J buffer the adapter route allocates and the fused "
            "solve does not, a device-to-device copy of y (reads and writes the bytes of y) and the fused every-problem-live round "
            "against it.  The figures are those of this run, on the MI355X it ran on, and nowhere else.", "",
            "| model | N | M | B | every problem live (max_iterations 1): " + half + " | whole solve: " + half +
            " | y MB | state read + written MB (at most) | x / J buffer not allocated MB | copy of y ms | copy GB/s | fused live round / copy |",
            "|---|---|---|---|" + "---|" * 24] + rows


def resources(new_path, parent_path, asm):
    new, old = parse_remarks(new_path), parse_remarks(parent_path)
    fmt = lambda d: " | ".join(str(d[k]) for k in KEYS)
    names = ["k_batch_round<8, 0, false, false>", "k_batch_round<8, 2, false, false>", "k_batch_round<8, 0, false, true>",
             "k_batch_round<8, 2, false, true>", "k_batch_round<8, 0, true, false>"]
    moved = [k for k, v in old.items() if k not in new or any(new[k][x] != v[x] for x in KEYS)]
    out = [MARK, "", "From the compiler's remarks (-Rpass-analysis=kernel-resource-usage, gfx950, the build's flags).", "",
           "### The new instantiations, k_batch_round<8, FORM_MODEL = 2, ROBUST = false, BOUNDED>, each under its J-form twin (and the "
           "robust J form, for scale)", "", "| kernel | " + " | ".join(KEYS) + " |", "|---|" + "---|" * len(KEYS)]
    out += [f"| {k} | {fmt(new[k])} |" for k in names]
    out += ["", f"Existing kernels of dense_batch_kernels.hip whose figures moved against the parent commit: {len(moved)} of {len(old)}"
            + (": " + ", ".join(moved) if moved else "") + "."]
    if asm:
        n, o = asm_functions(asm[0]), asm_functions(asm[1])
        ks = [k for k in o if re.search(r"k_batch_(round|uncertainty|query)", k)]
        differ = [k for k in ks if n.get(k) != o[k]]
        others = [k for k in o if k not in ks and n.get(k) != o[k]]
        added = [k for k in n if k not in o and "k_batch_" in k]
        out += ["", f"Instruction streams (hipcc --offload-device-only -S of both trees, block labels unnumbered): {len(ks)} existing "
                f"instantiations of k_batch_round, k_batch_uncertainty and k_batch_query compared, {len(ks) - len(differ)} are the same "
                f"stream, {len(differ)} differ.  Kernels this tree adds: {len(added)}.  Other kernels of the file that differ: "
                f"{len(others)}" + (" (" + ", ".join(re.sub(r'^_ZN\d+_GLOBAL__N_1\d+', '', k)[:14] for k in others) +
                                     ": the offset of the kernel argument behind BatchDev, which grew by the model record; nothing else)"
                                     if others else "") + "."]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-b", type=int, default=BATCHES[-1])
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a (case, B) step may take")
    ap.add_argument("--step", nargs=2, metavar=("KIND", "B"), help="run one step on the device and print its row")
    ap.add_argument("--resources", nargs=2, metavar=("NEW_REMARKS", "PARENT_REMARKS"))
    ap.add_argument("--asm", nargs=2, metavar=("NEW_S", "PARENT_S"), help="with --resources: compare the kernels' instructions too")
    a = ap.parse_args()
    if a.step:
        step(a.step[0], int(a.step[1]), a.reps)
        return
    kept, tail = [], []
    if a.out and os.path.exists(a.out):
        lines = open(a.out).read().splitlines()
        cut = lines.index(MARK) if MARK in lines else len(lines)
        kept, tail = lines[:cut], lines[cut:]
    if a.resources:
        tail = resources(*a.resources, a.asm)
        kept = kept or [TITLE, "", "not measured", ""]
    else:
        kept = bench(a) + [""]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(kept + tail) + "\n")


if __name__ == "__main__":
    main()
