#!/usr/bin/env python3
"""tools only: everything whole solves through dogleg_optimize* hand back over a fixed matrix, floats as hex, for comparing
two builds of the host driver record for record.

    python3 tools/driver_parity.py LIBRARY OUT.json

Builds nothing.  Run it once per library on the same machine; the two JSON files must be identical (cmp).  Several knobs
are read once per process, so every knob set (KNOBS) runs in a fresh child process, one after another, each under its own
time limit; the first child that fails stops the run.  Every child runs the same rows (rows()): host-callback sparse /
dense / dense-products solves, their device-callback twins, each with and without a returned context; two solves in a row
of one shape (same pattern, then another); a singular start; a start at the optimum; max_iterations = 2; runs that end on
trustregion_threshold and on update_threshold; two ranks as two host threads with the all-reduce hook.  Per solve: the
return value, the final p, ncallbacks, every field of every trial, p_trial and the step vectors, the library's lines on
stderr under debug = 1, and -- from a second solve under debug_vnlog -- the vnlog text on stdout; with a returned context
the host mirrors of beforeStep and factorization_dense."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import threading

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KNOBS = {"no knob": {}, "NO_PATTERN_OVERLAP": {"DOGLEG_AMD_NO_PATTERN_OVERLAP": "1"}, "NO_BETWEEN": {"DOGLEG_AMD_NO_BETWEEN": "1"},
         "NO_BACKEND_CACHE": {"DOGLEG_AMD_NO_BACKEND_CACHE": "1"}}
CHILD_SECONDS = 240


def hx(v):
    if isinstance(v, np.ndarray):
        return v.astype(np.float64).tobytes().hex()
    return float(v).hex() if isinstance(v, float) else v


# ---- the structs of include/dogleg.h a returned context is read through (compat cholmod shapes) ----
class OperatingPoint(C.Structure):
    _fields_ = [("p", C.POINTER(C.c_double)), ("x", C.POINTER(C.c_double)), ("norm2_x", C.c_double), ("J", C.c_void_p),
                ("Jt_x", C.POINTER(C.c_double)), ("updateCauchy", C.POINTER(C.c_double)), ("updateGN", C.c_void_p),
                ("norm2_updateCauchy", C.c_double), ("norm2_updateGN", C.c_double), ("bits", C.c_int * 3),
                ("step_to_here", C.POINTER(C.c_double)), ("norm2_step_to_here", C.c_double)]


class CholmodDense(C.Structure):
    _fields_ = [("nrow", C.c_size_t), ("ncol", C.c_size_t), ("nzmax", C.c_size_t), ("d", C.c_size_t),
                ("x", C.POINTER(C.c_double)), ("z", C.c_void_p), ("xtype", C.c_int), ("dtype", C.c_int)]


class CholmodFactor(C.Structure):
    _fields_ = [("n", C.c_size_t), ("minor", C.c_size_t), ("backend", C.c_void_p)]


class Context(C.Structure):
    _fields_ = [("common", C.c_char * 56), ("f", C.c_void_p), ("cookie", C.c_void_p),
                ("beforeStep", C.POINTER(OperatingPoint)), ("afterStep", C.POINTER(OperatingPoint)),
                ("factorization", C.c_void_p), ("lambda_", C.c_double), ("solve_type", C.c_int), ("Nstate", C.c_int),
                ("Nmeasurements", C.c_int), ("parameters", C.c_void_p)]


def read_context(ctxp):
    """the host mirrors of beforeStep, and the dense factor / the sparse factor handle"""
    ctx = C.cast(ctxp, C.POINTER(Context)).contents
    N, M, sparse = ctx.Nstate, ctx.Nmeasurements, ctx.solve_type == 1
    pt = ctx.beforeStep.contents
    bits = pt.bits[0]
    arr = lambda ptr, n: hx(np.ctypeslib.as_array(ptr, shape=(n,)).copy()) if ptr else None
    out = {"lambda": hx(ctx.lambda_), "solve_type": ctx.solve_type, "N": N, "M": M, "bits": bits, "norm2_x": hx(pt.norm2_x),
           "norm2_updateCauchy": hx(pt.norm2_updateCauchy) if bits & 1 else None,
           "norm2_updateGN": hx(pt.norm2_updateGN) if bits & 2 else None,
           "p": arr(pt.p, N), "x": arr(pt.x, M) if ctx.solve_type != 2 else None, "Jt_x": arr(pt.Jt_x, N),
           "updateCauchy": arr(pt.updateCauchy, N), "step_to_here": arr(pt.step_to_here, N)}
    if sparse:
        g = C.cast(pt.updateGN, C.POINTER(CholmodDense)).contents
        out["updateGN"] = arr(g.x, N)
        if ctx.factorization:
            f = C.cast(ctx.factorization, C.POINTER(CholmodFactor)).contents
            out["factor_handle"] = [f.n, f.minor]
        else:
            out["factor_handle"] = None
    else:
        out["updateGN"] = arr(C.cast(pt.updateGN, C.POINTER(C.c_double)), N)
        packed = ctx.solve_type == 0 or bool(C.cast(ctx.parameters, C.POINTER(C.c_int))[1] & 2)
        out["factorization_dense"] = arr(C.cast(ctx.factorization, C.POINTER(C.c_double)), N * (N + 1) // 2 if packed else N * N)
    return out


class Captured:
    """what the C library wrote to a file descriptor while the block ran"""

    def __init__(self, fd):
        self.fd, self.text = fd, ""

    def __enter__(self):
        C.CDLL(None).fflush(None)
        self.saved = os.dup(self.fd)
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        os.dup2(self.tmp.fileno(), self.fd)
        return self

    def __exit__(self, *exc):
        C.CDLL(None).fflush(None)
        os.dup2(self.saved, self.fd)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()
        if exc[0] is not None and self.fd == 2:
            sys.stderr.write(self.text)


def child(capi, oa):
    from libdogleg_amd.ctypes_defs import TraceBuffer, dptr, iptr
    L = capi.lib()

    def call(S, prm, want_ctx, trace):
        """one dogleg_optimize* call of the solve S = dict(kind, N, M, nnz, cb, cookie, p0[, pattern])"""
        p = np.array(S["p0"], dtype=np.float64, copy=True)
        ctx = C.c_void_p()
        rc = C.byref(ctx) if want_ctx else None
        N, M, nnz = S["N"], S["M"], S.get("nnz", 0)
        L.dlg_set_trace(C.cast(trace.byref(), C.c_void_p) if trace is not None else None)
        try:
            if S["kind"] == "sparse":
                r = L.dogleg_optimize2(dptr(p), N, M, nnz, S["cb"], S["cookie"], C.byref(prm), rc)
            elif S["kind"] == "dense":
                r = L.dogleg_optimize_dense2(dptr(p), N, M, S["cb"], S["cookie"], C.byref(prm), rc)
            elif S["kind"] == "products":
                r = L.dogleg_optimize_dense_products(dptr(p), N, S["cb"], S["cookie"], C.byref(prm), rc)
            else:
                Jp, Ji = S.get("pattern", (None, None))
                r = L.dogleg_optimize_device2(dptr(p), N, M, nnz, iptr(Jp) if nnz else None, iptr(Ji) if nnz else None,
                                              S["cb"], S["cookie"], C.byref(prm), rc)
        finally:
            L.dlg_set_trace(None)
        return r, p, ctx

    def params(S, **extra):
        prm = oa.default_params()
        for k, v in {**S.get("prm", {}), **extra}.items():
            setattr(prm, k, v)
        return prm

    def record(S, want_ctx, quiet=False):
        """the solve under debug = 1 with a trace (and a context), then again under debug_vnlog"""
        if "before" in S:
            S["before"]()
        tr = TraceBuffer(S["N"], 256)
        prm = params(S, debug=not quiet)
        with Captured(2) as err:
            r, p, ctx = call(S, prm, want_ctx, tr)
        out = {"return": hx(float(r)), "p": hx(p), "ncallbacks": tr.ncallbacks, "ntrials": tr.c.ntrials,
               "trials": [{k: hx(v) for k, v in t.items()} for t in tr.trials()],
               "p_trial": hx(tr.p_trial[:tr.ntrials]), "step": hx(tr.step[:tr.ntrials]),
               "stderr": [l for l in err.text.splitlines() if l.startswith("libdogleg_amd:")]}
        if want_ctx:
            out["context"] = read_context(ctx) if ctx.value else None
            if ctx.value:
                L.dogleg_freeContext(C.byref(ctx))
        if not quiet:
            prm = params(S, debug_vnlog=True)
            with Captured(1) as txt:
                r2, p2, _ = call(S, prm, False, None)
            out["vnlog"] = txt.text
            out["vnlog_return"] = [hx(float(r2)), hx(p2)]
        return out

    keep = []                                    # (callbacks and problems stay alive for the whole run)

    def host(prob, kind, **prm):
        cb = prob.cb_products if kind == "products" else prob.cb
        return dict(kind=kind, N=prob.N, M=prob.M, nnz=getattr(prob, "nnz", 0) if kind == "sparse" else 0, cb=cb,
                    cookie=prob.cookie, p0=prob.p0(), prm=prm)

    def device(prob, **prm):
        twin = oa.DeviceTwin(prob)
        keep.append(twin)
        sparse = hasattr(prob, "nnz")
        return dict(kind="device", N=prob.N, M=prob.M, nnz=prob.nnz if sparse else 0, cb=twin.cb, cookie=twin.cookie,
                    p0=prob.p0(), prm=prm, pattern=prob.pattern() if sparse else (None, None))

    def wrapped(prob, kind, edit):
        """the problem's host callback with its outputs edited in place: edit(x, J-values, call number)"""
        n = [0]
        if kind == "sparse":
            inner = capi.CB_SPARSE(prob.cb.value)

            @capi.CB_SPARSE
            def cb(p, x, Jt, cookie):
                inner(p, x, Jt, cookie)
                n[0] += 1
                edit(np.ctypeslib.as_array(x, shape=(prob.M,)),
                     np.ctypeslib.as_array(C.cast(Jt.contents.x, C.POINTER(C.c_double)), shape=(prob.nnz,)), n[0])
        else:
            inner = capi.CB_DENSE(prob.cb.value)

            @capi.CB_DENSE
            def cb(p, x, J, cookie):
                inner(p, x, J, cookie)
                n[0] += 1
                edit(np.ctypeslib.as_array(x, shape=(prob.M,)), np.ctypeslib.as_array(J, shape=(prob.M, prob.N)), n[0])
        keep.extend([inner, cb])
        S = host(prob, kind)
        S["cb"] = C.cast(cb, C.c_void_p)
        S["before"] = lambda: n.__setitem__(0, 0)
        return S

    P = oa.problems()
    res = {}
    ba_small = oa.BAProblem(4, 20, 60, seed=2, eps=0.4, p0_spread=0.8)
    ba = oa.BAProblem(12, 120, 720, seed=4, eps=0.4, p0_spread=0.6)
    dn = oa.DenseProblem(M=500, N=40, seed=7)
    keep.extend([ba_small, ba, dn])
    std = dict(max_iterations=12, trustregion0=3.0)

    # rows 1 - 5: every kind of solve, with and without a returned context
    solves = {"sparse 4x20x60": host(ba_small, "sparse", **std), "sparse 12x120x720": host(ba, "sparse", **std),
              "dense 500x40": host(dn, "dense", max_iterations=8),
              "device sparse 4x20x60": device(ba_small, **std), "device sparse 12x120x720": device(ba, **std),
              "device dense 500x40": device(dn, max_iterations=8)}
    for name, (packed, upper) in {"products unpacked": (0, 0), "products packed": (1, 0), "products packed upper": (1, 1)}.items():
        S = host(dn, "products", max_iterations=8, JtJ_packed=bool(packed), JtJ_upper=bool(upper))
        S["before"] = lambda packed=packed, upper=upper: P.synth_set_products_layout(packed, upper)
        solves[name] = S
    for name, S in solves.items():
        for want_ctx in (False, True):
            res[f"{name}, context {int(want_ctx)}"] = record(S, want_ctx)

    # row 6: solves in a row of one shape -- pattern A, A again, then B (another pattern of the same shape)
    pair = [oa.BAProblem(23, 400, 3000, seed=21, eps=0.4, p0_spread=0.5), oa.BAProblem(23, 400, 3000, seed=21, eps=0.4, p0_spread=0.5),
            oa.BAProblem(22, 402, 3000, seed=22, eps=0.4, p0_spread=0.5)]
    keep.extend(pair)
    assert pair[0].nnz == pair[2].nnz and pair[0].M == pair[2].M and pair[0].N == pair[2].N
    for k, prob in enumerate(pair):
        res[f"in a row, device, solve {k}"] = record(device(prob, max_iterations=8, trustregion0=3.0), k == 2)
    for k, prob in enumerate(pair):
        res[f"in a row, host, solve {k}"] = record(host(prob, "sparse", max_iterations=8, trustregion0=3.0), False)

    # row 9: a singular start that walks the lambda loop
    sing = oa.BAProblem(6, 40, 160, seed=7, n_zero_cols=2)
    keep.append(sing)
    res["singular sparse"] = record(host(sing, "sparse", max_iterations=6), True)
    res["singular device sparse"] = record(device(sing, max_iterations=6), True)

    def zero_cols(x, J, n):
        J[:, 3] = 0.0
        J[:, 17] = 0.0
    res["singular dense"] = record(dict(wrapped(dn, "dense", zero_cols), prm=dict(max_iterations=6)), True)

    # row 10: a start at the optimum (noise-free problem, p0 = p*), and a start that counts as one
    exact = oa.BAProblem(4, 20, 60, seed=2, eps=0.4, noise=0.0)
    keep.append(exact)
    for name, S in (("host", host(exact, "sparse")), ("device", device(exact))):
        S["p0"] = exact.pstar()
        res[f"start at the optimum, {name}"] = record(S, True)
    res["start below the gradient threshold"] = record(host(ba_small, "sparse", Jt_x_threshold=1e30), True)

    # row 11: max_iterations = 2
    for name, S in solves.items():
        if not name.startswith("products p"):
            res[f"{name}, max_iterations 2"] = record(dict(S, prm=dict(S["prm"], max_iterations=2)), True)

    # row 12: runs that end on trustregion_threshold
    rng = np.random.default_rng(4)
    M, N = 60, 5
    J0, xs = rng.standard_normal((M, N)), 3.0 * rng.standard_normal(M)

    @capi.CB_DENSE
    def huge_cb(p, x, J, cookie):
        pv = np.ctypeslib.as_array(p, shape=(N,)).copy()
        r = J0 @ pv - xs
        np.ctypeslib.as_array(x, shape=(M,))[:] = r + 2.5 * np.sin(r)
        np.ctypeslib.as_array(J, shape=(M * N,))[:] = (J0 * (1.0 + 2.5 * np.cos(r))[:, None]).ravel()
    keep.append(huge_cb)
    huge = dict(kind="dense", N=N, M=M, cb=C.cast(huge_cb, C.c_void_p), cookie=None, p0=np.full(N, 4.0))
    res["huge trust region"] = record(dict(huge, prm=dict(max_iterations=25, trustregion0=1e6)), True)
    res["huge trust region, threshold 1e-1"] = record(dict(huge, prm=dict(max_iterations=25, trustregion0=1e6, trustregion_threshold=1e-1)), True)

    def worse(x, J, n):
        if n > 1:
            x *= 50.0                              # every trial point: much worse than the start, rejected
    res["every trial rejected"] = record(dict(wrapped(ba, "sparse", worse),
                                              prm=dict(max_iterations=10, trustregion0=1e3, trustregion_threshold=1e-4)), True)

    # row 13: runs that end on update_threshold with a device callback (the deferred expected improvement of the terminal step)
    for name, prob in (("sparse", ba_small), ("dense", dn)):
        res[f"update_threshold, device {name}"] = record(device(prob, max_iterations=30, trustregion0=3.0, update_threshold=1e-3,
                                                                Jt_x_threshold=1e-300), True)
    res["update_threshold, host sparse"] = record(host(ba_small, "sparse", max_iterations=30, trustregion0=3.0, update_threshold=1e-3,
                                                       Jt_x_threshold=1e-300), True)

    # row 14: two ranks as two host threads with the all-reduce hook (stderr is not recorded: two threads write to it)
    class AllReduce:
        def __init__(self, world):
            self.world, self.slots, self.bar = world, [None] * world, threading.Barrier(world)

        def hook(self, rank):
            def fn(buf, count, cookie):
                try:
                    hostbuf = np.empty(count)
                    if L.dlg_mem_download(hostbuf.ctypes.data, buf, 8 * count) != 0:
                        return 1
                    self.slots[rank] = hostbuf
                    self.bar.wait(timeout=60)
                    total = self.slots[0].copy()
                    for r in range(1, self.world):
                        total += self.slots[r]
                    self.bar.wait(timeout=60)
                    return 0 if L.dlg_mem_upload(buf, total.ctypes.data, 8 * count) == 0 else 1
                except Exception as e:
                    print("in-process all-reduce failed:", e)
                    return 1
            return fn

    def ranks(S, world=2):
        ar = AllReduce(world)
        out, errs, hooks = [None] * world, [], []

        def run(rank):
            try:
                hook = capi.ALLREDUCE_FN(ar.hook(rank))
                hooks.append(hook)
                assert L.dogleg_amd_set_allreduce(rank, world, -1, C.cast(hook, C.c_void_p), None) == 0
                try:
                    tr = TraceBuffer(S["N"], 256)
                    r, p, ctx = call(S, params(S), True, tr)
                    nr = C.c_int(0)
                    out[rank] = {"return": hx(float(r)), "p": hx(p), "ncallbacks": tr.ncallbacks, "ntrials": tr.c.ntrials,
                                 "trials": [{k: hx(v) for k, v in t.items()} for t in tr.trials()],
                                 "p_trial": hx(tr.p_trial[:tr.ntrials]), "step": hx(tr.step[:tr.ntrials]),
                                 "rank": [L.dogleg_amd_rank(ctx, C.byref(nr)), nr.value] if ctx.value else None,
                                 "context": read_context(ctx) if ctx.value else None}
                    if ctx.value and S["kind"] == "device" and S.get("nnz", 0):
                        # a rank's backend holds x of ITS rows only (gathered on the device): the mirror's first part_nrows
                        # entries are those, behind them is whatever the slot's buffer held before
                        n, rows = C.c_int(0), C.POINTER(C.c_int)()
                        assert L.dlg_partition_rows(L.dogleg_amd_backend(ctx), C.byref(n), C.byref(rows)) == 0
                        out[rank]["context"]["x"] = out[rank]["context"]["x"][:16 * n.value]
                        out[rank]["rows"] = n.value
                    if ctx.value:
                        L.dogleg_freeContext(C.byref(ctx))
                finally:
                    L.dogleg_amd_clear_communicator()
            except Exception as e:
                errs.append((rank, repr(e)))
                try:
                    ar.bar.abort()
                except Exception:
                    pass
        th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        [t.start() for t in th]
        [t.join(timeout=120) for t in th]
        assert not errs and not any(t.is_alive() for t in th), errs
        return out

    L.dogleg_amd_rank.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    dn_odd = oa.DenseProblem(M=301, N=24, seed=2)
    keep.append(dn_odd)
    res["two ranks, sparse"] = ranks(host(ba, "sparse", **std))
    res["two ranks, dense"] = ranks(host(dn_odd, "dense", max_iterations=8))
    res["two ranks, device sparse"] = ranks(device(ba, **std))
    res["two ranks, device dense"] = ranks(device(dn_odd, max_iterations=8))
    return res


def count(v):
    """values in a row: every scalar, every double of a hex-coded array, every line of text"""
    if isinstance(v, dict):
        return sum(count(x) for x in v.values())
    if isinstance(v, list):
        return sum(count(x) for x in v)
    if isinstance(v, str) and len(v) >= 32 and len(v) % 16 == 0 and all(c in "0123456789abcdef" for c in v):
        return len(v) // 16
    return 1


def main():
    lib, out = os.path.abspath(sys.argv[1]), sys.argv[2]
    if len(sys.argv) > 3:                          # a child: one knob set (already in the environment)
        sys.path.insert(0, ROOT)
        from libdogleg_amd import capi
        capi.LIB_PATH = lib
        from tests import oracle_api as oa
        with open(out, "w") as f:
            json.dump(child(capi, oa), f, indent=1, sort_keys=True)
        return 0
    res = {}
    for name, env in KNOBS.items():
        e = {k: v for k, v in os.environ.items() if k not in sum((list(x) for x in KNOBS.values()), [])}
        e.update(env)
        part = out + ".part"
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), lib, part, name], env=e, timeout=CHILD_SECONDS).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"{name}: child failed with status {rc}; stopping", flush=True)
            return 1
        with open(part) as f:
            rows = json.load(f)
        os.remove(part)
        for row, v in rows.items():
            res[f"{name}: {row}"] = v
        print(f"{name}: {len(rows)} rows, {sum(count(v) for v in rows.values())} values", flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    with open(os.path.splitext(out)[0] + ".counts.txt", "w") as f:
        for row in sorted(res):
            f.write(f"{count(res[row])}\t{row}\n")
    print("rows:", len(res), "values:", sum(count(v) for v in res.values()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
