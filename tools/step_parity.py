#!/usr/bin/env python3
"""tools only: every number the step path returns over a fixed matrix, as hex, for comparing two builds bit for bit.

    python3 tools/step_parity.py LIBRARY OUT.json

Builds nothing.  Run it once per library on the same machine; the two JSON files must be identical (cmp).  The matrix:
sparse / dense / dense-products x dlg_backend_set_defer_tail off / on x speculation off / on x one environment knob (or
none); in every cell the three kinds of step through dlg_take_step, a retry through dlg_step after a rejected trial point, a
singular start that walks the lambda loop and eight dlg_run_steps steps.  Per backend type and defer setting, one profiled
pass records the per-phase launch counts, full and early (dlg_backend_get_profile / _early)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from libdogleg_amd import capi          # noqa: E402
capi.LIB_PATH = os.path.abspath(sys.argv[1])
from tests import oracle_api as oa      # noqa: E402

KNOBS = (None, "DOGLEG_AMD_EI_JPASS", "DOGLEG_AMD_DEVICE_FINALS", "DOGLEG_AMD_NO_PRESOLVE", "DOGLEG_AMD_NO_K8_PREDICT")
KINDS = {"cauchy": capi.KIND_CAUCHY, "gn": capi.KIND_GN, "interp": capi.KIND_INTERP}


def hx(v):
    if isinstance(v, np.ndarray):
        return v.astype(np.float64).tobytes().hex()
    return float(v).hex() if isinstance(v, float) else v


class Case:
    """a problem, a perturbed copy of its inputs (the trial point) and a singular variant, for one backend type"""

    def __init__(self, typ):
        self.typ = typ
        if typ == "sparse":
            self.prob = oa.BAProblem(6, 60, 400, seed=7)
            self.sing = oa.BAProblem(6, 40, 160, seed=7, n_zero_cols=2)
        else:
            self.prob = oa.DenseProblem(M=500, N=40, seed=7)
            self.sing = None
        self.p = self.prob.p0()
        self.ev = [self.prob.eval(self.p + 0.002 * c) for c in range(3)]

    def backend(self, defer, spec, singular=False):
        prob = self.sing if (singular and self.sing is not None) else self.prob
        if self.typ == "sparse":
            be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
            be.set_pattern(*prob.pattern())
        else:
            be = capi.Backend(capi.DLG_DENSE if self.typ == "dense" else capi.DLG_DENSE_PRODUCTS, prob.N, prob.M)
        be.set_speculation(spec)
        be.set_defer_tail(defer)
        p = prob.p0()
        be.set_p(0, p)
        x, J = prob.eval(p)
        if singular and self.sing is None:
            J = J.copy()
            J[:, 3] = 0.0
            J[:, 17] = 0.0
        self.put(be, 0, x, J)
        return be

    def put(self, be, slot, x, J):
        if self.typ == "products":
            be.upload_products(slot, float(x @ x), J.T @ x, J.T @ J)
        else:
            be.upload(slot, x, J)
        return be.eval(slot)


def take(be, tr, lam=0.0):
    lam, r, pn = be.take_step(0, 1, tr, lam)
    return {"lam": hx(lam), **{k: hx(float(v)) for k, v in r.items()}, "p": hx(pn), "step": hx(be.download(1, capi.VEC_STEP)),
            "ei_source": [be.ei_source()[0], hx(be.ei_source()[1])]}


def cell(case, defer, spec):
    out = {}
    be = case.backend(False, False)
    lo, hi = np.sqrt(be.cauchy(0)), np.sqrt(be.gauss_newton(0, 0.0)[1])
    be.close()
    trs = {"cauchy": 0.5 * lo, "gn": 2.0 * hi, "interp": 0.5 * (lo + hi)}
    for which, tr in trs.items():
        be = case.backend(defer, spec)
        out["take_" + which] = take(be, tr)
        # the trial point is evaluated and rejected: the retry from the cached vectors, a smaller trust region
        out["trial_" + which] = [hx(float(v)) for v in case.put(be, 1, *case.ev[1])]
        n2s, k, amax, ei, pn = be.step(0, 1, KINDS[which], 0.8 * tr if which != "interp" else lo + 0.4 * (hi - lo))
        out["retry_" + which] = [hx(n2s), hx(k), hx(amax), hx(ei), hx(pn), hx(be.download(1, capi.VEC_STEP))]
        be.close()
    be = case.backend(defer, spec, singular=True)
    n2c = be.cauchy(0)
    out["singular"] = take(be, 4.0 * np.sqrt(n2c))
    be.close()
    if case.typ != "products":
        be = case.backend(defer, spec)
        d_x = [capi.DeviceArray(x) for x, _ in case.ev]
        d_J = [capi.DeviceArray(J) for _, J in case.ev]
        r, kind = be.run_steps(0, 1, 8, [a.ptr for a in d_x], [a.ptr for a in d_J], 0, trs["interp"], 0.0)
        out["run_steps"] = {"kind": kind, **{k: hx(float(v)) for k, v in r.items()}, "p": hx(be.download(1, capi.VEC_P))}
        be.close()
    return out


def profiled(case, defer):
    """launch counts of a profiled pass: a singular start (early returns), then eight steps"""
    be = case.backend(defer, True, singular=True)
    be.set_profiling(True)
    n2c = be.cauchy(0)
    be.take_step(0, 1, 4.0 * np.sqrt(n2c), 0.0)
    out = {"singular": {k: v[1] for k, v in be.profile().items()}, "singular_early": {k: v[1] for k, v in be.profile_early().items()}}
    be.close()
    if case.typ != "products":
        be = case.backend(defer, True)
        be.set_profiling(True)
        d_x = [capi.DeviceArray(x) for x, _ in case.ev]
        d_J = [capi.DeviceArray(J) for _, J in case.ev]
        be.run_steps(0, 1, 8, [a.ptr for a in d_x], [a.ptr for a in d_J], 0, 1.0, 0.0)
        out["run_steps"] = {k: v[1] for k, v in be.profile().items()}
        out["run_steps_early"] = {k: v[1] for k, v in be.profile_early().items()}
        be.close()
    return out


def main():
    res = {}
    for typ in ("sparse", "dense", "products"):
        case = Case(typ)
        for defer in (False, True):
            for spec in (False, True):
                for knob in KNOBS:
                    for k in KNOBS[1:]:
                        os.environ.pop(k, None)
                    if knob:
                        os.environ[knob] = "1"              # (read when a backend is created / speculation is set)
                    row = f"{typ} defer={int(defer)} spec={int(spec)} {knob or 'no knob'}"
                    res[row] = cell(case, defer, spec)
                    print(row, "ok", flush=True)
            for k in KNOBS[1:]:
                os.environ.pop(k, None)
            res[f"{typ} defer={int(defer)} launch counts"] = profiled(case, defer)
    with open(sys.argv[2], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("rows:", len(res))


if __name__ == "__main__":
    main()
