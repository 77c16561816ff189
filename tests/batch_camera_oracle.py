"""A NumPy restatement of the Poisson fit with read noise of a calibrated camera record (include/dogleg.h, item 5 of the built-in
models: dogleg_amd_optimize_dense_batch_camera with DOGLEG_AMD_LIKELIHOOD_POISSON and maps), written from the definition, not from
include/dogleg_batch_models.h:

    datum  y_i = ((double)raw_i - (double)offset_i) (double)gain_inv_i,   v_i = (double)readvar_i
    with   f'_i = f_i + v_i,   y'_i = y_i + v_i, and 0 where that is < 0 (a comparison: a NaN stays)
    cost   F(p) = sum_i d_i,  d_i = 2 (r_i - y'_i log(f'_i / y'_i)),  r_i = f'_i - y'_i;  d_i = 2 f'_i where y'_i == 0.0
    g = sum (r_i / f'_i) grad f_i,   H = sum grad f_i grad f_i' / f'_i
    a row with !(f'_i > 0) makes the point infeasible: F = +inf, the row adds nothing to g and H

as a products hook on the loop of tests/batch_poisson_oracle.solve_one, which is not restated.  With v = 0 and data >= 0 the hook
returns what batch_poisson_oracle.poisson_products returns, bit for bit, so the solve is that oracle's exactly
(tests/test_dense_batch_camera_cpu.py asserts it).  Nothing of the library under test computes a number in here.

Margins and the allowance for the cost: those of batch_poisson_oracle with f', y' in the place of f, y and v_i among the terms f'_i
is summed from (k_i = (|A e_i| + |c| + v_i) / f'_i).

The tables.  The six 2D shapes of tests/batch_models_np.CASES at the two count levels of batch_poisson_oracle, B = 65, plain and
bounded (that file's bounds).  A 64 x 48 sensor with offset 100 +- 5 ADU, gain_inv in [0.4, 2.5] and readvar in [0.5, 3]
photoelectrons^2, one set of maps a shape; problem `seed` has the truth, the start and the Poisson counts n of
batch_poisson_oracle.problem, an origin of its own, and the readings a camera would deliver:
    raw = rint((n + sqrt(readvar) N(0, 1)) / gain_inv + offset)   as uint16
so that at the low level (offset 0.3 photons) many readings lie under their offset and some under offset - readvar / gain_inv:
there the clamp runs.  SEED0 and the recorded margins: find_seed0 below, run as `python -m tests.batch_camera_oracle`; every
problem of a table has decision margins above MARGIN_FLOOR and a cost allowance below COST_TOL of batch_poisson_oracle."""
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import BATCH_JTX, BATCH_SMALL_STEP, LIKELIHOOD_POISSON
from tests import batch_models_np as mz
from tests import batch_poisson_oracle as po
from tests.batch_robust_oracle import EPS

B = po.B
MARGIN_FLOOR = po.MARGIN_FLOOR
COST_TOL = po.COST_TOL
SENSOR = (64, 48)            # width, height
CASES = [c for c in mz.CASES if mz.is_2d(c[0])]
TABLES = [(case, level) for case in CASES for level in ("high", "low")]
table_id = po.table_id
params = po.params


# ---------------------------------------------------------------- the products
def camera_products(hp, v):
    """the hook of the Poisson fit with read noise: (F, g, H, F_err, feasibility margin, feasible); hp.y: the calibrated data"""
    y = hp.y

    def hook(p):
        f, G = po.model_values(hp, p)
        c = p[hp.N - 1]
        with np.errstate(all="ignore"):
            size = np.abs(f - c) + abs(c) + v        # |A e_i| + |c| + v_i
            fv = f + v
            ys = y + v
            yv = np.where(ys < 0.0, 0.0, ys)
            fmargin = float(np.min(np.abs(fv) / size)) if np.all(np.isfinite(fv)) else 0.0
            ok = fv > 0.0
            r = fv - yv
            lg = np.log(fv / np.where(yv == 0.0, 1.0, yv))
            ylg = np.where(yv == 0.0, 0.0, yv * lg)
            d = np.where(yv == 0.0, 2.0 * fv, 2.0 * (r - ylg))
            rf = np.where(ok, r / fv, 0.0)
            Gf = np.where(ok[:, None], G / fv[:, None], 0.0)
            Gz = np.where(ok[:, None], G, 0.0)
            g = Gz.T @ rf
            H = Gz.T @ Gf
            if not ok.all():
                return np.inf, g, H, 0.0, fmargin, False
            F = float(np.sum(d))
            Ferr = 2.0 * EPS * (2.0 * float(np.sum(14.0 * size / fv * np.abs(r) + 4.0 * np.abs(ylg))) + hp.M * abs(F))
        return F, g, H, Ferr, fmargin, True

    return hook


def solve_one(hp, v, prm, lo=None, hi=None):
    """batch_poisson_oracle.solve_one on the hook above; hp.y the calibrated data, v the read-noise variances"""
    return po.solve_one(hp, prm, LIKELIHOOD_POISSON, lo, hi, products=camera_products(hp, v))


# ---------------------------------------------------------------- the tables
# the first seed of every table and the smallest margin of its plain and of its bounded table, as find_seed0 gave them
FOUND = {
    ((2, (7, 7)), 'high'): (1, 0.00826, 0.00267),
    ((2, (7, 7)), 'low'): (1, 5.94e-05, 5.94e-05),
    ((2, (5, 9)), 'high'): (1, 0.000944, 0.000944),
    ((2, (5, 9)), 'low'): (1, 0.00173, 0.00173),
    ((2, (8, 8)), 'high'): (1, 0.0011, 0.0026),
    ((2, (8, 8)), 'low'): (1, 0.00166, 0.00166),
    ((3, (6, 7)), 'high'): (1, 0.00333, 0.000737),
    ((3, (6, 7)), 'low'): (1, 0.00131, 0.000639),
    ((3, (7, 7)), 'high'): (1, 0.000377, 0.000864),
    ((3, (7, 7)), 'low'): (1, 0.000983, 0.000137),
    ((3, (9, 5)), 'high'): (1, 0.00294, 0.000621),
    ((3, (9, 5)), 'low'): (1, 0.00205, 0.00429),
}
SEED0 = {t: v[0] for t, v in FOUND.items()}
MARGINS = {t: v[1:] for t, v in FOUND.items()}             # (plain, bounded)


@functools.lru_cache(maxsize=None)
def maps(case):
    """the sensor of a shape: dict(offset, gain_inv, readvar), (height, width) float32 each"""
    _, w, h = mz.case_shape(case)
    rng = np.random.default_rng([31, case[0], w, h])
    W, H = SENSOR
    return dict(offset=(100.0 + 5.0 * rng.uniform(-1.0, 1.0, size=(H, W))).astype(np.float32),
                gain_inv=rng.uniform(0.4, 2.5, size=(H, W)).astype(np.float32),
                readvar=rng.uniform(0.5, 3.0, size=(H, W)).astype(np.float32))


def window(m, origin, w, h):
    ox, oy = int(origin[0]), int(origin[1])
    return m[oy:oy + h, ox:ox + w].reshape(-1)


def calibrate(raw, case, origin):
    """(y, v) of one problem's readings by the definition, in float64"""
    _, w, h = mz.case_shape(case)
    mp = maps(case)
    off, gi, rv = (window(mp[k], origin, w, h).astype(np.float64) for k in ("offset", "gain_inv", "readvar"))
    return (raw.astype(np.float64) - off) * gi, rv


def problem(case, level, seed):
    """dict(raw (M,) uint16, origin (2,) int32, y, v (M,) float64, p0, truth) of one seed"""
    kind, _ = case
    M, w, h = mz.case_shape(case)
    q = po.problem(case, level, seed)
    rng = np.random.default_rng([37, kind, M, w, int(seed), 0 if level == "high" else 1])
    W, H = SENSOR
    origin = np.array([rng.integers(0, W - w + 1), rng.integers(0, H - h + 1)], dtype=np.int32)
    mp = maps(case)
    off, gi, rv = (window(mp[k], origin, w, h).astype(np.float64) for k in ("offset", "gain_inv", "readvar"))
    adu = np.rint((q["y"] + np.sqrt(rv) * rng.standard_normal(M)) / gi + off)
    raw = np.clip(adu, 0, 65535).astype(np.uint16)
    y, v = calibrate(raw, case, origin)
    return dict(raw=raw, origin=origin, y=y, v=v, p0=q["p0"], truth=q["truth"])


def batch(table, seed0=None, nb=B):
    """the arrays of a table's batch: the keys of batch_poisson_oracle.batch (y: the calibrated data) and raw (nb, M) uint16,
    origin (nb, 2) int32, v (nb, M), maps: the sensor's"""
    case, level = table
    kind, _ = case
    M, w, h = mz.case_shape(case)
    seed0 = SEED0.get(table, 1) if seed0 is None else seed0
    ps = [problem(case, level, seed0 + b) for b in range(nb)]
    los, his = zip(*[po.bounds_of(case, b, ps[b]["truth"]) for b in range(nb)])
    return dict(kind=kind, M=M, width=w, height=h, y=np.array([q["y"] for q in ps]), v=np.array([q["v"] for q in ps]),
                raw=np.array([q["raw"] for q in ps]), origin=np.array([q["origin"] for q in ps]), maps=maps(case),
                p0=np.array([q["p0"] for q in ps]), truth=np.array([q["truth"] for q in ps]), t=None, scale=None,
                lo=np.array(los), hi=np.array(his), t_mode=None)


@functools.lru_cache(maxsize=None)
def oracle_table(table, bounded, seed0=None, nb=B):
    """the oracle's solves of a table: a list of solve_one results.  Cached and never modified: the tests share it"""
    bt = batch(table, seed0, nb)
    prm = params()
    return [solve_one(mz.host_model(bt, b), bt["v"][b], prm, bt["lo"][b] if bounded else None, bt["hi"][b] if bounded else None)
            for b in range(nb)]


def find_seed0(table, nb=B, start=1, tries=400000, floor=MARGIN_FLOOR):
    """batch_poisson_oracle.find_seed0 for these tables: the first seed0 >= start such that the problems seed0 .. seed0 + nb - 1 all
    lie above `floor` in the plain and in the bounded table and end in JTX or SMALL_STEP with a cost whose own rounding allowance
    lies below COST_TOL; (seed0, plain margin, bounded margin)"""
    case, level = table
    prm = params()
    memo = {}

    def margin(seed, phase):
        if (seed, phase) not in memo:
            q = problem(case, level, seed)
            hp = mz.HostModel(case[0], q["y"], q["p0"], None, None, mz.case_shape(case)[1])
            lo, hi = po.bounds_of(case, phase, q["truth"])
            ms = []
            for o in (solve_one(hp, q["v"], prm), solve_one(hp, q["v"], prm, lo, hi)):
                ms.append(o["margin"] if o["status"] in (BATCH_JTX, BATCH_SMALL_STEP) and o["cost_error"] <= COST_TOL else -1.0)
            memo[(seed, phase)] = ms
        return memo[(seed, phase)]

    s0 = start
    while s0 < start + tries:
        bad = next((b for b in range(nb - 1, -1, -1) if min(margin(s0 + b, b % 6)) <= floor), None)
        if bad is None:
            return (s0,) + tuple(min(margin(s0 + b, b % 6)[k] for b in range(nb)) for k in (0, 1))
        s0 += bad + 1
    raise RuntimeError("no seed0 found")


if __name__ == "__main__":
    for table in TABLES:
        s0, mp, mb = find_seed0(table)
        print(f"    ({table[0]!r}, {table[1]!r}): ({s0}, {mp:.3g}, {mb:.3g}),", flush=True)
