"""The four built-in fit models of the batch solver (include/dogleg.h: dogleg_amd_batch_model_t) restated in NumPy from their
definitions, not from include/dogleg_batch_models.h, and the synthetic batches the model tests share.

    x_i = s_i (f_i(p) - y_i),  J = d x / d p,  s_i = 1 without a scale
    EXPDECAY          p = A, k, c              f_i = A exp(-k t_i) + c
    GAUSS1D           p = A, mu, sigma, c      f_i = A exp(-(t_i - mu)^2 / (2 sigma^2)) + c
    GAUSS2D           p = A, x0, y0, sigma, c  row i is pixel (i mod width, i div width): A exp(-((ix - x0)^2 + (iy - y0)^2) / (2 sigma^2)) + c
    GAUSS2D_ELLIPTIC  p = A, x0, y0, sx, sy, c the same with its own width per axis

HostModel has the .N, .M, .p0(), .eval(p) interface tests/batch_oracle.py, batch_robust_oracle.py and batch_bounds_oracle.py take
as hp (and .cb / .cookie, a host callback, for the first of them), so those oracles solve these problems unchanged.

The batches.  A case is (kind, shape): shape is M for the 1D kinds and (width, height) for the 2D kinds.  Problem b of a case has
seed SEED0[case] + b: a true p drawn per seed, data = the model at the truth + Gaussian noise of NOISE, a start perturbed from
the truth.  Variants of the same data: a scale s_i in [0.5, 2] per datum, abscissae t shared by the batch or per problem (without
them t_i = i; the true decay rate and width follow the span of t).  The bounds of the bounded tables: problem b gets c >= c_true +
0.3 if b mod 6 == 0 (an offset bound above the true offset), width <= 0.9 of the true width (EXPDECAY: k <= 0.9 k_true) if b mod 6
== 3, and no bound otherwise (a third of the problems end with a variable held); the start point is clamped into them by the solve.

The seeds.  SEED0 was chosen on the CPU with the oracle alone (find_seed0 below) such that every problem of the plain and of the
bounded table has its smallest decision margin (tests/batch_bounds_oracle.py) above MARGIN_FLOOR; tests/test_dense_batch_model_cpu.py
asserts that, and what the tables must contain, so no case is left out and none is vacuous.  Both tables stop at
update_threshold = Jt_x_threshold = 1e-6 (STOP_OVER): a problem held on a bound ends with a large residual, where Gauss-Newton
converges linearly and the last steps to 1e-8 improve norm2(x) by less than its rounding error, as tests/test_dense_batch_bounds_gpu.py
says of its own batches."""
import ctypes as C
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import (CB_DENSE, LOSS_TRIVIAL, MODEL_EXPDECAY, MODEL_GAUSS1D, MODEL_GAUSS2D,
                                       MODEL_GAUSS2D_ELLIPTIC, MODEL_NSTATE)
from tests import batch_bounds_oracle as bb
from tests import batch_robust_oracle as ro
from tests import oracle_api as oa

B = 65                       # 16 whole workgroups and one wavefront alone
NOISE = 0.05
MARGIN_FLOOR = 1e-6
STOP_OVER = (("update_threshold", 1e-6), ("Jt_x_threshold", 1e-6))
KIND_NAMES = {MODEL_EXPDECAY: "expdecay", MODEL_GAUSS1D: "gauss1d", MODEL_GAUSS2D: "gauss2d", MODEL_GAUSS2D_ELLIPTIC: "elliptic"}

# T = min(64, 256 / N) rows a tile: 64, 64, 51, 42 for N = 3, 4, 5, 6
CASES = ([(k, m) for k in (MODEL_EXPDECAY, MODEL_GAUSS1D) for m in (5, 64, 65, 150)] +
         [(MODEL_GAUSS2D, (7, 7)), (MODEL_GAUSS2D, (5, 9)), (MODEL_GAUSS2D, (8, 8)),
          (MODEL_GAUSS2D_ELLIPTIC, (6, 7)), (MODEL_GAUSS2D_ELLIPTIC, (7, 7)), (MODEL_GAUSS2D_ELLIPTIC, (9, 5))])
# the first seed of every case and the smallest margin of its two tables, as find_seed0 gave them
SEED0 = {c: 1 for c in CASES}
SEED0[(MODEL_EXPDECAY, 64)] = 114
MARGINS = {(MODEL_EXPDECAY, 5): 2.92e-3, (MODEL_EXPDECAY, 64): 1.89e-2, (MODEL_EXPDECAY, 65): 8.14e-3, (MODEL_EXPDECAY, 150): 5.71e-3,
           (MODEL_GAUSS1D, 5): 6.27e-3, (MODEL_GAUSS1D, 64): 8.43e-3, (MODEL_GAUSS1D, 65): 3.28e-3, (MODEL_GAUSS1D, 150): 4.01e-2,
           (MODEL_GAUSS2D, (7, 7)): 9.87e-3, (MODEL_GAUSS2D, (5, 9)): 1.42e-2, (MODEL_GAUSS2D, (8, 8)): 4.82e-3,
           (MODEL_GAUSS2D_ELLIPTIC, (6, 7)): 5.71e-4, (MODEL_GAUSS2D_ELLIPTIC, (7, 7)): 2.70e-3,
           (MODEL_GAUSS2D_ELLIPTIC, (9, 5)): 5.14e-3}


def case_id(case):
    kind, shape = case
    return f"{KIND_NAMES[kind]}-{shape if isinstance(shape, int) else 'x'.join(map(str, shape))}"


def is_2d(kind):
    return kind in (MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC)


def case_shape(case):
    """(M, width, height); width = height = 0 for the 1D kinds"""
    kind, shape = case
    return (shape[0] * shape[1], shape[0], shape[1]) if is_2d(kind) else (shape, 0, 0)


def model_eval(kind, p, y, t=None, scale=None, width=0):
    """(x (M,), J (M, N)) of one problem at p; t: (M,) or None (t_i = i), scale: (M,) or None"""
    p = np.asarray(p, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    M = y.shape[0]
    s = np.ones(M) if scale is None else np.asarray(scale, dtype=np.float64)
    idx = np.arange(M)
    one = np.ones(M)
    if kind == MODEL_EXPDECAY:
        t = idx.astype(np.float64) if t is None else np.asarray(t, dtype=np.float64)
        A, k, c = p
        e = np.exp(-k * t)
        f, cols = A * e + c, [e, -A * t * e, one]
    elif kind == MODEL_GAUSS1D:
        t = idx.astype(np.float64) if t is None else np.asarray(t, dtype=np.float64)
        A, mu, sigma, c = p
        d = t - mu
        g = np.exp(-d * d / (2.0 * sigma * sigma))
        f, cols = A * g + c, [g, A * g * d / sigma ** 2, A * g * d * d / sigma ** 3, one]
    elif kind == MODEL_GAUSS2D:
        A, x0, y0, sigma, c = p
        dx, dy = (idx % width) - x0, (idx // width) - y0
        g = np.exp(-(dx * dx + dy * dy) / (2.0 * sigma * sigma))
        f, cols = A * g + c, [g, A * g * dx / sigma ** 2, A * g * dy / sigma ** 2, A * g * (dx * dx + dy * dy) / sigma ** 3, one]
    elif kind == MODEL_GAUSS2D_ELLIPTIC:
        A, x0, y0, sx, sy, c = p
        dx, dy = (idx % width) - x0, (idx // width) - y0
        g = np.exp(-dx * dx / (2.0 * sx * sx) - dy * dy / (2.0 * sy * sy))
        f, cols = A * g + c, [g, A * g * dx / sx ** 2, A * g * dy / sy ** 2, A * g * dx * dx / sx ** 3, A * g * dy * dy / sy ** 3, one]
    else:
        raise ValueError(kind)
    with np.errstate(all="ignore"):
        return s * (f - y), s[:, None] * np.stack(cols, axis=1)


class HostModel:
    """one problem of a built-in model on the host: what the NumPy oracles take as hp"""

    def __init__(self, kind, y, p0, t=None, scale=None, width=0):
        self.kind, self.y, self.t, self.scale, self.width = kind, np.asarray(y, dtype=np.float64), t, scale, width
        self.N, self.M = MODEL_NSTATE[kind], self.y.shape[0]
        self._p0 = np.array(p0, dtype=np.float64).reshape(self.N)
        self._keep = None

    def p0(self):
        return self._p0.copy()

    def eval(self, p):
        return model_eval(self.kind, p, self.y, self.t, self.scale, self.width)

    @property
    def cb(self):
        """a dense host callback (tests/batch_oracle.py, the C oracle)"""
        if self._keep is None:
            N, M = self.N, self.M

            def f(p, x, J, cookie):
                xv, Jv = self.eval(np.ctypeslib.as_array(p, shape=(N,)).copy())
                np.ctypeslib.as_array(x, shape=(M,))[:] = xv
                np.ctypeslib.as_array(J, shape=(M, N))[:] = Jv

            self._keep = CB_DENSE(f)
        return C.cast(self._keep, C.c_void_p)

    cookie = None


def problem(case, seed, t_mode=None, with_scale=False):
    """dict(y, p0, truth, t, scale) of one seed of a case; t_mode: None, "shared" or "each"; t, scale: (M,) or None.  The noise
    and the start do not depend on the variant"""
    kind, _ = case
    M, w, h = case_shape(case)
    rng = np.random.default_rng([17, kind, M, w, int(seed)])
    u = rng.uniform(-1.0, 1.0, size=8)
    noise = NOISE * rng.standard_normal(M)
    start = rng.uniform(-1.0, 1.0, size=6)
    scale = rng.uniform(0.5, 2.0, size=M)
    jitter_each = rng.uniform(-0.3, 0.3, size=M)
    t = None
    if not is_2d(kind):
        t = np.arange(M, dtype=np.float64)
        if t_mode == "shared":
            t = 0.25 * (t + np.random.default_rng([23, kind, M]).uniform(-0.3, 0.3, size=M))
        elif t_mode == "each":
            t = 0.25 * (t + jitter_each)
        span = float(t[-1] - t[0])
    A, c = 7.5 + 2.5 * u[0], 1.5 + 0.5 * u[1]
    if kind == MODEL_EXPDECAY:
        truth = np.array([A, (3.5 + 1.5 * u[2]) / span, c])
        rel = np.array([0.15, 0.15, 0.15])
        p0 = truth * (1.0 + rel * start[:3])
    elif kind == MODEL_GAUSS1D:
        sigma = (0.16 + 0.04 * u[3]) * span
        truth = np.array([A, t[0] + span * (0.5 + 0.1 * u[2]), sigma, c])
        p0 = truth * (1.0 + np.array([0.15, 0.0, 0.15, 0.15]) * start[:4]) + np.array([0.0, 0.3 * sigma * start[1], 0.0, 0.0])
    elif kind == MODEL_GAUSS2D:
        sigma = 1.3 + 0.3 * u[3]
        truth = np.array([A, (w - 1) / 2.0 + 0.7 * u[2], (h - 1) / 2.0 + 0.7 * u[4], sigma, c])
        p0 = truth * (1.0 + np.array([0.15, 0.0, 0.0, 0.15, 0.15]) * start[:5]) + np.array([0.0, 0.4 * start[1], 0.4 * start[2], 0.0, 0.0])
    else:
        sx, sy = 1.3 + 0.3 * u[3], 1.3 + 0.3 * u[5]
        truth = np.array([A, (w - 1) / 2.0 + 0.7 * u[2], (h - 1) / 2.0 + 0.7 * u[4], sx, sy, c])
        p0 = (truth * (1.0 + np.array([0.15, 0.0, 0.0, 0.15, 0.15, 0.15]) * start[:6]) +
              np.array([0.0, 0.4 * start[1], 0.4 * start[2], 0.0, 0.0, 0.0]))
    x, _ = model_eval(kind, truth, np.zeros(M), None if is_2d(kind) else t, None, w)
    return dict(y=x + noise, p0=p0, truth=truth, t=None if t_mode is None else t, scale=scale if with_scale else None)


def bounds_of(case, b, truth):
    """(lo, hi) of problem b of a bounded table: the module's docstring"""
    kind, _ = case
    N = MODEL_NSTATE[kind]
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    if b % 6 == 0:
        lo[N - 1] = truth[N - 1] + 0.3
    elif b % 6 == 3:
        for i in {MODEL_EXPDECAY: (1,), MODEL_GAUSS1D: (2,), MODEL_GAUSS2D: (3,), MODEL_GAUSS2D_ELLIPTIC: (3, 4)}[kind]:
            hi[i] = 0.9 * truth[i]
    return lo, hi


def params(**over):
    prm = oa.default_params()
    for k, v in dict(STOP_OVER, **over).items():
        setattr(prm, k, v)
    return prm


def batch(case, seed0=None, nb=B, t_mode=None, with_scale=False):
    """the arrays of a batch: dict(kind, M, width, height, y (nb, M), p0 (nb, N), truth (nb, N), t (M,) / (nb, M) / None,
    scale (nb, M) / None, lo (nb, N), hi (nb, N))"""
    kind, _ = case
    M, w, h = case_shape(case)
    seed0 = SEED0.get(case, 1) if seed0 is None else seed0
    ps = [problem(case, seed0 + b, t_mode, with_scale) for b in range(nb)]
    los, his = zip(*[bounds_of(case, b, ps[b]["truth"]) for b in range(nb)])
    t = None if t_mode is None else ps[0]["t"] if t_mode == "shared" else np.array([q["t"] for q in ps])
    return dict(kind=kind, M=M, width=w, height=h, y=np.array([q["y"] for q in ps]), p0=np.array([q["p0"] for q in ps]),
                truth=np.array([q["truth"] for q in ps]), t=t, scale=np.array([q["scale"] for q in ps]) if with_scale else None,
                lo=np.array(los), hi=np.array(his), t_mode=t_mode)


def host_model(bt, b, p0=None):
    t = bt["t"] if bt["t"] is None or bt["t"].ndim == 1 else bt["t"][b]
    return HostModel(bt["kind"], bt["y"][b], bt["p0"][b] if p0 is None else p0, t,
                     None if bt["scale"] is None else bt["scale"][b], bt["width"])


@functools.lru_cache(maxsize=None)
def oracle_table(case, bounded, seed0=None, nb=B):
    """the oracle's solves of the base variant of a case (no scale, t_i = i): a list of batch_bounds_oracle.solve_one results.
    Cached and never modified: the tests share it"""
    bt = batch(case, seed0, nb)
    loss = ro.Loss(LOSS_TRIVIAL, 1.0, 1)
    prm = params()
    return [bb.solve_one(host_model(bt, b), prm, loss, bt["lo"][b] if bounded else None, bt["hi"][b] if bounded else None)
            for b in range(nb)]


def find_seed0(case, nb=B, start=1, tries=20000, floor=MARGIN_FLOOR):
    """the first seed0 >= start such that the problems seed0 .. seed0 + nb - 1 all lie above `floor` in the plain and in the
    bounded table and end in JTX or SMALL_STEP; (seed0, the smallest margin).  Problem b's bounds depend on b mod 6, so a window
    is solved anew where it moves by something that is no multiple of 6"""
    loss, prm = ro.Loss(LOSS_TRIVIAL, 1.0, 1), params()
    memo = {}

    def margin(seed, phase):
        if (seed, phase) not in memo:
            q = problem(case, seed)
            hp = HostModel(case[0], q["y"], q["p0"], None, None, case_shape(case)[1])
            lo, hi = bounds_of(case, phase, q["truth"])
            m = np.inf
            for o in (bb.solve_one(hp, prm, loss), bb.solve_one(hp, prm, loss, lo, hi)):
                m = min(m, o["margin"] if o["status"] in (1, 2) else -1.0)
            memo[(seed, phase)] = m
        return memo[(seed, phase)]

    s0 = start
    while s0 < start + tries:
        bad = next((b for b in range(nb - 1, -1, -1) if margin(s0 + b, b % 6) <= floor), None)
        if bad is None:
            return s0, min(margin(s0 + b, b % 6) for b in range(nb))
        s0 += bad + 1
    raise RuntimeError("no seed0 found")


if __name__ == "__main__":
    for case in CASES:
        print(case, find_seed0(case), flush=True)
