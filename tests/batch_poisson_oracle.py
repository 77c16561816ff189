"""A NumPy restatement of the Poisson maximum-likelihood fit of the built-in models (include/dogleg.h:
dogleg_amd_optimize_dense_batch_model_mle), written from the definition, not from include/dogleg_batch_models.h:

    cost  F(p) = sum_i d_i,  d_i = 2 (r_i - y_i log(f_i / y_i)),  r_i = f_i - y_i;  d_i = 2 f_i where y_i == 0.0
    g = sum (r_i / f_i) grad f_i = 1/2 grad F,   H = sum grad f_i grad f_i' / f_i  (the Fisher information)
    a row with !(f_i > 0) makes the point infeasible: F = +inf, the row adds nothing to g and H

and the loop of tests/batch_bounds_oracle.py restated on a products hook (solve_one below): statement by statement that loop, with
F, g, H from the hook.  An infeasible trial point is a rejected step by the ordinary rule (rho = -inf); an infeasible start point
fails.  With the least-squares hook (GAUSS) it reproduces batch_bounds_oracle.solve_one exactly, which
tests/test_dense_batch_poisson_cpu.py asserts.  Nothing of the library under test computes a number in here.

Decision margins: those of the bounds oracle, plus min_i |f_i| / (|A e_i| + |c|) at every evaluated point (how far a model value
lies from the feasibility test f > 0, relative to the terms it is summed from), and infeasible trials are counted.  The allowance
for the rounding of the gain ratio follows the cost: d_i = 2 (r_i - y_i lg_i) cancels (|r_i| ~ sqrt(f_i) against d_i ~ 1), f_i
carries about 6 eps of |A e_i| + |c| (tests/test_dense_batch_model_cpu.py) and dd_i / df_i = 2 r_i / f_i, the logarithm and the
quotient in it 1.5 eps, the product and the difference one eps each of their operands, the sum M eps of F:
    F_err = 2 eps (2 sum_i (14 k_i |r_i| + 4 |y_i lg_i|) + M F),  k_i = (|A e_i| + |c|) / f_i
for both points of a gain ratio together (the leading 2).  The same allowance says how well the returned cost itself is known: a
problem whose model nearly interpolates its data (M = 5 with N = 4 leaves one degree of freedom) can end with F ~ 1e-9 summed from
terms of size 1, and no two evaluations of the definition agree on such an F to 1e-8 relative.  So F_err / F <= COST_TOL = 1e-9 at
the returned point is one more condition a table's problems meet (cost_error; the seeds are chosen for it like for the margins).
A fallback step cut at a bound ends ON the bound by rule (batch_bounds_oracle.fallback_step, the library's rule: the component
whose own ratio sets alpha takes the bound, however p + alpha d rounds), so it is a decision like any other, with two margins:
is the step cut at all (|alpha_raw - 1|), and which component lands ((r2 - r1) / r2 of the two smallest ratios).  `landings` lists
what the plain sum would have done at each: "on", "beyond" or "short".

The tables.  The 14 shapes of tests/batch_models_np.CASES, B = 65, the problems of seeds SEED0 .. SEED0 + 64 of
batch_models_np.problem with the truth and the start moved to two count levels, data drawn from the Poisson distribution at the
truth:
    high   amplitude x 40, offset 10: no zero counts
    low    amplitude x 4, offset 0.3: 7 % (EXPDECAY) to 30 % (GAUSS2D 8 x 8) of the data are zero
plain and bounded.  Bounds of problem b: b mod 6 == 0: c >= 1.15 c_true; b mod 6 == 3: width <= 0.9 of the true width (EXPDECAY:
k); b mod 6 == 1: A >= 0; b mod 6 == 4: c >= 0; none otherwise.  Both stop at update_threshold = Jt_x_threshold = 1e-4: below
that the last steps improve F ~ M by less than its rounding error and the gain ratio of a step is noise.  SEED0 and the recorded
margins: find_seed0 below, run as `python -m tests.batch_poisson_oracle`."""
import functools

import numpy as np

from libdogleg_amd.ctypes_defs import (BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS, BATCH_FAILED,
                                       LOSS_TRIVIAL, MODEL_EXPDECAY, MODEL_GAUSS1D, MODEL_GAUSS2D, MODEL_GAUSS2D_ELLIPTIC,
                                       MODEL_NSTATE, LIKELIHOOD_GAUSS, LIKELIHOOD_POISSON)
from tests import batch_models_np as mz
from tests import batch_robust_oracle as ro
from tests.batch_bounds_oracle import FREE, held_set, clip, cholesky, expected_improvement, fallback_step, _rel
from tests.batch_robust_oracle import LAMBDA_INITIAL, EPS

B = mz.B
MARGIN_FLOOR = 1e-6
COST_TOL = 1e-9              # F_err / F of every returned point: a tenth of the 1e-8 the GPU tests ask of F (the docstring)
STOP_OVER = (("update_threshold", 1e-4), ("Jt_x_threshold", 1e-4))
LEVELS = {"high": (40.0, 10.0), "low": (4.0, 0.3)}          # amplitude factor, offset
CASES = mz.CASES
TABLES = [(case, level) for case in CASES for level in ("high", "low")]


# ---------------------------------------------------------------- the products
def gauss_products(hp):
    """the least-squares hook: (F, g, H, F_err, feasibility margin) as batch_bounds_oracle forms them"""
    loss = ro.Loss(LOSS_TRIVIAL, 1.0, 1)

    def hook(p):
        x, J = hp.eval(p)
        F, g, H, _, _ = ro.products(x, J, loss)
        return F, g, H, 2.0 * hp.M * EPS * F, np.inf, True

    return hook


def model_values(hp, p):
    """f (M,) and grad f (M, N) of the model at p"""
    return mz.model_eval(hp.kind, p, np.zeros(hp.M), hp.t, None, hp.width)


def poisson_products(hp):
    """the Poisson hook: (F, g, H, F_err, feasibility margin, feasible)"""
    y = hp.y

    def hook(p):
        f, G = model_values(hp, p)
        A, c = p[0], p[hp.N - 1]
        with np.errstate(all="ignore"):
            size = np.abs(f - c) + abs(c)            # |A e_i| + |c|
            fmargin = float(np.min(np.abs(f) / size)) if np.all(np.isfinite(f)) else 0.0
            ok = f > 0.0
            r = f - y
            lg = np.log(f / np.where(y == 0.0, 1.0, y))
            ylg = np.where(y == 0.0, 0.0, y * lg)
            d = np.where(y == 0.0, 2.0 * f, 2.0 * (r - ylg))
            rf = np.where(ok, r / f, 0.0)
            Gf = np.where(ok[:, None], G / f[:, None], 0.0)
            Gz = np.where(ok[:, None], G, 0.0)
            g = Gz.T @ rf
            H = Gz.T @ Gf
            if not ok.all():
                return np.inf, g, H, 0.0, fmargin, False
            F = float(np.sum(d))
            Ferr = 2.0 * EPS * (2.0 * float(np.sum(14.0 * size / f * np.abs(r) + 4.0 * np.abs(ylg))) + hp.M * abs(F))
        return F, g, H, Ferr, fmargin, True

    return hook


def products_of(hp, likelihood):
    return poisson_products(hp) if likelihood == LIKELIHOOD_POISSON else gauss_products(hp)


# ---------------------------------------------------------------- the loop
def solve_one(hp, prm, likelihood, lo=None, hi=None, max_rounds=100000, products=None, landing="bound"):
    """what batch_bounds_oracle.solve_one returns (without the weights), plus infeasible (trial points with a row !(f > 0)) and
    cost_error (F_err / F of the returned point: the relative rounding allowance of the returned cost).
    landing: batch_bounds_oracle.fallback_step's.  products: a hook p -> (F, g, H, F_err, feasibility margin, feasible), default: that of the likelihood"""
    N = hp.N
    products = products_of(hp, likelihood) if products is None else products
    lo = np.full(N, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(N, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    p_in = np.array(hp.p0(), dtype=np.float64)
    nothing = dict(held=np.zeros(N, dtype=np.uint8), clipped=0, fallbacks=0, held_steps=0, held_resteps=0, infeasible=0)
    if not np.all(lo <= hi):
        return dict(p=p_in, norm2_x=-1.0, trustregion=prm.trustregion0, lambda_=0.0, iterations=0, evaluations=0,
                    status=BATCH_FAILED, step_types=set(), rejected=0, margin=np.inf, first_p=None, cost_error=np.inf, landings=[], **nothing)
    p_trial = np.minimum(np.maximum(p_in, lo), hi)
    first_p = p_trial.copy()
    started = edge = have_cauchy = have_gn = False
    iters = evals = rejected = clipped_steps = fallbacks = held_steps = held_resteps = infeasible = 0
    tr, lam = prm.trustregion0, 0.0
    F_b = Ferr_b = EI = n2c = n2gn = 0.0
    p_b = g_b = H_b = cauchy = gn = held = g_F = None
    status = 0
    step_types, margins, landings = set(), [], []

    def gradient_margins(p, g):
        gmax = float(np.max(np.abs(g)))
        on = (p == lo) | (p == hi)
        if on.any() and gmax > 0.0:
            margins.append(float(np.min(np.abs(g[on]))) / gmax)

    for _ in range(max_rounds):
        F, g, H, Ferr, fmargin, feasible = products(p_trial)
        evals += 1
        margins.append(fmargin)
        take = restep = False
        # the cost of an infeasible point is +inf: no start point, but a trial point like any other once the problem has started
        cost_ok = np.isfinite(F) or (started and F == np.inf)
        if not (cost_ok and np.all(np.isfinite(g)) and np.all(np.isfinite(np.diag(H)))):
            status = BATCH_FAILED
        elif not started:
            take = True
        else:
            infeasible += not feasible
            rho = (F_b - F) / EI
            if rho != rho:
                status = BATCH_FAILED
            else:
                rho_err = Ferr_b / abs(EI)
                margins += [abs(rho - th) - rho_err
                            for th in (0.0, prm.trustregion_decrease_threshold, prm.trustregion_increase_threshold)]
                if rho < prm.trustregion_decrease_threshold:
                    if not edge:
                        tr = np.sqrt(n2gn)
                    tr *= prm.trustregion_decrease_factor
                elif rho > prm.trustregion_increase_threshold and edge:
                    tr *= prm.trustregion_increase_factor
                if rho > 0.0:
                    take = True
                    iters += 1
                else:
                    rejected += 1
                    restep = True
                    margins.append(_rel(tr, prm.trustregion_threshold))
                    if tr < prm.trustregion_threshold:
                        status = BATCH_TRUSTREGION
        if take:
            started, edge, have_cauchy, have_gn = True, False, False, False
            F_b, Ferr_b, g_b, H_b, p_b = F, Ferr, g, H, p_trial.copy()
            held = held_set(p_b, g_b, lo, hi)
            g_F = np.where(held != FREE, 0.0, g_b)
            gradient_margins(p_b, g_b)
            gfmax = float(np.max(np.abs(g_F)))
            margins.append(_rel(gfmax, prm.Jt_x_threshold))
            if gfmax <= prm.Jt_x_threshold:
                status = BATCH_JTX
            elif iters >= prm.max_iterations:
                status = BATCH_MAX_ITERATIONS
        if status != 0:
            break
        any_held = bool(np.any(held != FREE))
        held_steps += any_held
        held_resteps += any_held and restep
        tr2 = tr * tr
        if not have_cauchy:
            g2 = float(g_F @ g_F)
            k = -g2 / float(g_F @ H_b @ g_F)
            n2c, cauchy, have_cauchy = k * k * g2, k * g_F, True
        margins.append(_rel(n2c, tr2))
        if n2c >= tr2:
            step, edge = tr / np.sqrt(n2c) * cauchy, True
            kind = 0
        else:
            if not have_gn:
                while True:
                    Hl = H_b + lam * np.eye(N) if lam > 0.0 else H_b.copy()
                    h = held != FREE
                    Hl[h, :] = 0.0
                    Hl[:, h] = 0.0
                    Hl[h, h] = 1.0
                    L = cholesky(Hl)
                    if L is not None:
                        break
                    lam = LAMBDA_INITIAL if lam == 0.0 else lam * 10.0
                    if not np.isfinite(lam):
                        status = BATCH_FAILED
                        break
                if status != 0:
                    break
                z = np.linalg.solve(L, g_F)
                gn = -np.linalg.solve(L.T, z)
                gn[held != FREE] = 0.0
                n2gn, have_gn = float(gn @ gn), True
            margins.append(_rel(n2gn, tr2))
            if n2gn <= tr2:
                step, edge = gn, False
                kind = 1
            else:
                d = cauchy - gn
                l2, neg_c = float(d @ d), float(d @ cauchy)
                disc = max(neg_c * neg_c - l2 * (n2c - tr2), 0.0)
                k = (neg_c + np.sqrt(disc)) / l2
                step, edge = cauchy + k * (gn - cauchy), True
                kind = 2
        step_types.add(kind)
        t = p_b + step
        for bound in (lo, hi):
            fin = np.isfinite(bound)
            if fin.any():
                den = np.maximum(np.abs(step[fin]), np.abs(bound[fin]))
                gap = np.abs(t[fin] - bound[fin])
                ok = den > 0.0
                ok &= ~((step[fin] == 0.0) & (p_b[fin] == bound[fin]))
                if ok.any():
                    margins.append(float(np.min(gap[ok] / den[ok])))
        trial, step, clamped = clip(p_b, step, lo, hi)
        EI = expected_improvement(g_b, H_b, step)
        smax = float(np.max(np.abs(step)))
        if clamped.any():
            clipped_steps += 1
            margins.append(abs(EI) / (abs(2.0 * float(g_b @ step)) + float(step @ H_b @ step)))
            if EI <= 0.0 or smax <= prm.update_threshold:
                fallbacks += 1
                # (the landing rule and its two margins: batch_bounds_oracle.fallback_step, the one statement of step 6)
                trial, step, landed, ms = fallback_step(p_b, min(1.0, tr / np.sqrt(n2c)) * cauchy, lo, hi, landing)
                landings += landed
                margins += ms
                EI = expected_improvement(g_b, H_b, step)
                smax = float(np.max(np.abs(step)))
                edge = bool(n2c >= tr2)
                if not (EI > 0.0) or not np.isfinite(EI):
                    status = BATCH_FAILED
                    break
        margins.append(_rel(smax, prm.update_threshold))
        if smax <= prm.update_threshold:
            status = BATCH_SMALL_STEP
            break
        p_trial = trial
    else:
        raise RuntimeError("the oracle did not stop")
    failed = status == BATCH_FAILED
    held_out = np.zeros(N, dtype=np.uint8) if failed or p_b is None else held_set(p_b, g_b, lo, hi)
    return dict(p=p_in if failed or p_b is None else p_b, norm2_x=-1.0 if failed else F_b, trustregion=tr,
                lambda_=lam, iterations=iters, evaluations=evals, status=status,
                step_types=step_types, rejected=rejected, margin=min(margins) if margins else np.inf,
                held=held_out, clipped=clipped_steps, fallbacks=fallbacks,
                held_steps=held_steps, held_resteps=held_resteps, first_p=first_p, infeasible=infeasible,
                cost_error=Ferr_b / abs(F_b) if F_b != 0.0 else np.inf, landings=landings)


# ---------------------------------------------------------------- the tables
# the first seed of every table and the smallest margin of its plain and of its bounded table, as find_seed0 gave them
FOUND = {
    ((0, 5), 'high'): (743, 0.00556, 0.00206),
    ((0, 5), 'low'): (180453, 1.74e-05, 1.42e-05),
    ((0, 64), 'high'): (1, 0.0143, 0.000144),
    ((0, 64), 'low'): (1, 0.00795, 0.00262),
    ((0, 65), 'high'): (65, 0.000668, 0.000133),
    ((0, 65), 'low'): (65, 0.0037, 0.000404),
    ((0, 150), 'high'): (47, 0.00155, 9.76e-05),
    ((0, 150), 'low'): (1, 0.0272, 0.00109),
    ((1, 5), 'high'): (1, 0.00124, 0.000166),
    ((1, 5), 'low'): (728, 1.13e-06, 1.13e-06),
    ((1, 64), 'high'): (1, 0.00338, 0.000398),
    ((1, 64), 'low'): (14, 0.000784, 0.000784),
    ((1, 65), 'high'): (1, 0.00336, 0.00444),
    ((1, 65), 'low'): (11, 4.47e-05, 0.000346),
    ((1, 150), 'high'): (1, 0.00106, 0.00106),
    ((1, 150), 'low'): (1, 0.00239, 0.00973),
    ((2, (7, 7)), 'high'): (1, 0.00681, 0.00048),
    ((2, (7, 7)), 'low'): (22, 2.83e-05, 2.83e-05),
    ((2, (5, 9)), 'high'): (1, 0.00125, 0.00125),
    ((2, (5, 9)), 'low'): (1, 2.15e-05, 2.15e-05),
    ((2, (8, 8)), 'high'): (1, 0.00289, 0.00289),
    ((2, (8, 8)), 'low'): (1, 5.12e-05, 0.0009),
    ((3, (6, 7)), 'high'): (1, 0.00764, 0.00358),
    ((3, (6, 7)), 'low'): (96, 1.54e-05, 2.33e-05),
    ((3, (7, 7)), 'high'): (1, 0.00295, 0.00225),
    ((3, (7, 7)), 'low'): (1, 2.78e-05, 0.000146),
    ((3, (9, 5)), 'high'): (1, 0.000468, 0.000522),
    ((3, (9, 5)), 'low'): (67, 3.98e-06, 7.98e-06),
}
SEED0 = {t: v[0] for t, v in FOUND.items()}
MARGINS = {t: v[1:] for t, v in FOUND.items()}             # (plain, bounded)


def table_id(table):
    case, level = table
    return f"{mz.case_id(case)}-{level}"


def problem(case, level, seed):
    """dict(y, p0, truth) of one seed: the truth and the start of batch_models_np.problem at the level's counts, Poisson data"""
    kind, _ = case
    N = MODEL_NSTATE[kind]
    M, w, _ = mz.case_shape(case)
    q = mz.problem(case, seed)
    fac, off = LEVELS[level]
    truth, p0 = q["truth"].copy(), q["p0"].copy()
    p0[0] *= fac
    p0[N - 1] *= off / truth[N - 1]
    truth[0] *= fac
    truth[N - 1] = off
    f, _ = mz.model_eval(kind, truth, np.zeros(M), None, None, w)
    rng = np.random.default_rng([29, kind, M, w, int(seed), 0 if level == "high" else 1])
    return dict(y=rng.poisson(f).astype(np.float64), p0=p0, truth=truth)


def bounds_of(case, b, truth):
    kind, _ = case
    N = MODEL_NSTATE[kind]
    lo, hi = np.full(N, -np.inf), np.full(N, np.inf)
    if b % 6 == 0:
        lo[N - 1] = 1.15 * truth[N - 1]
    elif b % 6 == 3:
        for i in {MODEL_EXPDECAY: (1,), MODEL_GAUSS1D: (2,), MODEL_GAUSS2D: (3,), MODEL_GAUSS2D_ELLIPTIC: (3, 4)}[kind]:
            hi[i] = 0.9 * truth[i]
    elif b % 6 == 1:
        lo[0] = 0.0
    elif b % 6 == 4:
        lo[N - 1] = 0.0
    return lo, hi


def params(**over):
    return mz.params(**dict(STOP_OVER, **over))


def batch(table, seed0=None, nb=B):
    """the arrays of a table's batch, with the keys of batch_models_np.batch (t, scale: None)"""
    case, level = table
    kind, _ = case
    M, w, h = mz.case_shape(case)
    seed0 = SEED0.get(table, 1) if seed0 is None else seed0
    ps = [problem(case, level, seed0 + b) for b in range(nb)]
    los, his = zip(*[bounds_of(case, b, ps[b]["truth"]) for b in range(nb)])
    return dict(kind=kind, M=M, width=w, height=h, y=np.array([q["y"] for q in ps]), p0=np.array([q["p0"] for q in ps]),
                truth=np.array([q["truth"] for q in ps]), t=None, scale=None, lo=np.array(los), hi=np.array(his), t_mode=None)


@functools.lru_cache(maxsize=None)
def oracle_table(table, bounded, likelihood=LIKELIHOOD_POISSON, seed0=None, nb=B):
    """the oracle's solves of a table: a list of solve_one results.  Cached and never modified: the tests share it"""
    bt = batch(table, seed0, nb)
    prm = params()
    return [solve_one(mz.host_model(bt, b), prm, likelihood, bt["lo"][b] if bounded else None, bt["hi"][b] if bounded else None)
            for b in range(nb)]


def find_seed0(table, nb=B, start=1, tries=400000, floor=MARGIN_FLOOR):
    """the first seed0 >= start such that the problems seed0 .. seed0 + nb - 1 all lie above `floor` in the plain and in the
    bounded table, end in JTX or SMALL_STEP with a cost whose own rounding allowance lies below COST_TOL and, at the high level,
    have no zero count; (seed0, plain margin, bounded margin)"""
    case, level = table
    prm = params()
    memo = {}

    def margin(seed, phase):
        if (seed, phase) not in memo:
            q = problem(case, level, seed)
            hp = mz.HostModel(case[0], q["y"], q["p0"], None, None, mz.case_shape(case)[1])
            lo, hi = bounds_of(case, phase, q["truth"])
            ms = []
            for o in (solve_one(hp, prm, LIKELIHOOD_POISSON), solve_one(hp, prm, LIKELIHOOD_POISSON, lo, hi)):
                ms.append(o["margin"] if o["status"] in (BATCH_JTX, BATCH_SMALL_STEP) and o["cost_error"] <= COST_TOL else -1.0)
            if level == "high" and q["y"].min() == 0.0:
                ms = [-1.0, -1.0]
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
