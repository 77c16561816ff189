"""A NumPy restatement of the batch solver's loop for ONE problem under box bounds: the eight steps above
dogleg_amd_optimize_dense_batch_bounded (include/dogleg.h), on the products F, g, H, the Cholesky factorisation and the loop of
tests/batch_robust_oracle.py (with LOSS_TRIVIAL: norm2(x), Jt x, JtJ).  With bounds that clamp nothing every statement below
reduces to the one of batch_robust_oracle.solve_one, which tests/test_dense_batch_bounds_cpu.py holds it against.  Nothing of
the library under test computes a number in here."""
import numpy as np

from libdogleg_amd.ctypes_defs import (BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS, BATCH_FAILED,
                                       LOSS_HUBER)
from tests.batch_robust_oracle import LAMBDA_INITIAL, EPS, Loss, products, cholesky, _rel      # noqa: F401

FREE, AT_LOWER, AT_UPPER = 0, 1, 2


def held_set(p, g, lo, hi):
    """step 2: 0 free, 1 held at lower, 2 held at upper"""
    return np.where((p == lo) & (g > 0.0), AT_LOWER, np.where((p == hi) & (g < 0.0), AT_UPPER, FREE)).astype(np.uint8)


def clip(p, s, lo, hi):
    """step 5: (trial, the step applied, which components were clamped)"""
    t = p + s
    below, above = t < lo, t > hi
    t = np.where(below, lo, t)
    t = np.where(above, hi, t)
    clamped = below | above
    return t, np.where(clamped, t - p, s), clamped


def expected_improvement(g, H, s):
    return -2.0 * float(g @ s) - float(s @ H @ s)


def fallback_step(p, d, lo, hi, landing="bound"):
    """step 6 behind d = min(1, tr / |cauchy|) cauchy: (trial, the step applied, landings, margins).  The step is alpha d with
    alpha = min(1, min_i (far_i - p_i) / d_i) over the moving components, far the bound d_i points at.  landing == "bound", the
    rule of the library (k_bounds_fallback; batch_problem): a moving component whose own ratio equals alpha ends ON its bound,
    trial_i = far_i and step_i = far_i - p_i, whichever way p_i + alpha d_i rounds; the others are clipped as in step 5.
    landing == "sum": every component is p_i + alpha d_i, clipped -- what the rule replaces, kept for the tests that show what it
    changes.  landings: per component that the rule lands, what the sum would have done: "on" the bound's bits, "beyond" it
    (the clamp brings that back) or "short" of it.  margins: |alpha_raw - 1| relative (is the step cut at all) and, of a cut
    step, (r2 - r1) / r2 of the two smallest ratios (which component lands: a second one within rounding of the first would
    still land by its own sum)"""
    assert landing in ("bound", "sum")
    far = np.where(d > 0.0, hi, lo)
    mv = d != 0.0
    ratio = np.full(len(p), np.inf)
    ratio[mv] = (far[mv] - p[mv]) / d[mv]
    alpha_raw = float(np.min(ratio))
    alpha = min(1.0, alpha_raw)
    margins = [_rel(alpha_raw, 1.0)] if np.isfinite(alpha_raw) else []
    trial, step, _ = clip(p, alpha * d, lo, hi)
    land = mv & (ratio == alpha)
    landings = []
    if land.any():
        r = np.sort(ratio)
        if len(r) > 1 and np.isfinite(r[1]):
            margins.append((r[1] - r[0]) / r[1] if r[1] != 0.0 else 0.0)
        t = p + alpha * d
        for i in np.flatnonzero(land):
            past = t[i] > far[i] if d[i] > 0.0 else t[i] < far[i]
            landings.append("on" if t[i] == far[i] else "beyond" if past else "short")
        if landing == "bound":
            trial = np.where(land, far, trial)
            step = np.where(land, far - p, step)
    return trial, step, landings, margins


def solve_one(hp, prm, loss, lo=None, hi=None, max_rounds=100000, landing="bound"):
    """what batch_robust_oracle.solve_one returns, plus held (N,) at the returned point, clipped (steps with a clamped
    component), fallbacks, held_steps (steps taken with a held variable), held_resteps (of those, the ones behind a rejected
    trial), first_p (the first point evaluated) and landings (fallback_step's, over the solve).  margin also covers the new
    decisions: |g_i| against |g|_inf for variables on a bound, |p_i + s_i - bound_i| against max(|s_i|, |bound_i|) per
    component and bound, |EI'| against |2 g's'| + s''Hs' where a clip happened, the applied step against update_threshold, and
    fallback_step's two.  landing: fallback_step's"""
    N, M = hp.N, hp.M
    lo = np.full(N, -np.inf) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(N, np.inf) if hi is None else np.asarray(hi, dtype=np.float64)
    p_in = np.array(hp.p0(), dtype=np.float64)
    nothing = dict(held=np.zeros(N, dtype=np.uint8), clipped=0, fallbacks=0, held_steps=0, held_resteps=0, landings=[])
    # ---- 1. a NaN bound or lo > hi: FAILED alone, nothing evaluated
    if not np.all(lo <= hi):
        return dict(p=p_in, norm2_x=-1.0, trustregion=prm.trustregion0, lambda_=0.0, iterations=0, evaluations=0,
                    status=BATCH_FAILED, weights=np.full(M // loss.fs, np.nan), last_weights=None, step_types=set(), rejected=0,
                    margin=np.inf, huber_gap=np.inf, first_p=None, **nothing)
    p_trial = np.minimum(np.maximum(p_in, lo), hi)
    first_p = p_trial.copy()
    started = edge = have_cauchy = have_gn = False
    iters = evals = rejected = clipped_steps = fallbacks = held_steps = held_resteps = 0
    tr, lam = prm.trustregion0, 0.0
    F_b = EI = n2c = n2gn = 0.0
    p_b = g_b = H_b = w_b = cauchy = gn = held = g_F = None
    status = 0
    step_types, margins, huber, landings = set(), [], [], []

    def gradient_margins(p, g):
        gmax = float(np.max(np.abs(g)))
        on = (p == lo) | (p == hi)
        if on.any() and gmax > 0.0:
            margins.append(float(np.min(np.abs(g[on]))) / gmax)

    for _ in range(max_rounds):
        x, J = hp.eval(p_trial)
        evals += 1
        F, g, H, w, s = products(x, J, loss)
        if loss.kind == LOSS_HUBER:
            huber.append(float(np.min(np.abs(s - loss.c))) / loss.c)
        take = restep = False
        if not (np.isfinite(F) and np.all(np.isfinite(g)) and np.all(np.isfinite(np.diag(H)))):
            status = BATCH_FAILED
        elif not started:
            take = True
        else:
            rho = (F_b - F) / EI
            if rho != rho:
                status = BATCH_FAILED
            else:
                rho_err = 2.0 * M * EPS * F_b / abs(EI)
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
            F_b, g_b, H_b, w_b, p_b = F, g, H, w, p_trial.copy()
            # ---- 2., 3. the held set and the free gradient of the point now stepped from
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
        # (a rejected trial: the held set is the same function of p_b, g_b and the bounds, so the cached steps are its steps)
        any_held = bool(np.any(held != FREE))
        held_steps += any_held
        held_resteps += any_held and restep
        # ---- take_step on the free set
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
                    # ---- 4. lambda first, then the held rows and columns become those of the identity
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
                y = np.linalg.solve(L, g_F)
                gn = -np.linalg.solve(L.T, y)
                gn[held != FREE] = 0.0          # (exactly 0: the rows of the identity)
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
        # ---- 5. clip
        t = p_b + step
        for bound in (lo, hi):
            fin = np.isfinite(bound)
            if fin.any():
                den = np.maximum(np.abs(step[fin]), np.abs(bound[fin]))
                gap = np.abs(t[fin] - bound[fin])
                ok = den > 0.0
                # (a component that does not move and sits on its bound decides nothing: clamped or not, it stays)
                ok &= ~((step[fin] == 0.0) & (p_b[fin] == bound[fin]))
                if ok.any():
                    margins.append(float(np.min(gap[ok] / den[ok])))
        trial, step, clamped = clip(p_b, step, lo, hi)
        EI = expected_improvement(g_b, H_b, step)
        smax = float(np.max(np.abs(step)))
        if clamped.any():
            clipped_steps += 1
            margins.append(abs(EI) / (abs(2.0 * float(g_b @ step)) + float(step @ H_b @ step)))
            # ---- 6. the fallback
            if EI <= 0.0 or smax <= prm.update_threshold:
                fallbacks += 1
                trial, step, landed, ms = fallback_step(p_b, min(1.0, tr / np.sqrt(n2c)) * cauchy, lo, hi, landing)
                landings += landed
                margins += ms
                EI = expected_improvement(g_b, H_b, step)
                smax = float(np.max(np.abs(step)))
                edge = bool(n2c >= tr2)
                if not (EI > 0.0) or not np.isfinite(EI):
                    status = BATCH_FAILED
                    break
        # ---- 7.
        margins.append(_rel(smax, prm.update_threshold))
        if smax <= prm.update_threshold:
            status = BATCH_SMALL_STEP
            break
        p_trial = trial
    else:
        raise RuntimeError("the oracle did not stop")
    failed = status == BATCH_FAILED
    weights = np.full(M // loss.fs, np.nan) if failed or w_b is None else w_b
    held_out = np.zeros(N, dtype=np.uint8) if failed or p_b is None else held_set(p_b, g_b, lo, hi)
    return dict(p=p_in if failed or p_b is None else p_b, norm2_x=-1.0 if failed else F_b, trustregion=tr,
                lambda_=lam, iterations=iters, evaluations=evals, status=status, weights=weights, last_weights=w,
                step_types=step_types, rejected=rejected, margin=min(margins + huber) if margins else np.inf,
                huber_gap=min(huber) if huber else np.inf, held=held_out, clipped=clipped_steps, fallbacks=fallbacks,
                held_steps=held_steps, held_resteps=held_resteps, first_p=first_p, landings=landings)
