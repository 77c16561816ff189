"""A NumPy restatement of the batch solver's loop for ONE problem with a robust loss: the decisions of batch_problem
(libdogleg_amd/csrc/dense_batch.hip), which are those of dogleg.c, on F = sum rho(s_f), g = sum w_f J_f' x_f and
H = sum w_f J_f' J_f with w_f = rho'(s_f), s_f = |x_f|^2 (include/dogleg.h: dogleg_amd_batch_loss_t).  x and J come from a
host model (tests/batch_oracle.py's HostProblem, problems/batch_offsets.py's OffsetHostProblem).  solve_one returns what
batch_oracle.solve_one returns plus the weights at the returned point and the smallest decision margin of the solve.  Under
LOSS_TRIVIAL it is the plain loop, which tests/test_dense_batch_robust_cpu.py holds against the C oracle.  Nothing of the
library under test computes a number in here."""
import numpy as np

from libdogleg_amd.ctypes_defs import (BATCH_JTX, BATCH_SMALL_STEP, BATCH_TRUSTREGION, BATCH_MAX_ITERATIONS, BATCH_FAILED,
                                       LOSS_TRIVIAL, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY)

LAMBDA_INITIAL = 1e-10
EPS = np.finfo(float).eps


class Loss:
    """kind, scale a, featureSize"""

    def __init__(self, kind, scale=1.0, fs=1):
        self.kind, self.a, self.fs = kind, float(scale), max(int(fs), 1)
        self.c = self.a * self.a

    def rho_w(self, s):
        """(rho(s), rho'(s)) elementwise"""
        s = np.asarray(s)
        c, a = self.c, self.a
        if self.kind == LOSS_TRIVIAL:
            return s.copy(), np.ones_like(s)
        if self.kind == LOSS_HUBER:
            r = np.sqrt(np.where(s > c, s, c))
            return np.where(s <= c, s, 2.0 * a * r - c), np.where(s <= c, np.ones_like(s), a / r)
        if self.kind == LOSS_SOFT_L1:
            r = np.sqrt(1.0 + s / c)
            return 2.0 * s / (r + 1.0), 1.0 / r          # (2 c (r - 1) without its cancellation)
        if self.kind == LOSS_CAUCHY:
            return c * np.log1p(s / c), 1.0 / (1.0 + s / c)
        raise ValueError(self.kind)

    def s(self, x):
        x = np.asarray(x)
        return (x.reshape(-1, self.fs) ** 2).sum(axis=1)

    def cost(self, x):
        return float(self.rho_w(self.s(x))[0].sum())


def products(x, J, loss):
    """(F, g, H, w, s) of one point"""
    s = loss.s(x)
    rho, w = loss.rho_w(s)
    wr = np.repeat(w, loss.fs)
    return float(rho.sum()), J.T @ (wr * x), J.T @ (wr[:, None] * J), w, s


def cholesky(A):
    """the lower factor by columns, or None where a pivot is <= 0 (chol_packed)"""
    L = np.array(A, dtype=np.float64, copy=True)
    n = L.shape[0]
    for j in range(n):
        if not L[j, j] > 0.0:
            return None
        d = np.sqrt(L[j, j])
        L[j, j] = d
        L[j + 1:, j] /= d
        c = L[j + 1:, j]
        L[j + 1:, j + 1:] -= np.outer(c, c)
    return np.tril(L)


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def solve_one(hp, prm, loss, max_rounds=100000):
    """dict(p, norm2_x (= F), trustregion, lambda_, iterations, evaluations, status, weights (at p), last_weights (at the last
    point evaluated, which a rejected trial makes another one), step_types, rejected, margin, huber_gap); step types as
    include/dlg_trace.h: 0 Cauchy, 1 Gauss-Newton, 2 interpolated.  margin: as batch_oracle.margin, the allowance for the rounding of the gain ratio from F;
    under LOSS_HUBER also the smallest relative gap of an s_f to c at any evaluated point (huber_gap; rho and rho' are continuous
    there, so no decision hangs on it)"""
    N, M = hp.N, hp.M
    p_trial = np.array(hp.p0(), dtype=np.float64)
    started = edge = have_cauchy = have_gn = False
    iters = evals = rejected = 0
    tr, lam = prm.trustregion0, 0.0
    F_b = EI = n2c = n2gn = 0.0
    p_b = g_b = H_b = w_b = cauchy = gn = None
    status = 0
    step_types, margins, huber = set(), [], []
    for _ in range(max_rounds):
        x, J = hp.eval(p_trial)
        evals += 1
        F, g, H, w, s = products(x, J, loss)
        if loss.kind == LOSS_HUBER:
            huber.append(float(np.min(np.abs(s - loss.c))) / loss.c)
        take = False
        if not (np.isfinite(F) and np.all(np.isfinite(g)) and np.all(np.isfinite(np.diag(H)))):
            status = BATCH_FAILED
        elif not started:
            take = True
            margins.append(_rel(float(np.max(np.abs(g))), prm.Jt_x_threshold))
        else:
            rho = (F_b - F) / EI
            if rho != rho:
                status = BATCH_FAILED
            else:
                # F is a sum of M / fs terms with a relative rounding error of at most M eps whatever the order of summation:
                # two correct implementations may differ in rho by rho_err; that much of the gap does not count
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
                    margins.append(_rel(float(np.max(np.abs(g))), prm.Jt_x_threshold))
                else:
                    rejected += 1
                    margins.append(_rel(tr, prm.trustregion_threshold))
                    if tr < prm.trustregion_threshold:
                        status = BATCH_TRUSTREGION
        if take:
            started, edge, have_cauchy, have_gn = True, False, False, False
            F_b, g_b, H_b, w_b, p_b = F, g, H, w, p_trial.copy()
            if float(np.max(np.abs(g_b))) <= prm.Jt_x_threshold:
                status = BATCH_JTX
            elif iters >= prm.max_iterations:
                status = BATCH_MAX_ITERATIONS
        if status != 0:
            break
        # ---- take_step
        tr2 = tr * tr
        if not have_cauchy:
            g2 = float(g_b @ g_b)
            k = -g2 / float(g_b @ H_b @ g_b)
            n2c, cauchy, have_cauchy = k * k * g2, k * g_b, True
        margins.append(_rel(n2c, tr2))
        if n2c >= tr2:
            step, edge = tr / np.sqrt(n2c) * cauchy, True
            step_types.add(0)
        else:
            if not have_gn:
                while True:
                    L = cholesky(H_b + lam * np.eye(N) if lam > 0.0 else H_b)
                    if L is not None:
                        break
                    lam = LAMBDA_INITIAL if lam == 0.0 else lam * 10.0
                    if not np.isfinite(lam):
                        status = BATCH_FAILED
                        break
                if status != 0:
                    break
                y = np.linalg.solve(L, g_b)
                gn = -np.linalg.solve(L.T, y)
                n2gn, have_gn = float(gn @ gn), True
            margins.append(_rel(n2gn, tr2))
            if n2gn <= tr2:
                step, edge = gn, False
                step_types.add(1)
            else:
                d = cauchy - gn
                l2, neg_c = float(d @ d), float(d @ cauchy)
                disc = max(neg_c * neg_c - l2 * (n2c - tr2), 0.0)
                k = (neg_c + np.sqrt(disc)) / l2
                step, edge = cauchy + k * (gn - cauchy), True
                step_types.add(2)
        EI = -2.0 * float(g_b @ step) - float(step @ H_b @ step)
        smax = float(np.max(np.abs(step)))
        margins.append(_rel(smax, prm.update_threshold))
        if smax <= prm.update_threshold:
            status = BATCH_SMALL_STEP
            break
        p_trial = p_b + step
    else:
        raise RuntimeError("the oracle did not stop")
    failed = status == BATCH_FAILED
    weights = np.full(M // loss.fs, np.nan) if failed or w_b is None else w_b
    return dict(p=np.array(hp.p0()) if failed or p_b is None else p_b, norm2_x=-1.0 if failed else F_b, trustregion=tr,
                lambda_=lam, iterations=iters, evaluations=evals, status=status, weights=weights, last_weights=w,
                step_types=step_types,
                rejected=rejected, margin=min(margins + huber) if margins else np.inf,
                huber_gap=min(huber) if huber else np.inf)

