"""Patterns that are not bundle adjustment, and an extended-precision reference, for the users of the held factor
(dlg_solve_with_factor, dlg_solve_multi, dlg_pseudoinverse_chunk, dlg_feature_leverage, dlg_covariance_blocks,
dlg_marginal_variances, dlg_covariance_entries, dlg_query_covariance).  HELPER of test_factor_users_zoo_cpu.py and
test_factor_users_zoo_gpu.py; no library call is made here.

zoo() returns the named cases; each puts a shape edge of the blocked kernels (k_msolve_fwd_level, k_msolve_bwd_level,
k_lev_fwd_level, k_cov_fwd_level, the selected inverse) in front of them -- STRUCTURE below is what
test_factor_users_zoo_cpu.py asserts of the symbolic phase, so that a case stays on its edge:

  dense-N        every row touches every variable: ONE supernode of width N with no rows below.  128 is the widest
                 supernode the blocked kernels take, 65 the first width with a second column tile in the backward
                 product, 17 and 127 are off the 8-column step of the forward product and off the 16-row tile.  (With
                 no rows below, the products below the top block have no terms: these cases are about the staging and
                 the sweeps of the whole top block.  dense-129, the arrows, wide-* and ba-tiny have wide supernodes
                 WITH rows below, and those reach the second column tile.)
  dense-129      the first width that is cut: supernodes of 120 and 9 columns
  scattered      2 - 6 random variables a row: fill, a wide root
  banded         a long elimination chain: many levels, narrow supernodes
  holes          empty rows, variables that no row touches (Sigma_ii = 1 / lambda there)
  arrow-BxK+T    K leaf blocks of B variables that meet only in a tail of T variables: sibling leaves merged into one
                 supernode (a block-diagonal top of 63 / 64 columns, correct only where its off-diagonal part was cleared),
                 roots of 5 / 17 / 70 / 128 columns; the last one's selected-inverse fronts do not fit LDS
  wide-children, wide-root   two dense groups with a shared dense separator (test_selected_inverse_gpu._wide_problem)
  ba-tiny        the control: a bundle-adjustment problem

truth(case) is inv(JtJ + lambda I) in numpy.longdouble (the 80-bit type: asserted), refined from the float64 inverse by
X <- X + X (I - A X), at most 4 times, until max|I - A X| <= 2^-60 max(1, g) with g the growth of the residual's own sums
(residual_floor: the 80-bit format cannot show 2^-60 itself where g > 1; g is 1.6 .. 3e3 here).  On every case the first
refinement meets it.  The correction X (I - A X) is 1e-13 of X and less and is formed in float64; the residual is not.

Error measures (u = 2^-53, kappa = numpy.linalg.cond of the float64 JtJ + lambda I: a property of the reference alone):
  solves, pseudoinverse rows   per right-hand side max|got - want| / max|want|
  entries of Sigma             |got_ij - Sigma_ij| / sqrt(Sigma_ii Sigma_jj)
  leverage and query blocks    entry (a, c) scaled by sqrt(A_aa A_cc) of the exact block A; an exact 0 must come back as 0.0
  bound for all of them        max(16 u kappa, 64 N u)
u kappa is the first-order forward error of a backward-stable solve (the blocked sweeps multiply by inverted diagonal
tiles, which stays within that class); 64 N u is a floor for sums of N terms taken in another order.  The bound comes from
the reference and the number format, never from what the library returns.

What plain float64 numpy (numpy.linalg.inv) loses against truth(), entries of Sigma, beside the bound
(test_factor_users_zoo_cpu.py keeps this table true: kappa and bound to 5 %, the error within a factor of 8):

TABLE
  case              N      kappa    float64 inv      bound
  dense-16          16   3.34e+01        8.0e-16   1.14e-13
  dense-17          17   1.86e+01        1.5e-15   1.21e-13
  dense-64          64   2.51e+01        1.3e-15   4.55e-13
  dense-65          65   2.89e+01        2.3e-15   4.62e-13
  dense-127        127   2.85e+01        2.3e-15   9.02e-13
  dense-128        128   3.28e+01        2.3e-15   9.09e-13
  dense-129        129   2.82e+01        2.4e-15   9.17e-13
  scattered        120   8.49e+00        1.1e-15   8.53e-13
  banded           400   1.64e+04        2.6e-13   2.92e-11
  holes             60   3.82e+04        7.4e-16   6.78e-11
  arrow-3x60+70    250   2.39e+04        3.1e-14   4.25e-11
  arrow-1x300+5    305   2.87e+03        1.6e-14   5.10e-12
  arrow-3x200+17   617   1.21e+04        2.7e-14   2.14e-11
  arrow-9x40+128   488   9.38e+03        5.7e-13   1.67e-11
  wide-children    240   1.14e+02        4.5e-15   1.71e-12
  wide-root        208   4.27e+01        2.6e-15   1.48e-12
  ba-tiny          438   1.22e+02        1.7e-15   3.11e-12
ENDTABLE
"""
import functools

import numpy as np

assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is not the 80-bit extended type on this machine"

U = 2.0 ** -53
DENSE_N = (16, 17, 64, 65, 127, 128, 129)
ARROWS = ((3, 60, 70), (1, 300, 5), (3, 200, 17), (9, 40, 128))          # (block width, blocks, tail)

# what the symbolic phase makes of each case: (supernodes, levels) of capi.symbolic_probe, wmax of
# capi.covariance_entries_probe.  A change of the supernode rules that moves a case off its edge fails here: the case is
# then chosen again, the claim is not dropped.
STRUCTURE = {f"dense-{n}": (1, 1, n) for n in (16, 17, 64, 65, 127, 128)}
STRUCTURE.update({
    "dense-129": (2, 2, 120),
    "scattered": (12, 3, 108),
    "banded": (28, 15, 16),
    "holes": (12, 3, 45),
    "arrow-3x60+70": (4, 2, 70),            # 3 merged leaves of 21 blocks (63 columns, the last 54) and the root
    "arrow-1x300+5": (6, 2, 64),            # 5 merged leaves of 64 blocks (the last 44) and the root
    "arrow-3x200+17": (11, 2, 63),          # 10 merged leaves and the root
    "arrow-9x40+128": (81, 4, 121),
    "wide-children": (5, 3, 92),
    "wide-root": (5, 4, 96),
    "ba-tiny": (8, 6, 99),
})
FRONT_DOUBLES = {"arrow-9x40+128": 665640}                 # the selected inverse's front scratch: more than LDS holds


def _rows_to_csr(rows):
    Jp, Ji = [0], []
    for r in rows:
        Ji.extend(sorted(set(int(i) for i in r)))
        Jp.append(len(Ji))
    return np.array(Jp, dtype=np.int32), np.array(Ji, dtype=np.int32)


def _dense(N):
    rng = np.random.default_rng(N)
    M = 2 * N
    Jp = np.arange(0, (M + 1) * N, N, dtype=np.int32)
    Ji = np.tile(np.arange(N, dtype=np.int32), M)
    return N, M, Jp, Ji, rng.standard_normal(M * N), rng.standard_normal(M), 0.0


def _scattered():
    rng = np.random.default_rng(3)
    N, M = 120, 900
    Jp, Ji = _rows_to_csr([rng.choice(N, size=rng.integers(2, 7), replace=False) for _ in range(M)])
    return N, M, Jp, Ji, rng.standard_normal(Jp[-1]), rng.standard_normal(M), 0.0


def _banded():
    rng = np.random.default_rng(5)
    N = 400
    rows = [[i, i + 1, i + 2] for i in range(N - 2)] + [[i] for i in range(0, N, 7)]
    Jp, Ji = _rows_to_csr(rows)
    return N, len(rows), Jp, Ji, rng.standard_normal(Jp[-1]) + 2.0, rng.standard_normal(len(rows)), 0.0


def _holes():
    rng = np.random.default_rng(6)
    N, M = 60, 200
    rows = [[] if r % 17 == 0 else rng.choice(np.arange(0, N - 5), size=4, replace=False) for r in range(M)]
    Jp, Ji = _rows_to_csr(rows)
    return N, M, Jp, Ji, rng.standard_normal(Jp[-1]), rng.standard_normal(M), 1e-3


def _arrow(bw, nb, tail):
    """6 rows a block: a block of more than 6 variables has no full column rank, such a case gets a lambda"""
    lam = 0.0 if bw <= 6 else 0.1
    rng = np.random.default_rng(1000 * bw + nb)
    N = bw * nb + tail
    t = np.arange(bw * nb, N)
    rows = [np.r_[bw * b:bw * (b + 1), t] for b in range(nb) for _ in range(6)] + [t] * (tail + 10)
    Jp, Ji = _rows_to_csr(rows)
    return N, len(rows), Jp, Ji, rng.standard_normal(Jp[-1]), rng.standard_normal(len(rows)), lam


def _wide(wa, ws):
    from tests.test_selected_inverse_gpu import _wide_problem
    N, M, Jp, Ji, Jx, x = _wide_problem(wa, ws, wa + ws + 40, 7)
    return N, M, Jp, Ji, Jx, x, 1e-3


def _ba_tiny():
    from tests import oracle_api as oa
    prob = oa.BAProblem(12, 120, 720, seed=3)
    x, Jx = prob.eval(prob.p0())
    Jp, Ji = prob.pattern()
    return prob.N, prob.M, Jp, Ji, Jx, x, 0.0


_MAKERS = {f"dense-{n}": functools.partial(_dense, n) for n in DENSE_N}
_MAKERS.update({"scattered": _scattered, "banded": _banded, "holes": _holes})
_MAKERS.update({f"arrow-{bw}x{nb}+{t}": functools.partial(_arrow, bw, nb, t) for bw, nb, t in ARROWS})
_MAKERS.update({"wide-children": functools.partial(_wide, 100, 40), "wide-root": functools.partial(_wide, 40, 128),
                "ba-tiny": _ba_tiny})
NAMES = tuple(_MAKERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(N, M, Jp, Ji, Jx, x, lam) of one named case; the arrays are shared: leave them unchanged"""
    N, M, Jp, Ji, Jx, x, lam = _MAKERS[name]()
    out = (int(N), int(M), np.ascontiguousarray(Jp, dtype=np.int32), np.ascontiguousarray(Ji, dtype=np.int32),
           np.ascontiguousarray(Jx, dtype=np.float64), np.ascontiguousarray(x, dtype=np.float64), float(lam))
    for a in out[2:6]:
        a.setflags(write=False)
    return out


def zoo():
    """{name: (N, M, Jp, Ji, Jx, x, lam)}"""
    return {name: case(name) for name in NAMES}


@functools.lru_cache(maxsize=None)
def dense_J(name):
    N, M, Jp, Ji, Jx, _, _ = case(name)
    J = np.zeros((M, N))
    for r in range(M):
        J[r, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def system(name):
    """the float64 A = JtJ + lambda I and its condition number"""
    N, lam = case(name)[0], case(name)[6]
    J = dense_J(name)
    A = J.T @ J + lam * np.eye(N)
    A.setflags(write=False)
    return A, float(np.linalg.cond(A))


def bound(name):
    return max(16.0 * U * system(name)[1], 64.0 * case(name)[0] * U)


@functools.lru_cache(maxsize=None)
def truth(name):
    """inv(JtJ + lambda I) in numpy.longdouble, converged (asserted; see residual_floor): (X, max|I - A X|)"""
    N, M, Jp, Ji, Jx, _, lam = case(name)
    A = np.longdouble(lam) * np.eye(N, dtype=np.longdouble)
    for r in range(M):                                     # JtJ row by row: only the entries a row holds
        idx = Ji[Jp[r]:Jp[r + 1]]
        v = Jx[Jp[r]:Jp[r + 1]].astype(np.longdouble)
        A[np.ix_(idx, idx)] += np.outer(v, v)
    eye = np.eye(N, dtype=np.longdouble)
    X = np.linalg.inv(system(name)[0]).astype(np.longdouble)
    for rounds in range(5):                                # at most 4 refinements
        R = eye - A @ X
        res = float(np.max(np.abs(R)))
        floor = residual_floor(A, X)
        if res <= floor:
            break
        if rounds < 4:
            # (the correction is 1e-13 of X and less: float64 carries it further than the 80-bit format can hold)
            X = X + (X.astype(np.float64) @ R.astype(np.float64)).astype(np.longdouble)
    assert res <= floor, f"{name}: the extended-precision inverse did not converge (max|I - A X| = {res:.2e} > {floor:.2e})"
    # the reference's own error is out of the picture: |X - inv A| <= |inv A| |R|, and N max|R| is far below the bound
    assert N * res <= bound(name) / 256, (name, res)
    X.setflags(write=False)
    return X, res


def residual_floor(A, X):
    """2^-60 where the 80-bit format can show it.  Entry (i, j) of I - A X is a sum of N products that cancel to nothing,
    and the computed value carries the rounding of that sum: a few 2^-64 times sum_k |A_ik| |X_kj|.  That sum is the
    growth g = max_ij (|A| |X|)_ij, 1.6 on `scattered` and 3e3 on `banded`, and no refinement in this format gets the
    COMPUTED residual below it: on `banded` it is 1.7e-13 for the float64 inverse, 1.4e-16 after the first refinement --
    which meets the criterion, 2.8e-15 there, so truth() stops -- and further rounds would only move it about (1.1e-16,
    1.1e-16, 6.9e-17 after the second to fourth; 2^-60 is 8.7e-19).  The criterion is
    therefore max|I - A X| <= 2^-60 max(1, g)."""
    return 2.0 ** -60 * max(1.0, float(np.max(np.abs(A).astype(np.float64) @ np.abs(X).astype(np.float64))))


# ---------------------------------------------------------------- error measures
def solve_error(got, want):
    """rows = right-hand sides: the worst max|got - want| / max|want| (want: longdouble)"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    d = np.max(np.abs(got.astype(np.longdouble) - want), axis=1)
    s = np.max(np.abs(want), axis=1)
    assert np.all(got[s == 0] == 0.0), "a solve whose exact value is 0 did not come back as 0.0"
    return float(np.max(np.where(s > 0, d / np.where(s > 0, s, 1), 0), initial=0.0))


def entry_error(got, want, di, dj):
    """entries of Sigma: |got - want| / sqrt(Sigma_ii Sigma_jj); di, dj the exact diagonal at the entries' rows and columns"""
    e = np.abs(np.asarray(got).astype(np.longdouble) - want) / np.sqrt(di * dj)
    return float(np.max(e, initial=0.0))


def block_error(got, want):
    """a leverage or query block against the exact A: entry (a, c) scaled by sqrt(A_aa A_cc); where that is 0 the
    exact entry is 0 (A is positive semi-definite) and the value must be exactly 0.0"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    d = np.diag(want)
    sc = np.sqrt(np.outer(d, d))
    zero = sc == 0
    assert np.all(got[zero] == 0.0), "an entry whose exact value is 0 did not come back as 0.0"
    e = np.abs(got.astype(np.longdouble) - want) / np.where(zero, 1, sc)
    return float(np.max(np.where(zero, 0, e), initial=0.0))


# ---------------------------------------------------------------- exact values of what the entry points return
def measurement_rows(name, r0, r1):
    """rows r0 .. r1 - 1 of J as (variables, values)"""
    _, _, Jp, Ji, Jx, _, _ = case(name)
    return [(Ji[Jp[r]:Jp[r + 1]], Jx[Jp[r]:Jp[r + 1]]) for r in range(r0, r1)]


def _dense_rows(rows, N, dtype):
    Q = np.zeros((len(rows), N), dtype=dtype)
    for i, (var, val) in enumerate(rows):
        np.add.at(Q[i], np.asarray(var, dtype=np.int64), np.asarray(val, dtype=dtype))      # a variable named twice: summed
    return Q


def exact_blocks(name, groups, S=None):
    """Q S Q^T for every group of rows (variables, values), S = truth(name) unless given: only the variables a group names
    are touched"""
    S = truth(name)[0] if S is None else S
    out = []
    for rows in groups:
        idx = np.unique(np.concatenate([np.asarray(v, dtype=np.int64) for v, _ in rows] + [np.zeros(0, dtype=np.int64)]))
        pos = {int(v): k for k, v in enumerate(idx)}
        Q = _dense_rows([([pos[int(v)] for v in var], val) for var, val in rows], len(idx), S.dtype)
        out.append(Q @ S[np.ix_(idx, idx)] @ Q.T)
    return out


def exact_sandwich_blocks(name, groups, nobs):
    """Q S J[:nobs]^T J[:nobs] S Q^T for every group of rows, in longdouble"""
    N = case(name)[0]
    S = truth(name)[0]
    Q = _dense_rows([r for rows in groups for r in rows], N, np.longdouble)
    T = dense_J(name)[:nobs].astype(np.longdouble) @ (S @ Q.T)
    out, o = [], 0
    for rows in groups:
        out.append(T[:, o:o + len(rows)].T @ T[:, o:o + len(rows)])
        o += len(rows)
    return out
