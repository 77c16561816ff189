"""The expected improvement of a step in exact arithmetic, and Jacobians on which the shortcut for it goes wrong.

K8 (computeExpectedImprovement, dogleg.c:1085-1165) hands out

    -2 <Jt x, step> - |J step|^2                (DLG_SPARSE, DLG_DENSE)
    -2 <Jt x, step> - step' (JtJ) step          (DLG_DENSE_PRODUCTS: from the products the callback gave)

Here every float64 input is taken at its exact binary value, the whole expression is formed with integers under
one common power-of-two scale -- fractions.Fraction arithmetic without the gcd at every operation -- and rounded
to a double once, at the end.  Standard library and numpy only (numpy for the binary decomposition of the inputs,
which is exact).  Nothing here imports the product or the oracle.

The fixtures are Jacobians whose Cholesky factor has unit pivots (max L_ii / min L_ii = 1, any pivot-ratio test
lets them through) while cond(JtJ) is 1e11 - 1e13: the value of |J gn|^2 read off the solved system,
-<Jt x, gn> - lambda |gn|^2, then carries the solve's backward error times cond, and the pass over J does not.
"""
from fractions import Fraction

import numpy as np


def _ints(a):
    """float64 array -> (list of Python ints, e) with a[i] == ints[i] * 2**e exactly"""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    assert np.all(np.isfinite(a))
    m, ex = np.frexp(a)                                  # a = m 2^ex, |m| in [0.5, 1): m 2^53 is an integer
    mi = np.ldexp(m, 53).astype(np.int64)
    ex = ex.astype(np.int64) - 53
    nz = mi != 0
    e0 = int(ex[nz].min()) if nz.any() else 0
    sh = np.where(nz, ex - e0, 0)
    return [int(v) << int(s) for v, s in zip(mi.tolist(), sh.tolist())], e0


def _scaled(n, e):
    return Fraction(n * 2 ** e) if e >= 0 else Fraction(n, 2 ** -e)


def _Jv(J, v):
    """J v exactly: (list of ints, e).  J: dense (M, N) ndarray or (Jp, Ji, Jx) -- the rows of J in CSR form (the
    callback's CSC arrays of Jt)"""
    vi, ev = _ints(v)
    if isinstance(J, np.ndarray):
        M, N = J.shape
        Ji, eJ = _ints(J)
        rows = [sum(Ji[r * N + c] * vi[c] for c in range(N)) for r in range(M)]
    else:
        Jp, Jc, Jx = J
        Ji, eJ = _ints(Jx)
        Jp, Jc = np.asarray(Jp).tolist(), np.asarray(Jc).tolist()
        rows = [sum(Ji[k] * vi[Jc[k]] for k in range(Jp[r], Jp[r + 1])) for r in range(len(Jp) - 1)]
    return rows, eJ + ev


def expected_improvement(J, x, step):
    """-2 <Jt x, step> - |J step|^2 of float64 J, x, step in exact arithmetic, rounded once.
    J: dense (M, N) ndarray or (Jp, Ji, Jx) as the sparse callback gives it (CSR of J)."""
    Js, es = _Jv(J, step)
    xi, ex = _ints(x)
    assert len(xi) == len(Js)
    xJs = sum(a * b for a, b in zip(xi, Js))
    JsJs = sum(a * a for a in Js)
    return float(-2 * _scaled(xJs, ex + es) - _scaled(JsJs, 2 * es))


def expected_improvement_products(Jtx, JtJ, step):
    """-2 <Jt x, step> - step' JtJ step of float64 products (DLG_DENSE_PRODUCTS) in exact arithmetic, rounded once"""
    N = len(step)
    si, es = _ints(step)
    gi, eg = _ints(Jtx)
    Ai, eA = _ints(JtJ)
    gs = sum(a * b for a, b in zip(gi, si))
    sAs = sum(si[r] * sum(Ai[r * N + c] * si[c] for c in range(N)) for r in range(N))
    return float(-2 * _scaled(gs, eg + es) - _scaled(sAs, eA + 2 * es))


# ---------------------------------------------------------------------------------------------------- fixtures --
def dense_qr(M, N, c, seed):
    """J = Q R: Q an orthonormal M x N matrix, R = I - c triu(ones, 1).  JtJ = Rt R, so the Cholesky factor is Rt --
    every pivot is 1 -- while cond(R) grows like (1 + c)^N.  Returns (J, x), x a seeded residual vector."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((M, N)))
    R = np.eye(N) - c * np.triu(np.ones((N, N)), 1)
    return np.ascontiguousarray(Q @ R), rng.standard_normal(M)


def dense_as_csr(J):
    """the full pattern of a dense J: (Jp, Ji, Jx) with every row listing all N columns"""
    M, N = J.shape
    return (np.arange(0, (M + 1) * N, N, dtype=np.int32), np.tile(np.arange(N, dtype=np.int32), M),
            np.ascontiguousarray(J).ravel().copy())


def chain(N, t, seed):
    """the square upper bidiagonal J with rows e_i - t e_(i+1) (the last row e_(N-1)): JtJ is tridiagonal, and in the
    identity ordering its Cholesky factor is Jt itself, unit pivots; cond(J) grows like t^N.  Returns ((Jp, Ji, Jx), x)."""
    rng = np.random.default_rng(seed)
    Jp = np.concatenate([[0], np.cumsum([2] * (N - 1) + [1])]).astype(np.int32)
    Ji = np.array([c for i in range(N) for c in ((i, i + 1) if i < N - 1 else (i,))], dtype=np.int32)
    Jx = np.array([v for i in range(N) for v in ((1.0, -t) if i < N - 1 else (1.0,))])
    return (Jp, Ji, Jx), rng.standard_normal(N)


def to_dense(J, N):
    if isinstance(J, np.ndarray):
        return J
    Jp, Ji, Jx = J
    D = np.zeros((len(Jp) - 1, N))
    for r in range(len(Jp) - 1):
        D[r, Ji[Jp[r]:Jp[r + 1]]] = Jx[Jp[r]:Jp[r + 1]]
    return D


# name -> (backend type, M, N, J, x, lambda > 0).  J: the dense ndarray for DLG_DENSE, (Jp, Ji, Jx) for DLG_SPARSE.
# cond(JtJ) 6e11 - 3e12 with unit pivots; the damped lambda keeps cond(JtJ + lambda I) above 5e11.  N = 130 is not a
# multiple of 64, N = 256 takes the tiled dense factor / solve; "dense40_sparse" is the same J as "dense40" through the
# sparse path (all N columns in every row: one supernode); the chain is ordered as it stands (N <= 200: the identity),
# so its sparse factor is Jt itself -- several supernodes and levels.
def fixtures():
    out = {}
    for name, (M, N, c) in {"dense40": (200, 40, 0.35), "dense130": (200, 130, 0.1), "dense256": (400, 256, 0.052)}.items():
        J, x = dense_qr(M, N, c, seed=N)
        out[name] = ("dense", M, N, J, x, 1e-11)
        if N == 40:
            out["dense40_sparse"] = ("sparse", M, N, dense_as_csr(J), x, 1e-11)
    J, x = chain(160, 1.07, seed=3)
    out["chain160"] = ("sparse", 160, 160, J, x, 1e-12)
    return out
