"""tests/exact_ei.py: the exact expected improvement against a plain Fraction loop, and the fixtures' properties --
what makes them tell the value from the solved system apart from the pass over J on any machine (LAPACK's Cholesky)."""
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg as sla

from libdogleg_amd import capi
from tests import exact_ei as xe
from tests import oracle_api as oa

EPS = sys.float_info.epsilon
ERR_MAX = 1e-12         # dlg_backend::IDENT_ERR_MAX (libdogleg_amd/csrc/dlg_internal.h)
FIX = xe.fixtures()


def _fraction_ei(D, x, s):
    F = [[Fraction(v) for v in row] for row in D]
    xs, ss = [Fraction(v) for v in x], [Fraction(v) for v in s]
    Js = [sum(a * b for a, b in zip(row, ss)) for row in F]
    return float(-2 * sum(a * b for a, b in zip(xs, Js)) - sum(v * v for v in Js))


def test_the_exact_value_is_the_fraction_loop():
    """dense and CSR forms against Fraction arithmetic written out, on values over 60 binary orders of magnitude and on a
    step where the float64 formula loses every digit"""
    rng = np.random.default_rng(5)
    for M, N in ((7, 3), (30, 11), (64, 64)):
        D = rng.standard_normal((M, N)) * np.exp2(rng.integers(-30, 30, (M, N)))
        D[rng.random((M, N)) < 0.3] = 0.0
        x, s = rng.standard_normal(M), rng.standard_normal(N) * np.exp2(rng.integers(-20, 20, N))
        want = _fraction_ei(D, x, s)
        assert xe.expected_improvement(D, x, s) == want
        Jp = np.concatenate([[0], np.cumsum((D != 0).sum(1))]).astype(np.int32)
        Ji = np.concatenate([np.flatnonzero(r) for r in D]).astype(np.int32)
        assert xe.expected_improvement((Jp, Ji, D[D != 0]), x, s) == want
    # -2 <Jt x, s> and |J s|^2 equal to 1e-17: the float64 formula returns 0 or noise, the exact value is 2^-60
    D = np.array([[1.0, 0.0], [0.0, 1.0]])
    s = np.array([1.0, 2.0 ** -30])
    x = -0.5 * (D @ s)
    x[1] -= 2.0 ** -60 / s[1] / 2.0
    assert xe.expected_improvement(D, x, s) == _fraction_ei(D, x, s) == 2.0 ** -60


def test_the_products_form_is_the_pass_over_J_where_the_products_are_exact():
    """small integers: JtJ and Jt x come out of float64 exactly, so both forms must give the same value"""
    rng = np.random.default_rng(6)
    D = rng.integers(-8, 9, (40, 12)).astype(np.float64)
    x = rng.integers(-8, 9, 40).astype(np.float64)
    s = rng.standard_normal(12)
    want = xe.expected_improvement(D, x, s)
    assert xe.expected_improvement_products(D.T @ x, np.ascontiguousarray(D.T @ D), s) == want
    assert want == _fraction_ei(D, x, s)


def test_the_chain_is_factored_in_its_own_order():
    """the product's symbolic analysis keeps the identity ordering for the chain, over several supernodes and levels:
    its sparse factor is Jt, every pivot 1"""
    kind, M, N, (Jp, Ji, Jx), x, _ = FIX["chain160"]
    st, perm = capi.symbolic_probe(N, M, Jp, Ji, want_perm=True)
    assert np.array_equal(perm, np.arange(N)), perm
    assert st["supernodes"] > 1 and st["levels"] > 1, st


def _lapack(D, x, lam):
    """the Gauss-Newton step by LAPACK's Cholesky; the value from the solved system and the pass over J for it"""
    N = D.shape[1]
    g = D.T @ x
    A = D.T @ D + lam * np.eye(N)
    L = np.linalg.cholesky(A)
    gn = -sla.cho_solve((L, True), g)
    Js = D @ gn
    jpass = -2.0 * (g @ gn) - Js @ Js
    solved = -2.0 * (g @ gn) + (g @ gn) + lam * (gn @ gn)
    est = EPS * np.diag(L).max() ** 2 * (gn @ gn) / -(g @ gn)
    return gn, jpass, solved, est, np.diag(L), np.linalg.cond(A)


@pytest.mark.parametrize("damped", [False, True], ids=["lambda0", "damped"])
@pytest.mark.parametrize("name", list(FIX))
def test_the_fixtures_tell_the_two_forms_apart(name, damped):
    """unit pivots, cond(JtJ + lambda I) in [1e11, 1e13]; the value from the solved system misses the exact value by more
    than 1e-8, the pass over J by less than 1e-11, and the error estimate of the product's gate is far above its bound"""
    kind, M, N, J, x, lam_d = FIX[name]
    lam = lam_d if damped else 0.0
    gn, jpass, solved, est, piv, cond = _lapack(xe.to_dense(J, N), x, lam)
    assert piv.max() / piv.min() <= 1.05, piv
    assert 1e11 <= cond <= 1e13, cond
    ex = xe.expected_improvement(J, x, gn)
    assert abs(solved - ex) > 1e-8 * abs(ex), (solved, ex)
    assert abs(jpass - ex) < 1e-11 * abs(ex), (jpass, ex)
    assert est > 1e3 * ERR_MAX, est


@pytest.mark.parametrize("shape", [dict(Nc=12, Np=120, Nobs=720), dict(Nc=37, Np=411, Nobs=5003)], ids=["tiny", "ragged"])
def test_the_gate_passes_bundle_adjustment(shape):
    """the error estimate on the shapes the value from the solved system is meant for: far below the product's bound"""
    prob = oa.BAProblem(**shape, seed=21)
    p = prob.p0()
    x, Jx = prob.eval(p)
    Jp, Ji = prob.pattern()
    D = xe.to_dense((Jp, Ji, Jx), prob.N)
    gn, jpass, solved, est, piv, cond = _lapack(D, x, 0.0)
    assert piv.max() / piv.min() <= 212.0
    assert est < 1e-2 * ERR_MAX, est
    ex = xe.expected_improvement((Jp, Ji, Jx), x, gn)
    assert abs(solved - ex) <= 1e-12 * abs(ex)
