"""The cases of tests/factor_user_zoo.py without a GPU: each still stands on the edge it was chosen for (the host probes of
the symbolic phase and of the selected inverse), is well enough conditioned, has a converged extended-precision
reference, and leaves an honest float64 solve an eighth of the bound or less in each of the three error measures.  The
table in the helper's docstring is kept true."""
import numpy as np
import pytest

from libdogleg_amd import capi
from tests import factor_user_zoo as zoo


def _table():
    doc = zoo.__doc__
    body = doc[doc.index("TABLE\n") + 6:doc.index("ENDTABLE")]
    rows = {}
    for line in body.splitlines()[1:]:
        if line.strip():
            name, n, kappa, err, bnd = line.split()
            rows[name] = (int(n), float(kappa), float(err), float(bnd))
    return rows


def test_the_cases_are_the_ones_the_table_lists():
    assert list(_table()) == list(zoo.NAMES) == list(zoo.zoo())
    assert set(zoo.STRUCTURE) == set(zoo.NAMES)


@pytest.mark.parametrize("name", zoo.NAMES)
def test_structure(name):
    N, M, Jp, Ji, Jx, x, lam = zoo.case(name)
    assert len(Jp) == M + 1 and Jp[-1] == len(Ji) == len(Jx) and len(x) == M
    sym = capi.symbolic_probe(N, M, Jp, Ji)
    _, st = capi.covariance_entries_probe(N, M, Jp, Ji, [0], [0])
    got = (sym["supernodes"], sym["levels"], st["wmax"])
    print(f"{name}: N={N} M={M} supernodes, levels, widest {got}; front {st['front_doubles']} doubles")
    assert got == zoo.STRUCTURE[name]
    assert st["wmax"] <= 128                                # the blocked kernels take every case
    if name in zoo.FRONT_DOUBLES:
        assert st["front_doubles"] == zoo.FRONT_DOUBLES[name]
        assert st["front_doubles"] * 8 > 160 * 1024         # the fronts do not fit LDS
    if name.startswith("dense-"):
        assert np.all(np.diff(Jp) == N) and M == 2 * N and lam == 0.0
    if name == "holes":
        assert np.sum(np.diff(Jp) == 0) == len(range(0, M, 17))
        assert Ji.max() == N - 6                            # the last 5 variables are in no row
        S, _ = zoo.truth(name)
        assert np.all(np.abs(np.diag(S)[N - 5:] * lam - 1) <= 2.0 ** -60)
        assert np.all(S[N - 5:, :N - 5] == 0)


@pytest.mark.parametrize("name", zoo.NAMES)
def test_reference_and_the_room_under_the_bound(name):
    N, M, Jp, Ji, Jx, x, lam = zoo.case(name)
    A, kappa = zoo.system(name)
    bnd = zoo.bound(name)
    assert kappa <= 5e4
    assert bnd <= 1e-10                                     # never above what the suite allows the same entry points
    S, res = zoo.truth(name)                                # (asserts that it converged)
    d = np.diag(S)
    assert np.all(d > 0)
    # an honest float64 solve, in the three measures
    rhs = np.random.default_rng(1).standard_normal((3, N))
    Lc = np.linalg.cholesky(A)
    u = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs.T)).T
    e_solve = zoo.solve_error(u, rhs.astype(np.longdouble) @ S)
    S64 = np.linalg.inv(A)
    e_entry = zoo.entry_error(S64, S, d[:, None], d[None, :])
    rows = zoo.measurement_rows(name, 0, M)
    want = zoo.exact_blocks(name, [[r] for r in rows])
    got = zoo.exact_blocks(name, [[r] for r in rows], S=S64)
    e_lev = max(zoo.block_error(g, w) for g, w in zip(got, want))
    print(f"{name}: kappa {kappa:.3g}, bound {bnd:.2e}, residual of the reference {res:.1e}; float64: solve {e_solve:.2e}, "
          f"entries {e_entry:.2e}, leverage {e_lev:.2e}")
    assert max(e_solve, e_entry, e_lev) <= bnd / 8
    # the table of the helper's docstring
    tn, tk, te, tb = _table()[name]
    assert tn == N
    assert abs(tk - kappa) <= 0.05 * kappa and abs(tb - bnd) <= 0.05 * bnd
    assert te / 8 <= e_entry <= te * 8


def test_error_measures_see_what_they_should():
    want = np.array([[4.0, 0.0], [0.0, 0.0]], dtype=np.longdouble)
    assert zoo.block_error(np.array([[4.0, 0.0], [0.0, 0.0]]), want) == 0.0
    assert zoo.block_error(np.array([[4.0 + 4e-6, 0.0], [0.0, 0.0]]), want) == pytest.approx(1e-6, rel=1e-3)
    with pytest.raises(AssertionError):
        zoo.block_error(np.array([[4.0, 1e-300], [0.0, 0.0]]), want)          # an exact 0 must come back as 0.0
    w = np.array([[1.0, -2.0], [0.0, 0.0]], dtype=np.longdouble)
    assert zoo.solve_error(np.array([[1.0, -2.0 + 2e-6], [0.0, 0.0]]), w) == pytest.approx(1e-6, rel=1e-3)
    assert zoo.entry_error(np.array([1.0 + 6e-6]), np.longdouble(1.0), np.longdouble(4.0), np.longdouble(9.0)) == \
        pytest.approx(1e-6, rel=1e-3)
