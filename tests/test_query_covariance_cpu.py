"""Query covariance without a GPU: the symbols are exported and their prototypes compile against the headers, and the
packing of a query batch into chunks (dlg_query_covariance_plan_probe: the symbolic phase and the plan on the host)."""
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from tests import oracle_api as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, BC, BP = 6, 6, 3
BACKEND = ["dlg_query_covariance", "dlg_query_covariance_stats", "dlg_query_covariance_plan_seconds",
           "dlg_query_covariance_plan_probe"]
PUBLIC = ["dogleg_amd_query_covariance"]


def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in BACKEND + PUBLIC:
        assert n in exported, n
    for n in BACKEND:
        assert n in capi.BACKEND_SYMBOLS
    for n in PUBLIC:
        assert n in capi.DOGLEG_SYMBOLS


def test_prototypes_compile_and_link(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text("""
#include <stdio.h>
#include <dlg_backend.h>
#include <dogleg.h>
int (*a)(dlg_backend_t*, int, int, const int*, const int*, const int*, const double*, int, double*) = dlg_query_covariance;
int (*b)(dlg_backend_t*, long*, long*, int*) = dlg_query_covariance_stats;
double (*c)(dlg_backend_t*) = dlg_query_covariance_plan_seconds;
int (*d)(int, int, const int*, const int*, int, const int*, const int*, const int*, int*, long*, int) = dlg_query_covariance_plan_probe;
int (*e)(double*, int, const int*, const int*, const int*, const double*, int, dogleg_operatingPoint_t*,
         dogleg_solverContext_t*) = dogleg_amd_query_covariance;
int main(void)
{
  /* no point, no context: -1, never an exit */
  double out[4];
  const int qrow[2] = {0, 1}, rowptr[2] = {0, 1}, var[1] = {0};
  const double val[1] = {1.0};
  printf("%d\\n", e(out, 1, qrow, rowptr, var, val, -1, NULL, NULL));
  return !(a && b && c && d && e);
}
""")
    exe = str(tmp_path / "proto")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", libdir, "-ldogleg_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1"]


@pytest.fixture(scope="module")
def config3():
    Nc, Np = 499, 9000
    prob = oa.BAProblem(Nc, Np, 100000, seed=1)
    Jp, Ji = prob.pattern()
    return prob, Jp, Ji, Nc, Np


def _csr(queries):
    """queries: lists of rows, each row a list of (var, val): (qrow, rowptr, var, val)"""
    qrow, rowptr, var, val = [0], [0], [], []
    for rows in queries:
        for row in rows:
            var += [v for v, _ in row]
            val += [x for _, x in row]
            rowptr.append(len(var))
        qrow.append(len(rowptr) - 1)
    return (np.array(qrow, dtype=np.int32), np.array(rowptr, dtype=np.int32), np.array(var, dtype=np.int32),
            np.array(val))


def _pixel_query(Nc, cam, pt, rows=2):
    """rows over the globals, a camera and a point (15 variables)"""
    cam0, pt0 = G, G + BC * Nc
    vs = list(range(G)) + list(range(cam0 + BC * cam, cam0 + BC * cam + BC)) + list(range(pt0 + BP * pt, pt0 + BP * pt + BP))
    return [[(v, 1.0) for v in vs] for _ in range(rows)]


def _probe(prob, Jp, Ji, queries):
    qrow, rowptr, var, _ = _csr(queries)
    return capi.query_covariance_plan_probe(prob.N, prob.M, Jp, Ji, qrow, rowptr, var)


def test_plan_packing_config3(config3):
    prob, Jp, Ji, Nc, Np = config3
    rng = np.random.default_rng(3)
    sizes = rng.choice([1, 2, 3, 5, 7, 16], 600)
    queries = []
    for fs in sizes:
        cam, pt = int(rng.integers(Nc)), int(rng.integers(Np))
        queries.append(_pixel_query(Nc, cam, pt, int(fs)))
    ch, st = _probe(prob, Jp, Ji, queries)
    # greedy packing in query order, never split, at most 16 rows a chunk
    expect, cur, rows = [], 0, 0
    for fs in sizes:
        if rows + fs > 16:
            cur, rows = cur + 1, 0
        expect.append(cur)
        rows += fs
    assert np.array_equal(ch, np.array(expect))
    assert st["chunks"] == expect[-1] + 1
    per = np.bincount(ch, weights=sizes)
    assert per.max() <= 16 and per.max() == st["maxrows"]
    nsn = capi.symbolic_probe(prob.N, prob.M, Jp, Ji)["supernodes"]
    print(f"{len(queries)} queries -> {st['chunks']} chunks, {st['visits'] / st['chunks']:.1f} of {nsn} supernodes per chunk")
    assert st["chunks"] <= st["visits"] < st["chunks"] * nsn
    ch2, st2 = _probe(prob, Jp, Ji, queries)
    assert np.array_equal(ch, ch2) and st == st2


def test_visits_are_the_union_of_the_paths(config3):
    """a chunk's visits are the supernodes on the union of its variables' paths to the root: chunks whose variables form
    a camera and a run of 3 points give, summed, what the covariance plan gives for the same variable sets as requests
    (one request per chunk), and a chunk of repeated queries visits what one of them does"""
    prob, Jp, Ji, Nc, Np = config3
    cam0, pt0 = G, G + BC * Nc
    rng = np.random.default_rng(7)
    queries, reqs = [], []
    for _ in range(40):
        cam, p = int(rng.integers(Nc)), int(rng.integers(Np - 3))
        # 8 two-row queries on the camera and points p, p + 1, p + 2: one chunk, 15 distinct variables
        for i in range(8):
            queries.append([[(v, 1.0) for v in list(range(cam0 + BC * cam, cam0 + BC * cam + BC))
                             + list(range(pt0 + BP * (p + i % 3), pt0 + BP * (p + i % 3) + BP))]] * 2)
        reqs.append((cam0 + BC * cam, BC, pt0 + BP * p, 3 * BP))
    ch, st = _probe(prob, Jp, Ji, queries)
    assert st["chunks"] == 40 and st["maxrows"] == 16
    total = 0
    for r in reqs:
        _, cst = capi.covariance_plan_probe(prob.N, prob.M, Jp, Ji, *([a] for a in r))
        assert cst["chunks"] == 1
        total += cst["visits"]
    assert st["visits"] == total
    # one 16-row query alone, and the same 2-row query eight times in one chunk: the same reach
    _, s1 = _probe(prob, Jp, Ji, [_pixel_query(Nc, 5, 17, 16)])
    _, s8 = _probe(prob, Jp, Ji, [_pixel_query(Nc, 5, 17, 2)] * 8)
    assert s1["chunks"] == s8["chunks"] == 1 and s1["visits"] == s8["visits"]


def test_plan_refusals(config3):
    prob, Jp, Ji, Nc, Np = config3
    ok = _pixel_query(Nc, 0, 0)
    with pytest.raises(capi.DlgError) as e:
        _probe(prob, Jp, Ji, [ok, [[(0, 1.0)]] * 17])
    assert "dlg_solve_multi" in str(e.value)
    with pytest.raises(capi.DlgError):
        _probe(prob, Jp, Ji, [ok, []])
    with pytest.raises(capi.DlgError):
        _probe(prob, Jp, Ji, [ok, [[(prob.N, 1.0)]]])
    with pytest.raises(capi.DlgError):
        _probe(prob, Jp, Ji, [ok, [[(-1, 1.0)]]])
    # 16 rows, empty rows and duplicated, unsorted indices are taken
    ch, st = _probe(prob, Jp, Ji, [[[(0, 1.0)]] * 16, [[], [(7, 1.0), (3, 2.0), (7, 1.0)]]])
    assert list(ch) == [0, 1] and st["maxrows"] == 16
