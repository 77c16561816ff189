"""The selected inverse without a GPU: its symbols are exported and their prototypes compile against the headers, and
the host probe's verdict on the structure of the factor agrees with a symbolic Cholesky done in numpy (elimination tree
fill) under the factor's own ordering."""
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from tests import oracle_api as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dlg_covariance_entries", "dlg_covariance_entries_stats", "dlg_covariance_entries_probe",
           "dogleg_amd_covariance_entries"]


def test_symbols_exported():
    L = capi.lib()
    for name in SYMBOLS:
        getattr(L, name)
    for name in SYMBOLS[:3]:
        assert name in capi.BACKEND_SYMBOLS
    assert SYMBOLS[3] in capi.DOGLEG_SYMBOLS


def test_prototypes_compile(tmp_path):
    src = tmp_path / "proto.c"
    src.write_text("""
#include <dlg_backend.h>
#include <dogleg.h>
int (*a)(dlg_backend_t*, int, long, const int*, const int*, double*) = dlg_covariance_entries;
int (*b)(dlg_backend_t*, double*, long*, long*) = dlg_covariance_entries_stats;
int (*c)(int, int, const int*, const int*, long, const int*, const int*, int*, long*, int) = dlg_covariance_entries_probe;
int (*d)(double*, long, const int*, const int*, dogleg_operatingPoint_t*, dogleg_solverContext_t*) = dogleg_amd_covariance_entries;
int main(void) { return !(a && b && c && d); }
""")
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(tmp_path / "proto"), "-L", os.path.join(ROOT, "libdogleg_amd"), "-ldogleg_amd",
                    "-Wl,-rpath," + os.path.join(ROOT, "libdogleg_amd")], check=True)


def _symbolic_fill(N, Jp, Ji, perm):
    """lower structure (boolean N x N, elimination positions) of the Cholesky factor of JtJ permuted by perm, by the
    elimination tree: column k's structure is its own rows of A plus those of its children below k"""
    iperm = np.empty(N, dtype=np.int64)
    iperm[perm] = np.arange(N)
    A = np.zeros((N, N), dtype=bool)
    for r in range(len(Jp) - 1):
        c = iperm[Ji[Jp[r]:Jp[r + 1]]]
        A[np.ix_(c, c)] = True
    Lst = np.tril(A)
    parent = -np.ones(N, dtype=np.int64)
    for k in range(N):
        rows = np.nonzero(Lst[k + 1:, k])[0] + k + 1
        if len(rows):
            parent[k] = rows[0]
            Lst[rows, parent[k]] = True
    return Lst, iperm


@pytest.mark.parametrize("shape,seed", [((4, 30, 150), 1), ((12, 120, 720), 3), ((7, 60, 200), 9)])
def test_probe_matches_symbolic_cholesky(shape, seed):
    prob = oa.BAProblem(*shape, seed=seed)
    N, M = prob.N, prob.M
    Jp, Ji = prob.pattern()
    _, perm = capi.symbolic_probe(N, M, Jp, Ji, want_perm=True)
    fill, iperm = _symbolic_fill(N, Jp, Ji, perm)
    ii, jj = np.tril_indices(N)
    ins, st = capi.covariance_entries_probe(N, M, Jp, Ji, ii, jj)
    pi, pj = iperm[ii], iperm[jj]
    exact = fill[np.maximum(pi, pj), np.minimum(pi, pj)]
    # every entry of the exact fill is in the structure; the structure is that fill plus the explicit zeros of merged
    # supernodes (at most a small share here); nnz counts the structure
    assert np.all(ins[exact])
    assert st["nnz"] == int(np.sum(ins))
    extra = int(np.sum(ins & ~exact))
    print(f"{shape}: {int(np.sum(exact))} entries of the fill, {st['nnz']} of the structure ({extra} explicit zeros)")
    assert extra <= 0.25 * int(np.sum(exact))
    # either order gives the same verdict
    ins2, _ = capi.covariance_entries_probe(N, M, Jp, Ji, jj, ii)
    assert np.array_equal(ins, ins2)


def test_probe_disconnected_blocks_are_off():
    """two independent dense groups: no entry between them is in the fill, and none is in the structure"""
    N = 20
    groups = [np.arange(0, 10), np.arange(10, 20)]
    Jp, Ji = [0], []
    for g in groups:
        for _ in range(15):
            Ji.extend(g.tolist())
            Jp.append(len(Ji))
    Jp, Ji = np.array(Jp, dtype=np.int32), np.array(Ji, dtype=np.int32)
    M = len(Jp) - 1
    i, j = np.meshgrid(np.arange(10, 20), np.arange(0, 10), indexing="ij")
    ins, st = capi.covariance_entries_probe(N, M, Jp, Ji, i.ravel(), j.ravel())
    assert not np.any(ins)
    ii, jj = np.tril_indices(10)
    ins, _ = capi.covariance_entries_probe(N, M, Jp, Ji, np.r_[ii, ii + 10], np.r_[jj, jj + 10])
    assert np.all(ins) and st["nnz"] == 2 * 55


def test_probe_refuses_bad_entries():
    prob = oa.BAProblem(4, 30, 150, seed=1)
    Jp, Ji = prob.pattern()
    with pytest.raises(capi.DlgError):
        capi.covariance_entries_probe(prob.N, prob.M, Jp, Ji, [0, prob.N], [0, 0])
    with pytest.raises(capi.DlgError):
        capi.covariance_entries_probe(prob.N, prob.M, Jp, Ji, [-1], [0])
