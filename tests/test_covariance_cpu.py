"""The covariance entry points as a C user compiles against them, and the packing of requests into chunks of 16
variables (dlg_covariance_plan_probe: the symbolic phase and the plan on the host, no GPU)."""
import math
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from tests import oracle_api as oa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, BC, BP = 6, 6, 3

PROBE = r'''
#include <stdio.h>
#include "dogleg.h"
#include "dlg_backend.h"

typedef int (*blocks_fn)(double*, int, const int*, const int*, const int*, const int*, dogleg_operatingPoint_t*,
                         dogleg_solverContext_t*);
typedef int (*var_fn)(double*, dogleg_operatingPoint_t*, dogleg_solverContext_t*);
typedef int (*be_blocks_fn)(dlg_backend_t*, int, int, const int*, const int*, const int*, const int*, double*);
typedef int (*be_var_fn)(dlg_backend_t*, int, double*);

int main(void)
{
  blocks_fn f = &dogleg_amd_covariance_blocks;
  var_fn v = &dogleg_amd_marginal_variances;
  be_blocks_fn bf = &dlg_covariance_blocks;
  be_var_fn bv = &dlg_marginal_variances;
  /* no point, no context: -1, never an exit */
  double out[4];
  const int z = 0, one = 1;
  printf("%d %d\n", f(out, 1, &z, &one, &z, &one, NULL, NULL), v(out, NULL, NULL));
  return (f && v && bf && bv) ? 0 : 1;
}
'''

NEW = ["dogleg_amd_covariance_blocks", "dogleg_amd_marginal_variances", "dlg_covariance_blocks", "dlg_marginal_variances",
       "dlg_covariance_stats", "dlg_covariance_plan_probe", "dlg_covariance_plan_seconds"]


def test_prototypes_compile_and_link(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", libdir, "-ldogleg_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["-1", "-1"]


def test_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NEW:
        assert n in exported, n
    for n in NEW:
        assert n in capi.BACKEND_SYMBOLS + capi.DOGLEG_SYMBOLS, n


@pytest.fixture(scope="module")
def config3():
    Nc, Np = 499, 9000
    prob = oa.BAProblem(Nc, Np, 100000, seed=1)
    Jp, Ji = prob.pattern()
    obs = {}
    for r in range(0, prob.M, 2):
        cols = Ji[Jp[r]:Jp[r + 1]]
        c, p = (int(cols[G]) - G) // BC, (int(cols[G + BC]) - G - BC * Nc) // BP
        obs.setdefault(c, set()).add(p)
    return prob, Jp, Ji, Nc, Np, obs


def _probe(prob, Jp, Ji, req):
    r0, nr, c0, nc = (np.array(a, dtype=np.int32) for a in zip(*req))
    return capi.covariance_plan_probe(prob.N, prob.M, Jp, Ji, r0, nr, c0, nc)


def test_plan_packing_config3(config3):
    prob, Jp, Ji, Nc, Np, obs = config3
    cam0, pt0 = G, G + BC * Nc
    rng = np.random.default_rng(3)
    req = [(0, G, 0, G)]
    req += [(cam0 + BC * c, BC, cam0 + BC * c, BC) for c in range(Nc)]
    req += [(pt0 + BP * p, BP, pt0 + BP * p, BP) for p in range(0, Np, 5)]
    cross = [(cam0 + BC * c, BC, pt0 + BP * p, BP) for c in range(0, Nc, 4) for p in sorted(obs[c])]
    req += cross
    req += [(0, G, cam0 + BC * c, BC) for c in range(0, Nc, 10)]
    order = rng.permutation(len(req))
    req = [req[i] for i in order]
    ch, st = _probe(prob, Jp, Ji, req)
    # every request lands in exactly one chunk; no chunk has more than 16 distinct variables
    assert ch.shape == (len(req),) and ch.min() >= 0 and ch.max() == st["chunks"] - 1
    assert len(np.unique(ch)) == st["chunks"]
    assert 0 < st["maxvar"] <= 16
    members = {}
    for q, k in enumerate(ch):
        r0, nr, c0, nc = req[q]
        members.setdefault(int(k), set()).update(range(r0, r0 + nr), range(c0, c0 + nc))
    assert max(len(v) for v in members.values()) == st["maxvar"]
    # requests that share a camera share a chunk when they fit: a camera's 6 columns serve 3 of its points per chunk
    by_cam = {}
    for q, (r0, nr, c0, nc) in enumerate(req):
        if nr == BC and nc == BP:
            by_cam.setdefault(r0, set()).add(int(ch[q]))
    for cam, chunks in by_cam.items():
        k = len(obs[(cam - cam0) // BC])
        assert len(chunks) <= math.ceil(k / 3) + 1, (cam, k, len(chunks))
    # the reach: a few paths to the root per chunk, not the whole factor
    nsn = capi.symbolic_probe(prob.N, prob.M, Jp, Ji)["supernodes"]
    print(f"{len(req)} requests -> {st['chunks']} chunks, {st['visits'] / st['chunks']:.1f} of {nsn} supernodes per chunk")
    assert st["chunks"] <= st["visits"] < st["chunks"] * nsn
    # the same list again: the same plan
    ch2, st2 = _probe(prob, Jp, Ji, req)
    assert np.array_equal(ch, ch2) and st == st2


def test_plan_refuses_oversized_requests(config3):
    prob, Jp, Ji, Nc, Np, obs = config3
    ok = (G, 6, G, 6)
    for bad in [(0, 17, 0, 17), (0, 9, 100, 8), (0, 6, 100, 11), (0, 0, 0, 6), (prob.N - 2, 3, 0, 3)]:
        with pytest.raises(capi.DlgError) as e:
            _probe(prob, Jp, Ji, [ok, bad])
        if bad[1] > 0 and bad[0] + bad[1] <= prob.N:
            assert "dlg_solve_multi" in str(e.value)
    # 16 distinct variables are taken: a 16-wide diagonal block, disjoint 6 + 10, overlapping 9 and 11 (15 distinct)
    ch, st = _probe(prob, Jp, Ji, [(0, 16, 0, 16), (0, 6, 200, 10), (0, 9, 4, 11)])
    assert st["maxvar"] == 16 and 2 <= st["chunks"] <= 3
