"""CPU tests of the product's host side: the shared library loads and exports every
declared symbol, struct layouts, the symbolic phase, error behaviour without a GPU,
and the row-sharding arithmetic under a 2-rank gloo group."""
import ctypes as C
import functools
import os
import re
import subprocess
import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import Parameters2, dptr, iptr
from tests import factor_user_zoo as zoo, oracle_api as oa, sparse_patterns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b((?:dlg|dogleg)_[A-Za-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    L = capi.lib()
    for hdr in ("dlg_backend.h", "dogleg.h"):
        names = [n for n in _declared(hdr) if not n.endswith("_t") and n not in ("dogleg_callback_t",)]
        assert names, hdr
        for n in names:
            assert hasattr(L, n), f"{n} declared in include/{hdr} but not exported"
    for n in capi.BACKEND_SYMBOLS + capi.DOGLEG_SYMBOLS:
        assert hasattr(L, n)


def test_parameter_struct_layout():
    """reference test-misc.c:7-12: debug_vnlog lands on bit 30; offsetof(trustregion0) == 8"""
    p = capi.default_parameters()
    assert Parameters2.trustregion0.offset == 2 * C.sizeof(C.c_int)
    assert p.max_iterations == 100 and p.trustregion0 == 1.0e3           # dogleg.c:117-128
    assert p.trustregion_decrease_factor == 0.1 and p.trustregion_increase_factor == 2
    assert p.Jt_x_threshold == 1e-8 and p.update_threshold == 1e-8 and p.trustregion_threshold == 1e-8
    q = Parameters2()
    q.debug_vnlog = True
    assert q.dogleg_debug == (1 << 30)
    # the C side agrees on the bit positions: compile a probe against include/dogleg.h
    import subprocess, tempfile
    src = r'''
#include <stdio.h>
#include "dogleg.h"
int main(void){ dogleg_parameters2_t p = {0}; p.debug_vnlog = 1; printf("%d ", p.dogleg_debug == DOGLEG_DEBUG_VNLOG);
 dogleg_parameters2_t q = {0}; q.JtJ_packed = 1; printf("%d ", q.dogleg_debug); q.JtJ_upper = 1; printf("%d\n", q.dogleg_debug); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"),
                        "-o", os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1", "2", "6"]


def test_no_gpu_means_loud_failure():
    """the product has no CPU fallback: without a device every entry point refuses"""
    L = capi.lib()
    if L.dlg_device_count() > 0:
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    rc = L.dlg_backend_create(C.byref(h), capi.DLG_DENSE, 4, 10, 0, 0, -1)
    assert rc == 5 and not h.value                                        # DLG_ERR_NODEVICE
    assert b"no CPU fallback" in L.dlg_last_error()
    P = oa.problems()
    p0 = np.zeros(6)
    P.sample_init(dptr(p0))
    r = L.dogleg_optimize_dense2(dptr(p0), 6, 100, oa.fn_addr(P, "sample_cb_dense"), None, None, None)
    assert r == -1.0                                                      # dogleg.h:277 error convention


def test_argument_checks_match_reference():
    """dogleg.c:1659-1689,1762-1766: NJnnz rules and the -1.0 return"""
    L = capi.lib()
    P = oa.problems()
    p0 = np.zeros(6)
    assert L.dogleg_optimize2(dptr(p0), 6, 100, 0, oa.fn_addr(P, "sample_cb_sparse"), None, None, None) == -1.0
    assert L.dogleg_optimize2(dptr(p0), 6, 100, 600, None, None, None, None) == -1.0


def _dense_symbolic_nnzL(N, M, Jp, Ji, perm):
    """reference fill count: boolean Cholesky of the permuted JtJ pattern"""
    A = np.zeros((N, N), dtype=bool)
    ip = np.empty(N, dtype=np.int64)
    ip[perm] = np.arange(N)
    for r in range(M):
        idx = ip[Ji[Jp[r]:Jp[r+1]]]
        A[np.ix_(idx, idx)] = True
    A |= np.eye(N, dtype=bool)
    for k in range(N):
        rows = np.nonzero(A[k+1:, k])[0] + k + 1
        A[np.ix_(rows, rows)] = True
    return int(np.tril(A).sum())


def test_symbolic_phase_invariants():
    for (Nc, Np, Nobs) in ((4, 20, 60), (9, 60, 300)):
        prob = oa.BAProblem(Nc, Np, Nobs, seed=3)
        Jp, Ji = prob.pattern()
        st, perm = capi.symbolic_probe(prob.N, prob.M, Jp, Ji, want_perm=True)
        assert sorted(perm.tolist()) == list(range(prob.N))
        # nnz(tril JtJ) from the pattern
        A = np.zeros((prob.N, prob.N), dtype=bool)
        for r in range(prob.M):
            idx = Ji[Jp[r]:Jp[r+1]]
            A[np.ix_(idx, idx)] = True
        assert st["nnz_JtJ_lower"] == int(np.tril(A).sum())
        # nnz(L) under the chosen ordering equals an independent symbolic Cholesky
        assert st["nnz_L"] == _dense_symbolic_nnzL(prob.N, prob.M, Jp, Ji, perm)
        assert st["panel_doubles"] >= st["nnz_L"]
        assert st["levels"] >= 1 and st["supernodes"] >= 1


def test_symbolic_phase_on_the_sample_pattern_and_errors():
    Jp = np.arange(0, 601, 6, dtype=np.int32)
    Ji = np.tile(np.arange(6, dtype=np.int32), 100)
    st = capi.symbolic_probe(6, 100, Jp, Ji)
    assert st["nnz_JtJ_lower"] == 21 and st["nnz_L"] == 21 and st["supernodes"] == 1
    bad = Ji.copy()
    bad[1] = 0                                                 # not strictly ascending
    with pytest.raises(capi.DlgError):
        capi.symbolic_probe(6, 100, Jp, bad)
    bad = Ji.copy()
    bad[5] = 6                                                 # out of range
    with pytest.raises(capi.DlgError):
        capi.symbolic_probe(6, 100, Jp, bad)


def test_symbolic_shards_partition_the_contributions():
    """row sharding: every row-block contribution is owned by exactly one rank"""
    prob = oa.BAProblem(9, 60, 300, seed=3)
    Jp, Ji = prob.pattern()
    full = capi.symbolic_probe(prob.N, prob.M, Jp, Ji)
    cuts = [0, 150, 151, 400, prob.M]
    parts = [capi.symbolic_probe(prob.N, prob.M, Jp, Ji, row0=a, row1=b) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in ("nnz_L", "supernodes", "levels", "panel_doubles"):
        assert all(p[k] == full[k] for p in parts)             # same factor structure on every rank
    # a shard cut inside an observation's row pair splits that row-block in two: contributions
    # are counted per row-block, so compare weighted by rows instead: every row is covered once
    assert sum(p["contribs"] for p in parts) >= full["contribs"]


def _gloo_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    O = oa.oracle()
    prob = oa.BAProblem(6, 40, 160, seed=5)
    Jp, Ji = prob.pattern()
    p = prob.p0()
    x, Jx = prob.eval(p)
    N, M = prob.N, prob.M
    row0, row1 = (M * rank) // world, (M * (rank + 1)) // world
    q0, q1 = Jp[row0], Jp[row1]
    Jp_loc = np.ascontiguousarray(Jp[row0:row1 + 1] - q0)
    Ji_loc = np.ascontiguousarray(Ji[q0:q1])
    Jx_loc = np.ascontiguousarray(Jx[q0:q1])
    x_loc = np.ascontiguousarray(x[row0:row1])
    # the fused buffer of dlg_point_eval: [Jt_x | norm2_x]
    g = np.zeros(N + 1)
    O.orc_spmv_Jt_x(dptr(g[:N]), N, row1 - row0, iptr(Jp_loc), iptr(Ji_loc), dptr(Jx_loc), dptr(x_loc))
    g[N] = O.orc_norm2(dptr(x_loc), row1 - row0)
    t = torch.from_numpy(g)
    dist.all_reduce(t)
    Jg2 = np.array([O.orc_norm2_J_v(row1 - row0, iptr(Jp_loc), iptr(Ji_loc), dptr(Jx_loc), dptr(np.ascontiguousarray(g[:N])))])
    t2 = torch.from_numpy(Jg2)
    dist.all_reduce(t2)
    # partial JtJ (dense here) summed over ranks
    Jd = np.zeros((row1 - row0, N))
    for r in range(row1 - row0):
        Jd[r, Ji_loc[Jp_loc[r]:Jp_loc[r+1]]] = Jx_loc[Jp_loc[r]:Jp_loc[r+1]]
    JtJ = Jd.T @ Jd
    t3 = torch.from_numpy(JtJ)
    dist.all_reduce(t3)
    if rank == 0:
        gf = np.zeros(N)
        O.orc_spmv_Jt_x(dptr(gf), N, M, iptr(Jp), iptr(Ji), dptr(Jx), dptr(x))
        Jf = np.zeros((M, N))
        for r in range(M):
            Jf[r, Ji[Jp[r]:Jp[r+1]]] = Jx[Jp[r]:Jp[r+1]]
        ok = (np.allclose(g[:N], gf, rtol=1e-12, atol=1e-12)
              and abs(g[N] - O.orc_norm2(dptr(x), M)) <= 1e-12 * g[N]
              and abs(Jg2[0] - O.orc_norm2_J_v(M, iptr(Jp), iptr(Ji), dptr(Jx), dptr(gf))) <= 1e-10 * Jg2[0]
              and np.allclose(JtJ, Jf.T @ Jf, rtol=1e-11, atol=1e-11))
        q.put(bool(ok))
    dist.destroy_process_group()


def test_row_sharding_with_gloo_world_size_2():
    """N>1 path on CPU: rows partitioned over 2 ranks, partial Jt_x | norm2_x, |Jg|^2 and
    JtJ summed with an all-reduce equal the single-rank quantities (what
    dlg_backend_set_shard + the all-reduce hook do on GPUs with RCCL)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert q.get(timeout=5) is True


def _capture_stdout(fn):
    """run fn() and return what the C library printed on stdout (fd 1)"""
    import tempfile
    C.CDLL(None).fflush(None)
    saved = os.dup(1)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 1)
        try:
            fn()
            C.CDLL(None).fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        tmp.seek(0)
        return tmp.read().decode()


@pytest.mark.parametrize("mode", ["sparse", "dense"])
def test_gradient_check_tool_on_the_sample_problem(mode):
    """dogleg_testGradient{,_dense} (reference dogleg.h:312-322; sample.c runs it with --test-gradient):
    the table has one row per measurement and the sample problem's analytic gradients agree with
    central differences; host only, no GPU"""
    L, P = capi.lib(), oa.problems()
    p0 = np.zeros(6)
    P.sample_init(dptr(p0))
    var = 2
    U = C.c_uint
    if mode == "sparse":
        L.dogleg_testGradient.argtypes = [U, C.POINTER(C.c_double), U, U, U, C.c_void_p, C.c_void_p]
        L.dogleg_testGradient.restype = None
        out = _capture_stdout(lambda: L.dogleg_testGradient(var, dptr(p0), 6, 100, 600,
                                                            oa.fn_addr(P, "sample_cb_sparse"), None))
    else:
        L.dogleg_testGradient_dense.argtypes = [U, C.POINTER(C.c_double), U, U, C.c_void_p, C.c_void_p]
        L.dogleg_testGradient_dense.restype = None
        out = _capture_stdout(lambda: L.dogleg_testGradient_dense(var, dptr(p0), 6, 100,
                                                                  oa.fn_addr(P, "sample_cb_dense"), None))
    lines = out.strip().splitlines()
    assert lines[0] == "# ivar imeasurement gradient_reported gradient_observed error error_relative"
    rows = [l.split() for l in lines[1:]]
    assert len(rows) == 100
    assert [int(r[0]) for r in rows] == [var] * 100 and [int(r[1]) for r in rows] == list(range(100))
    rep = np.array([float(r[2]) for r in rows]); obs = np.array([float(r[3]) for r in rows])
    assert np.max(np.abs(rep)) > 0
    assert np.max(np.abs(rep - obs)) <= 1e-4 * max(1.0, np.max(np.abs(rep)))


def test_host_side_compiles_against_a_real_cholmod_header(tmp_path):
    """VERDICT r1 item 8 / INTEGRATION.md: where SuiteSparse is installed <cholmod.h> is used instead
    of include/dogleg_cholmod_compat.h.  The driver (the host pass of every file of it that sees a
    dogleg_solverContext_t, driver_internal.h: driver.hip, driver_cache.hip, driver_comm.cpp, driver_records.cpp,
    api_extensions.cpp) and a user translation
    unit must compile against CHOLMOD's public struct shapes: no by-value cholmod_factor with
    compat-only fields, the backend pointer lives in the driver."""
    inc = os.path.join(ROOT, "tests", "c", "cholmod_shape")
    hipcc = "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "libdogleg_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".cpp"))
             and "driver_internal.h" in open(os.path.join(csrc, f)).read()]
    assert {"driver.hip", "driver_cache.hip", "driver_comm.cpp", "driver_records.cpp", "api_extensions.cpp"} <= set(users)
    for f in users:
        lang = ["--offload-arch=gfx950", "--cuda-host-only"] if f.endswith(".hip") else ["-x", "c++"]
        r = subprocess.run([hipcc, "-std=c++17"] + lang + ["-fsyntax-only", "-I", inc, os.path.join(csrc, f)],
                           capture_output=True, text=True)
        assert r.returncode == 0, (f, r.stderr[-3000:])
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", inc,
                        os.path.join(ROOT, "tests", "c", "real_cholmod_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # and with the compat header forced the same user code still compiles (the default in this image)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-DDOGLEG_FORCE_CHOLMOD_COMPAT",
                        "-I", inc, "-include", os.path.join(ROOT, "include", "dogleg.h"), "-x", "c++", "/dev/null"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


# ---------------------------------------------------------------- subtree partition ----
def _rows_to_dense(Jp, Ji, Jx, rows, N):
    Jd = np.zeros((len(rows), N))
    for k, r in enumerate(rows):
        Jd[k, Ji[Jp[r]:Jp[r+1]]] = Jx[Jp[r]:Jp[r+1]]
    return Jd


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_subtree_partition_covers_every_row_once(nranks):
    """dlg_backend_set_partition: the symbolic phase cuts the elimination tree and deals the subtrees
    (and with them the measurement rows) to the ranks.  Every row belongs to exactly one rank, every
    rank sees the same cut and the same amount of data to sum, and that amount is a small part of the
    panel buffer (what the simple row sharding has to sum)."""
    prob = oa.BAProblem(199, 3600, 40000, seed=3)
    Jp, Ji = prob.pattern()
    owned = np.zeros(prob.M, dtype=int)
    stats = []
    for r in range(nranks):
        st, mine = capi.partition_probe(prob.N, prob.M, Jp, Ji, r, nranks)
        owned += mine
        stats.append(st)
        assert st["rows_mine"] == int(mine.sum())
    assert np.all(owned == 1), "every measurement row must be held by exactly one rank"
    for k in ("cut_level", "supernodes_above_cut", "reduced_doubles", "panel_doubles"):
        assert len({st[k] for st in stats}) == 1, k
    assert sum(st["nnz_mine"] for st in stats) == prob.nnz
    # balance: no rank holds more than twice its share of the rows
    assert max(st["rows_mine"] for st in stats) <= 2.0 * prob.M / nranks
    # the point of the partition: what crosses the ranks per factorisation is a fraction of JtJ
    assert stats[0]["reduced_doubles"] * 2 <= stats[0]["panel_doubles"]
    full = capi.symbolic_probe(prob.N, prob.M, Jp, Ji)
    assert stats[0]["panel_doubles"] == full["panel_doubles"]
    print(f"nranks={nranks}: cut above level {stats[0]['cut_level']}, {stats[0]['supernodes_above_cut']} replicated supernodes, "
          f"{stats[0]['reduced_doubles']*8/1e6:.2f} MB summed of {stats[0]['panel_doubles']*8/1e6:.1f} MB, rows/rank "
          f"{[st['rows_mine'] for st in stats]}")


def test_subtree_partition_of_config4_over_8_ranks():
    """BASELINE.json config #4 (1M x 150k) over the 8 GPUs of a node: what each rank holds and what
    crosses the ranks per factorisation (DESIGN.md quotes these numbers)"""
    prob = oa.BAProblem(2499, 45000, 500000, seed=11)
    Jp, Ji = prob.pattern()
    stats = [capi.partition_probe(prob.N, prob.M, Jp, Ji, r, 8)[0] for r in (0, 3, 7)]
    st = stats[0]
    assert len({s["reduced_doubles"] for s in stats}) == 1 and len({s["cut_level"] for s in stats}) == 1
    assert st["reduced_doubles"] * 8 <= 4e6, "a few MB at most cross the ranks"
    assert st["reduced_doubles"] * 20 <= st["panel_doubles"]
    rows = [s["rows_mine"] for s in stats]
    assert max(rows) <= 1.3 * prob.M / 8 and min(rows) >= 0.7 * prob.M / 8
    print(f"config #4 / 8 ranks: cut above level {st['cut_level']}, {st['supernodes_above_cut']} replicated supernodes, "
          f"{st['reduced_doubles']*8/1e6:.2f} MB summed per factorisation (panel buffer {st['panel_doubles']*8/1e6:.0f} MB), "
          f"rows of ranks 0/3/7: {rows}")


def test_subtree_partition_of_config5_over_8_ranks():
    """BASELINE.json config #5 (5M x 500 001, 75M non-zeros: the other configuration that names 8 GPUs): the
    product's partition as ranks 0 and 7 see it -- every row held exactly once is checked on two complementary
    masks' disjointness, the cut and what crosses the ranks agree"""
    prob = oa.BAProblem(8333, 149999, 2500000, seed=13, scale_decades=4.0, n_zero_cols=3)
    Jp, Ji = prob.pattern()
    (s0, m0), (s7, m7) = [capi.partition_probe(prob.N, prob.M, Jp, Ji, r, 8) for r in (0, 7)]
    assert s0["cut_level"] == s7["cut_level"] and s0["reduced_doubles"] == s7["reduced_doubles"]
    assert not np.any(m0 & m7), "a measurement row held by two ranks"
    for st in (s0, s7):
        assert 0.6 * prob.M / 8 <= st["rows_mine"] <= 1.4 * prob.M / 8
    assert s0["reduced_doubles"] * 8 <= 16e6 and s0["reduced_doubles"] * 20 <= s0["panel_doubles"]
    print(f"config #5 / 8 ranks: cut above level {s0['cut_level']}, {s0['supernodes_above_cut']} replicated supernodes, "
          f"{s0['reduced_doubles']*8/1e6:.2f} MB summed per factorisation (panel buffer {s0['panel_doubles']*8/1e6:.0f} MB), "
          f"rows of ranks 0/7: {s0['rows_mine']}, {s7['rows_mine']}")


@pytest.mark.parametrize("shape,ncu", [((49, 900, 10000), 256), ((499, 9000, 100000), 256), ((2499, 45000, 500000), 256),
                                       ((2499, 45000, 500000), 64)])
def test_one_launch_region_schedule_invariants(shape, ncu, monkeypatch):
    """The top of the elimination tree is factored by ONE launch whose workgroups trust their schedule blindly:
    replicas of a supernode that each form a slice of its update matrix, destination lists into LDS, children
    that must come before their parents.  dlg_sparse_region_probe builds that schedule with the library's own
    set-up code (no GPU) and checks every destination against the workgroup's LDS, the slices against the update
    matrix (every tile column formed exactly once), the order of the workgroups."""
    prob = oa.BAProblem(*shape, seed=11)
    Jp, Ji = prob.pattern()
    st = capi.region_probe(prob.N, prob.M, Jp, Ji, ncu)
    assert st["workgroups"] >= st["supernodes"] > 0 and st["lds_bytes"] <= 160 * 1024
    if shape[0] == 2499 and ncu == 256:
        # config #4: every update matrix of the region is staged in LDS (whole or in slices), none summed in HBM
        assert st["hbm_update_matrices"] == 0 and st["sliced_workgroups"] > 0 and st["level0"] == 1
    for knob, val in (("DOGLEG_AMD_FRONT_REPLICAS", "1"), ("DOGLEG_AMD_FRONT_REPLICAS", "8"), ("DOGLEG_AMD_NO_FRONT_SLICES", "1")):
        monkeypatch.setenv(knob, val)
        st2 = capi.region_probe(prob.N, prob.M, Jp, Ji, ncu)
        assert st2["supernodes"] == st["supernodes"]
        monkeypatch.delenv(knob)


# The schedule of the one-launch region and the per-level launch parameters of the factorisation, pinned bit for bit:
# shape (seed 11) -> (level_params_hash, {CUs: schedule_hash under each of _REGION_KNOBS}).  The literals were produced by
# the set-up code as it stood before the planner moved to sparse_region.cpp (the same hash added to its probe, nothing else).
_REGION_KNOBS = (None, ("DOGLEG_AMD_FRONT_REPLICAS", "1"), ("DOGLEG_AMD_NO_FRONT_SLICES", "1"), ("DOGLEG_AMD_PERSIST_MAX", "3"))
_REGION_KW = {(833, 15000, 250000): dict(scale_decades=4.0, n_zero_cols=3)}
_REGION_HASHES = {
    (49, 900, 10000): (0x333b848517a32945, {
        256: (0x326b590a32d9185e, 0x70c58b34c19d29a5, 0x4c81fc5572e6cd7, 0x85ff7d46b93fa5d4),
        64: (0x326b590a32d9185e, 0x70c58b34c19d29a5, 0x4c81fc5572e6cd7, 0x85ff7d46b93fa5d4),
    }),
    (99, 1800, 20000): (0xba8e82bdc66c367a, {
        256: (0xcc0d6b20c48c0603, 0x494b9475902aad8, 0x86cc3f11aa9c9b29, 0x768e908f52d85f0e),
        64: (0xcc0d6b20c48c0603, 0x494b9475902aad8, 0x86cc3f11aa9c9b29, 0x768e908f52d85f0e),
    }),
    (199, 3000, 30000): (0x22f1eb75a2c3699, {
        256: (0x1f1948b3d5d148ea, 0xdafb7f7f66e49649, 0x7d015f0c776266ec, 0x5d250adda8309ba7),
        64: (0xa2807df0e24bae0, 0xdafb7f7f66e49649, 0x7ba90210648bccc9, 0x5d250adda8309ba7),
    }),
    (499, 9000, 100000): (0xc964bc1e7c6dd4ec, {
        256: (0x21e99ac484e03af8, 0x5351d94e0dc4df78, 0x793a71e47be5293a, 0x6ccc7847d97b071a),
        64: (0xf0152a0407c0896b, 0x5351d94e0dc4df78, 0xd93fa4170d887b39, 0x6ccc7847d97b071a),
    }),
    (2499, 45000, 500000): (0xa647c3c90a236a63, {
        256: (0x61b7ecdc3dbda781, 0x10f88cf952fd21a4, 0x28911526ea5ef954, 0xc9c9dc680ba7251e),
        64: (0xfe2360a10a4a1370, 0xa4834725e4a7e66b, 0xb6bcf5b63f7d5d40, 0xc9c9dc680ba7251e),
    }),
    (833, 15000, 250000): (0x6abc9502c289e5f, {
        256: (0x330ee472dd1709a7, 0x366a698f0b698db8, 0xa3434c6c32bb3677, 0x29272c3a73b4af50),
        64: (0x330ee472dd1709a7, 0x366a698f0b698db8, 0xa3434c6c32bb3677, 0x29272c3a73b4af50),
    }),
}
_region_patterns = {}


def _region_pattern(shape):
    if shape not in _region_patterns:
        prob = oa.BAProblem(*shape, seed=11, **_REGION_KW.get(shape, {}))
        _region_patterns[shape] = (prob.N, prob.M) + tuple(prob.pattern())
    return _region_patterns[shape]


def _set_knob(monkeypatch, knob):
    for k in _REGION_KNOBS[1:]:
        monkeypatch.delenv(k[0], raising=False)
    if knob:
        monkeypatch.setenv(*knob)


def test_one_launch_region_schedule_is_pinned(monkeypatch):
    """Every field of every work item, children record and destination of the region, and every per-level launch
    parameter, hashed (dlg_sparse_region_probe: schedule_hash, level_params_hash) and compared with what the set-up
    code produced before it was taken apart: six patterns x 256 / 64 CUs x {default, one replica, no slices,
    DOGLEG_AMD_PERSIST_MAX=3 (which shortens the region of every pattern: it starts at level 2, 7, 4, 5, 7, 26
    instead of 1, 6, 1, 1, 1, 18)}.  The set holds the three forms of a work item: whole update matrix in LDS, a slice
    of it in LDS (up to 663 workgroups: config #4 at 256 CUs), and summed in HBM (up to 23 update matrices: config #4
    without slices) -- among the latter the HBM replicas (rsv2 > 1, not sliced, jsp < 0), e.g. 8 workgroups of
    (49, 900, 10000) and 40 of (833, 15000, 250000) with the default knobs; the assertion finds them where nothing is
    sliced, (99, 1800, 20000) with one replica: 5 workgroups for 4 supernodes."""
    wrong, sliced, hbm, hbm_replicas = [], 0, 0, 0
    for shape, (lvl_hash, by_ncu) in _REGION_HASHES.items():
        N, M, Jp, Ji = _region_pattern(shape)
        for ncu, hashes in by_ncu.items():
            for knob, want in zip(_REGION_KNOBS, hashes):
                _set_knob(monkeypatch, knob)
                st = capi.region_probe(N, M, Jp, Ji, ncu)
                sliced = max(sliced, st["sliced_workgroups"])
                hbm = max(hbm, st["hbm_update_matrices"])
                # with slices allowed a replica either keeps a slice (counted above) or owns a stretch in HBM: more
                # workgroups than supernodes and none sliced can only be the latter
                if knob != _REGION_KNOBS[2] and st["sliced_workgroups"] == 0 and st["hbm_update_matrices"] > 0:
                    hbm_replicas = max(hbm_replicas, st["workgroups"] - st["supernodes"])
                if (st["schedule_hash"], st["level_params_hash"]) != (want, lvl_hash):
                    wrong.append((shape, ncu, knob, hex(st["schedule_hash"]), hex(st["level_params_hash"])))
    assert not wrong, wrong
    assert sliced > 0 and hbm > 0 and hbm_replicas > 0


def _sanitizing_compiler(tmp, flags=None):
    """the first of g++ / clang++ / ROCm's clang++ that links and runs a program sanitized with `flags` (_SAN_FLAGS)"""
    from libdogleg_amd import build as B
    hello = tmp / "hello.cpp"
    hello.write_text("#include <vector>\nint main(){std::vector<int> v(3); return v[2];}\n")
    for cc in ("g++", "clang++", os.path.join(os.path.dirname(B.HIPCC), "amdclang++")):
        try:
            subprocess.run([cc] + (flags or _SAN_FLAGS) + [str(hello), "-o", str(tmp / "hello")], check=True, capture_output=True)
            subprocess.run([str(tmp / "hello")], check=True, capture_output=True)
            return cc
        except (OSError, subprocess.CalledProcessError):
            continue
    return None


_SAN_FLAGS = ["-std=c++17", "-O0", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
_TSAN_FLAGS = ["-std=c++17", "-O1", "-fsanitize=thread", "-pthread"]


def _symbolic_objects(cc, flags, tmp):
    """(csrc, the host sources of the symbolic phase compiled with `flags` into tmp): what a stand-alone program that
    calls sym_analyze links"""
    csrc = os.path.join(ROOT, "libdogleg_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.startswith("sparse_symbolic") and f.endswith(".cpp"))
    subprocess.run([cc] + flags + ["-I", csrc, "-c"] + [os.path.join(csrc, f) for f in names], check=True, cwd=tmp)
    return csrc, [str(tmp / (f[:-4] + ".o")) for f in names]


def _write_pattern(path, N, M, Jp, Ji):
    np.concatenate([[N, M], Jp, Ji]).astype(np.int32).tofile(path)


def test_region_planner_is_clean_under_sanitizers(tmp_path, monkeypatch):
    """The symbolic phase, the planner and its check as a stand-alone program (tests/c/region_plan_main.cpp: plain C++,
    no HIP) under AddressSanitizer and UndefinedBehaviorSanitizer: exit status 0, nothing reported, and the hashes
    the library computes for the same pattern, CUs and knobs."""
    cc = _sanitizing_compiler(tmp_path)
    if cc is None:
        pytest.skip("no compiler here links a program with -fsanitize=address,undefined")
    csrc, sym_objs = _symbolic_objects(cc, _SAN_FLAGS, tmp_path)
    exe, sym_exe = str(tmp_path / "region_plan_main"), str(tmp_path / "symbolic_main")
    subprocess.run([cc] + _SAN_FLAGS + ["-I", csrc, os.path.join(ROOT, "tests", "c", "region_plan_main.cpp")] + sym_objs +
                   [os.path.join(csrc, "sparse_region.cpp"), "-o", exe], check=True)
    subprocess.run([cc] + _SAN_FLAGS + ["-I", csrc, os.path.join(ROOT, "tests", "c", "symbolic_main.cpp")] + sym_objs + ["-o", sym_exe],
                   check=True)
    for shape in list(_REGION_HASHES)[:3]:
        N, M, Jp, Ji = _region_pattern(shape)
        pat = tmp_path / "pattern.bin"
        _write_pattern(pat, N, M, Jp, Ji)
        _set_knob(monkeypatch, None)
        # the symbolic phase alone: the whole pattern, a row shard, one rank of a partition -- the library's sym_hash
        for args, want in (([], capi.symbolic_probe(N, M, Jp, Ji)), (["rows", "150", "401"], capi.symbolic_probe(N, M, Jp, Ji, row0=150, row1=401)),
                           (["part", "1", "2"], capi.partition_probe(N, M, Jp, Ji, 1, 2)[0])):
            r = subprocess.run([sym_exe, str(pat)] + args, capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", (shape, args, r.returncode, r.stderr[-2000:])
            assert int(r.stdout, 16) == want["sym_hash"], (shape, args)
        for ncu in (256, 64):
            for knob in _REGION_KNOBS:
                _set_knob(monkeypatch, knob)
                r = subprocess.run([exe, str(pat), str(ncu)], capture_output=True, text=True)
                assert r.returncode == 0 and r.stderr == "", (shape, ncu, knob, r.returncode, r.stderr[-2000:])
                st = capi.region_probe(N, M, Jp, Ji, ncu)
                assert [int(h, 16) for h in r.stdout.split()] == [st["schedule_hash"], st["level_params_hash"]], (shape, ncu, knob)


def test_symbolic_schedule_threads_are_clean_under_thread_sanitizer(tmp_path, monkeypatch):
    """The four schedules of the symbolic phase (factor updates, Jt*x lists, assembly, solve gather lists) run on four
    threads that share the analysis so far read-only and fill a record each: tests/c/symbolic_main.cpp under
    ThreadSanitizer reports nothing, exits 0 and prints the library's hash, on three bundle adjustments and on one rank of
    a partition."""
    cc = _sanitizing_compiler(tmp_path, _TSAN_FLAGS)
    if cc is None:
        pytest.skip("no compiler here links a program with -fsanitize=thread")
    csrc, sym_objs = _symbolic_objects(cc, _TSAN_FLAGS, tmp_path)
    exe = str(tmp_path / "symbolic_main")
    subprocess.run([cc] + _TSAN_FLAGS + ["-I", csrc, os.path.join(ROOT, "tests", "c", "symbolic_main.cpp")] + sym_objs + ["-o", exe], check=True)
    for k in _SYM_KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for shape in _SYM_BA:
        N, M, Jp, Ji = _region_pattern(shape)
        pat = tmp_path / "pattern.bin"
        _write_pattern(pat, N, M, Jp, Ji)
        runs = [([], capi.symbolic_probe(N, M, Jp, Ji))]
        if shape == _SYM_BA[1]:
            runs.append((["part", "7", "8"], capi.partition_probe(N, M, Jp, Ji, 7, 8)[0]))
        for args, want in runs:
            r = subprocess.run([exe, str(pat)] + args, capture_output=True, text=True)
            assert r.returncode == 0 and r.stderr == "", (shape, args, r.returncode, r.stderr[-3000:])
            assert int(r.stdout, 16) == want["sym_hash"], (shape, args)


def test_id_file_rendezvous_is_clean_under_sanitizers(tmp_path):
    """The id file of the multi-GPU environment contract as a stand-alone program (tests/c/id_file_main.cpp: it links
    id_file.cpp alone -- plain C++, no HIP, no backend) under AddressSanitizer and UndefinedBehaviorSanitizer: publish then
    wait, a file of another run id (the wait runs out), a truncated file, a file one byte too long."""
    cc = _sanitizing_compiler(tmp_path)
    if cc is None:
        pytest.skip("no compiler here links a program with -fsanitize=address,undefined")
    csrc = os.path.join(ROOT, "libdogleg_amd", "csrc")
    exe = str(tmp_path / "id_file_main")
    subprocess.run([cc] + _SAN_FLAGS + ["-I", csrc, os.path.join(ROOT, "tests", "c", "id_file_main.cpp"),
                                        os.path.join(csrc, "id_file.cpp"), "-o", exe], check=True)
    work = tmp_path / "ids"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stdout, r.stderr[-2000:])
    # (the library's messages of the waits that ran out, nothing from a sanitizer)
    assert all(l.startswith("libdogleg_amd: ") for l in r.stderr.splitlines()), r.stderr[-2000:]


def test_subtree_partition_rows_form_closed_subtrees():
    """the property the partition rests on: a rank's rows touch only its own subtrees' variables and
    the replicated ones -- so J_r' J_r of rank r is zero in every (variable of another rank, *) entry"""
    prob = oa.BAProblem(29, 500, 5000, seed=2)
    Jp, Ji = prob.pattern()
    nranks = 4
    touched = []
    for r in range(nranks):
        st, mine = capi.partition_probe(prob.N, prob.M, Jp, Ji, r, nranks)
        v = np.zeros(prob.N, dtype=bool)
        for row in np.nonzero(mine)[0]:
            v[Ji[Jp[row]:Jp[row+1]]] = True
        touched.append(v)
    shared = np.sum(touched, axis=0) > 1                  # variables seen by more than one rank: the replicated top
    _, perm = capi.symbolic_probe(prob.N, prob.M, Jp, Ji, want_perm=True)
    pos = np.empty(prob.N, dtype=int)
    pos[perm] = np.arange(prob.N)
    # every shared variable is eliminated after every variable private to a rank that also touches a shared one ...
    # simpler and sufficient: the shared variables are few
    assert shared.sum() < 0.25 * prob.N
    assert all(t.any() for t in touched)


def _gloo_partition_worker(rank, world, port, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prob = oa.BAProblem(12, 120, 720, seed=5)
    Jp, Ji = prob.pattern()
    p = prob.p0()
    x, Jx = prob.eval(p)
    N, M = prob.N, prob.M
    # the PRODUCT's partition (libdogleg_amd symbolic phase), this rank's view of it
    st, mine = capi.partition_probe(N, M, Jp, Ji, rank, world)
    rows = np.nonzero(mine)[0]
    Jd = _rows_to_dense(Jp, Ji, Jx, rows, N)
    # the three sums of a step: [Jt x | norm2 x], then JtJ (here dense: the panels above the cut are
    # a subset of it), then the solution -- summed over the ranks they are the single-rank quantities
    g = np.concatenate([Jd.T @ x[rows], [x[rows] @ x[rows]]])
    t = torch.from_numpy(g)
    dist.all_reduce(t)
    A = Jd.T @ Jd
    t2 = torch.from_numpy(A)
    dist.all_reduce(t2)
    sizes = torch.tensor([st["reduced_doubles"], st["cut_level"], st["rows_mine"]], dtype=torch.int64)
    gathered = [torch.zeros_like(sizes) for _ in range(world)]
    dist.all_gather(gathered, sizes)
    if rank == 0:
        Jf = _rows_to_dense(Jp, Ji, Jx, np.arange(M), N)
        ok = (np.allclose(g[:N], Jf.T @ x, rtol=1e-12, atol=1e-12) and abs(g[N] - x @ x) <= 1e-12 * g[N]
              and np.allclose(A, Jf.T @ Jf, rtol=1e-12, atol=1e-12)
              and len({int(v[0]) for v in gathered}) == 1 and len({int(v[1]) for v in gathered}) == 1
              and sum(int(v[2]) for v in gathered) == M)
        q.put(bool(ok))
    dist.destroy_process_group()


def test_subtree_partition_with_gloo_world_size_2():
    """N > 1 on CPU: two processes, the rows dealt out by the product's own partition logic
    (dlg_sparse_partition_probe = the symbolic phase the GPU path runs), partial sums combined with
    torch.distributed (gloo) as RCCL combines them on GPUs"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gloo_partition_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert q.get(timeout=5) is True


def test_documented_limits_are_reported_cleanly():
    """DESIGN.md section 3, "Limits": a pattern outside them makes dlg_sparse_set_pattern (here: the
    host-only probe of the same symbolic phase) return an error with a message -- no crash, no exit"""
    N, M = 70010, 3
    Jp = np.array([0, 70000, 70001, 70002], dtype=np.int32)
    Ji = np.concatenate([np.arange(70000), [5], [7]]).astype(np.int32)
    with pytest.raises(capi.DlgError, match="at most 65535"):
        capi.symbolic_probe(N, M, Jp, Ji)
    # a row touching 300 separate var-blocks is within the limits of the symbolic phase
    rows = [np.arange(0, 3000, 10)] + [np.array([10 * k, 10 * k + 1]) for k in range(300)]
    Jp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    Ji = np.concatenate(rows).astype(np.int32)
    st = capi.symbolic_probe(3000, len(rows), Jp, Ji)
    assert st["supernodes"] > 0


def _id_file_reader(path, run_id, q):
    import ctypes as C
    from libdogleg_amd import capi
    L = capi.lib()
    out = (C.c_ubyte * 128)()
    rc = L.dogleg_amd_id_file_wait(path.encode(), out, run_id.encode(), 20000)
    q.put((rc, bytes(out)))


def test_id_file_rendezvous_between_two_processes(tmp_path):
    """the id file of the environment contract (DOGLEG_AMD_RCCL_ID_FILE; reference interface behind it:
    dogleg.h:278-302): a reader process waits while the path holds nothing, a half-written file, a file of an
    EARLIER launch (other run id) -- and takes this launch's 128 bytes once rank 0 has published them.  No GPU
    call on either side."""
    import multiprocessing as mp
    import time
    L = capi.lib()
    path = str(tmp_path / "id")
    stale = bytes(range(128))
    assert L.dogleg_amd_id_file_publish(path.encode(), stale, b"launch-1") == 0
    assert os.path.getsize(path) == 144
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    pr = ctx.Process(target=_id_file_reader, args=(path, "launch-2", q))
    pr.start()
    time.sleep(1.0)
    assert q.empty(), "the reader took the id of another launch"
    open(path, "wb").write(b"\x01" * 77)                       # a torn file is not an id either
    time.sleep(0.5)
    assert q.empty()
    fresh = bytes((7 * i + 3) % 256 for i in range(128))
    assert L.dogleg_amd_id_file_publish(path.encode(), fresh, b"launch-2") == 0
    rc, got = q.get(timeout=30)
    pr.join(30)
    assert rc == 0 and got == fresh
    assert not os.path.exists(path + ".tmp")
    # a reader whose launch never publishes gives up with -1 (and says so), it does not hang
    out = (C.c_ubyte * 128)()
    t0 = time.time()
    assert L.dogleg_amd_id_file_wait(path.encode(), out, b"launch-3", 300) == -1
    assert time.time() - t0 < 5
    assert L.dogleg_amd_id_file_wait(None, out, b"", 10) == -1


def test_symbolic_debug_output_changes_nothing(monkeypatch, capfd):
    """DOGLEG_AMD_SYM_DEBUG (1: what the symbolic phase decided, 2: + the wall time of its steps, on stderr) is a
    diagnostic: the schedules are the same"""
    prob = oa.BAProblem(20, 300, 3000, seed=3)
    Jp, Ji = prob.pattern()
    monkeypatch.delenv("DOGLEG_AMD_SYM_DEBUG", raising=False)
    a = capi.symbolic_probe(prob.N, prob.M, Jp, Ji)
    capfd.readouterr()
    monkeypatch.setenv("DOGLEG_AMD_SYM_DEBUG", "2")
    b = capi.symbolic_probe(prob.N, prob.M, Jp, Ji)
    err = capfd.readouterr().err
    assert a == b
    assert "sym_analyze" in err or "ms" in err


# ---- the symbolic analysis pinned bit for bit: sym_hash (64-bit FNV-1a over every field of SymHost, records field by
# field) of every case below.  The literals were produced by sym_analyze as it stood while it was one function: that
# tree with the same sym_hash and probe entry added and nothing else (profiles/symbolic_refactor.md).
_SYM_KNOB_NAMES = ("DOGLEG_AMD_SLICE_CAP", "DOGLEG_AMD_ND_LEAF", "DOGLEG_AMD_LDS_SPLIT", "DOGLEG_AMD_MF_LEVEL",
                   "DOGLEG_AMD_SYRK_MIN", "DOGLEG_AMD_ASM_MFMA", "DOGLEG_AMD_RIDER_MIN", "DOGLEG_AMD_SYM_DEBUG")
_SYM_KNOBS = (("DOGLEG_AMD_SLICE_CAP", "3000"), ("DOGLEG_AMD_ND_LEAF", "50"), ("DOGLEG_AMD_LDS_SPLIT", "0"),
              ("DOGLEG_AMD_MF_LEVEL", "-1"), ("DOGLEG_AMD_SYRK_MIN", "1"), ("DOGLEG_AMD_ASM_MFMA", "0"),
              ("DOGLEG_AMD_ASM_MFMA", "2"), ("DOGLEG_AMD_RIDER_MIN", "64"))
_SYM_BA = ((49, 900, 10000), (99, 1800, 20000), (199, 3000, 30000))


@functools.lru_cache(maxsize=None)
def _sym_pattern(key):
    """(N, M, Jp, Ji) of ("zoo", name), ("ba", Ncam, Npt, Nobs) (seed 11, _REGION_KW), ("ba-small",), ("structured",
    seed, scale), ("ragged", seed)"""
    if key[0] == "zoo":
        return zoo.case(key[1])[:4]
    if key[0] == "ba":
        return _region_pattern(key[1:])
    if key[0] == "ba-small":
        prob = oa.BAProblem(9, 60, 300, seed=3)                # (test_symbolic_shards_partition_the_contributions)
        return (prob.N, prob.M) + tuple(prob.pattern())
    rng = np.random.default_rng(key[1])
    if key[0] == "structured":
        N, rows, _ = sparse_patterns.random_structured_pattern(rng, scale=key[2])
    else:
        N, _, rows = sparse_patterns.ragged_rows(rng, key[1])
    return (N, len(rows)) + sparse_patterns.rows_to_csc(rows, N)


def _sym_cases():
    """(id, pattern key, ("rows", row0, row1 or None) / ("part", rank, nranks), ((knob, value), ...))"""
    cases = [("zoo:" + n, ("zoo", n), ("rows", 0, None), ()) for n in zoo.NAMES]
    ba = [("ba", *s) for s in _SYM_BA]
    cases += [("ba:%d-%d-%d" % k[1:], k, ("rows", 0, None), ()) for k in ba + [("ba", 833, 15000, 250000)]]
    cases += [("structured:%d" % s, ("structured", s, 1), ("rows", 0, None), ()) for s in (1000, 1001, 1002, 1007)]
    # (the dense block with many row layouts reaches the riders' left-over rows with this threshold only)
    cases += [("structured-x20:9026", ("structured", 9026, 20), ("rows", 0, None), (("DOGLEG_AMD_RIDER_MIN", "8"),)),
              ("ragged:21", ("ragged", 21), ("rows", 0, None), ())]
    cuts = [0, 150, 151, 400, None]
    cases += [("shard:%d" % a, ("ba-small",), ("rows", a, b), ()) for a, b in zip(cuts[:-1], cuts[1:])]
    cases += [("part:%d-%d-%d:%d/%d" % (k[1:] + (r, n)), k, ("part", r, n), ()) for k in ba for n in (2, 8) for r in (0, n - 1)]
    for knob in _SYM_KNOBS:
        cases += [("%s=%s:%s" % (knob[0][11:], knob[1], "-".join(str(x) for x in k[1:])), k, ("rows", 0, None), (knob,))
                  for k in ba + [("zoo", "arrow-9x40+128"), ("zoo", "wide-children")]]
    # (RIDER_MIN=64 leaves the riders of the cases above as they are: a threshold under which a structured pattern gets
    # riders and one over which the bundle adjustment loses them)
    cases += [("%s=%s:%s" % (knob[11:], val, "-".join(str(x) for x in k[1:])), k, ("rows", 0, None), ((knob, val),))
              for knob, val, k in (("DOGLEG_AMD_RIDER_MIN", "16", ("structured", 1000, 1)), ("DOGLEG_AMD_RIDER_MIN", "100000", ba[0]))]
    return cases


_SYM_CASES = _sym_cases()
_SYM_HASHES = {
    "zoo:dense-16": 0xe56393d9dd65ddfa,
    "zoo:dense-17": 0x10c58f1d2d9c104,
    "zoo:dense-64": 0x90dbc6204da1479a,
    "zoo:dense-65": 0x684a008f18e4c5e7,
    "zoo:dense-127": 0x91c03db4a99cc3fc,
    "zoo:dense-128": 0x69497d787ac655d,
    "zoo:dense-129": 0xa97e4dfc8d9f96aa,
    "zoo:scattered": 0x4c5a067246a9c3fe,
    "zoo:banded": 0xe9cf819581db143c,
    "zoo:holes": 0x659912a2d92ae390,
    "zoo:arrow-3x60+70": 0xf28406672058e945,
    "zoo:arrow-1x300+5": 0x7accb3803507705,
    "zoo:arrow-3x200+17": 0xc7c72686a1935c40,
    "zoo:arrow-9x40+128": 0xfaecc8b5d56d9d02,
    "zoo:wide-children": 0xebcd5d7e607528f2,
    "zoo:wide-root": 0xcbcfb61f57d80aae,
    "zoo:ba-tiny": 0x5435f4623e3607e9,
    "ba:49-900-10000": 0x83612db5b6142cde,
    "ba:99-1800-20000": 0xcc244183a9f443d2,
    "ba:199-3000-30000": 0xf27ea9f74f442cff,
    "ba:833-15000-250000": 0x95c8da4316ff3745,
    "structured:1000": 0x7f2a1d4fdcac2db6,
    "structured:1001": 0x657e030b42a4b960,
    "structured:1002": 0xb3149f9043d23bf5,
    "structured:1007": 0x5e5bc182363ec093,
    "structured-x20:9026": 0xda38389bdf9a0377,
    "ragged:21": 0x8d4f6f30d6870cf,
    "shard:0": 0x6f4c1aad988225e4,
    "shard:150": 0x5806c1dc82b82d1a,
    "shard:151": 0x13d4edc4a573eeb8,
    "shard:400": 0x4f11c4d79c5dcff1,
    "part:49-900-10000:0/2": 0x15fb1d7a8239ffb3,
    "part:49-900-10000:1/2": 0x4699987c353e6ae9,
    "part:49-900-10000:0/8": 0xf1602fe5731be79e,
    "part:49-900-10000:7/8": 0xde28613c94c121c4,
    "part:99-1800-20000:0/2": 0xfec566a1771fd082,
    "part:99-1800-20000:1/2": 0x408508e1171ce739,
    "part:99-1800-20000:0/8": 0x28f5ad1f27444d8c,
    "part:99-1800-20000:7/8": 0x559177d72e5b2b9d,
    "part:199-3000-30000:0/2": 0x55e4b77fe1c76385,
    "part:199-3000-30000:1/2": 0xfa9fe7930b0dcca7,
    "part:199-3000-30000:0/8": 0x6aebac4eed6d8999,
    "part:199-3000-30000:7/8": 0xf60b25542d5a7e7b,
    "SLICE_CAP=3000:49-900-10000": 0x533156d4e1d7a9b2,
    "SLICE_CAP=3000:99-1800-20000": 0x8e677ce7c76f28bd,
    "SLICE_CAP=3000:199-3000-30000": 0xafc0f55268b17702,
    "SLICE_CAP=3000:arrow-9x40+128": 0xea9f69c2140e94b8,
    "SLICE_CAP=3000:wide-children": 0xd0b6204e85b22de7,
    "ND_LEAF=50:49-900-10000": 0x83612db5b6142cde,
    "ND_LEAF=50:99-1800-20000": 0xc276ec144467c51,
    "ND_LEAF=50:199-3000-30000": 0xf27ea9f74f442cff,
    "ND_LEAF=50:arrow-9x40+128": 0xfaecc8b5d56d9d02,
    "ND_LEAF=50:wide-children": 0xebcd5d7e607528f2,
    "LDS_SPLIT=0:49-900-10000": 0x766d86f3f6caf53b,
    "LDS_SPLIT=0:99-1800-20000": 0x561827911d20b81a,
    "LDS_SPLIT=0:199-3000-30000": 0x5e69443655abd2c3,
    "LDS_SPLIT=0:arrow-9x40+128": 0xfaecc8b5d56d9d02,
    "LDS_SPLIT=0:wide-children": 0xebcd5d7e607528f2,
    "MF_LEVEL=-1:49-900-10000": 0x16d63d0e95029ac8,
    "MF_LEVEL=-1:99-1800-20000": 0xbe7de81c06224b53,
    "MF_LEVEL=-1:199-3000-30000": 0x474ef0662d5a9509,
    "MF_LEVEL=-1:arrow-9x40+128": 0x8fd1760aa6bb0b00,
    "MF_LEVEL=-1:wide-children": 0x769b1cefa5ae990,
    "SYRK_MIN=1:49-900-10000": 0xbef88fcc3160bfd8,
    "SYRK_MIN=1:99-1800-20000": 0xcc244183a9f443d2,
    "SYRK_MIN=1:199-3000-30000": 0xf27ea9f74f442cff,
    "SYRK_MIN=1:arrow-9x40+128": 0xfaecc8b5d56d9d02,
    "SYRK_MIN=1:wide-children": 0xebcd5d7e607528f2,
    "ASM_MFMA=0:49-900-10000": 0x753ebbf8f3c47235,
    "ASM_MFMA=0:99-1800-20000": 0xec28a9ea27c24325,
    "ASM_MFMA=0:199-3000-30000": 0xcd6d4bb0fb02ad9a,
    "ASM_MFMA=0:arrow-9x40+128": 0xebcc7ae66c05c67c,
    "ASM_MFMA=0:wide-children": 0x355bed998c5bef0b,
    "ASM_MFMA=2:49-900-10000": 0x83eeb1e6314637ab,
    "ASM_MFMA=2:99-1800-20000": 0x76ab8b07d8c6d15f,
    "ASM_MFMA=2:199-3000-30000": 0x3d5c15e0c490c452,
    "ASM_MFMA=2:arrow-9x40+128": 0xbd1ec51cd880a4c3,
    "ASM_MFMA=2:wide-children": 0xbd99a1d8b76fdf8f,
    "RIDER_MIN=64:49-900-10000": 0x83612db5b6142cde,
    "RIDER_MIN=64:99-1800-20000": 0xcc244183a9f443d2,
    "RIDER_MIN=64:199-3000-30000": 0xf27ea9f74f442cff,
    "RIDER_MIN=64:arrow-9x40+128": 0xfaecc8b5d56d9d02,
    "RIDER_MIN=64:wide-children": 0xebcd5d7e607528f2,
    "RIDER_MIN=16:1000-1": 0xa1c7321c8d511cc1,
    "RIDER_MIN=100000:49-900-10000": 0xb3af2d8be9a8c73,
}


def _sym_case_hash(key, mode):
    N, M, Jp, Ji = _sym_pattern(key)
    if mode[0] == "part":
        return capi.partition_probe(N, M, Jp, Ji, mode[1], mode[2])[0]["sym_hash"]
    return capi.symbolic_probe(N, M, Jp, Ji, row0=mode[1], row1=mode[2])["sym_hash"]


@pytest.mark.parametrize("case", _SYM_CASES, ids=[c[0] for c in _SYM_CASES])
def test_symbolic_analysis_is_pinned(case, monkeypatch):
    """Every array and scalar the symbolic phase hands the kernels, hashed and compared with what sym_analyze produced
    before it was split into phases: every pattern of the factor-user zoo, four bundle adjustments (one with scaled and
    zero columns), random structured patterns, the dense block with many row layouts, ragged rows; the row shards of
    test_symbolic_shards_partition_the_contributions; subtree partitions over 2 and 8 ranks as the first and the last
    rank see them; every knob of the phase at a non-default value.  Between them the cases reach MFMA and scalar
    assembly tasks, riders, partial-sum stages with intermediates, k-groups with and without inline destinations,
    sliced supernodes, two-phase levels, empty and non-empty multifrontal regions, update units with partial slabs,
    chunked Jt*x lists and a partition cut (the list per case: profiles/symbolic_refactor.md)."""
    cid, key, mode, env = case
    for k in _SYM_KNOB_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    assert hex(_sym_case_hash(key, mode)) == hex(_SYM_HASHES[cid])
