"""The Jacobian check's host side: its exports, the first-fit colouring against a numpy restatement, the refusals that need
no device (each returns -1 and leaves every output as it was), and the planner as a stand-alone sanitized program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (CB_DEVICE_BATCH, BATCH_MAX_NSTATE, JacobianReport, JacobianEntry, dptr, iptr)
from tests import oracle_api as oa
from tests import jacobian_patterns as jp
from tests.test_library_cpu import _sanitizing_compiler, _SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CB_DEVICE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
BA_SHAPES = [(3, 8, 24), (7, 50, 400), (12, 120, 720)]
NEW_SYMBOLS = ["dogleg_amd_jacobian_colouring", "dogleg_amd_check_jacobian_device", "dogleg_amd_check_jacobian_device_batch",
               "dogleg_amd_testGradient_device", "dogleg_amd_check_jacobian_last_stats"]


def _patterns():
    out = []
    for shape in BA_SHAPES:
        prob = oa.BAProblem(*shape)
        Jp, Ji = prob.pattern()
        out.append((f"ba{shape}", prob.N, prob.M, Jp, Ji))
    Jp, Ji = jp.ragged_pattern()
    out.append(("ragged", 40, 70, Jp, Ji))
    Jp, Ji = jp.full_pattern(5, 4)
    out.append(("dense5x4", 4, 5, Jp, Ji))
    return out


def test_symbols_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NEW_SYMBOLS:
        assert n in exported and n in capi.DOGLEG_SYMBOLS, n


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "dogleg.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(dogleg_amd_jacobian_report_t), offsetof(dogleg_amd_jacobian_report_t, max_error),
         offsetof(dogleg_amd_jacobian_report_t, worst_var), offsetof(dogleg_amd_jacobian_report_t, worst_reported),
         offsetof(dogleg_amd_jacobian_report_t, ncolours), offsetof(dogleg_amd_jacobian_report_t, evaluations));
  printf("%zu %zu %zu %d\n", sizeof(dogleg_amd_jacobian_entry_t), offsetof(dogleg_amd_jacobian_entry_t, meas),
         offsetof(dogleg_amd_jacobian_entry_t, reported), DOGLEG_AMD_JACOBIAN_ONE_AT_A_TIME);
  return 0;
}
''')
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    R, E = JacobianReport, JacobianEntry
    assert [int(v) for v in lines[0].split()] == [C.sizeof(R), R.max_error.offset, R.worst_var.offset, R.worst_reported.offset,
                                                  R.ncolours.offset, R.evaluations.offset]
    assert [int(v) for v in lines[1].split()] == [C.sizeof(E), E.meas.offset, E.reported.offset, 1]


@pytest.mark.parametrize("name,N,M,Jp,Ji", _patterns(), ids=[p[0] for p in _patterns()])
def test_colouring_is_first_fit(name, N, M, Jp, Ji):
    nc, colour = capi.jacobian_colouring(N, M, Jp, Ji)
    want = jp.first_fit(N, M, Jp, Ji)
    assert np.array_equal(colour, want)
    assert nc == int(want.max()) + 1
    for r in range(M):                                        # no row holds two variables of one colour
        cs = colour[Ji[Jp[r]:Jp[r + 1]]]
        assert len(set(cs.tolist())) == len(cs), r
    assert nc <= jp.max_neighbours(N, M, Jp, Ji) + 1          # the first-fit guarantee
    if name.startswith("ba"):
        assert np.all(np.diff(Jp) == 15) and nc == 15         # the row length, hence the optimum
    if name == "ragged":
        assert colour[29] == 0 and Jp[13] == Jp[14]           # the variable in no row; the empty row is there
    if name == "dense5x4":
        assert np.array_equal(colour, np.arange(4))


def test_colouring_refusals():
    Jp, Ji = jp.ragged_pattern()
    L = capi.lib()
    colour = np.full(40, -7, dtype=np.int32)

    def call(n=40, m=70, cp=Jp, ri=Ji, out=colour):
        rc = L.dogleg_amd_jacobian_colouring(n, m, None if cp is None else iptr(cp), None if ri is None else iptr(ri),
                                             None if out is None else iptr(out))
        assert np.all(colour == -7)
        return rc

    assert call(n=0) == -1 and call(m=0) == -1 and call(cp=None) == -1 and call(ri=None) == -1 and call(out=None) == -1
    bad = Ji.copy()
    k = int(np.nonzero(np.diff(Jp) >= 2)[0][0])
    bad[Jp[k]], bad[Jp[k] + 1] = Ji[Jp[k] + 1], Ji[Jp[k]]
    assert call(ri=bad) == -1                                 # not ascending within a column
    bad = Ji.copy()
    bad[3] = 40
    assert call(ri=bad) == -1                                 # a row index out of range
    cp = Jp.copy()
    cp[0] = 1
    assert call(cp=cp) == -1


def _refusal_setup():
    L = capi.lib()
    calls = []
    cb = CB_DEVICE(lambda *a: calls.append(a))
    cbb = CB_DEVICE_BATCH(lambda *a: calls.append(a))
    return L, calls, cb, cbb


def test_refusals_leave_the_outputs_alone(capfd):
    L, calls, cb, _ = _refusal_setup()
    f = C.cast(cb, C.c_void_p)
    N, M = 40, 70
    Jp, Ji = jp.ragged_pattern()
    nnz = len(Ji)
    p0 = np.linspace(-1.0, 1.0, N)
    rep = JacobianReport()
    C.memset(C.byref(rep), 0x5a, C.sizeof(rep))
    keep_rep = bytes(rep)
    ve = np.full(N, -7.5)
    bad = (JacobianEntry * 4)()
    C.memset(bad, 0x5a, C.sizeof(bad))
    keep_bad = bytes(bad)

    def call(p=p0, n=N, m=M, nz=nnz, cp=Jp, ri=Ji, fn=f, rtol=0.0, atol=1e-7, report=rep, flags=0):
        rc = L.dogleg_amd_check_jacobian_device(None if p is None else dptr(p), n, m, nz, None if cp is None else iptr(cp),
                                                None if ri is None else iptr(ri), fn, None, 0.0, rtol, atol, flags,
                                                None if report is None else C.byref(report), dptr(ve), bad, 4)
        assert bytes(rep) == keep_rep and bytes(bad) == keep_bad and np.all(ve == -7.5)
        return rc

    assert call(p=None) == -1 and call(fn=None) == -1 and call(report=None) == -1
    assert call(n=0) == -1 and call(m=0) == -1
    assert call(nz=nnz + 1) == -1 and call(nz=nnz - 1) == -1          # the pattern disagrees with NJnnz
    assert call(nz=0) == -1                                           # dense takes no pattern
    assert call(cp=None) == -1 and call(ri=None) == -1
    swapped = Ji.copy()
    k = int(np.nonzero(np.diff(Jp) >= 2)[0][0])
    swapped[Jp[k]], swapped[Jp[k] + 1] = Ji[Jp[k] + 1], Ji[Jp[k]]
    assert call(ri=swapped) == -1                                     # row indices not ascending within a column
    dup = Ji.copy()
    dup[Jp[k] + 1] = dup[Jp[k]]
    assert call(ri=dup) == -1                                         # ... nor repeated
    assert call(rtol=-1e-3) == -1 and call(atol=-1.0) == -1 and call(rtol=float("nan")) == -1 and call(atol=float("nan")) == -1
    fn = capi.ALLREDUCE_FN(lambda b_, n_, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call() == -1                                           # a communicator is set: one rank only
    finally:
        L.dogleg_amd_clear_communicator()
    capfd.readouterr()
    assert call(ri=swapped) == -1
    assert "not ascending" in capfd.readouterr().err
    assert not calls


def test_batch_refusals_leave_the_outputs_alone(capfd):
    L, calls, _, cbb = _refusal_setup()
    f = C.cast(cbb, C.c_void_p)
    B, N, M = 4, 3, 12
    p0 = np.arange(1.0, 1.0 + B * N).reshape(B, N)
    reps = (JacobianReport * B)()
    C.memset(reps, 0x5a, C.sizeof(reps))
    keep = bytes(reps)
    bad = (JacobianEntry * 4)()
    C.memset(bad, 0x5a, C.sizeof(bad))
    keep_bad = bytes(bad)
    total = C.c_longlong(-9)

    def call(p=p0, b=B, n=N, m=M, fn=f, rtol=0.0, atol=1e-7, reports=reps):
        rc = L.dogleg_amd_check_jacobian_device_batch(None if p is None else dptr(p), b, n, m, fn, None, 0.0, rtol, atol,
                                                      reports, bad, 4, C.byref(total))
        assert bytes(reps) == keep and bytes(bad) == keep_bad and total.value == -9
        return rc

    assert call(p=None) == -1 and call(fn=None) == -1 and call(reports=None) == -1
    assert call(b=0) == -1 and call(n=0) == -1 and call(m=0) == -1
    big = np.ones((1, BATCH_MAX_NSTATE + 1))
    assert call(p=big, b=1, n=BATCH_MAX_NSTATE + 1) == -1             # above the cap
    assert call(rtol=-1.0) == -1 and call(atol=float("nan")) == -1
    # device memory that cannot fit: refused from the sizes alone (p0 is not read), the message names the size
    capfd.readouterr()
    bmax, mmax = 0x7fffffff // 4, 0x7fffffff // (N + 1)
    assert call(b=bmax, m=mmax) == -1
    err = capfd.readouterr().err
    # x and J on either side, the three p, and per problem a live byte, an accumulator and 64 slots of 32 bytes; 4 records
    want = 16.0 * bmax * mmax * (N + 1.0) + 24.0 * bmax * N + bmax * (1.0 + 48.0 + 32.0 * 64) + 32.0 * 4
    assert want > 1e15 and "bytes of device memory" in err and f"{want:.3g}" in err, err
    fn = capi.ALLREDUCE_FN(lambda b_, n_, cookie: 0)
    assert L.dogleg_amd_set_allreduce(0, 2, -1, C.cast(fn, C.c_void_p), None) == 0
    try:
        assert call() == -1
    finally:
        L.dogleg_amd_clear_communicator()
    assert not calls


def test_valid_calls_without_a_device_fail_cleanly(capfd):
    L, calls, cb, cbb = _refusal_setup()
    if L.dlg_device_count() > 0:
        pytest.skip("a GPU is present: the valid calls are tests/test_jacobian_check_gpu.py's")
    Jp, Ji = jp.ragged_pattern()
    out = capi.check_jacobian_device(np.zeros(40), 40, 70, len(Ji), Jp, Ji, C.cast(cb, C.c_void_p), None, atol=1e-7)
    assert out["rc"] == -1 and out["report"]["nchecked"] == 0 and not out["var_error"].any() and not out["bad"]
    out = capi.check_jacobian_device_batch(np.zeros((4, 3)), 3, 12, C.cast(cbb, C.c_void_p), None, atol=1e-7)
    assert out["rc"] == -1 and not out["bad"] and all(r["nchecked"] == 0 for r in out["reports"])
    capfd.readouterr()
    L.dogleg_amd_testGradient_device(1, dptr(np.zeros(40)), 40, 70, len(Ji), iptr(Jp), iptr(Ji), C.cast(cb, C.c_void_p), None)
    cap = capfd.readouterr()
    assert cap.out == "" and "no HIP device" in cap.err
    assert not calls


def test_planner_is_clean_under_sanitizers(tmp_path):
    """tests/c/gradcheck_plan_main.cpp (plain C++, no HIP) under AddressSanitizer and UndefinedBehaviorSanitizer: exit
    status 0, nothing reported, both plans pass the planner's own check, and the colours are the library's."""
    cc = _sanitizing_compiler(tmp_path)
    if cc is None:
        pytest.skip("no compiler here links a program with -fsanitize=address,undefined")
    csrc = os.path.join(ROOT, "libdogleg_amd", "csrc")
    exe = str(tmp_path / "gradcheck_plan_main")
    subprocess.run([cc] + _SAN_FLAGS + ["-I", csrc, os.path.join(ROOT, "tests", "c", "gradcheck_plan_main.cpp"),
                                        os.path.join(csrc, "gradcheck_plan.cpp"), "-o", exe], check=True)
    for name, N, M, Jp, Ji in _patterns():
        pat = tmp_path / "pattern.bin"
        np.concatenate([[N, M], Jp, Ji]).astype(np.int32).tofile(pat)
        r = subprocess.run([exe, str(pat)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        nc, colour = capi.jacobian_colouring(N, M, Jp, Ji)
        lines = r.stdout.splitlines()
        assert int(lines[0]) == nc and [int(v) for v in lines[1].split()] == colour.tolist(), name
