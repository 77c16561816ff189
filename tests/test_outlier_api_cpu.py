"""The outlier API of the reference's dogleg.h (dogleg.h:331-392) as a C user compiles against it: a probe built with
gcc against include/dogleg.h assigns each of the four entry points to a pointer typed with the reference's prototype,
checks the layout of struct dogleg_outliers_t, links against libdogleg_amd.so and finds the four symbols there.  No GPU."""
import ctypes as C
import os
import subprocess

from libdogleg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <stdio.h>
#include <stdbool.h>
#include "dogleg.h"

/* the reference's prototypes, written out as pointer types */
typedef bool (*factors_fn)(double*, double*, int, int, int, dogleg_operatingPoint_t*, dogleg_solverContext_t*);
typedef bool (*mark_fn)(struct dogleg_outliers_t*, double*, int*, double (*)(int), int, int,
                        dogleg_operatingPoint_t*, dogleg_solverContext_t*);
typedef void (*report_fn)(double (*)(int), double*, int, int, int, dogleg_operatingPoint_t*, dogleg_solverContext_t*);
typedef double (*trace_fn)(const double*, int, int, int, int, dogleg_operatingPoint_t*, dogleg_solverContext_t*);

_Static_assert(sizeof(struct dogleg_outliers_t) == 1, "struct dogleg_outliers_t is one byte");

int main(void)
{
  factors_fn f = &dogleg_getOutliernessFactors;
  mark_fn    m = &dogleg_markOutliers;
  report_fn  r = &dogleg_reportOutliers;
  trace_fn   t = &dogleg_getOutliernessTrace_newFeature_sparse;
  struct dogleg_outliers_t o[2] = {{0}, {0}};
  o[1].marked = 1;
  printf("%d %d %d\n", (int)sizeof(struct dogleg_outliers_t), o[0].marked, o[1].marked);
  return (f && m && r && t) ? 0 : 1;
}
'''

NAMES = ["dogleg_getOutliernessFactors", "dogleg_markOutliers", "dogleg_reportOutliers",
         "dogleg_getOutliernessTrace_newFeature_sparse"]


def test_outlier_prototypes_compile_and_link(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = str(tmp_path / "probe")
    libdir = os.path.join(ROOT, "libdogleg_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", libdir, "-ldogleg_amd", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["1", "0", "1"]


def test_outlier_symbols_exported():
    L = capi.lib()
    for n in NAMES + ["dlg_feature_leverage", "dlg_outlierness_factors", "dlg_leverage_query", "dlg_leverage_stats"]:
        assert hasattr(L, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for n in NAMES:
        assert n in exported, n


def test_outlier_api_refuses_without_a_context():
    """NULL point / context: false or -1.0 with a message, never an exit"""
    L = capi.lib()
    L.dogleg_getOutliernessFactors.restype = C.c_bool
    L.dogleg_getOutliernessFactors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    f = (C.c_double * 4)()
    scale = C.c_double(-1.0)
    assert not L.dogleg_getOutliernessFactors(f, C.byref(scale), 2, 2, 0, None, None)
    L.dogleg_getOutliernessTrace_newFeature_sparse.restype = C.c_double
    L.dogleg_getOutliernessTrace_newFeature_sparse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                               C.c_void_p, C.c_void_p]
    Jq = (C.c_double * 4)()
    assert L.dogleg_getOutliernessTrace_newFeature_sparse(Jq, 0, 2, 2, 0, None, None) == -1.0
    assert L.dogleg_getOutliernessTrace_newFeature_sparse(Jq, 0, 2, 3, 0, None, None) == -1.0
