"""Host side of the lean leaf launch: which panel buffer still holds the assembled rows
below its merged leaves' member blocks is plain C++ (libdogleg_amd/csrc/leaf_rows_state.h).  No GPU."""
import os
import subprocess

import pytest

from tests.test_library_cpu import _SAN_FLAGS, _sanitizing_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_leaf_rows_state_machine_is_clean_under_sanitizers(tmp_path):
    """tests/c/leaf_rows_state_main.cpp walks assemble -> factor -> swap -> hold -> restore -> materialise (and the
    write-back mode, a stopped factorisation, a buffer without a slot, a new pattern) under AddressSanitizer and
    UndefinedBehaviorSanitizer: exit status 0, "ok", nothing on stderr."""
    cc = _sanitizing_compiler(tmp_path)
    if cc is None:
        pytest.skip("no compiler here links a program with -fsanitize=address,undefined")
    exe = str(tmp_path / "leaf_rows_state_main")
    subprocess.run([cc] + _SAN_FLAGS + ["-I", os.path.join(ROOT, "libdogleg_amd", "csrc"),
                                        os.path.join(ROOT, "tests", "c", "leaf_rows_state_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", (r.returncode, r.stdout, r.stderr[-2000:])


def test_leaf_rows_stats_symbol_is_declared_and_listed():
    from libdogleg_amd import capi
    assert "dlg_sparse_leaf_rows_stats" in capi.BACKEND_SYMBOLS
    assert "dlg_sparse_leaf_rows_stats" in open(os.path.join(ROOT, "include", "dlg_backend.h")).read()
