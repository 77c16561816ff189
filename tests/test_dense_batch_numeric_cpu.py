"""The numeric-Jacobian adapter of the dense batch (dogleg_amd_batch_numeric_*), what needs no GPU: the exported step rule
against its numpy restatement (tests/batch_numeric_oracle.py) bit for bit, every refusal of dogleg_amd_batch_numeric_create --
all of them are decided from the arguments before a device is touched, so they are tested here --, the struct layout and the
restatement's own Jacobian on a model with a known one."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from libdogleg_amd import capi
from libdogleg_amd.ctypes_defs import (NumericOptions, NUMERIC_FORWARD, NUMERIC_CENTRAL, NUMERIC_DELTA_DEFAULT, NUMERIC_TILE_ROWS,
                                       BATCH_MAX_NSTATE, CB_DEVICE_BATCH_VALUES)
from tests import batch_numeric_oracle as bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SCHEMES = [NUMERIC_FORWARD, NUMERIC_CENTRAL]


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def step_cases():
    """(p, lo, hi): the cases the step rule has"""
    big, tiny = 1.0e300, 5e-324
    cases = [(0.0, -INF, INF), (-0.0, -INF, INF), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0)]
    cases += [(s * v, -INF, INF) for s in (1.0, -1.0) for v in (big, 1.7e308, tiny, 2.2e-308, 1.0e-200, 3.0, 1.0 / 3.0)]
    cases += [(2.5, -INF, 2.5), (-2.5, -INF, -2.5), (1e9, 0.0, 1e9)]                       # p on hi
    cases += [(2.5, 2.5, INF), (-2.5, -2.5, INF), (1e-9, 1e-9, 1.0)]                       # p on lo
    cases += [(1.0, 1.0 - 1e-12, 1.0 + 1e-12), (1.0, 1.0 - 1e-9, 1.0 + 1e-12),             # p + h > hi with p - h < lo
              (-3.0, -3.0 - 1e-10, -3.0 + 1e-11), (0.0, -1e-12, 1e-12)]
    cases += [(1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-7.25, -7.25, -7.25), (1e300, 1e300, 1e300)]      # lo == hi
    cases += [(1.0, -INF, 1.0 + 1e-12), (1.0, 1.0 - 1e-12, INF), (1.7e308, -INF, INF), (-1.7e308, -INF, INF)]   # infinite bounds
    cases += [(float("nan"), -INF, INF), (float("nan"), 0.0, 1.0)]
    rng = np.random.default_rng(11)
    for _ in range(200):
        p = float(rng.normal() * 10.0 ** rng.integers(-12, 12))
        w = abs(p) * 10.0 ** rng.integers(-12, 1) + 10.0 ** rng.integers(-14, 0)
        a, b = sorted((p - w * rng.random(), p + w * rng.random()))
        cases.append((p, a, b))
    return cases


@pytest.mark.parametrize("scheme", SCHEMES)
def test_step_rule_matches_numpy_bit_for_bit(scheme):
    cases = step_cases()
    p, lo, hi = (np.array(c) for c in zip(*cases))
    for dr, da in (bn.deltas(scheme), (1e-3, 0.0), (0.0, 1e-5), (0.25, 1e-300), (1e-7, 3e-9)):
        tp, tm, d = bn.step(scheme, p, lo, hi, dr, da)
        for i, (pi, loi, hii) in enumerate(cases):
            got = capi.numeric_step(scheme, pi, loi, hii, dr, da)
            want = (tp[i], tm[i], d[i])
            assert bits(got) == bits(want), f"scheme {scheme}, deltas ({dr}, {da}), p {pi!r} in [{loi!r}, {hii!r}]: {got} != {want}"


@pytest.mark.parametrize("scheme", SCHEMES)
def test_step_rule_properties(scheme):
    """what the rule promises, on the restatement and so (by the test above) on the library: inside the box, a zero divisor
    exactly where the box is a point, one-sided on a bound"""
    dr, da = bn.deltas(scheme)
    for p, lo, hi in step_cases():
        if not (lo <= p <= hi):
            continue
        tp, tm, d = (float(v) for v in bn.step(scheme, p, lo, hi, dr, da))
        assert lo <= tp <= hi and lo <= tm <= hi
        if lo == hi:
            assert d == 0.0 and tp == p and tm == p
        elif abs(p) < 1e300:
            assert d != 0.0
        if scheme == NUMERIC_CENTRAL and p == hi and lo < hi:
            assert tp == p and tm < p
        if scheme == NUMERIC_CENTRAL and p == lo and lo < hi:
            assert tm == p and tp > p
        if scheme == NUMERIC_FORWARD and p == hi and lo < hi:
            assert tp < p and d < 0.0
    assert NUMERIC_DELTA_DEFAULT == {NUMERIC_FORWARD: 2.0 ** -26, NUMERIC_CENTRAL: 2.0 ** -17}


def test_default_deltas_of_the_header():
    txt = open(os.path.join(ROOT, "include", "dogleg_numeric_step.h")).read()
    fwd = float(re.search(r"DOGLEG_NUMERIC_DELTA_FORWARD\s+(\S+)", txt).group(1))
    cen = float(re.search(r"DOGLEG_NUMERIC_DELTA_CENTRAL\s+(\S+)", txt).group(1))
    assert fwd == 2.0 ** -26 and cen == 2.0 ** -17
    hdr = open(os.path.join(ROOT, "include", "dogleg.h")).read()
    assert re.search(r"#define DOGLEG_AMD_NUMERIC_FORWARD\s+0\b", hdr) and re.search(r"#define DOGLEG_AMD_NUMERIC_CENTRAL\s+1\b", hdr)
    src = open(os.path.join(ROOT, "libdogleg_amd", "csrc", "batch_numeric.hip")).read()
    assert int(re.search(r"constexpr int NUM_TR = (\d+);", src).group(1)) == NUMERIC_TILE_ROWS


def test_options_struct_layout():
    offs = {n: getattr(NumericOptions, n).offset for n, _ in NumericOptions._fields_}
    assert offs == {"scheme": 0, "delta_rel": 8, "delta_abs": 16, "lower": 24, "upper": 32, "bounds_on_device": 40}
    assert C.sizeof(NumericOptions) == 48
    # the C side agrees: a probe compiled against include/dogleg.h
    import subprocess
    import tempfile
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "dogleg.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(dogleg_amd_numeric_options_t, scheme),
  offsetof(dogleg_amd_numeric_options_t, delta_rel), offsetof(dogleg_amd_numeric_options_t, delta_abs),
  offsetof(dogleg_amd_numeric_options_t, lower), offsetof(dogleg_amd_numeric_options_t, upper),
  offsetof(dogleg_amd_numeric_options_t, bounds_on_device), sizeof(dogleg_amd_numeric_options_t)); return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                       check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [0, 8, 16, 24, 32, 40, 48]


def _values_cb():
    return CB_DEVICE_BATCH_VALUES(lambda *a: None)


def _create(B, N, M, f, opt):
    L = capi.lib()
    return L.dogleg_amd_batch_numeric_create(B, N, M, f, None, C.byref(opt) if opt is not None else None)


def test_create_refusals(capfd):
    """every refusal, each with NULL and a message, none of which is the complaint about a missing device: they come first"""
    keep = _values_cb()
    f = C.cast(keep, C.c_void_p)
    B, N, M = 3, 4, 9
    ok_lo, ok_hi = np.full((B, N), -1.0), np.full((B, N), 1.0)

    def opts(**kw):
        o, k = capi.numeric_options(**kw)
        return o, k

    cases = [("B 0", (0, N, M, f, None), "must not be 0"), ("Nstate 0", (B, 0, M, f, None), "must not be 0"),
             ("Nmeas 0", (B, N, 0, f, None), "must not be 0"),
             ("Nstate too large", (B, BATCH_MAX_NSTATE + 1, M, f, None), "DOGLEG_AMD_BATCH_MAX_NSTATE"),
             ("NULL f", (B, N, M, None, None), "f is NULL")]
    for scheme in (2, -1):
        cases.append((f"scheme {scheme}", (B, N, M, f, opts(scheme=scheme)), "unknown scheme"))
    for dr, da in ((-1e-8, 0.0), (0.0, -1e-8), (float("nan"), 1e-8), (1e-8, float("nan"))):
        cases.append((f"deltas {dr} {da}", (B, N, M, f, opts(scheme=NUMERIC_FORWARD, delta_rel=dr, delta_abs=da)), "negative or NaN"))
    bad_lo = ok_lo.copy()
    bad_lo[2, 1] = 1.5
    cases.append(("lower > upper", (B, N, M, f, opts(scheme=NUMERIC_CENTRAL, lower=bad_lo, upper=ok_hi)), "problem 2, variable 1"))
    cases.append(("a NaN bound", (B, N, M, f, opts(scheme=NUMERIC_FORWARD, lower=np.full((B, N), np.nan))),
                  "problem 0, variable 0"))
    # a size that does not fit: refused from the arithmetic, and the message names the size
    cases.append(("too large", (2 ** 31, 64, 2 ** 31, f, None), "bytes of device memory"))
    for what, (b, n, m, fn, opt), msg in cases:
        o = opt[0] if isinstance(opt, tuple) else opt
        capfd.readouterr()
        h = _create(b, n, m, fn, o)
        err = capfd.readouterr().err
        assert not h, what
        assert msg in err and "no HIP device" not in err, f"{what}: {err!r}"
        assert b"dogleg_amd_batch_numeric_create" in capi.lib().dlg_last_error()
    assert "e+" in err or "E+" in err          # (the last case: the size, in bytes)
    # +-inf bounds and lower == upper are NOT refused: without a device this reaches the device check, with one it succeeds
    o, k = capi.numeric_options(scheme=NUMERIC_CENTRAL, lower=np.full((B, N), -INF), upper=np.where(np.arange(N) % 2, INF, -INF) * np.ones((B, 1)))
    capfd.readouterr()
    h = _create(B, N, M, f, o)
    err = capfd.readouterr().err
    if h:
        capi.lib().dogleg_amd_batch_numeric_destroy(h)
    else:
        assert "no HIP device" in err


def test_destroy_and_stats_take_null():
    L = capi.lib()
    L.dogleg_amd_batch_numeric_destroy(None)
    out = (C.c_double * 6)()
    assert L.dogleg_amd_batch_numeric_stats(None, out, 6) == 0
    assert L.dogleg_amd_batch_numeric_buffers(None, None, None, None) == -1


@pytest.mark.parametrize("scheme", SCHEMES)
def test_restated_jacobian_on_a_known_model(scheme):
    """the restatement's copies and quotients on x = A p + 0.5 (A p)^2: within the truncation error of the scheme, zero
    columns where lo == hi, the copy layout of the contract"""
    rng = np.random.default_rng(3)
    B, N, M = 5, 4, 7
    A = rng.normal(size=(B, M, N))
    p = rng.normal(size=(B, N))
    lo, hi = p - 0.5, p + 0.5
    lo[:, 2] = hi[:, 2] = p[:, 2]           # a held variable
    hi[1, 0] = p[1, 0]                      # on a bound
    dr, da = bn.deltas(scheme)
    pc, d = bn.copies(scheme, p, lo, hi, dr, da)
    K = 2 * N + 1 if scheme == NUMERIC_CENTRAL else N + 1
    assert pc.shape == (K, B, N) and bits(pc[0]) == bits(p)
    for k, j in itertools.product(range(1, K), range(N)):
        moved = (k - 1) % N == j
        assert moved or bits(pc[k, :, j]) == bits(p[:, j])
    assert np.all(pc >= lo[None]) and np.all(pc <= hi[None])

    def model(q):
        u = np.einsum("bmn,bn->bm", A, q)
        return u + 0.5 * u * u

    xc = np.stack([model(pc[k]) for k in range(K)])
    J = bn.jacobian(scheme, xc, d)
    u = np.einsum("bmn,bn->bm", A, p)
    Jtrue = A * (1.0 + u)[:, :, None]
    assert np.all(J[:, :, 2] == 0.0) and not np.any(np.signbit(J[:, :, 2]))
    free = [0, 1, 3]
    err = np.max(np.abs(J[:, :, free] - Jtrue[:, :, free]))
    # d2x/dp_j2 = A_j^2, so a one-sided quotient is off by at most max(A^2) |d| / 2 (a symmetric one by far less), and the
    # rounding of the two x adds at most 4 eps max|x| / min|d|
    dnz = np.abs(d[:, free])
    bound = 0.5 * np.max(A * A) * np.max(dnz) + 4.0 * np.finfo(float).eps * np.max(np.abs(xc)) / np.min(dnz)
    print(f"scheme {scheme}: max |J - J_true| {err:.3g}, bound {bound:.3g}")
    assert err <= bound
