"""Where p_new goes does not change what a step computes.

dlg_make_step, dlg_step and dlg_take_step hand p_new to the caller's buffer.  A page-locked buffer (what capi.Backend and
the driver pass) is written by a copy engine or by the step's last kernel; a pageable one goes through the backend's
staging vector behind the step's synchronisation, and with dlg_backend_set_defer_tail it sends dlg_step / dlg_take_step down
their in-line form; no buffer at all is allowed too.  The other tests only ever pass the page-locked one.  Here each call
runs with all three, the expected improvement's pass over J in line and behind the decision point, for the three kinds of
step: every scalar, the expected improvement (after dlg_step_tail where it is pending) and p_new are the same bits, and
p_new is the slot's p on the device.  A step taken afterwards on the same backend gives the bits of a fresh backend: a
form that bails out leaves nothing behind.

Which form ran is asserted, not assumed: with dlg_backend_set_defer_tail a page-locked or absent destination leaves the
value pending for dlg_step_tail, a pageable one does not.

What makes the expected improvement the same bits in both forms: sparse, the pass over J leaves its partial sums in
page-locked memory and the host adds them in index order, in line and behind the decision point alike.  Dense, the in-line
pass is summed by a tree on the device, so equal bits hold only where the value comes from the solved system (no pass over
J, dlg_backend_ei_source) -- which these well-conditioned shapes do, and which the test asserts for every dense value;
DOGLEG_AMD_EI_JPASS and the other knobs of the step path are cleared for the test."""
import functools
import struct

import numpy as np
import pytest

from libdogleg_amd import capi
from tests import oracle_api as oa

pytestmark = pytest.mark.gpu

KINDS = {"cauchy": capi.KIND_CAUCHY, "gn": capi.KIND_GN, "interp": capi.KIND_INTERP}
DESTS = ("page-locked", "pageable", "absent")


@functools.lru_cache(maxsize=None)
def _problem(kind):
    """(make a backend with slot 0 evaluated, N, sqrt|cauchy|^2, sqrt|gn|^2) -- the smallest shapes of the neighbouring tests"""
    if kind == "sparse":
        prob = oa.BAProblem(6, 60, 400, seed=7)
        Jp, Ji = prob.pattern()
    else:
        prob = oa.DenseProblem(M=500, N=40, seed=7)
    p = prob.p0()
    x, J = prob.eval(p)

    def fresh(defer):
        if kind == "sparse":
            be = capi.Backend(capi.DLG_SPARSE, prob.N, prob.M, prob.nnz)
            be.set_pattern(Jp, Ji)
        else:
            be = capi.Backend(capi.DLG_DENSE, prob.N, prob.M)
        be.set_defer_tail(defer)
        be.set_p(0, p)
        evaluate(be)
        return be

    def evaluate(be):
        be.upload(0, x, J)
        be.eval(0)
    be = fresh(False)
    n2c = be.cauchy(0)
    _, n2g = be.gauss_newton(0, 0.0)
    be.close()
    lo, hi = np.sqrt(n2c), np.sqrt(n2g)
    assert lo < hi
    return fresh, evaluate, prob.N, lo, hi


def _bits(v):
    return None if v is None else (v.tobytes() if isinstance(v, np.ndarray) else struct.pack("<d", v))


@pytest.mark.parametrize("defer", [False, True], ids=["inline", "defer_tail"])
@pytest.mark.parametrize("which", sorted(KINDS))
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_the_destination_of_p_new_changes_no_bit(gpu, monkeypatch, kind, which, defer):
    for knob in ("DOGLEG_AMD_EI_JPASS", "DOGLEG_AMD_DEVICE_FINALS", "DOGLEG_AMD_NO_K8_PREDICT", "DOGLEG_AMD_NO_PRESOLVE"):
        monkeypatch.delenv(knob, raising=False)
    fresh, evaluate, N, lo, hi = _problem(kind)
    # three trust regions that all ask for this kind of step: dlg_take_step's, the retry's (dlg_step), dlg_make_step's
    trs = {"cauchy": [0.5 * lo, 0.4 * lo, 0.3 * lo], "gn": [2.0 * hi, 3.0 * hi, 4.0 * hi],
           "interp": [lo + f * (hi - lo) for f in (0.5, 0.4, 0.3)]}[which]

    def run(dest):
        be = fresh(defer)
        want_p = dest != "absent"
        buf = lambda: np.full(N, np.nan) if dest == "pageable" else None
        rec = []

        def note(scalars, pn):
            on_device = be.download(1, capi.VEC_P)
            if want_p:
                assert np.array_equal(pn, on_device), (dest, len(rec))
            rec.append([_bits(float(v)) for v in scalars] + [_bits(on_device)])

        def tail(ei):
            """the value of the call just made; the form it took is the one its destination allows"""
            deferred = be.step_tail_pending()
            assert deferred == (defer and dest != "pageable"), (dest, len(rec))
            assert np.isnan(ei) == deferred
            ei = be.step_tail() if deferred else ei
            assert kind == "sparse" or be.ei_source()[0], "dense: the value did not come from the solved system"
            return ei

        lam, r, pn = be.take_step(0, 1, trs[0], 0.0, want_p=want_p, p_out=buf(), tail=False)
        assert r["kind"] == KINDS[which]
        r["ei"] = tail(r["ei"])
        first = (lam, r["n2c"], r["n2g"], r["n2s"], r["k"], r["amax"], r["ei"])
        note(first, pn)
        n2s, k, amax, ei, pn = be.step(0, 1, KINDS[which], trs[1], want_p=want_p, p_out=buf(), tail=False)
        note((n2s, k, amax, tail(ei)), pn)
        n2s, k, amax, pn = be.make_step(0, 1, KINDS[which], trs[2], want_p=want_p, p_out=buf())
        note((n2s, k, amax), pn)
        # the next point of the solve on this backend: nothing of the calls above is left behind
        evaluate(be)
        lam, r, pn = be.take_step(0, 1, trs[0], 0.0)
        note((lam, r["n2c"], r["n2g"], r["n2s"], r["k"], r["amax"], r["ei"]), pn)
        be.close()
        return rec

    want = run("page-locked")
    assert want[3] == want[0], "a second dlg_take_step does not give the first one's bits"
    for dest in DESTS[1:]:
        got = run(dest)
        for call, a, b in zip(("take_step", "step", "make_step", "take_step of a fresh backend"), got, want):
            assert a == b, (dest, call, [i for i, (u, v) in enumerate(zip(a, b)) if u != v])
