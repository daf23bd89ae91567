"""The single-transform form's running accumulator (csrc/singlefft.hip.h), whole, at every size the form accepts.

tests/test_gpu_single_form.py compares what the calls emit: the first `nframes` slots of an n_ref-long accumulator.  The rest
reaches an output only n_ref / nframes calls later, and at the long sizes those tests stop long before that - a fault in one row
of the second inverse pass (a twiddle, sf_slot, a Stockham index at M = 1024, a Q8 cut one row off) would pass them.  Here the
accumulator is read through mc_debug_read item 4 after 4 - 6 calls and compared position by position with the one
oracle/refcompat_np.py keeps (tests/single_form_np.py), per row b of the second pass (frames [512 b, 512 b + 512)) and per residue
class a of the first (frames = a mod 512).  With M = n_ref / 512 and AT = max(1, min(8, 2048 / M)) the sizes also differ in path:
k_sf_inv2w (M <= 512; R = 512 / M down to 1 at 262144) or k_sf_inv2 (above, or MCCONV_SF_STOCKHAM at any size) with AT rows per
workgroup, AT = 8 (up to 131072), 4 (262144), 2 (524288), 1 (1048576).

Inputs: two different IRs of stationary noise (no decay: make_ir's envelope leaves the far rows empty), n_ref - 1024 taps each,
one per half; unequal halves; white noise of deviation 0.25.  A call's contribution reaches frame predelay + n_ref - 1025 of the
accumulator it leaves behind, so with no predelay the last row that holds signal is row M - 3; those cases run with 1024-frame
periods, where rows M - 2 and M - 1 lie beyond n_ref - nframes and are not asked to hold any (they are compared all the same).

Conditions on the oracle, asserted before the engine runs (no case can pass on an empty or a clamped accumulator): peak < 0.5;
every row that lies wholly inside [predelay, n_ref - nframes), and every residue class over those rows, has RMS >= 100 RMS_TOL.
Bars (tests/helpers.py, the rule of tests/test_gpu_spectral_probe.py for its worst block): outputs and the whole accumulator
<= RMS_TOL, the worst row and the worst class <= 2 RMS_TOL; the last nframes positions are exactly 0.  Measured: DESIGN.md §7."""
import functools

import numpy as np
import pytest

from helpers import BASE, RMS_TOL, rms
from single_form_np import acc_errors, describe, drive, flat_ir, oracle_run, white_input

pytestmark = pytest.mark.gpu

P0 = dict(BASE, select=0, wet=0.6, panWet=0.3, panDry=-0.2)
P1 = dict(BASE, select=1, wet=0.4, level=0.8, panWet=-0.5, dry=0.3)
# what happens between the calls of the case with events: the predelay goes 301 -> 0 (what earlier calls added stays where it
# is) and half 1 starts towards the other IR with vsteps = 3: its live spectra are still moving when the accumulator is read
EVENTS = {3: ((0, dict(predelay=0)), (1, dict(select=0, vsteps=3, speed=3)))}
# name: n_ref, period, predelay at the start (the largest in force: where the live range begins), calls, IR noise scale, events
CASES = {
    "N4096": (4096, 1024, 0, 6, 0.02, {}),  # (6 x 1024 frames: the ring's origin wraps)
    "N16384": (16384, 512, 301, 5, 0.012, {}),
    "N131072": (131072, 1024, 8192, 4, 0.012, {}),  # the shipped size; Q8 over the last 16 rows
    "N131072_events": (131072, 1024, 301, 6, 0.012, EVENTS),
    "N262144": (262144, 256, 301, 4, 0.012, {}),  # k_sf_inv2w with R = 1
    "N524288": (524288, 512, 8192, 4, 0.012, {}),  # k_sf_inv2, AT = 2
    "N1048576": (1048576, 1024, 0, 4, 0.012, {}),  # k_sf_inv2, AT = 1; the forward pass folds two terms per lane
    "N1048576_q8": (1048576, 1024, 8192, 4, 0.012, {}),
    # Q4: IRs loud enough that the accumulator sits at +-1 at more than 1000 positions that no call has emitted yet
    "N16384_clamp": (16384, 256, 301, 6, 0.2, {}),
}
# case, MCCONV_SF_STOCKHAM: the LDS transform of the long sizes with AT = 8 and with AT = 4
RUNS = [(k, False) for k in CASES if k != "N16384_clamp"] + [("N16384", True), ("N262144", True)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case and the oracle's outputs and accumulator, computed once and left unchanged."""
    n_ref, period, pd, ncalls, scale, events = CASES[name]
    irs = [flat_ir(n_ref - 1024, 100, scale), flat_ir(n_ref - 1024, 200, scale)]
    x = white_input(ncalls * period, 7)
    ev = dict(events)
    ev[0] = ((0, dict(P0, predelay=pd)), (1, P1))
    want = oracle_run(n_ref, irs, x, ev, period)
    for a in (*irs, x, *want):
        a.setflags(write=False)
    return irs, x, ev, want


def _run(monkeypatch, name, stockham, clamped=False):
    n_ref, period, pd, ncalls, _, _ = CASES[name]
    if stockham:
        monkeypatch.setenv("MCCONV_SF_STOCKHAM", "1")
    else:
        monkeypatch.delenv("MCCONV_SF_STOCKHAM", raising=False)
    irs, x, ev, want = _case(name)
    # 1. the oracle alone
    r0 = acc_errors(want[1].astype(np.float32), want[1], lo=pd, hi=n_ref - period)
    at_rail = int((np.abs(want[1][:, period:]) == 1.0).sum())
    print(f"{name} oracle: peak {r0['peak']:.3f}, row floor {r0['row_floor']:.4f}, class floor {r0['class_floor']:.4f} over rows "
          f"{r0['live_rows'][0]} .. {r0['live_rows'][-1]} of {n_ref // 512}, rms(out) {rms(want[0]):.4f}, at +-1 beyond the first period: {at_rail}")
    if clamped:
        assert at_rail > 1000
    else:
        assert r0["peak"] < 0.5
    assert r0["row_floor"] >= 100 * RMS_TOL and r0["class_floor"] >= 100 * RMS_TOL
    assert np.all(want[1][:, n_ref - period:] == 0)
    # 2. the engine
    d = drive(n_ref, irs, x, ev, period, oracle=want)
    out_err = rms(d["got_out"] - d["want_out"])
    r = acc_errors(d["got_acc"], d["want_acc"], lo=pd, hi=n_ref - period)
    print(f"{name}{' (k_sf_inv2)' if stockham else ''}: outputs rms {out_err:.3e}; accumulator {describe(r)}")
    assert out_err <= RMS_TOL, f"outputs: rms {out_err:.3e}"
    assert r["rms"] <= RMS_TOL, describe(r)
    assert r["worst_row"] <= 2 * RMS_TOL and r["worst_class"] <= 2 * RMS_TOL, describe(r)
    assert np.all(d["got_acc"][:, n_ref - period:] == 0), "the far end of the accumulator is not clear"


@pytest.mark.parametrize("name,stockham", RUNS, ids=[k + ("_lds_transform" if s else "") for k, s in RUNS])
def test_whole_accumulator_matches_the_reference(gpu_lib, monkeypatch, name, stockham):
    _run(monkeypatch, name, stockham)


def test_whole_accumulator_is_clamped_on_every_call(gpu_lib, monkeypatch):
    """Q4 (conv.cu:98): the reference clamps its running accumulator everywhere on every call, not only what it emits;
    test_running_accumulator_saturates_like_the_reference sees that where it is emitted, this reads it where it is kept."""
    _run(monkeypatch, "N16384_clamp", False, clamped=True)
