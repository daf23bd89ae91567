"""The tap probe of tests/tap_probe.py proved on the oracle alone (no GPU): its closed form is what the oracle's linear mode
computes, faults planted in the late partitions of an IR read far above the bar the GPU tests use, and the same kind of fault
in the decaying IRs of the parity tests stays below the whole-signal bar the suite had until now: the gap the probe closes
(DESIGN.md §2.5b)."""
import functools

import numpy as np
import pytest

from helpers import RMS_TOL
from tap_probe import AMP, BLOCK, SIGMA, WARM, coefficient, compare, describe, place_impulses, probe_ir, response_end, stream, want

N_REF = 8192
GPU_BAR = 1e-4      # test_gpu_tap_probe.py asserts worst <= this
FAULT_FLOOR = 0.025  # 10 % of the smallest tap (0.5 SIGMA) under the smallest settled impulse (0.5 AMP), in U
CALL = 7            # blocks per call of the streams laid out here


def _irs(P, full=False):
    taps = BLOCK * P - (0 if full else 77)
    return [probe_ir(taps, 100 + P), probe_ir(taps, 200 + P)]


def _layout(irs, predelay, ramp):
    """Impulses around a call inside the cold-start ramp or after the warm-up, and the stream's length in blocks: the last
    response's end plus two blocks."""
    P = -(-irs[0].shape[0] // BLOCK)
    start = 0 if ramp else -(-(WARM + P) // CALL) * CALL
    bounds = [start + CALL * j for j in range(4)]
    imp = place_impulses(bounds, seed=7 + predelay + ramp, batch=1 if ramp else 2, first=start, extra=(start + 2, start + 3) if ramp else ())
    nb = -(-response_end(irs, imp, predelay) // BLOCK) + 2
    return imp, nb


def _oracle(irs, x, predelay):
    import oracle

    u = oracle.Upols(N_REF, compat=False)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
    for h in (0, 1):
        u.set(h, select=h, predelay=predelay, dry=0.0, wet=1.0, level=1.0, panWet=0.0, panDry=0.0, vsteps=0, speed=100)
    out = u.process(x[0], x[1])
    u.close()
    return out


@functools.lru_cache(maxsize=None)
def _settled(P):
    """A settled stream over P partitions, its closed form and the oracle's output of the clean IRs."""
    irs = _irs(P)
    imp, nb = _layout(irs, 0, False)
    x = stream(imp, nb * BLOCK)
    w = want(irs, imp, nb * BLOCK)
    clean = _oracle(irs, x, 0)
    for a in (x, w, clean):
        a.setflags(write=False)
    return irs, imp, x, w, clean


def test_the_helper_places_what_it_promises():
    bounds = [200, 207, 214, 221]
    imp = place_impulses(bounds, seed=1, first=200)
    blocks = [n // BLOCK for _, n, _ in imp]
    assert 5 <= len(imp) <= 8
    assert 214 in blocks and 220 in blocks and any(207 <= b < 214 for b in blocks)
    assert any(b % 2 == 0 for b in blocks) and any(b % 2 == 1 for b in blocks)
    assert {0, 255} <= {n % BLOCK for _, n, _ in imp} and any(0 < n % BLOCK < 255 for _, n, _ in imp)
    assert {i for i, _, _ in imp} == {0, 1}
    assert all(0.5 * AMP <= abs(a) <= AMP for _, _, a in imp)
    with pytest.raises(ValueError):
        place_impulses(bounds, seed=1, batch=0, first=201)
    h = probe_ir(1000, 3)
    assert h.dtype == np.float32 and h.shape == (1000, 2) and np.abs(h).min() >= 0.5 * SIGMA * (1 - 1e-6) and np.abs(h).max() <= SIGMA
    assert not np.array_equal(h[:, 0], h[:, 1]) and not np.array_equal(h, probe_ir(1000, 4))
    assert coefficient(0) == pytest.approx(0.2) and coefficient(WARM) == 1.0


@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
@pytest.mark.parametrize("predelay", [0, 301])
@pytest.mark.parametrize("P,full", [(16, False), (16, True), (17, False)], ids=["P16", "P16full", "P17"])
def test_the_closed_form_is_what_the_oracle_computes(oracle_mod, P, full, predelay, ramp):
    """(a) <= 1e-6 U; measured 4e-15 U (the oracle's double transforms; the amplitudes and taps are the float32 values in both)."""
    irs = _irs(P, full)
    imp, nb = _layout(irs, predelay, ramp)
    assert 5 <= len(imp) <= 8
    x = stream(imp, nb * BLOCK)
    w = want(irs, imp, nb * BLOCK, predelay)
    got = _oracle(irs, x, predelay)
    r = compare(got, w, irs, imp, predelay)
    print(f"P {P} full {full} predelay {predelay} ramp {ramp}: {describe(r)}; peak {np.abs(w).max():.3f}")
    assert np.abs(w).max() < 0.4
    assert r["worst"] <= 1e-6, describe(r)
    assert np.abs(got[:, -2 * BLOCK:]).max() <= 1e-12  # (double rounding of the last partition's transform, not signal)


def _fault(name, h, P):
    h = h.copy()
    taps = h.shape[0]
    if name == "last_partition_zeroed":
        h[BLOCK * (P - 1):] = 0
    elif name == "partitions_swapped":
        a = h[BLOCK * (P - 3):BLOCK * (P - 2)].copy()
        h[BLOCK * (P - 3):BLOCK * (P - 2)] = h[BLOCK * (P - 2):BLOCK * (P - 1)]
        h[BLOCK * (P - 2):BLOCK * (P - 1)] = a
    elif name == "last_3_percent_scaled":
        h[taps - (3 * taps) // 100:] *= np.float32(0.9)
    elif name == "single_tap_zeroed":
        h[BLOCK * (P - 1) - 1] = 0
    return h


FAULTS = {"last_partition_zeroed": lambda t, P: t >= BLOCK * (P - 1), "partitions_swapped": lambda t, P: BLOCK * (P - 3) <= t < BLOCK * (P - 1),
          "last_3_percent_scaled": lambda t, P: t >= (BLOCK * P - 77) - (3 * (BLOCK * P - 77)) // 100, "single_tap_zeroed": lambda t, P: t == BLOCK * (P - 1) - 1}


@pytest.mark.parametrize("P", [16, 17])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_fault_in_the_late_taps_fails_the_probe(oracle_mod, fault, P):
    """(b) each fault, in either input's IR, moves `worst` by >= 0.025 U, 250 times the GPU tests' bar, and `compare` names a tap
    the fault touched."""
    irs, imp, x, w, clean = _settled(P)
    r0 = compare(clean, w, irs, imp)
    assert r0["worst"] <= 1e-6
    for which in (0, 1):
        bad = list(irs)
        bad[which] = _fault(fault, irs[which], P)
        r = compare(_oracle(bad, x, 0), w, irs, imp)
        print(f"P {P} {fault} in IR {which}: {describe(r)}")
        assert r["worst"] - r0["worst"] >= FAULT_FLOOR, describe(r)
        assert r["worst"] > 100 * GPU_BAR
        assert any(imp[k][0] == which and FAULTS[fault](t, P) for k, t in r["covering"]), describe(r)


def _tail_rms(ir, first_tap, wet=0.5, x_rms=0.1447):
    """What silencing the taps from first_tap on moves the output of a parity case by, RMS over both channels: two independent
    white inputs of RMS x_rms (synth.make_input: uniform(-0.25, 0.25) + 0.01) through the same IR at gain wet (helpers.BASE), so
    per channel the variance is 2 x_rms^2 wet^2 sum h^2 over the silenced taps."""
    e = np.sum(ir[first_tap:].astype(np.float64) ** 2, axis=0)
    return float(np.sqrt(np.mean(2.0 * x_rms ** 2 * wet ** 2 * e)))


def test_the_parity_cases_do_not_see_their_last_partitions():
    """(c) The blindness the probe closes, from the decaying IRs' own energies (no long oracle run).  make_ir(88200, norm=0.02),
    the IR of test_fast_fir_form... and test_second_level_transform...: with the last 10 of its 345 partitions missing
    altogether the output moves by 9.9e-6 RMS.  make_ir(441000), the headline IR: with its last partition missing, 7.1e-6.
    Both are below RMS_TOL, the only bar those cases hold the late partitions to."""
    from cuda_audio_amd.synth import make_ir

    ten = _tail_rms(make_ir(88200, seed=5678, norm=0.02), BLOCK * 335)
    one = _tail_rms(make_ir(441000, seed=5678), BLOCK * 1722)
    print(f"88200 taps, last 10 of 345 partitions: {ten:.2e}; 441000 taps, last of 1723: {one:.2e}; RMS_TOL {RMS_TOL:.0e}")
    assert 5e-6 < ten < RMS_TOL
    assert 3e-6 < one < RMS_TOL
