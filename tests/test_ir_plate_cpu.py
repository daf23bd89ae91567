"""The plate's definition without a GPU: the library's mode table and plan (mc_ir_plate_modes, mc_ir_plate_plan: host arithmetic)
against the float64 restatement (tests/ir_plate_np.py), and the restatement itself against what the physics says: Weyl's mode
count, the level the amplitudes are scaled for, the decay per octave band, one mode's closed form."""
import math

import numpy as np
import pytest

import ir_decay_np
import ir_plate_np

RATE = 48000
CASES = [dict(high_hz=400.0), dict(high_hz=16000.0), dict(size=(2.0, 1.0), high_hz=3000.0), dict(size=(0.3, 0.2), thickness_mm=3.0, low_hz=200.0, high_hz=300.0, driver=(0.11, 0.07), pickups=((0.07, 0.13), (0.21, 0.06))),
         dict(material=(70.0, 2700.0, 0.33), thickness_mm=1.0, driver=(1.02, 0.3), pickups=((1.02, 0.5), (0.4, 0.485)), t60=(0.0, 2.0), low_hz=100.0,
              high_hz=2500.0, damp_hz=500.0, gain=3.0)]


def _iplate(fields):
    from cuda_audio_amd.engine import IrPlate

    return IrPlate(**fields)


@pytest.mark.parametrize("fields", CASES)
def test_the_table_and_the_plan_match_the_restatement(fields):
    from cuda_audio_amd.engine import plate_modes, plate_plan

    want = ir_plate_np.modes(fields, RATE)
    rows = plate_modes(_iplate(fields), RATE)
    assert len(rows) == want["M"] > 0
    np.testing.assert_array_equal(rows[:, 0], want["m"])
    np.testing.assert_array_equal(rows[:, 1], want["n"])
    np.testing.assert_allclose(rows[:, 2], want["f"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rows[:, 3], want["sigma"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rows[:, 4:], want["a"], rtol=1e-12, atol=0)
    # m ascending, n ascending within each m
    key = rows[:, 0] * 1e6 + rows[:, 1]
    assert (np.diff(key) > 0).all()
    # a slice is the table's rows
    if len(rows) > 5:
        np.testing.assert_array_equal(plate_modes(_iplate(fields), RATE, first=3, count=2), rows[3:5])
    got, wplan = plate_plan(_iplate(fields), RATE, 4000), ir_plate_np.plan(fields, RATE, 4000)
    assert got["modes"] == wplan["modes"] and got["pairs"] == wplan["pairs"] == 4000 * want["M"]
    for k in ("lowest", "highest", "kappa", "density"):
        assert got[k] == pytest.approx(wplan[k], rel=1e-12), k
    assert got["t60"] == pytest.approx(wplan["t60"], rel=1e-12)
    assert plate_plan(_iplate(dict(fields, last=100)), RATE, 4000)["pairs"] == 100 * want["M"]


def test_the_one_mode_plate_holds_one_mode():
    tb = ir_plate_np.modes(CASES[3], RATE)
    assert tb["M"] == 1 and (int(tb["m"][0]), int(tb["n"][0])) == (1, 1) and 255.0 < tb["f"][0] < 265.0


@pytest.mark.parametrize("high,margin", [(400.0, 0.07), (16000.0, 0.025)])
def test_the_mode_count_against_weyl(high, margin):
    """M against S / (2 kappa) (high - low).  The count runs under Weyl's leading term by the edge correction, which grows as the
    square root of the bandwidth: measured on the restatement, 472 against 492.3 (4.1 %) and 20531 against 20701.9 (0.8 %) for the
    default plate, 478 against 497.6 and 20760 against 20923.7 for 2 x 1 m.  The margins are those with room for both plates."""
    from cuda_audio_amd.engine import plate_plan

    for size in ((2.04, 0.97), (2.0, 1.0)):
        fields = dict(size=size, high_hz=high)
        plan = plate_plan(_iplate(fields), RATE, 1)
        weyl = plan["density"] * (high - 20.0)
        M = ir_plate_np.modes(fields, RATE)["M"]
        print(f"{size} to {high} Hz: {M} modes, Weyl {weyl:.1f}")
        assert plan["modes"] == M and (1.0 - margin) * weyl < M < weyl


def test_the_first_milliseconds_have_the_level_of_gain():
    """4 sqrt(2 / M) makes the expected RMS of M cosines of random phase `gain`: within 1 dB over the first 50 ms of the default
    plate cut at 400 Hz (measured on the restatement: 0.956 and 0.930 of gain)."""
    for gain in (1.0, 0.25):
        y, info = ir_plate_np.frames64(dict(high_hz=400.0, gain=gain), RATE, frames=2400, late_gain=0.0)
        r = np.sqrt((y * y).mean(axis=0)) / gain
        print("rms / gain:", r, info["modes"])
        assert (np.abs(20.0 * np.log10(r)) < 1.0).all()


def test_the_decay_per_octave_band():
    """T30 of the restated IR in the octaves at 250 Hz and 1 kHz (ir_decay_np: the measurement's own restatement) against
    3 ln 10 / sigma.  sigma grows linearly with f, so an octave band holds modes whose decay times run from 3 ln 10 / sigma(f sqrt 2)
    to 3 ln 10 / sigma(f / sqrt 2), and a regression over its decay lies between the two, nearer the slow edge the later it looks
    because the slow modes outlast the fast ones.  Measured on the restatement: 0.2971 s in [0.2614, 0.3162] s (the centre's time is
    0.2909 s) and 0.1841 s in [0.1282, 0.1941] s (the centre's 0.1600 s).  The bounds are the band edges' times, not the measured
    ones; that the time falls from the low band to the high band is asserted too."""
    rate = 8000
    plate = dict(high_hz=2000.0, t60=(0.4, 0.1), damp_hz=2000.0)
    y, info = ir_plate_np.frames(plate, rate, frames=4000, late_gain=0.0)
    res = ir_decay_np.decay(y, rate, bands=(250.0, 1000.0), onset_db=0.0)
    s0, s1 = ir_plate_np.loss(0.4), ir_plate_np.loss(0.1)
    t60_at = lambda hz: 3.0 * math.log(10.0) / (s0 + (s1 - s0) * hz / 2000.0)  # noqa: E731
    got = []
    for b, hz in ((1, 250.0), (2, 1000.0)):
        fast, slow = t60_at(hz * math.sqrt(2.0)), t60_at(hz / math.sqrt(2.0))
        t30 = res["rows"][(b, "LR")]["t30"]
        print(f"{hz} Hz: T30 {t30:.4f} s in [{fast:.4f}, {slow:.4f}] s, the centre's {t60_at(hz):.4f} s")
        assert fast < t30 < slow
        got.append(t30)
    assert got[1] < got[0]


def test_one_mode_is_its_closed_form():
    plate = dict(CASES[3], t60=(0.5, 0.5), gain=0.7)
    tb = ir_plate_np.modes(plate, RATE)
    assert tb["M"] == 1
    F = 3000
    y, _ = ir_plate_np.frames64(plate, RATE, frames=F, late_gain=0.0)
    t = np.arange(F, dtype=np.float64)
    for ch in range(2):
        want = tb["a"][0, ch] * np.exp(-tb["sigma"][0] * t / RATE) * np.cos(2.0 * np.pi * tb["f"][0] * t / RATE)
        assert np.abs(y[:, ch] - want).max() < 1e-11  # (a quantum of 2^-40 is 9.1e-13; the phase in plain double adds a few 1e-13)
    assert abs(tb["sigma"][0] - 3.0 * math.log(10.0) / 0.5) < 1e-12 and np.abs(y).max() > 0.1
    # without loss the envelope is flat: the last period peaks where the first does
    flat, _ = ir_plate_np.frames64(dict(plate, t60=(0.0, 0.0)), RATE, frames=F, late_gain=0.0)
    assert abs(np.abs(flat[-400:, 0]).max() / np.abs(flat[:400, 0]).max() - 1.0) < 1e-3
    # and frames from `last` on get nothing
    cut, info = ir_plate_np.frames64(dict(plate, last=1000), RATE, frames=F, late_gain=0.0)
    assert info["last"] == 1000 and not cut[1000:].any() and np.array_equal(cut[:1000], y[:1000])
