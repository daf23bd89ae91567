"""Walls and air per frequency band in the room (mc_synth_ir_room_bands) without a GPU: the restatement
(tests/ir_room_bands_np.py) against the algebraically equal other form of its join, the exact statement the bit-identity tests on
the device rely on (equal bands are the unbanded room), what the feature is for (the decay of a band follows its walls and its
air), and the reverberation times of mc_ir_room_bands_plan."""
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_room_bands_np
import ir_room_np

RATE = 48000
F3 = 12000
XOVERS3 = (500.0, 2000.0)
WALLS = dict(xovers=XOVERS3, beta=(0.95, 0.85, 0.6))
# air alone: 0.1 dB/m more per band is 4.3 dB more over the 42.9 m sound travels between the centres of the two windows
AIR = dict(xovers=XOVERS3, beta=0.9, air=(0.0, 0.1, 0.2))
EARLY, LATE = slice(2000, 5000), slice(8000, 11000)


@functools.lru_cache(maxsize=None)
def _accs(name):
    accs, _, info = ir_room_bands_np.accumulators({}, None, dict(WALLS=WALLS, AIR=AIR)[name], RATE, F3)
    for a in accs:
        a.setflags(write=False)
    return accs, info


def _drops(r):
    """The energy drop in dB from EARLY to LATE in each band of r under the split at XOVERS3."""
    parts = ir_damp_np.bands(r, ir_damp_np.lowpasses(r, XOVERS3, RATE))
    e = lambda a: float((a * a).sum())
    return [10.0 * np.log10(e(p[EARLY]) / e(p[LATE])) for p in parts]


def test_the_difference_form_is_the_sum_over_the_bands():
    """r written by the differences of neighbouring accumulators against sum_j B_j(acc_j): equal algebraically, different in
    every rounding, so the restatement is checked against something other than itself."""
    accs, _ = _accs("WALLS")
    r = ir_room_bands_np.join(accs, XOVERS3, RATE)
    other = ir_room_bands_np.by_bands(accs, XOVERS3, RATE)
    err = float(np.abs(r - other).max() / np.abs(r).max())
    print("difference form against the sum over bands:", err)
    assert err <= 1e-12
    assert not np.array_equal(accs[0], accs[1]) and not np.array_equal(accs[1], accs[2])


@pytest.mark.parametrize("xovers", [(), (700.0,), (200.0, 1000.0, 5000.0)])
@pytest.mark.parametrize("mics", [None, dict(pattern=(0.5, 0.25), az=(30.0, -100.0), source_pattern=0.366, source_az=200.0)])
def test_equal_bands_are_the_unbanded_room_exactly(xovers, mics):
    import ir_room_mics_np

    room = dict(order=2, beta=(0.9, 0.8, -0.7, 0.95, 0.6, 0.85))
    synth = dict(frames=3000, seed=5, late_start=100, t60=2000, late_gain=0.02, direct=1.0)
    bands = dict(xovers=xovers, beta=(room["beta"],) * (len(xovers) + 1))
    got, cov, info = ir_room_bands_np.frames64(room, mics, bands, RATE, **synth)
    want, wcov, winfo = ir_room_np.frames64(room, RATE, **synth) if mics is None else ir_room_mics_np.frames64(room, mics, RATE, **synth)
    assert got.tobytes() == want.tobytes()
    np.testing.assert_array_equal(cov, wcov)
    assert info["images"] == winfo["images"] and info["order"] == winfo["order"]


def test_the_decay_of_a_band_follows_its_walls():
    """The default room, beta 0.95, 0.85 and 0.6 below 500 Hz, up to 2 kHz and above: the flat renderings drop 1.4, 16 and 53 dB
    between the two windows, the bands of the joined result -1.6, 5.2 and 14.2 dB: the skirts of the split blur it, and it stays
    well separated."""
    accs, _ = _accs("WALLS")
    flat = [_drops(a.astype(np.float64) / ir_room_np.Q) for a in accs]
    drops = _drops(ir_room_bands_np.join(accs, XOVERS3, RATE))
    print("drops of the result's bands:", drops, "of the flat renderings, broadband:",
          [10.0 * np.log10(float((a[EARLY].astype(np.float64) ** 2).sum()) / float((a[LATE].astype(np.float64) ** 2).sum())) for a in accs], flat)
    assert drops[1] - drops[0] >= 3.0 and drops[2] - drops[1] >= 3.0


def test_the_decay_of_a_band_follows_its_air():
    """Equal walls, the air's loss rising with the band by 0.1 dB/m each: flat renderings would differ by 4.3 dB per band between
    the windows.  The walls' case keeps under half of its flat differences through the skirts; 1.5 dB is about a third here."""
    accs, _ = _accs("AIR")
    drops = _drops(ir_room_bands_np.join(accs, XOVERS3, RATE))
    print("drops with air alone:", drops)
    assert drops[1] - drops[0] >= 1.5 and drops[2] - drops[1] >= 1.5


def test_the_air_factor_in_its_place():
    """Beta 0: the direct sound alone, at d metres; a band with a dB/m stores it a d dB lower, to the quantum."""
    room = dict(size=(8.0, 6.0, 3.0), source=(6.0, 3.0, 1.5), receiver=(2.0, 3.0, 1.5), spacing=0.0, order=1)
    plain, _, _ = ir_room_bands_np.render_band(room, None, (0.0,) * 6, 0.0, RATE, 1000)
    want, _, _ = ir_room_np.render(dict(room, beta=0.0), RATE, 1000)
    np.testing.assert_array_equal(plain, want)  # (no air: ir_room_np's rendering to the integer)
    aired, _, _ = ir_room_bands_np.render_band(room, None, (0.0,) * 6, 0.5, RATE, 1000)
    factor = 10.0 ** (-0.5 * 4.0 / 20.0)  # 4 m at 0.5 dB/m
    assert np.count_nonzero(plain[:, 0]) == 32 and np.abs(aired - factor * plain).max() <= 1 + 1e-15 * ir_room_np.Q


PLAN_CASES = [({}, dict(xovers=(), beta=0.9, air=0.0)), ({}, WALLS), ({}, AIR),
              (dict(size=(7.0, 5.0, 2.5), speed=340.0), dict(xovers=(250.0, 1000.0, 4000.0), beta=((0.9, 0.8, 0.7, 0.95, 0.6, -0.5), 0.8, (1.0,) * 6, 0.0),
                                                             air=(0.0, 0.001, 0.0, 1.0))),
              (dict(beta=0.5), dict(xovers=(1000.0,), beta=(1.0, 1.0), air=(0.0, 0.01)))]


@pytest.mark.parametrize("room,bands", PLAN_CASES)
def test_the_plan_matches_the_restatement(room, bands):
    """A time is a dozen double roundings of positive terms: 1e-14 relative."""
    from cuda_audio_amd.engine import IrRoom, IrRoomBands, room_bands_plan

    got = room_bands_plan(IrRoom(**room), IrRoomBands(**bands), RATE, 4000)
    want = ir_room_bands_np.plan(room, bands, RATE, 4000)
    print(got, want)
    assert got["bands"] == want["bands"] == len(bands["xovers"]) + 1 and got["xovers"] == want["xovers"]
    for k in ("sabine", "eyring"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-14, atol=0)


def test_without_air_the_times_are_the_rooms():
    """Sabine and Eyring with air reduce to ir_room_np.plan's at air 0, band by band; nothing absorbing gives 0, and air alone
    a finite time."""
    from cuda_audio_amd.engine import IrRoom, IrRoomBands, room_bands_plan, room_plan

    rows = ((0.9, 0.8, 0.7, 0.95, 0.6, -0.5), (0.5,) * 6, (1.0,) * 6)
    bands = dict(xovers=(300.0, 3000.0), beta=rows)
    want = ir_room_bands_np.plan({}, bands, RATE, 4000)
    got = room_bands_plan(IrRoom(), IrRoomBands(**bands), RATE, 4000)
    for j, row in enumerate(rows):
        flat = ir_room_np.plan(dict(beta=row), RATE, 4000)
        lib = room_plan(IrRoom(beta=row), RATE, 4000)
        assert want["sabine"][j] == flat["sabine"] and want["eyring"][j] == flat["eyring"]
        np.testing.assert_allclose((got["sabine"][j], got["eyring"][j]), (lib["sabine"], lib["eyring"]), rtol=1e-14, atol=0)
    assert got["sabine"][2] == got["eyring"][2] == 0.0
    aired = room_bands_plan(IrRoom(), IrRoomBands(xovers=(300.0,), beta=1.0, air=(0.0, 0.01)), RATE, 4000)
    assert aired["sabine"][0] == 0.0 and aired["sabine"][1] == aired["eyring"][1] > 0.0
    # 24 ln 10 / c * V / (4 m V) = 60 dB / (c * 0.01 dB/m): 6000 m of travel
    np.testing.assert_allclose(aired["sabine"][1], 60.0 / (343.0 * float(np.float32(0.01))), rtol=1e-12)


def test_the_shapes_bands_take():
    from cuda_audio_amd.engine import IrRoomBands

    b = IrRoomBands(xovers=(500, 2000), beta=(0.95, (0.9, 0.8, 0.7, 0.6, 0.5, 0.4), 0.6), air=0.01).to_c()
    assert b.n_xovers == 2 and list(b.xover_hz) == [500.0, 2000.0, 0.0]
    f = lambda v: float(np.float32(v))
    assert [list(r) for r in b.beta][:3] == [[f(0.95)] * 6, [f(v) for v in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4)], [f(0.6)] * 6]
    assert list(b.air_db_per_m) == [f(0.01)] * 3 + [0.0]
    a = IrRoomBands.from_absorption((1000,), (0.19, (0.36,) * 6), air=(0.0, 0.02)).to_c()
    np.testing.assert_allclose([a.beta[0][0], a.beta[1][5]], [0.9, 0.8], rtol=1e-7)
    assert list(a.air_db_per_m)[:2] == [0.0, f(0.02)]
    for bad in (dict(xovers=(1, 2, 3, 4)), dict(xovers=(500,), beta=(0.9, 0.8, 0.7)), dict(xovers=(500,), air=(0.1,)), dict(beta=((0.9,) * 5,))):
        with pytest.raises(ValueError):
            IrRoomBands(**bad).to_c()
    with pytest.raises(ValueError):
        IrRoomBands.from_absorption((), 1.5)


def test_bands_without_a_room_raise():
    from cuda_audio_amd.engine import Convolution, IrRoomBands, IrSynth

    with pytest.raises(ValueError) as ex:  # (before the engine is looked at: no engine is needed to see it)
        Convolution.prepare_synth(None, 0, IrSynth(frames=100, rate=RATE), bands=IrRoomBands())
    assert "need a room" in str(ex.value)
