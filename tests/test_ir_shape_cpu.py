"""IR shaping on load, the part that needs no GPU: the layout and defaults of mc_ir_shape, every refused field (checked before
the engine is looked at, so a null engine will do), and properties of the float64 restatement (tests/ir_shape_np.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from cuda_audio_amd import _lib
from ir_shape_np import assert_onset_margin, onset_margin, onset_of, quiet_lead_ir, session_frames, shape, shape64


def _default():
    s = _lib.McIrShape()
    _lib.load().mc_default_ir_shape(C.byref(s))
    return s


def test_struct_layout_and_defaults():
    assert C.sizeof(_lib.McIrShape) == 56
    # no implicit padding: the fields' sizes add up to the struct's
    assert sum(C.sizeof(t) for _, t in _lib.McIrShape._fields_) == 56
    s = _default()
    assert s.struct_size == 56
    assert (s.flags, s.start, s.length, s.decay_t60, s.fade_out, s.pre_roll, s.normalize) == (0, 0, 0, 0, 0, 0, _lib.MC_NORM_NONE)
    assert s.trim_db == 0.0 and s.target == 1.0
    for name in ("mc_default_ir_shape", "mc_load_ir_shaped", "mc_ir_shape_info"):
        assert name in _lib.SYMBOLS


def _refused(rates=(0, 0), **fields):
    L = _lib.load()
    s = _default()
    for k, v in fields.items():
        setattr(s, k, v)
    rc = L.mc_load_ir_shaped(None, 0, None, 100, 1024, rates[0], rates[1], C.byref(s))
    return rc, L.mc_last_error().decode()


@pytest.mark.parametrize("fields,named", [
    (dict(trim_db=1.0), "trim_db"),
    (dict(trim_db=-121.0), "trim_db"),
    (dict(trim_db=math.nan), "trim_db"),
    (dict(flags=2), "flags"),
    (dict(flags=0x80000001), "flags"),
    (dict(normalize=3), "normalize"),
    (dict(normalize=_lib.MC_NORM_PEAK, target=0.0), "target"),
    (dict(normalize=_lib.MC_NORM_ENERGY, target=-1.0), "target"),
    (dict(normalize=_lib.MC_NORM_PEAK, target=math.inf), "target"),
    (dict(struct_size=52), "struct_size"),
])
def test_bad_fields_are_refused_before_the_engine_is_looked_at(fields, named):
    rc, msg = _refused(**fields)
    assert rc == -1 and named in msg, msg


@pytest.mark.parametrize("rates,named", [
    ((0, 48000), "ir_rate"), ((44100, 0), "session_rate"), ((7999, 48000), "ir_rate"), ((384001, 48000), "ir_rate"),
    ((44100, 7999), "session_rate"), ((44100, 384001), "session_rate"),
])
def test_bad_rates_are_refused_before_the_engine_is_looked_at(rates, named):
    rc, msg = _refused(rates, fade_out=10)
    assert rc == -1 and named in msg, msg


def test_a_good_shape_reaches_the_pointer_checks():
    """The shape and the rates first, the pointers after them: with everything valid the null engine is what is refused."""
    for rates in ((0, 0), (44100, 48000), (48000, 48000)):
        for fields in (dict(), dict(fade_out=10), dict(trim_db=-120.0, normalize=_lib.MC_NORM_ENERGY, target=0.25, flags=_lib.MC_SHAPE_REVERSE)):
            rc, msg = _refused(rates, **fields)
            assert rc == -1 and "null" in msg, msg
    # a target is not looked at while no normalisation is on
    rc, msg = _refused(target=-1.0, fade_out=3)
    assert rc == -1 and "null" in msg, msg
    assert _lib.load().mc_ir_shape_info(None, 0, (C.c_double * 8)()) == -1


def test_python_shape_maps_onto_the_struct():
    from cuda_audio_amd.engine import IrShape

    s = IrShape(start=3, trim_db=-20, pre_roll=16, length=99, reverse=True, decay_t60=6000, fade_out=512, normalize="energy", target=0.25).to_c()
    assert (s.struct_size, s.flags, s.start, s.pre_roll, s.length, s.decay_t60, s.fade_out) == (56, 1, 3, 16, 99, 6000, 512)
    assert (s.trim_db, s.normalize, s.target) == (-20.0, _lib.MC_NORM_ENERGY, 0.25)
    d = IrShape().to_c()
    assert bytes(d) == bytes(_default())
    assert IrShape(normalize="peak").to_c().normalize == _lib.MC_NORM_PEAK
    with pytest.raises(ValueError):
        IrShape(normalize="loud").to_c()


# -- the restatement itself -------------------------------------------------------------------------------------------
def test_everything_off_returns_the_input():
    ir = quiet_lead_ir(3000)
    taps, info = shape(ir, 1 << 20)
    np.testing.assert_array_equal(taps, ir)
    assert info == dict(frames=3700, onset=0, first=0, taps=3700, gain=1.0, peak=float(np.abs(ir).max()),
                        energy=float(np.sqrt((ir.astype(np.float64) ** 2).sum() / 2)))
    np.testing.assert_array_equal(shape(ir, 1000)[0], ir[:1000])


def test_reversing_twice_is_the_identity():
    ir = quiet_lead_ir(3000)
    once, _ = shape(ir, 1 << 20, reverse=True)
    np.testing.assert_array_equal(once, ir[::-1])
    np.testing.assert_array_equal(shape(once, 1 << 20, reverse=True)[0], ir)


@pytest.mark.parametrize("rates", [(None, None), (44100, 48000)])
def test_energy_and_peak_reach_the_target(rates):
    ir = quiet_lead_ir(3000)
    v, info = shape64(ir, 1 << 20, *rates, trim_db=-20, decay_t60=2000, fade_out=300, normalize="energy", target=0.25)
    assert abs(np.sqrt((v * v).sum() / 2) / 0.25 - 1) <= 1e-12
    assert abs(info["gain"] * info["energy"] / 0.25 - 1) <= 1e-12
    v, info = shape64(ir, 1 << 20, *rates, normalize="peak", target=0.02)
    assert abs(np.abs(v).max() / float(np.float32(0.02)) - 1) <= 1e-12


def test_order_of_operations():
    """The cut comes before the fade and the normalisation; the decay and the fade act on tap positions after the reverse."""
    ir = quiet_lead_ir(3000)
    cap = 2000
    v, info = shape64(ir, cap, start=100, length=5000, fade_out=64, normalize="peak", target=0.02)
    assert info["taps"] == cap and info["first"] == 100 and info["frames"] == 3700
    k = np.arange(64)
    fade = 0.5 * (1 + np.cos(np.pi * (k + 1) / 65))
    want = ir[100:100 + cap].astype(np.float64)
    want[-64:] *= fade[:, None]
    np.testing.assert_allclose(v, want * 0.02 / np.abs(want).max(), rtol=1e-7)  # (the target is float32(0.02))
    # decay: 60 dB down at tap decay_t60, on the reversed sequence
    d, _ = shape64(ir, 1 << 20, reverse=True, decay_t60=1000)
    np.testing.assert_allclose(d[1000], ir[::-1][1000].astype(np.float64) * 1e-3, rtol=1e-12)
    np.testing.assert_array_equal(d[0], ir[-1].astype(np.float64))
    # pre-roll reaches back from the onset but never before `start`
    assert shape(ir, 1 << 20, trim_db=-20, pre_roll=16)[1]["first"] == 700 - 16
    assert shape(ir, 1 << 20, start=690, trim_db=-20, pre_roll=16)[1]["first"] == 690
    with pytest.raises(ValueError):
        shape(ir, 1 << 20, start=3700)
    # a fade longer than what is stored is clamped to it
    f, _ = shape64(ir, 10, fade_out=1000)
    np.testing.assert_allclose(f, ir[:10].astype(np.float64) * (0.5 * (1 + np.cos(np.pi * (np.arange(10) + 1) / 11)))[:, None], rtol=1e-15)


TRIMS = [(44100, 44100, -16, 700), (44100, 44100, -20, 700), (44100, 44100, -40, 700), (44100, 44100, -60, 0),
         (44100, 48000, -16, 762), (44100, 48000, -20, 762), (96000, 44100, -16, 322), (96000, 44100, -20, 322)]


@pytest.mark.parametrize("src,dst,trim_db,onset", TRIMS)
def test_onset_margins_of_the_gpu_tests(src, dst, trim_db, onset):
    """Every trimming case the GPU and the host tests use keeps the largest frame before the onset at most 0.8 x the threshold and
    the onset frame at least 1.25 x the threshold, so the device's float32 frames cannot move the onset."""
    xs = session_frames(quiet_lead_ir(), src, dst)
    assert_onset_margin(xs, 0, trim_db)
    assert onset_of(xs, 0, trim_db)[1] == onset


@pytest.mark.parametrize("frames,seed,norm,src,dst,trim_db,onset", [
    (7000, 11, 0.05, 44100, 48000, -20, 763), (9000, 22, 0.05, 48000, 48000, 0, 0),  # the pair every engine path plays
    (36000, 4, 0.05, 44100, 44100, -16, 700), (36000, 4, 0.05, 44100, 48000, -16, 762),  # truncation
    (125000, 10, 0.02, 44100, 48000, -20, 762),  # the shipped tail-drop regime
])
def test_onset_margins_of_the_other_gpu_irs(frames, seed, norm, src, dst, trim_db, onset):
    xs = session_frames(quiet_lead_ir(frames, seed=seed, norm=norm), src, dst)
    if trim_db:
        assert_onset_margin(xs, 0, trim_db)
    assert onset_of(xs, 0, trim_db)[1] == onset


def test_minus_40_db_fails_the_margin_after_conversion():
    """Why the converted cases do not use -40 dB: the band-limited pre-ringing climbs to within rounding of that threshold."""
    for src, dst in ((44100, 48000), (96000, 44100)):
        below, above = onset_margin(session_frames(quiet_lead_ir(), src, dst), 0, -40)
        assert below > 0.8 or above < 1.25


def test_all_zero_ir_has_onset_zero():
    z = np.zeros((50, 2), np.float32)
    taps, info = shape(z, 100, trim_db=-20, normalize="energy", target=0.5)
    assert info["onset"] == 0 and info["gain"] == 1.0 and info["taps"] == 50
    np.testing.assert_array_equal(taps, z)
