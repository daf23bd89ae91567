"""A plate reverberator's IR on the device (mc_synth_ir_plate, csrc/irplate.hip.h): the stored taps, the information, the sums
and the spectra against the float64 restatement (tests/ir_plate_np.py), the edges of the kernel's tiling in modes and in frames,
one mode against its closed form, the bits (two loads, two lengths, two orders of loading), a long phase against the restatement
in extended precision, a pickup on a nodal line, the synthesis' own terms under the plate, the chain into ir_decay and the tail
step, the engine's paths against the oracle fed the restated taps, and the refusals.

The bar for taps is test_gpu_ir_shape._check_taps (1e-6 relative RMS, 1e-5 of the peak): a contribution differs from numpy's by a
few ulp of a double (exp, sincospi, the turns of the recurrence), hence by at most a quantum of 2^-40 before the one rounding to
float32, which is the situation that bar was set for."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_plate_np
import ir_synth_np
from helpers import RMS_TOL, apply_params, rms
from test_gpu_ir_eq import _check_sums_and_spectra
from test_gpu_ir_shape import P0, P1, _check_level, _check_taps

pytestmark = pytest.mark.gpu

RATE = 48000
ALONE = dict(late_gain=0.0, direct=0.0)  # the synthesis' own terms off: the plate alone
CUT = dict(high_hz=400.0)                # the default plate cut at 400 Hz: 472 modes, two slabs
SMALL = dict(size=(0.3, 0.2), thickness_mm=3.0, driver=(0.11, 0.07), pickups=((0.07, 0.13), (0.21, 0.06)))  # (1, 1) near 260 Hz
SLAB = ir_plate_np.SLAB                  # MC_PLATE_SLAB: the rows a workgroup stages at a time
TILE = 256 * ir_plate_np.GROUP           # the frames of a workgroup: 256 lanes of one group of MC_PLATE_GROUP frames each


def _conv(n_ref=16384, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irplate", n_ref, sample_rate=rate, **kw)


def _iplate(fields):
    from cuda_audio_amd.engine import IrPlate

    return IrPlate(**fields)


def _isynth(fields):
    from cuda_audio_amd.engine import IrSynth

    return IrSynth(**fields)


def _freeze(v):
    return tuple(sorted((k, _freeze(x)) for k, x in v.items())) if isinstance(v, dict) else v


@functools.lru_cache(maxsize=None)
def _restated_cached(plate, synth):
    out, info = ir_plate_np.frames64(dict(plate), RATE, **dict(synth))
    out.setflags(write=False)
    return out, info


def _restated(plate, synth):
    """(frames float64 [F, 2], info) of a plate over a synthesis, computed once."""
    return _restated_cached(_freeze(plate), _freeze(synth))


def _check_info(info, winfo):
    print("plate info:", info, "restated:", winfo)
    assert info["modes"] == winfo["modes"] and info["sounding"] == winfo["sounding"] and info["last"] == winfo["last"]
    for k in ("lowest", "highest", "kappa"):
        assert info[k] == pytest.approx(winfo[k], rel=1e-12), k


def _load_and_check(c, idx, plate, synth, **kw):
    """Load, then the taps and the plate's information against the restatement."""
    want, winfo = _restated(plate, synth)
    c.prepare_synth(idx, _isynth(synth), plate=_iplate(plate), **kw)
    got = c.ir_taps(idx)
    assert len(got) == len(want)
    if np.abs(want).max() > 0:
        _check_taps(got, want)
    else:
        np.testing.assert_array_equal(got, want.astype(np.float32))
    _check_info(c.ir_plate_info(idx), winfo)
    return got, want, winfo


def test_the_plate_alone_matches_the_restatement(gpu_lib):
    F = 4000
    c = _conv()
    got, want, winfo = _load_and_check(c, 0, CUT, dict(ALONE, frames=F))
    assert winfo["modes"] == 472 and winfo["sounding"] == (472, 472) and winfo["last"] == F
    sinfo = c.ir_shape_info(0)
    assert (sinfo["frames"], sinfo["onset"], sinfo["first"], sinfo["taps"], sinfo["gain"], sinfo["eq_bands"]) == (F, 0, 0, F, 1.0, 0)
    assert abs(sinfo["peak"] - np.abs(want).max()) <= 1e-6 * np.abs(want).max()
    assert c.ir_synth_info(0) == dict(frames=F, reflections=0, late_start=0)
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    c.close()
    # dense from the first millisecond: no silent frame, and the first 50 ms have the level of gain within 1 dB (as
    # tests/test_ir_plate_cpu.py asserts of the restatement)
    assert np.count_nonzero(got) == got.size
    assert all(abs(20.0 * np.log10(rms(got[:2400, ch]))) < 1.0 for ch in range(2))


@pytest.mark.parametrize("count", [1, 2, SLAB - 1, SLAB + 1])
def test_mode_counts_at_the_edges_of_a_slab(gpu_lib, count):
    lo, hi = ir_plate_np.bracket({}, RATE, count)
    from cuda_audio_amd import _lib

    plate = dict(low_hz=lo, high_hz=hi)
    assert ir_plate_np.modes(plate, RATE)["M"] == count and SLAB == _lib.MC_PLATE_SLAB == 256  # (tests/test_abi_plate.py ties it to the header)
    c = _conv()
    _, _, winfo = _load_and_check(c, 0, plate, dict(ALONE, frames=600))
    c.close()
    assert winfo["modes"] == count


def test_a_thousand_modes(gpu_lib):
    plate = dict(high_hz=800.0)
    M = ir_plate_np.modes(plate, RATE)["M"]
    assert 900 < M < 1100 and M % SLAB  # (four slabs, the last one partly filled)
    c = _conv()
    _load_and_check(c, 0, plate, dict(ALONE, frames=1500))
    c.close()


@pytest.mark.parametrize("F", [1, 7, TILE - 1, TILE + 1, 4097])
def test_lengths(gpu_lib, F):
    """A lone frame, part of one group, a workgroup's frames less one and plus one (a second workgroup with one live lane), and a
    length that ends a frame into a group."""
    from cuda_audio_amd import _lib

    assert TILE == 256 * _lib.MC_PLATE_GROUP == 8192
    c = _conv()
    got, want, _ = _load_and_check(c, 0, CUT, dict(ALONE, frames=F))
    assert len(got) == F and c.ir_shape_info(0)["frames"] == F
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    c.close()


@pytest.mark.parametrize("F,last", [(3000, 1000), (3000, 1), (700, 5000), (8300, 8191)])
def test_frames_from_last_on_are_exactly_zero(gpu_lib, F, last):
    c = _conv()
    got, _, winfo = _load_and_check(c, 0, dict(CUT, last=last), dict(ALONE, frames=F))
    E = min(last, F)
    assert winfo["last"] == E and not got[E:].any() and got[:E].all()
    # and the frames before it are those of the load without `last`, bit for bit
    c.prepare_synth(1, _isynth(dict(ALONE, frames=F)), plate=_iplate(CUT))
    np.testing.assert_array_equal(c.ir_taps(1)[:E], got[:E])
    c.close()


def test_one_mode_is_its_closed_form(gpu_lib):
    F = 3000
    plate = dict(SMALL, low_hz=200.0, high_hz=300.0, t60=(0.5, 0.5), gain=0.7)
    tb = ir_plate_np.modes(plate, RATE)
    assert tb["M"] == 1 and (int(tb["m"][0]), int(tb["n"][0])) == (1, 1) and 255.0 < tb["f"][0] < 265.0
    t = np.arange(F, dtype=np.float64)
    c = _conv()
    got, _, _ = _load_and_check(c, 0, plate, dict(ALONE, frames=F))
    want = tb["a"][0][None, :] * (np.exp(-tb["sigma"][0] * t / RATE) * np.cos(2.0 * np.pi * tb["f"][0] * t / RATE))[:, None]
    _check_taps(got, want)
    # without loss the envelope is flat
    flat, _, _ = _load_and_check(c, 1, dict(plate, t60=(0.0, 0.0)), dict(ALONE, frames=F))
    c.close()
    want = tb["a"][0][None, :] * np.cos(2.0 * np.pi * tb["f"][0] * t / RATE)[:, None]
    _check_taps(flat, want)
    assert abs(np.abs(flat[-400:, 0]).max() / np.abs(flat[:400, 0]).max() - 1.0) < 1e-3


def test_the_same_struct_stores_the_same_bits(gpu_lib):
    """Twice into one engine; frame t whatever F; and the slots of one engine loaded in another order."""
    plates = [CUT, dict(high_hz=800.0), dict(SMALL, low_hz=200.0, high_hz=2000.0)]
    c = _conv()
    a, _, _ = _load_and_check(c, 0, CUT, dict(ALONE, frames=4096))
    b, _, _ = _load_and_check(c, 1, CUT, dict(ALONE, frames=4096))
    assert a.tobytes() == b.tobytes() and c.ir_spectra(0).tobytes() == c.ir_spectra(1).tobytes()
    assert c.ir_info(0) == c.ir_info(1) and c.ir_plate_info(0) == c.ir_plate_info(1)
    short, _, _ = _load_and_check(c, 2, CUT, dict(ALONE, frames=1000))
    assert short.tobytes() == a[:1000].tobytes()
    for idx, p in enumerate(plates):
        c.prepare_synth(idx, _isynth(dict(ALONE, frames=2000 + idx)), plate=_iplate(p))
    first = [c.ir_taps(idx).tobytes() for idx in range(3)]
    c.close()
    c = _conv()
    for idx in (2, 0, 1):
        c.prepare_synth(idx, _isynth(dict(ALONE, frames=2000 + idx)), plate=_iplate(plates[idx]))
    assert [c.ir_taps(idx).tobytes() for idx in range(3)] == first
    c.close()


def test_a_long_phase(gpu_lib):
    """Eight undamped modes over 2^20 frames, of which the shape keeps the last 8192, against the restatement, whose phase is
    np.longdouble's.  nu t is some 2^14 turns there: a phase kept in float, a recurrence that is never seeded again and loses or
    gains level, or an envelope that is not flat shows.  (What float32 taps cannot show is the last few quanta of 2^-40.)"""
    from cuda_audio_amd.engine import IrShape

    F, keep = 1 << 20, 8192
    lo, hi = ir_plate_np.bracket(dict(low_hz=900.0), RATE, 8)
    plate = dict(low_hz=lo, high_hz=hi, t60=(0.0, 0.0))
    tb = ir_plate_np.modes(plate, RATE)
    assert tb["M"] == 8 and (tb["sigma"] == 0).all() and np.finfo(np.longdouble).nmant >= 63
    want = ir_plate_np.sums(plate, RATE, np.arange(F - keep, F)).astype(np.float64) / ir_plate_np.Q
    c = _conv()
    c.prepare_synth(0, _isynth(dict(ALONE, frames=F)), plate=_iplate(plate), shape=IrShape(start=F - keep))
    got = c.ir_taps(0)
    info, sinfo = c.ir_plate_info(0), c.ir_shape_info(0)
    c.close()
    assert (info["modes"], info["last"]) == (8, F) and sinfo["frames"] == F and sinfo["taps"] == keep
    _check_taps(got, want)
    # undamped: as loud at the end as a plate of this level is at the start
    assert 0.3 < rms(got) < 3.0


@pytest.mark.parametrize("x", [0.15, 0.1500002])
def test_a_pickup_on_a_nodal_line(gpu_lib, x):
    """(2, 1) alone, the left pickup at Lx / 2 or a fifth of a micrometre beside it.  In double the sine of 2 pi x / Lx is small
    there and not zero, so the mode counts as sounding in both channels.  At 0.15f over 0.3f the amplitude is 4e-16: every
    contribution is under half a quantum and rounds to 0, which the restatement says too (that, not silence, is what is asserted);
    beside the line the left channel is faint and the quanta show."""
    plate = dict(SMALL, low_hz=450.0, high_hz=550.0, pickups=((x, 0.13), (0.21, 0.06)), t60=(0.3, 0.3))
    tb = ir_plate_np.modes(plate, RATE)
    assert tb["M"] == 1 and (int(tb["m"][0]), int(tb["n"][0])) == (2, 1)
    assert 0.0 < abs(tb["a"][0, 0]) < 1e-5 * abs(tb["a"][0, 1])
    c = _conv()
    got, want, winfo = _load_and_check(c, 0, plate, dict(ALONE, frames=2000))
    c.close()
    assert winfo["sounding"] == (1, 1)
    # the faint channel on its own: within a quantum and the rounding to float32
    assert np.abs(got[:, 0].astype(np.float64) - want[:, 0]).max() <= 2.0 ** -40 + 1e-7 * np.abs(want[:, 0]).max()
    if x == 0.15:
        assert abs(tb["a"][0, 0]) * ir_plate_np.Q < 0.5 and not want[:, 0].any()
        np.testing.assert_array_equal(got[:, 0], want[:, 0].astype(np.float32))
    else:
        assert np.abs(want[:, 0]).max() > 1000 * 2.0 ** -40 and np.count_nonzero(got[:, 0]) > 1000


FULL = dict(frames=5000, seed=(0x1234 << 32) | 7, late_start=1500, t60=20000, build_up=2000, late_gain=0.05, direct=1.0, n_early=12, early_first=100,
            early_last=1400, early_gain=0.5, width=0.7)


def test_plate_late_field_direct_and_reflections_round_once(gpu_lib):
    c = _conv()
    got, want, _ = _load_and_check(c, 0, dict(CUT, last=3000, gain=0.3), FULL)
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    assert c.ir_synth_info(0) == dict(frames=5000, reflections=12, late_start=1500)
    # the restatement is ir_synth_np's three terms and the plate's in double, then one cast
    acc, _ = ir_plate_np.render(dict(CUT, last=3000, gain=0.3), RATE, 5000)
    np.testing.assert_array_equal(want, ir_synth_np.frames64(**FULL) + acc.astype(np.float64) / ir_plate_np.Q)
    # the plate is a fourth term: without it the frames are mc_synth_ir's
    c.prepare_synth(1, _isynth(FULL))
    plain = c.ir_taps(1)
    c.close()
    assert not np.array_equal(got[:3000], plain[:3000])
    np.testing.assert_array_equal(got[3000:], plain[3000:])  # (from E on the plate adds nothing)


def test_without_a_plate_the_call_is_mc_synth_ir_room_without_a_room(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, IrTail

    shape, eq, damp = IrShape(fade_out=100, normalize="peak", target=0.05), IrEq(bands=[("lowcut", 120)]), IrDamp(xovers=(400, 1600), decay=(0, 4800, 1600), origin=37)
    tail = IrTail(mode="cut", knee=(3000,), fade=64)
    c = _conv()
    L = c._L
    s, sh, q, d, t = _isynth(dict(FULL, rate=RATE)).to_c(), shape.to_c(), eq.to_c(), damp.to_c(), tail.to_c()
    assert L.mc_synth_ir_room(c._h, 0, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), None) == 0
    assert L.mc_synth_ir_plate(c._h, 1, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), None) == 0
    assert L.mc_synth_ir_room(c._h, 2, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), C.byref(t)) == 0
    assert L.mc_synth_ir_plate(c._h, 3, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), C.byref(t)) == 0
    c.prepare_synth(4, _isynth(FULL), shape=shape, eq=eq, damp=damp, plate=None)
    for a, b in ((0, 1), (2, 3), (0, 4)):
        assert c.ir_taps(a).tobytes() == c.ir_taps(b).tobytes() and c.ir_spectra(a).tobytes() == c.ir_spectra(b).tobytes()
        assert c.ir_info(a) == c.ir_info(b) and c.ir_shape_info(a) == c.ir_shape_info(b) and c.ir_synth_info(a) == c.ir_synth_info(b)
    assert c.ir_taps(0).tobytes() != c.ir_taps(2).tobytes() and c.ir_tail_info(3) == c.ir_tail_info(2)
    for idx in range(5):
        with pytest.raises(McError) as ex:
            c.ir_plate_info(idx)
        assert ex.value.code == -3
    c.close()


CHAIN = dict(high_hz=4000.0, t60=(0.2, 0.05), damp_hz=4000.0, gain=0.2)  # T60 0.145 s at 500 Hz, 0.080 s at 2 kHz
CHAIN_F = 8000


def test_the_chain_into_the_decay_measurement_and_the_tail_step(gpu_lib):
    """plate -> ir_decay: T30 falls from the octave at 500 Hz to the one at 2 kHz, each inside the decay times of its band's edges
    (tests/test_ir_plate_cpu.py has the reasoning); plate -> tail=cut: the tail step runs on the plate's frames."""
    import math

    import ir_tail_np
    from cuda_audio_amd.engine import IrTail

    c = _conv()
    got, want, winfo = _load_and_check(c, 0, CHAIN, dict(ALONE, frames=CHAIN_F))
    assert winfo["modes"] > 4000
    res = c.ir_decay(0, bands=(500.0, 2000.0), onset_db=0.0)
    s0, s1 = ir_plate_np.loss(0.2), ir_plate_np.loss(0.05)
    t60_at = lambda hz: 3.0 * math.log(10.0) / (s0 + (s1 - s0) * hz / 4000.0)  # noqa: E731
    t30 = [res["rows"][(b, "LR")]["t30"] for b in (1, 2)]
    print("T30:", t30, [t60_at(500.0), t60_at(2000.0)])
    for hz, t in zip((500.0, 2000.0), t30):
        assert t60_at(hz * math.sqrt(2.0)) < t < t60_at(hz / math.sqrt(2.0))
    assert t30[1] < t30[0]
    spec = dict(xovers=(1000,), knee=(3000, 2500), fade=64)
    c.prepare_synth(1, _isynth(dict(ALONE, frames=CHAIN_F)), plate=_iplate(CHAIN), tail=IrTail(mode="cut", **spec))
    cut = c.ir_taps(1)
    y, tinfo = ir_tail_np.tail64(want.astype(np.float32), RATE, "cut", **spec)
    _check_taps(cut, y)
    assert c.ir_tail_info(1) == tinfo and c.ir_plate_info(1) == c.ir_plate_info(0) and not cut[3000:].any()
    np.testing.assert_array_equal(cut[:tinfo["first"]], got[:tinfo["first"]])
    c.close()


# -- the engine plays a plate --------------------------------------------------------------------------------------------------
PLAY_PLATE = dict(high_hz=1500.0, t60=(0.5, 0.1), damp_hz=1500.0, gain=0.01)
PLAY_SYNTH = dict(ALONE, frames=7000)
PLAY_OTHER = dict(frames=5000, seed=3, late_start=0, t60=4000, late_gain=0.01, width=1.0)


def _play_taps(n_ref):
    a = _restated(PLAY_PLATE, PLAY_SYNTH)[0].astype(np.float32)[:n_ref - 1024]
    return [a, ir_synth_np.frames(**PLAY_OTHER)[:n_ref - 1024]]


def _prepare_play(c):
    c.prepare_synth(0, _isynth(PLAY_SYNTH), plate=_iplate(PLAY_PLATE))
    c.prepare_synth(1, _isynth(PLAY_OTHER))


def _oracle_want(oracle_mod, n_ref, taps, x, **kw):
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, P0, P1, True)
    want = ref.process(x[0], x[1], **kw)
    _check_level(want, x, P0, P1)
    return want


def test_jack_period_matches_the_oracle(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, period, ncalls = 16384, 256, 160
    taps = _play_taps(n_ref)
    x = make_input(ncalls * period)
    want = _oracle_want(oracle_mod, n_ref, taps, x, block=period)
    c = _conv(n_ref, max_batch=16, period=period)
    _prepare_play(c)
    _check_taps(c.ir_taps(0), taps[0].astype(np.float64))
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period])) for k in range(ncalls)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_single_transform_form(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 64
    taps = _play_taps(n_ref)
    x = make_input(nb * 256)
    want = _oracle_want(oracle_mod, n_ref, taps, x)
    c = _conv(n_ref, max_batch=32, form="single")
    _prepare_play(c)
    _check_info(c.ir_plate_info(0), _restated(PLAY_PLATE, PLAY_SYNTH)[1])
    assert c.ir_info(0)["taps"] == len(taps[0])
    np.testing.assert_allclose(c.ir_info(0)["sigma"], taps[0].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, IrEq, IrRoom, IrShape, IrTail
    from cuda_audio_amd.synth import make_ir

    synth = dict(ALONE, frames=3000)
    tail = IrTail(mode="cut", knee=(2000,), fade=64)
    c = _conv()
    c.prepare_synth(0, _isynth(synth), plate=_iplate(CUT), tail=tail, shape=IrShape(fade_out=100))
    c.prepare_synth(1, _isynth(dict(synth, late_gain=0.01, seed=5)))  # a second IR, without a plate
    state = lambda: (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0), c.ir_plate_info(0),  # noqa: E731
                     c.ir_tail_info(0), c.ir_taps(1).tobytes(), c.ir_info(1), c.num_irs())
    before = state()
    assert c.ir_plate_info(0)["modes"] == 472
    bad_plates = [dict(size=(0.01, 1.0)), dict(thickness_mm=0.0), dict(material=(0.0, 7850.0, 0.3)), dict(material=(200.0, 1.0, 0.3)), dict(material=(200.0, 7850.0, 0.5)),
                  dict(driver=(2.04, 0.4)), dict(pickups=((0.3, 0.97), (1.5, 0.3))), dict(low_hz=0.0), dict(high_hz=10.0), dict(t60=(1.0, 4.0)),
                  dict(damp_hz=0.0), dict(gain=0.0), dict(gain=17.0), dict(high_hz=24000.0), dict(low_hz=20.0, high_hz=20.5),
                  dict(size=(10.0, 10.0), thickness_mm=0.05)]
    for fields in bad_plates:
        for idx in (0, 1, 2):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), plate=_iplate(fields))
            assert ex.value.code == -1, fields
    # the work cap: the whole default plate over 2^22 frames is 1.57 times what is allowed
    with pytest.raises(McError) as ex:
        c.prepare_synth(0, _isynth(dict(ALONE, frames=1 << 22)), plate=_iplate({}))
    assert ex.value.code == -1 and "pairs" in str(ex.value) and "1.57 times" in str(ex.value)
    # a plate together with a room is not offered
    with pytest.raises(ValueError):
        c.prepare_synth(0, _isynth(synth), plate=_iplate(CUT), room=IrRoom(order=2))
    good = _iplate(CUT)
    for kw in (dict(tail=IrTail(mode="extend", knee=(100,), t60=(0,))), dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=3000)),
               dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(damp=IrDamp(xovers=(1600, 400), decay=(0, 1, 2))), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), plate=good, **kw)
            assert ex.value.code == -1
    with pytest.raises(McError) as ex:
        c.prepare_synth(1, _isynth(dict(synth, frames=0)), plate=good)
    assert ex.value.code == -1
    nosr = _conv(16384, None)  # (an engine without a session rate: the plate needs one)
    with pytest.raises(McError) as ex:
        nosr.prepare_synth(0, _isynth(synth), plate=good)
    assert ex.value.code == -1 and "rate" in str(ex.value) and nosr.num_irs() == 0
    nosr.close()
    with pytest.raises(McError) as ex:
        c.ir_plate_info(1)
    assert ex.value.code == -3
    with pytest.raises(McError) as ex:
        c.ir_plate_info(2)
    assert ex.value.code == -1
    assert state() == before
    # a WAV load over the index forgets the plate, and so does a synthesis without one
    c.prepare(0, make_ir(3000, seed=2, norm=0.05))
    with pytest.raises(McError) as ex:
        c.ir_plate_info(0)
    assert ex.value.code == -3
    c.prepare_synth(0, _isynth(synth), plate=good)
    assert c.ir_plate_info(0)["modes"] == 472
    c.prepare_synth(0, _isynth(dict(synth, direct=1.0)))
    with pytest.raises(McError) as ex:
        c.ir_plate_info(0)
    assert ex.value.code == -3
    c.close()
