"""The reflections of a rectangular room on the device (mc_synth_ir_room, csrc/irroom.hip.h): the stored taps, the shape
information, the sums and the spectra against the float64 restatement (tests/ir_room_np.py), the parts of the definition that
are exact (which frames are zero, how many images are kept, the whole-frame delay, equal channels at spacing 0, the same bits
from two loads), the edges of the accumulator and of the store walk, the chain through ir_floor and the tail step, the engine's
paths against the oracle fed the restated taps, and the refusals.

The bar for taps is test_gpu_ir_shape._check_taps (1e-6 relative RMS, 1e-5 of the peak): a contribution differs from numpy's
by a few ulp of a double (sqrt, sin, cos, the contraction of a multiply and an add), hence by at most a quantum of 2^-40 each
before the one rounding to float32, which is the situation that bar was set for.  Every comparison of counts or of zero
patterns first asserts on the restatement that no delay lies where a rounding could move its floor
(ir_room_np.assert_floor_margin)."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_room_np
import ir_synth_np
import ir_tail_np
from helpers import BASE, RMS_TOL, apply_params, rms
from test_gpu_ir_eq import _check_sums_and_spectra
from test_gpu_ir_shape import P0, P1, _check_level, _check_taps

pytestmark = pytest.mark.gpu

RATE = 48000
ALONE = dict(late_gain=0.0, direct=0.0)  # the synthesis' own terms off: the room alone
WHOLE = dict(size=(10.0, 10.0, 10.0), source=(2.0, 5.0, 5.0), receiver=(3.0, 5.0, 5.0), spacing=0.0, speed=480.0, beta=0.0, gain=0.5)
CROWDED = dict(size=(4.0, 4.0, 4.0), source=(2.0, 2.0, 2.0), receiver=(2.5, 2.0, 2.0), order=8)


def _conv(n_ref=16384, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irroom", n_ref, sample_rate=rate, **kw)


def _iroom(fields):
    from cuda_audio_amd.engine import IrRoom

    return IrRoom(**fields)


def _isynth(fields):
    from cuda_audio_amd.engine import IrSynth

    return IrSynth(**fields)


def _freeze(v):
    return tuple(sorted((k, _freeze(x)) for k, x in v.items())) if isinstance(v, dict) else v


@functools.lru_cache(maxsize=None)
def _restated_cached(room, synth):
    room, synth = dict(room), dict(synth)
    out, covered, info = ir_room_np.frames64(room, RATE, **synth)
    im = ir_room_np.images(room, RATE, synth["frames"])
    for a in (out, covered):
        a.setflags(write=False)
    return out, covered, info, im["tau"]


def _restated(room, synth):
    """(frames float64 [F, 2], covered, info, every tau) of a room over a synthesis, computed once."""
    return _restated_cached(_freeze(room), _freeze(synth))


def _load_and_check(c, idx, room, synth, exact=0, **kw):
    """Load, then taps, room information, kept counts and the zero pattern against the restatement."""
    want, covered, winfo, tau = _restated(room, synth)
    ir_room_np.assert_floor_margin(tau, winfo["last"], exact=exact)
    c.prepare_synth(idx, _isynth(synth), room=_iroom(room), **kw)
    got = c.ir_taps(idx)
    cap = len(got)
    w = want[:cap]
    if np.abs(w).max() > 0:
        _check_taps(got, w)
    else:
        np.testing.assert_array_equal(got, w.astype(np.float32))
    info = c.ir_room_info(idx)
    print("room info:", info, "restated:", winfo)
    assert info["order"] == winfo["order"] and info["images"] == winfo["images"] and info["last"] == winfo["last"] and info["complete"] == winfo["complete"]
    np.testing.assert_allclose(info["direct"], winfo["direct"], rtol=1e-14, atol=0)
    if not synth.get("late_gain", 1.0) and not synth.get("direct", 0.0) and not synth.get("n_early", 0):
        # frames that no kept window reaches are exactly zero, on the device and in the restatement
        silent = ~covered[:cap]
        assert not w[silent].any() and not got[silent].any()
    return got, w, covered[:cap], winfo


@pytest.mark.parametrize("order", [2, 6])
def test_the_room_alone_matches_the_restatement(gpu_lib, order):
    F = 4000
    synth = dict(ALONE, frames=F)
    c = _conv()
    got, want, covered, winfo = _load_and_check(c, 0, dict(order=order), synth)
    sinfo = c.ir_shape_info(0)
    assert (sinfo["frames"], sinfo["onset"], sinfo["first"], sinfo["taps"], sinfo["gain"], sinfo["eq_bands"]) == (F, 0, 0, F, 1.0, 0)
    assert abs(sinfo["peak"] - np.abs(want).max()) <= 1e-6 * np.abs(want).max()
    assert c.ir_synth_info(0) == dict(frames=F, reflections=0, late_start=0)
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    c.close()
    silent = int((~covered).all(axis=1).sum())
    print(f"order {order}: images kept {winfo['images']}, {silent} of {F} frames that no window reaches")
    if order == 2:
        assert winfo["images"] == (931, 927) and silent > 400  # (the lattice ends before F: gaps between the late windows)
    else:
        assert min(winfo["images"]) > 1500 and winfo["complete"] > F  # (complete: every image before F)


def test_a_whole_frame_delay_is_exactly_one_tap(gpu_lib):
    c = _conv()
    got, want, _, winfo = _load_and_check(c, 0, WHOLE, dict(ALONE, frames=300), exact=2)
    c.close()
    exact = np.zeros((300, 2), np.float32)
    exact[100] = 0.5
    np.testing.assert_array_equal(got, exact)
    assert winfo["images"] == (1, 1) and winfo["direct"] == (100.0, 100.0)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_spacing_zero_gives_equal_channels(gpu_lib, axis):
    c = _conv()
    got, _, _, winfo = _load_and_check(c, 0, dict(spacing=0.0, axis=axis, order=3), dict(ALONE, frames=3000))
    np.testing.assert_array_equal(got[:, 0], got[:, 1])
    assert winfo["images"][0] == winfo["images"][1] and np.count_nonzero(got[:, 0]) > 1000
    # and with a spacing the axis matters: the channels differ
    wide, _, _, _ = _load_and_check(c, 1, dict(spacing=0.4, axis=axis, order=3), dict(ALONE, frames=3000))
    c.close()
    assert not np.array_equal(wide[:, 0], wide[:, 1])


def test_a_negative_beta(gpu_lib):
    c = _conv()
    room = dict(beta=(-0.9, 0.8, -0.7, 0.95, 0.6, -1.0), order=4)
    got, want, _, _ = _load_and_check(c, 0, room, dict(ALONE, frames=5000))
    plain, _, _, _ = _load_and_check(c, 1, dict(room, beta=(0.9, 0.8, 0.7, 0.95, 0.6, 1.0)), dict(ALONE, frames=5000))
    c.close()
    assert not np.array_equal(got, plain)


def test_beta_zero_leaves_the_direct_sound_alone(gpu_lib):
    """Against the closed form: gain / d times a Hann-windowed sinc about tau, per channel."""
    room = dict(beta=0.0, gain=2.0, spacing=0.3, axis=1)
    F = 1000
    c = _conv()
    got, _, _, winfo = _load_and_check(c, 0, room, dict(ALONE, frames=F))
    c.close()
    L, s, r, _, speed, gain = ir_room_np.geometry(room)
    want = np.zeros((F, 2))
    for ch in range(2):
        d = float(np.sqrt(((s - r[ch]) ** 2).sum()))
        tau = d * RATE / speed
        m = np.arange(int(np.floor(tau)) - 15, int(np.floor(tau)) + 17)
        want[m, ch] = gain / d * np.sinc(m - tau) * (1.0 + np.cos(np.pi * (m - tau) / 16.0)) / 2.0
    _check_taps(got, want)
    assert np.count_nonzero(got) == 64  # (the other images are kept and counted, and add nothing)


@pytest.mark.parametrize("F,last", [(1500, 1490), (1500, 990), (995, 0)])
def test_windows_cut_at_both_ends(gpu_lib, F, last):
    """The receiver 0.1 m from the source: tau is about 14 and the direct sound's first taps fall before frame 0.  With last
    just inside F a kept image's window crosses F; with last far inside the accumulator ends before the IR does."""
    room = dict(source=(1.0, 1.5, 1.2), receiver=(1.1, 1.5, 1.2), spacing=0.0, last=last, gain=0.05)
    want, covered, winfo, tau = _restated(room, dict(ALONE, frames=F))
    E = winfo["last"]
    k0 = np.floor(tau)
    assert 13 <= winfo["direct"][0] < 15 and E == (last or F)
    if E + 16 > F:
        assert ((k0 < E) & (k0 + 16 >= F)).any()  # a kept window crosses F
    else:
        assert ((k0 >= E) & (k0 < F)).any() and covered[E + 16:].sum() == 0 and covered[E:E + 16].any()  # (images left out; a window past E)
    c = _conv()
    got, _, _, _ = _load_and_check(c, 0, room, dict(ALONE, frames=F))
    c.close()
    assert got[0].all()  # (the direct sound's window reaches frame 0)


@pytest.mark.parametrize("F", [1, 2, 3, 511, 512, 513, 777])
def test_lengths(gpu_lib, F):
    """The store walk's edges (a lone frame, one pair, a pair and a frame, a workgroup's span and a frame either side)."""
    room = dict(source=(1.0, 1.5, 1.2), receiver=(1.3, 1.5, 1.2), spacing=0.2, gain=0.05)  # (the direct sound at 28 and 56 frames)
    synth = dict(frames=F, seed=99, late_start=0, t60=500, build_up=40, late_gain=0.01, direct=0.5, n_early=3, early_first=0, early_last=max(F - 1, 0),
                 early_gain=0.25, width=0.6)
    c = _conv()
    got, want, _, _ = _load_and_check(c, 0, room, synth)
    assert len(got) == F and c.ir_shape_info(0)["frames"] == F
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    c.close()


def test_order_zero_picks_the_plan_and_the_maximum_holds(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import room_plan

    F = 2500
    c = _conv()
    _, _, _, winfo = _load_and_check(c, 0, {}, dict(ALONE, frames=F))
    plan = room_plan(_iroom({}), RATE, F)
    assert plan["order"] == winfo["order"] == ir_room_np.plan({}, RATE, F)["order"] == 3 and winfo["complete"] >= F
    # the same images as a lattice two orders larger keeps: order 0 is complete
    _, _, _, wider = _load_and_check(c, 1, dict(order=5), dict(ALONE, frames=F))
    assert wider["images"] == winfo["images"]
    np.testing.assert_array_equal(c.ir_taps(0), c.ir_taps(1))
    for bad in (dict(order=33), {}):  # (an order above the maximum; order 0 over a second needs 58)
        with pytest.raises(McError) as ex:
            c.prepare_synth(2, _isynth(dict(ALONE, frames=F if bad else 48000)), room=_iroom(bad), nframes=1024)
        assert ex.value.code == -1 and "order" in str(ex.value)
    assert c.num_irs() == 2
    c.close()


def test_many_images_on_one_frame_give_the_same_bits(gpu_lib):
    """A cube with the source at its centre: thousands of images on a few hundred arrival frames, dozens on one.  Integer sums
    do not depend on the order of arrival: two loads store the same bits."""
    F = 6000
    want, _, winfo, tau = _restated(CROWDED, dict(ALONE, frames=F))
    k0 = np.floor(tau[:, 0])
    k0 = k0[k0 < F].astype(np.int64)
    print(f"{len(k0)} images on {len(np.unique(k0))} arrival frames, up to {np.bincount(k0).max()} on one")
    assert len(k0) == 5137 and len(np.unique(k0)) < 500 and np.bincount(k0).max() >= 24
    c = _conv()
    a, _, _, _ = _load_and_check(c, 0, CROWDED, dict(ALONE, frames=F))
    b, _, _, _ = _load_and_check(c, 1, CROWDED, dict(ALONE, frames=F))
    assert a.tobytes() == b.tobytes() and c.ir_spectra(0).tobytes() == c.ir_spectra(1).tobytes()
    assert c.ir_info(0) == c.ir_info(1) and c.ir_room_info(0) == c.ir_room_info(1)
    c.close()


FULL = dict(frames=9000, seed=(0x1234 << 32) | 7, late_start=1500, t60=20000, build_up=2000, late_gain=0.05, direct=1.0, n_early=12, early_first=100,
            early_last=1400, early_gain=0.5, width=0.7)


def test_room_late_field_direct_and_reflections_round_once(gpu_lib):
    c = _conv()
    got, want, _, _ = _load_and_check(c, 0, dict(last=3000), FULL)
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    assert c.ir_synth_info(0) == dict(frames=9000, reflections=12, late_start=1500)
    # the room is a fourth term: without it the frames are mc_synth_ir's
    c.prepare_synth(1, _isynth(FULL))
    plain = c.ir_taps(1)
    c.close()
    assert not np.array_equal(got[:3016], plain[:3016])
    np.testing.assert_array_equal(got[3016:], plain[3016:])  # (past E + 16 the accumulator adds nothing)


def test_without_room_and_tail_the_call_is_mc_synth_ir(gpu_lib):
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, IrTail

    shape, eq, damp = IrShape(fade_out=100, normalize="peak", target=0.05), IrEq(bands=[("lowcut", 120)]), IrDamp(xovers=(400, 1600), decay=(0, 4800, 1600), origin=37)
    c = _conv()
    L = c._L
    c.prepare_synth(0, _isynth(FULL), shape=shape, eq=eq, damp=damp)
    s, sh, q, d = _isynth(dict(FULL, rate=RATE)).to_c(), shape.to_c(), eq.to_c(), damp.to_c()
    off = IrTail(mode="off").to_c()
    assert L.mc_synth_ir_room(c._h, 1, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), None) == 0
    assert L.mc_synth_ir_room(c._h, 2, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), C.byref(off)) == 0
    c.prepare_synth(3, _isynth(FULL), shape=shape, eq=eq, damp=damp, room=None, tail=IrTail(mode="off"))
    from cuda_audio_amd._lib import McError

    for idx in (1, 2, 3):
        assert c.ir_taps(idx).tobytes() == c.ir_taps(0).tobytes() and c.ir_spectra(idx).tobytes() == c.ir_spectra(0).tobytes()
        assert c.ir_info(idx) == c.ir_info(0) and c.ir_shape_info(idx) == c.ir_shape_info(0) and c.ir_synth_info(idx) == c.ir_synth_info(0)
        for info in (c.ir_room_info, c.ir_tail_info):
            with pytest.raises(McError) as ex:
                info(idx)
            assert ex.value.code == -3
    c.close()


def test_a_tail_without_a_room(gpu_lib):
    """prepare_synth(tail=): the tail step acts on the synthesised frames."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrTail

    p = dict(frames=3000, seed=4, late_start=10, t60=2500, late_gain=0.1, direct=1.0, width=0.3)
    spec = dict(xovers=(1000,), knee=(1500, 1400), t60=(3000, 2000), level_db=((-50.0, -51.0), (-55.0, -54.0)), fade=32, length=5000, seed=5, width=0.5)
    want, winfo = ir_tail_np.tail64(ir_synth_np.frames(**p), RATE, "extend", **spec)
    c = _conv()
    c.prepare_synth(0, _isynth(p), tail=IrTail(mode="extend", **spec))
    _check_taps(c.ir_taps(0), want)
    assert c.ir_tail_info(0) == winfo and c.ir_shape_info(0)["frames"] == 5000 and c.ir_synth_info(0)["frames"] == 3000
    with pytest.raises(McError) as ex:
        c.ir_room_info(0)
    assert ex.value.code == -3
    c.close()


CHAIN_ROOM = dict(gain=0.2)
CHAIN_F = 12000  # 0.25 s
CHAIN_SHAPE = dict(fade_out=2000, normalize="peak", target=0.05)
CHAIN_BANDS = (("lowcut", 80), ("highshelf", 6000, -3.0))
CHAIN_DAMP = ((400, 1600), (0, 40000, 20000), 300)


def test_the_chain_from_the_room_through_the_floor_to_the_tail(gpu_lib):
    """The room rendered for a quarter of a second, its floor found, the tail continued at its own slope and level for a
    second, then shaping, damping and EQ: against the restated chain."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, tail_from_floor

    n_ref = 65536
    synth = dict(ALONE, frames=CHAIN_F)
    c = _conv(n_ref)
    room_only, want_room, _, winfo = _load_and_check(c, 0, CHAIN_ROOM, synth)
    assert winfo["order"] == 15 and winfo["complete"] >= CHAIN_F
    # (a quarter of a second of this room decays some 18 dB: with the search's default margin of 10 dB over its own last tenth the
    # line crosses past the last frame and the band would be left alone; 5 dB puts the knee inside)
    floor = c.ir_floor(0, margin_db=5.0)
    tail = tail_from_floor(floor, mode="extend", fade=256, length=48000, seed=11)
    print("tail:", tail)
    assert len(tail.knee) == 1 and tail.knee[0] is not None and CHAIN_F // 2 < tail.knee[0] < CHAIN_F, tail
    assert 0.6 * RATE < tail.t60[0] < 1.2 * RATE  # (the room's own slope: about 0.85 s, where Eyring's formula says 0.49 s)
    xovers, decay, origin = CHAIN_DAMP
    c.prepare_synth(0, _isynth(synth), room=_iroom(CHAIN_ROOM), tail=tail, shape=IrShape(**CHAIN_SHAPE), eq=IrEq(bands=list(CHAIN_BANDS)),
                    damp=IrDamp(xovers=xovers, decay=decay, origin=origin))
    got = c.ir_taps(0)
    spec = dict(xovers=tail.xovers, knee=tail.knee, t60=tail.t60, level_db=tail.level_db, fade=256, length=48000, seed=11, width=1.0)
    y, wtinfo = ir_tail_np.tail64(want_room.astype(np.float32), RATE, "extend", **spec)
    want, wsinfo, wdinfo = ir_damp_np.damped(y.astype(np.float32), n_ref - 1024, None, RATE, xovers, decay, origin, CHAIN_BANDS, **CHAIN_SHAPE)
    _check_taps(got, want.astype(np.float64))
    assert c.ir_tail_info(0) == wtinfo and wtinfo["frames"] == CHAIN_F and wtinfo["length"] == 48000
    rinfo = c.ir_room_info(0)
    assert rinfo["order"] == 15 and rinfo["images"] == winfo["images"] and rinfo["last"] == CHAIN_F
    assert c.ir_damp_info(0) == wdinfo and c.ir_shape_info(0)["frames"] == 48000 and c.ir_shape_info(0)["taps"] == 48000
    # the extension carries on where the room stopped: the second quarter second is not silent, and quieter than the first
    e = lambda a: float((a.astype(np.float64) ** 2).sum())
    assert 0 < e(got[CHAIN_F:2 * CHAIN_F]) < e(got[:CHAIN_F])
    c.close()


# -- the engine plays a rendered room ------------------------------------------------------------------------------------------
PLAY_ROOM = dict(gain=0.05, order=4)
PLAY_SYNTH = dict(frames=7000, seed=11, late_start=2000, t60=5000, build_up=600, late_gain=0.002, direct=0.0, width=0.7)
PLAY_OTHER = dict(frames=5000, seed=3, late_start=0, t60=4000, late_gain=0.01, width=1.0)


def _play_taps(n_ref):
    a = _restated(PLAY_ROOM, PLAY_SYNTH)[0].astype(np.float32)[:n_ref - 1024]
    return [a, ir_synth_np.frames(**PLAY_OTHER)[:n_ref - 1024]]


def _prepare_play(c):
    c.prepare_synth(0, _isynth(PLAY_SYNTH), room=_iroom(PLAY_ROOM))
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
    winfo = _restated(PLAY_ROOM, PLAY_SYNTH)[2]
    assert c.ir_room_info(0)["images"] == winfo["images"] and c.ir_info(0)["taps"] == len(taps[0])
    np.testing.assert_allclose(c.ir_info(0)["sigma"], taps[0].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, IrTail
    from cuda_audio_amd.synth import make_ir

    synth = dict(ALONE, frames=3000)
    tail = IrTail(mode="extend", knee=(2000,), t60=(3000,), level_db=((-60.0, -60.0),), fade=64, length=4000, seed=3)
    c = _conv()
    c.prepare_synth(0, _isynth(synth), room=_iroom(dict(order=3)), tail=tail, shape=IrShape(fade_out=100))
    state = lambda: (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0), c.ir_room_info(0),
                     c.ir_tail_info(0), c.num_irs())
    before = state()
    assert c.ir_room_info(0)["order"] == 3 and c.ir_tail_info(0)["length"] == 4000
    bad_rooms = [dict(order=33), dict(size=(0.4, 4.0, 3.0)), dict(source=(5.0, 1.5, 1.2)), dict(receiver=(3.5, 2.0, 3.0)), dict(beta=1.5), dict(spacing=-1.0),
                 dict(axis=3), dict(spacing=3.2), dict(speed=50.0), dict(gain=0.0), dict(source=(3.45, 2.0, 1.5)), dict(order=32, gain=8.0)]
    for fields in bad_rooms:
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), room=_iroom(fields))
            assert ex.value.code == -1
    good = _iroom(dict(order=2))
    for kw in (dict(tail=IrTail(mode="extend", knee=(100,), t60=(0,))), dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=3000)),
               dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(damp=IrDamp(xovers=(1600, 400), decay=(0, 1, 2))), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), room=good, **kw)
            assert ex.value.code == -1
    with pytest.raises(McError) as ex:
        c.prepare_synth(1, _isynth(dict(synth, frames=0)), room=good)
    assert ex.value.code == -1
    nosr = _conv(16384, None)  # (an engine without a session rate: the room needs one)
    with pytest.raises(McError) as ex:
        nosr.prepare_synth(0, _isynth(synth), room=good)
    assert ex.value.code == -1 and "rate" in str(ex.value) and nosr.num_irs() == 0
    nosr.close()
    with pytest.raises(McError) as ex:
        c.ir_room_info(1)
    assert ex.value.code == -1
    assert state() == before
    # a WAV load over the index forgets the room, and so does a synthesis without one
    c.prepare(0, make_ir(3000, seed=2, norm=0.05))
    with pytest.raises(McError) as ex:
        c.ir_room_info(0)
    assert ex.value.code == -3
    c.prepare_synth(0, _isynth(synth), room=good)
    assert c.ir_room_info(0)["order"] == 2
    c.prepare_synth(0, _isynth(dict(synth, direct=1.0)))
    with pytest.raises(McError) as ex:
        c.ir_room_info(0)
    assert ex.value.code == -3
    c.close()
