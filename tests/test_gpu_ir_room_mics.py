"""Directional microphones and a directional source in the room on the device (mc_synth_ir_room_mics, k_room<true> of
csrc/irroom.hip.h): the stored taps, the sums and the spectra against the float64 restatement (tests/ir_room_mics_np.py), and
the parts of the definition that are exact: omni everywhere stores the bits of the room without microphones, a
figure-of-eight's null plane stores zeros, a setup that mirrors in y stores equal channels, two loads store the same bits, the
kept counts stay those of the room; then the closed form of the direct sound, the chain through ir_floor and the tail step,
and the refusals.

The bar for taps is test_gpu_ir_shape._check_taps, for the reason tests/test_gpu_ir_room.py gives: the factor adds a handful of
double roundings per image (two dot products, two divisions, two fused multiply-adds, two multiplies; numpy rounds the dot
products' adds where the device fuses them), each a relative 1e-16 on a contribution that is then rounded to a quantum of
2^-40 anyway.  Every comparison of counts or of zero patterns first asserts on the restatement that no delay lies where a
rounding could move its floor (ir_room_np.assert_floor_margin)."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_room_mics_np
import ir_room_np
import ir_tail_np
from helpers import rms
from test_gpu_ir_eq import _check_sums_and_spectra
from test_gpu_ir_room import ALONE, CHAIN_BANDS, CHAIN_DAMP, CHAIN_F, CHAIN_ROOM, CHAIN_SHAPE, CROWDED, RATE, _conv, _freeze, _iroom, _isynth
from test_gpu_ir_shape import _check_taps
from test_ir_room_mics_cpu import GENERAL, MIRRORED, ROOM_S, ROOM_Z

pytestmark = pytest.mark.gpu


def _imics(fields):
    from cuda_audio_amd.engine import IrRoomMics

    return IrRoomMics(**fields)


def _fields(mics):
    """An IrRoomMics as the restatement's fields."""
    return dict(pattern=mics.pattern, az=mics.az, el=mics.el, source_pattern=mics.source_pattern, source_az=mics.source_az, source_el=mics.source_el)


@functools.lru_cache(maxsize=None)
def _restated_cached(room, mics, synth):
    room, mics, synth = dict(room), dict(mics), dict(synth)
    out, covered, info = ir_room_mics_np.frames64(room, mics, RATE, **synth)
    im = ir_room_np.images(room, RATE, synth["frames"])
    for a in (out, covered):
        a.setflags(write=False)
    return out, covered, info, im["tau"]


def _restated(room, mics, synth):
    """(frames float64 [F, 2], covered, info, every tau) of a room with microphones over a synthesis, computed once."""
    return _restated_cached(_freeze(room), _freeze(mics), _freeze(synth))


def _load_and_check(c, idx, room, mics, synth, **kw):
    """Load, then taps, both informations, kept counts and the zero pattern against the restatement."""
    want, covered, winfo, tau = _restated(room, mics, synth)
    ir_room_np.assert_floor_margin(tau, winfo["last"])
    c.prepare_synth(idx, _isynth(synth), room=_iroom(room), mics=_imics(mics), **kw)
    got = c.ir_taps(idx)
    w = want[:len(got)]
    if np.abs(w).max() > 0:
        err = got.astype(np.float64) - w
        print(f"relative rms {rms(err) / rms(w):.2e}")
        _check_taps(got, w)
    else:
        np.testing.assert_array_equal(got, w.astype(np.float32))
    info = c.ir_room_info(idx)
    print("room info:", info, "restated:", winfo)
    assert info["order"] == winfo["order"] and info["images"] == winfo["images"] and info["last"] == winfo["last"] and info["complete"] == winfo["complete"]
    np.testing.assert_allclose(info["direct"], winfo["direct"], rtol=1e-14, atol=0)
    minfo = c.ir_room_mics_info(idx)
    for k in ("source", "receiver", "factor"):
        np.testing.assert_allclose(minfo[k], winfo["mics"][k], rtol=0, atol=1e-14)
    silent = ~covered[:len(got)]  # (ALONE: frames that no kept window reaches are exactly zero)
    assert not w[silent].any() and not got[silent].any()
    return got, w, winfo


def _bits(c, idx):
    return c.ir_taps(idx).tobytes(), c.ir_spectra(idx).tobytes()


@pytest.mark.parametrize("order", [2, 6])
def test_the_general_case_matches_the_restatement(gpu_lib, order):
    """Different patterns, aims off every axis, a supercardioid source: rear lobes, a third to a half of the factors negative."""
    from cuda_audio_amd.engine import room_mics_plan

    F = 4000
    synth, room = dict(ALONE, frames=F), dict(order=order)
    c = _conv()
    got, want, winfo = _load_and_check(c, 0, room, GENERAL, synth)
    assert 0.3 <= winfo["negative"] <= 0.5 and (got < 0).any() and (got > 0).any()
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    assert c.ir_room_mics_info(0) == room_mics_plan(_iroom(room), _imics(GENERAL), RATE, F)
    c.prepare_synth(1, _isynth(synth), room=_iroom(room))
    assert c.ir_room_info(1) == c.ir_room_info(0)  # (the counts, the delays and E are the room's, whatever the microphones)
    assert not np.array_equal(c.ir_taps(1), got)
    c.close()


def test_omni_microphones_store_the_bits_of_the_room(gpu_lib):
    F = 4000
    synth, room = dict(ALONE, frames=F), dict(order=4, beta=(0.9, -0.8, 0.7, 0.95, 0.6, 1.0))
    c = _conv()
    c.prepare_synth(0, _isynth(synth), room=_iroom(room))
    c.prepare_synth(1, _isynth(synth), room=_iroom(room), mics=_imics(dict(az=(123.0, -77.0), el=(40.0, -80.0), source_az=211.0, source_el=33.0)))
    c.prepare_synth(2, _isynth(synth), room=_iroom(room), mics=None)
    c.prepare_synth(3, _isynth(synth), room=_iroom(room), mics=_imics({}))
    assert np.count_nonzero(c.ir_taps(0)) > 4000
    for idx in (1, 2, 3):
        assert _bits(c, idx) == _bits(c, 0) and c.ir_info(idx) == c.ir_info(0) and c.ir_room_info(idx) == c.ir_room_info(0)
    assert c.ir_room_mics_info(1) == dict(source=(1.0, 1.0), receiver=(1.0, 1.0), factor=(1.0, 1.0))
    c.close()


def test_a_figure_of_eight_is_deaf_in_its_plane(gpu_lib):
    """Room Z: every image that carries amplitude lies at p_x = 0.  L, a figure-of-eight aimed along x, stores zeros; R, omni,
    stores the room's R; the images are counted all the same."""
    F = 3000
    synth = dict(ALONE, frames=F)
    c = _conv()
    c.prepare_synth(1, _isynth(synth), room=_iroom(ROOM_Z))
    plain = c.ir_taps(1)
    got, _, winfo = _load_and_check(c, 0, ROOM_Z, dict(pattern=(0.0, 1.0), az=0.0), synth)
    assert np.count_nonzero(plain[:, 0]) == 1936 and not got[:, 0].any()
    assert got[:, 1].tobytes() == plain[:, 1].tobytes()
    assert c.ir_room_info(0) == c.ir_room_info(1) and min(winfo["images"]) > 0
    assert c.ir_room_mics_info(0)["factor"] == (0.0, 1.0)
    c.close()


@pytest.mark.parametrize("spacing,mics", MIRRORED)
def test_a_mirrored_setup_stores_equal_channels(gpu_lib, spacing, mics):
    c = _conv()
    got, _, winfo = _load_and_check(c, 0, dict(ROOM_S, spacing=spacing), mics, dict(ALONE, frames=3000))
    c.close()
    assert got[:, 0].tobytes() == got[:, 1].tobytes() and np.count_nonzero(got[:, 0]) > 1000
    assert winfo["images"][0] == winfo["images"][1]


def test_beta_zero_leaves_the_direct_sound_alone(gpu_lib):
    """Against the closed form: gain / d times the plan's factor times a Hann-windowed sinc about tau, per channel."""
    from cuda_audio_amd.engine import IrRoomMics, room_mics_plan

    room = dict(beta=0.0, gain=2.0, spacing=0.3, axis=1)
    mics = IrRoomMics.pair(facing=150.0, angle=90.0, pattern="cardioid")
    F = 1000
    c = _conv()
    c.prepare_synth(0, _isynth(dict(ALONE, frames=F)), room=_iroom(room), mics=mics)
    got = c.ir_taps(0)
    assert c.ir_room_mics_info(0) == room_mics_plan(_iroom(room), mics, RATE, F)
    c.close()
    factor = room_mics_plan(_iroom(room), mics, RATE, F)["factor"]
    print("factors:", factor)
    assert 0.2 < min(factor) < max(factor) < 1.0 and factor[0] != factor[1]
    L, s, r, _, speed, gain = ir_room_np.geometry(room)
    want = np.zeros((F, 2))
    for ch in range(2):
        d = float(np.sqrt(((s - r[ch]) ** 2).sum()))
        tau = d * RATE / speed
        m = np.arange(int(np.floor(tau)) - 15, int(np.floor(tau)) + 17)
        want[m, ch] = gain / d * factor[ch] * np.sinc(m - tau) * (1.0 + np.cos(np.pi * (m - tau) / 16.0)) / 2.0
    _check_taps(got, want)
    assert np.count_nonzero(got) == 64  # (the other images are kept and counted, and add nothing)


def test_many_images_on_one_frame_give_the_same_bits(gpu_lib):
    """CROWDED with a Blumlein pair: thousands of images of both signs on a few hundred frames; integer sums do not depend on the
    order of arrival."""
    from cuda_audio_amd.engine import IrRoomMics

    F = 6000
    mics = _fields(IrRoomMics.pair(facing=20.0, angle=90.0, pattern="fig8"))
    c = _conv()
    a, _, winfo = _load_and_check(c, 0, CROWDED, mics, dict(ALONE, frames=F))
    b, _, _ = _load_and_check(c, 1, CROWDED, mics, dict(ALONE, frames=F))
    assert winfo["images"][0] == 5137 and 0.3 < winfo["negative"] < 0.7
    assert _bits(c, 0) == _bits(c, 1)
    assert c.ir_info(0) == c.ir_info(1) and c.ir_room_info(0) == c.ir_room_info(1) and c.ir_room_mics_info(0) == c.ir_room_mics_info(1)
    c.close()


def test_the_chain_from_the_room_through_the_floor_to_the_tail(gpu_lib):
    """test_gpu_ir_room's chain with an XY pair and a cardioid source in the room."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrRoomMics, IrShape, tail_from_floor

    n_ref = 65536
    synth = dict(ALONE, frames=CHAIN_F)
    mics = _fields(IrRoomMics.pair(facing=180.0, source_pattern="cardioid", source_az=30.0))
    c = _conv(n_ref)
    _, want_room, winfo = _load_and_check(c, 0, CHAIN_ROOM, mics, synth)
    assert winfo["order"] == 15 and winfo["complete"] >= CHAIN_F
    floor = c.ir_floor(0, margin_db=5.0)  # (the margin: see test_gpu_ir_room's chain)
    tail = tail_from_floor(floor, mode="extend", fade=256, length=48000, seed=11)
    print("tail:", tail)
    assert len(tail.knee) == 1 and tail.knee[0] is not None and CHAIN_F // 2 < tail.knee[0] < CHAIN_F, tail
    xovers, decay, origin = CHAIN_DAMP
    c.prepare_synth(0, _isynth(synth), room=_iroom(CHAIN_ROOM), mics=_imics(mics), tail=tail, shape=IrShape(**CHAIN_SHAPE), eq=IrEq(bands=list(CHAIN_BANDS)),
                    damp=IrDamp(xovers=xovers, decay=decay, origin=origin))
    got = c.ir_taps(0)
    spec = dict(xovers=tail.xovers, knee=tail.knee, t60=tail.t60, level_db=tail.level_db, fade=256, length=48000, seed=11, width=1.0)
    y, wtinfo = ir_tail_np.tail64(want_room.astype(np.float32), RATE, "extend", **spec)
    want, _, wdinfo = ir_damp_np.damped(y.astype(np.float32), n_ref - 1024, None, RATE, xovers, decay, origin, CHAIN_BANDS, **CHAIN_SHAPE)
    _check_taps(got, want.astype(np.float64))
    assert c.ir_tail_info(0) == wtinfo and wtinfo["frames"] == CHAIN_F and wtinfo["length"] == 48000
    assert c.ir_room_info(0)["images"] == winfo["images"] and c.ir_damp_info(0) == wdinfo and c.ir_shape_info(0)["taps"] == 48000
    for k in ("source", "receiver", "factor"):
        np.testing.assert_allclose(c.ir_room_mics_info(0)[k], winfo["mics"][k], rtol=0, atol=1e-14)
    c.close()


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrShape

    synth = dict(ALONE, frames=3000)
    room = _iroom(dict(order=3))
    c = _conv()
    c.prepare_synth(0, _isynth(synth), room=room, mics=_imics(GENERAL), shape=IrShape(fade_out=100))
    state = lambda: (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0), c.ir_room_info(0),
                     c.ir_room_mics_info(0), c.num_irs())
    before = state()
    bad = [("mic_pattern[0]", dict(pattern=(1.5, 0.5))), ("mic_pattern[1]", dict(pattern=(0.5, -0.1))), ("mic_az_deg[1]", dict(az=(0.0, 400.0))),
           ("mic_el_deg[0]", dict(el=(91.0, 0.0))), ("mic_el_deg[1]", dict(el=(0.0, float("nan")))), ("src_pattern", dict(source_pattern=2.0)),
           ("src_az_deg", dict(source_az=float("inf"))), ("src_el_deg", dict(source_el=-100.0))]
    for name, fields in bad:
        for idx in (0, 1):  # (a loaded and a fresh index)
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), room=room, mics=_imics(fields))
            assert ex.value.code == -1 and name in str(ex.value)
    for idx in (0, 1):
        with pytest.raises(ValueError):
            c.prepare_synth(idx, _isynth(synth), mics=_imics(GENERAL))
        s = _isynth(dict(synth, rate=RATE)).to_c()
        assert c._L.mc_synth_ir_room_mics(c._h, idx, 1024, C.byref(s), None, C.byref(_imics(GENERAL).to_c()), None, None, None, None) == -1
        assert "the microphones need a room" in c._L.mc_last_error().decode()
    with pytest.raises(McError) as ex:  # (a bad room with bad microphones: the room is named)
        c.prepare_synth(0, _isynth(synth), room=_iroom(dict(order=33)), mics=_imics(dict(el=99.0)))
    assert ex.value.code == -1 and "order" in str(ex.value)
    with pytest.raises(McError) as ex:
        c.ir_room_mics_info(1)
    assert ex.value.code == -1  # (not loaded)
    assert state() == before and c.num_irs() == 1
    # a later load without microphones forgets them; the room still answers
    c.prepare_synth(0, _isynth(synth), room=room)
    with pytest.raises(McError) as ex:
        c.ir_room_mics_info(0)
    assert ex.value.code == -3 and "microphones" in str(ex.value)
    assert c.ir_room_info(0)["order"] == 3
    c.prepare_synth(0, _isynth(synth), room=room, mics=_imics(GENERAL))
    assert c.ir_room_mics_info(0) == before[6]
    c.prepare_synth(0, _isynth(dict(synth, direct=1.0)))
    for info in (c.ir_room_mics_info, c.ir_room_info):
        with pytest.raises(McError) as ex:
            info(0)
        assert ex.value.code == -3
    c.close()
