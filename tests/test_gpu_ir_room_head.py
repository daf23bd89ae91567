"""The binaural listener in the room on the device (mc_synth_ir_room_head: k_room's HEAD instantiations and k_room_head of
csrc/irroom.hip.h): the stored taps, the sums and the spectra against the float64 restatement (tests/ir_room_head_np.py), and
the parts of the definition that are exact: shadow 0 leaves the pure delays, a setup that mirrors in y stores equal channels, two
loads store the same bits, equal bands store the unbanded head's bits, head=None stores the bits of the room without one; then
the closed form of the direct sound, the shelf's magnitudes as ir_response reads them, the interaural delay as ir_iacc reads it,
the shelf's ringing over long carries, the chain through ir_floor and the tail step, and the refusals.

The bar for taps is test_gpu_ir_shape._check_taps, for the reason tests/test_gpu_ir_room.py gives: per image and ear the head adds
a dot product, a division, an arc cosine, a fused multiply-add and a cosine, each a relative 1e-16 or so on a delay near 1e3
frames and on a factor of magnitude at most 1, and the contribution is then rounded to a quantum of 2^-40 anyway; the shelf is a
first-order recurrence whose chunked form differs from the sequential one by roundings of the same size.  Every comparison of
counts first asserts on the restatement that no delay lies where a rounding could move its floor
(ir_room_np.assert_floor_margin)."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_room_head_np
import ir_room_np
import ir_tail_np
from helpers import rms
from test_gpu_ir_eq import _check_sums_and_spectra
from test_gpu_ir_room import ALONE, CHAIN_BANDS, CHAIN_DAMP, CHAIN_F, CHAIN_ROOM, CHAIN_SHAPE, CROWDED, RATE, _conv, _freeze, _iroom, _isynth
from test_gpu_ir_shape import _check_taps
from test_ir_room_head_cpu import GENERAL_HEAD, LATERAL, ROOM_S

pytestmark = pytest.mark.gpu

BANDS = dict(xovers=(500.0, 2000.0), beta=(0.95, 0.85, 0.6), air=(0.0, 0.005, 0.03))


def _ihead(fields):
    from cuda_audio_amd.engine import IrRoomHead

    return IrRoomHead(**fields)


def _imics(fields):
    from cuda_audio_amd.engine import IrRoomMics

    return IrRoomMics(**fields) if fields is not None else None


def _ibands(fields):
    from cuda_audio_amd.engine import IrRoomBands

    return IrRoomBands(**fields) if fields is not None else None


@functools.lru_cache(maxsize=None)
def _restated_cached(room, mics, bands, head, synth):
    thaw = lambda v: dict(v) if v is not None else None
    out, covered, info = ir_room_head_np.frames64(dict(room), thaw(mics), thaw(bands), dict(head), RATE, **dict(synth))
    for a in (out, covered):
        a.setflags(write=False)
    return out, covered, info


def _restated(room, head, synth, mics=None, bands=None):
    """(frames float64 [F, 2], covered, info) of a room with a head over a synthesis, computed once."""
    fr = lambda v: _freeze(v) if v is not None else None
    return _restated_cached(_freeze(room), fr(mics), fr(bands), _freeze(head), _freeze(synth))


def _load_and_check(c, idx, room, head, synth, mics=None, bands=None, **kw):
    """Load, then taps, both informations and the kept counts against the restatement."""
    from cuda_audio_amd.engine import room_head_plan

    want, covered, winfo = _restated(room, head, synth, mics, bands)
    ir_room_np.assert_floor_margin(winfo["tau"], winfo["last"])
    c.prepare_synth(idx, _isynth(synth), room=_iroom(room), head=_ihead(head), mics=_imics(mics), bands=_ibands(bands), **kw)
    got = c.ir_taps(idx)
    w = want[:len(got)]
    err = got.astype(np.float64) - w
    print(f"relative rms {rms(err) / rms(w):.2e}")
    _check_taps(got, w)
    info = c.ir_room_info(idx)
    print("room info:", info, "restated:", {k: v for k, v in winfo.items() if k not in ("tau", "h")})
    assert info["order"] == winfo["order"] and info["images"] == winfo["images"] and info["last"] == winfo["last"] and info["complete"] == winfo["complete"]
    np.testing.assert_allclose(info["direct"], winfo["direct"], rtol=1e-13, atol=0)
    assert c.ir_room_head_info(idx) == room_head_plan(_iroom(room), _ihead(head), RATE, synth["frames"])
    assert c.ir_room_head_info(idx)["direct"] == info["direct"]
    return got, w, winfo


def _bits(c, idx):
    return c.ir_taps(idx).tobytes(), c.ir_spectra(idx).tobytes()


@pytest.mark.parametrize("order", [2, 6])
def test_the_general_case_matches_the_restatement(gpu_lib, order):
    """A head that faces off every axis with its ears behind the axis through it: both signs of the shadow factor."""
    F = 4000
    synth, room = dict(ALONE, frames=F), dict(order=order)
    c = _conv()
    got, want, winfo = _load_and_check(c, 0, room, GENERAL_HEAD, synth)
    assert 0.3 <= winfo["negative"] <= 0.8 and (got < 0).any() and (got > 0).any()
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    c.prepare_synth(1, _isynth(synth), room=_iroom(room))
    assert not np.array_equal(c.ir_taps(1), got)
    c.close()


def test_shadow_zero_leaves_the_pure_delays(gpu_lib):
    """The restatement's term is then the plain accumulator's alone (test_ir_room_head_cpu asserts it); the lateral source's
    interaural delay is what ir_iacc finds."""
    F = 4000
    head = dict(GENERAL_HEAD, shadow=0.0)
    c = _conv()
    got, want, _ = _load_and_check(c, 0, dict(order=3), head, dict(ALONE, frames=F))
    accP, accS, _, _ = ir_room_head_np.render_band(dict(order=3), None, head, None, 0.0, RATE, F)
    assert not accS.any()
    np.testing.assert_array_equal(got, (accP.astype(np.float64) / ir_room_np.Q).astype(np.float32)[:len(got)])  # (S is +0.0: the bits of the delays alone)
    _, _, winfo = _load_and_check(c, 1, LATERAL, dict(shadow=0.0), dict(ALONE, frames=1000))
    itd = winfo["direct"][1] - winfo["direct"][0]
    row = c.ir_iacc(1, max_lag=48, onset_db=0.0)["rows"][(0, "all")]
    print("itd", itd, "iacc row", row)
    assert 31.0 < itd < 32.0 and abs(row["lag"] - itd) <= 1.0  # (the peak is a whole lag; R is late: positive)
    c.close()


@pytest.mark.parametrize("ear", [90.0, 100.0])
def test_a_mirrored_setup_stores_equal_channels(gpu_lib, ear):
    c = _conv()
    got, _, winfo = _load_and_check(c, 0, ROOM_S, dict(ear=ear), dict(ALONE, frames=3000))
    c.close()
    assert got[:, 0].tobytes() == got[:, 1].tobytes() and np.count_nonzero(got[:, 0]) > 1000
    assert winfo["images"][0] == winfo["images"][1]


def test_beta_zero_leaves_the_direct_sound_alone(gpu_lib):
    """Against the closed form: gain / d times a Hann-windowed sinc about each ear's tau, plus h times the same sinc through the
    shelf; then the shelf's magnitudes for a lateral source as ir_response reads them, Brown and Duda's figures."""
    from cuda_audio_amd.engine import room_head_plan

    room, F = dict(beta=0.0, gain=2.0), 1000
    c = _conv()
    for idx, head in enumerate((GENERAL_HEAD, dict(facing=150.0))):
        c.prepare_synth(idx, _isynth(dict(ALONE, frames=F)), room=_iroom(room), head=_ihead(head))
        got = c.ir_taps(idx)
        plan = room_head_plan(_iroom(room), _ihead(head), RATE, F)
        assert c.ir_room_head_info(idx) == plan
        print("plan:", plan)
        L, s, r, _, speed, gain = ir_room_np.geometry(ir_room_head_np.centred(room))
        d = float(np.sqrt(((s - r[0]) ** 2).sum()))
        plain, shadow = np.zeros((F, 2)), np.zeros((F, 2))
        for ch in range(2):
            tau = plan["direct"][ch]
            m = np.arange(int(np.floor(tau)) - 15, int(np.floor(tau)) + 17)
            plain[m, ch] = gain / d * np.sinc(m - tau) * (1.0 + np.cos(np.pi * (m - tau) / 16.0)) / 2.0
            shadow[m, ch] = plan["shadow"][ch] * plain[m, ch]
        _check_taps(got, ir_room_head_np.highpass(shadow, room, head, RATE) + plain)
    assert min(plan["shadow"]) < 0 < max(plan["shadow"])
    # a lateral source: the near ear's shelf and the far ear's, 180 degrees off its axis
    c.prepare_synth(2, _isynth(dict(ALONE, frames=4000)), room=_iroom(dict(LATERAL, gain=2.0)), head=_ihead({}))
    rsp = c.ir_response(2, hz=[100.0, 10000.0], onset_db=0.0)
    db = rsp["db"][0] - 20.0 * np.log10(2.0 / 3.0)
    print("shelf dB [ear, hz]:", db)
    np.testing.assert_allclose(db, [[0.08, 5.98], [-0.03, -10.48]], rtol=0, atol=0.05)  # (the far ear at 100 Hz: |1 - 0.7186 HP| is -0.03 dB)
    c.close()


def test_many_images_on_one_frame_give_the_same_bits(gpu_lib):
    """CROWDED: thousands of images on a few hundred frames, into two accumulators; integer sums do not depend on the order of
    arrival, and the head's pass has no atomics."""
    F = 6000
    c = _conv()
    a, _, winfo = _load_and_check(c, 0, CROWDED, GENERAL_HEAD, dict(ALONE, frames=F))
    b, _, _ = _load_and_check(c, 3, CROWDED, GENERAL_HEAD, dict(ALONE, frames=F))
    print("negative:", winfo["negative"])
    assert 0.5 <= winfo["negative"] <= 0.7 and min(winfo["images"]) > 4000
    assert _bits(c, 0) == _bits(c, 3)
    assert c.ir_info(0) == c.ir_info(3) and c.ir_room_info(0) == c.ir_room_info(3) and c.ir_room_head_info(0) == c.ir_room_head_info(3)
    c.close()


@pytest.mark.parametrize("F", [257, 16385, 40000])
def test_the_shelf_rings_on_over_long_carries(gpu_lib, F):
    """last = 3000: the accumulators end at frame 3016 (or at F) and the shelf's state carries on across every chunk boundary
    behind it, against the sequential recurrence.  (The source is half a metre from the head: its sound is there within 257 frames.)"""
    room = dict(last=3000, order=4, source=(3.0, 1.8, 1.4))
    c = _conv(65536)
    got, want, winfo = _load_and_check(c, 0, room, GENERAL_HEAD, dict(ALONE, frames=F))
    _load_and_check(c, 1, room, GENERAL_HEAD, dict(ALONE, frames=F))
    assert _bits(c, 0) == _bits(c, 1)
    A = min(winfo["last"] + 16, F)
    if F > A:
        ring = got[A:A + 64]
        print("ringing past A:", np.abs(ring).max(), "of", np.abs(got).max())
        assert (ring != 0).all() and np.abs(ring[0]).min() > 1e-6 * np.abs(got).max()
        err = ring.astype(np.float64) - want[A:A + 64]
        assert rms(err) <= 1e-6 * rms(want[A:A + 64])
    c.close()


def test_bands_join_both_accumulators(gpu_lib):
    F = 4000
    synth, room = dict(ALONE, frames=F), dict(order=3)
    c = _conv()
    got, want, _ = _load_and_check(c, 0, room, GENERAL_HEAD, synth, bands=BANDS)
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    # the same bands all equal and without air: the bits of the unbanded room with the same head, with and without a crossover
    c.prepare_synth(1, _isynth(synth), room=_iroom(room), head=_ihead(GENERAL_HEAD))
    c.prepare_synth(2, _isynth(synth), room=_iroom(room), head=_ihead(GENERAL_HEAD), bands=_ibands(dict(xovers=BANDS["xovers"])))
    c.prepare_synth(3, _isynth(synth), room=_iroom(room), head=_ihead(GENERAL_HEAD), bands=_ibands({}))
    assert _bits(c, 2) == _bits(c, 1) and _bits(c, 3) == _bits(c, 1) and _bits(c, 0) != _bits(c, 1)
    assert c.ir_room_head_info(2) == c.ir_room_head_info(1) and c.ir_room_bands_info(2)["bands"] == 3
    c.close()


def test_without_a_head_the_call_is_the_room_itself(gpu_lib):
    """head=None through mc_synth_ir_room_head against mc_synth_ir_room_bands, with and without microphones and bands."""
    from cuda_audio_amd.engine import IrRoomMics

    F = 3000
    synth, room = _isynth(dict(ALONE, frames=F, rate=RATE)).to_c(), _iroom(dict(order=3)).to_c()
    mics, bands = IrRoomMics.pair(facing=20.0, source_pattern="cardioid").to_c(), _ibands(BANDS).to_c()
    c = _conv()
    ref = lambda v: C.byref(v) if v is not None else None
    for m, b in ((None, None), (mics, None), (None, bands), (mics, bands)):
        assert c._L.mc_synth_ir_room_bands(c._h, 0, 1024, C.byref(synth), C.byref(room), ref(m), ref(b), None, None, None, None) == 0
        assert c._L.mc_synth_ir_room_head(c._h, 1, 1024, C.byref(synth), C.byref(room), ref(m), ref(b), None, None, None, None, None) == 0
        assert _bits(c, 0) == _bits(c, 1) and np.count_nonzero(c.ir_taps(0)) > 1000
        assert c.ir_info(0) == c.ir_info(1) and c.ir_room_info(0) == c.ir_room_info(1)
    c.close()


def test_a_directional_source_with_a_head(gpu_lib):
    from cuda_audio_amd._lib import McError

    F = 4000
    synth, room = dict(ALONE, frames=F), dict(order=3)
    mics = dict(source_pattern=0.366, source_az=200.0, source_el=-15.0, az=(10.0, 70.0))  # (omni ears: their aims do not matter)
    c = _conv()
    got, _, _ = _load_and_check(c, 0, room, GENERAL_HEAD, synth, mics=mics)
    c.prepare_synth(1, _isynth(synth), room=_iroom(room), head=_ihead(GENERAL_HEAD))
    assert not np.array_equal(c.ir_taps(1), got) and c.ir_room_info(1) == c.ir_room_info(0)
    before = _bits(c, 0)
    with pytest.raises(McError) as ex:
        c.prepare_synth(0, _isynth(synth), room=_iroom(room), head=_ihead(GENERAL_HEAD), mics=_imics(dict(mics, pattern=("omni", "cardioid"))))
    assert ex.value.code == -1 and "mic_pattern[1]" in str(ex.value) and _bits(c, 0) == before
    c.close()


def test_the_chain_from_the_room_through_the_floor_to_the_tail(gpu_lib):
    """test_gpu_ir_room_mics' chain with a head in the room."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, tail_from_floor

    n_ref = 65536
    synth = dict(ALONE, frames=CHAIN_F)
    c = _conv(n_ref)
    _, want_room, winfo = _load_and_check(c, 0, CHAIN_ROOM, GENERAL_HEAD, synth)
    assert winfo["order"] == 15 and winfo["complete"] >= CHAIN_F
    floor = c.ir_floor(0, margin_db=5.0)  # (the margin: see test_gpu_ir_room's chain)
    tail = tail_from_floor(floor, mode="extend", fade=256, length=48000, seed=11)
    print("tail:", tail)
    assert len(tail.knee) == 1 and tail.knee[0] is not None and CHAIN_F // 2 < tail.knee[0] < CHAIN_F, tail
    xovers, decay, origin = CHAIN_DAMP
    c.prepare_synth(0, _isynth(synth), room=_iroom(CHAIN_ROOM), head=_ihead(GENERAL_HEAD), tail=tail, shape=IrShape(**CHAIN_SHAPE), eq=IrEq(bands=list(CHAIN_BANDS)),
                    damp=IrDamp(xovers=xovers, decay=decay, origin=origin))
    got = c.ir_taps(0)
    spec = dict(xovers=tail.xovers, knee=tail.knee, t60=tail.t60, level_db=tail.level_db, fade=256, length=48000, seed=11, width=1.0)
    y, wtinfo = ir_tail_np.tail64(want_room.astype(np.float32), RATE, "extend", **spec)
    want, _, wdinfo = ir_damp_np.damped(y.astype(np.float32), n_ref - 1024, None, RATE, xovers, decay, origin, CHAIN_BANDS, **CHAIN_SHAPE)
    _check_taps(got, want.astype(np.float64))
    assert c.ir_tail_info(0) == wtinfo and wtinfo["frames"] == CHAIN_F and wtinfo["length"] == 48000
    assert c.ir_room_info(0)["images"] == winfo["images"] and c.ir_damp_info(0) == wdinfo and c.ir_shape_info(0)["taps"] == 48000
    c.close()


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrShape

    synth = dict(ALONE, frames=3000)
    room = _iroom(dict(order=3))
    c = _conv()
    c.prepare_synth(0, _isynth(synth), room=room, head=_ihead(GENERAL_HEAD), shape=IrShape(fade_out=100))
    state = lambda: (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0), c.ir_room_info(0),
                     c.ir_room_head_info(0), c.num_irs())
    before = state()
    bad = [("radius_m", dict(radius=0.2)), ("radius_m", dict(radius=float("nan"))), ("facing_az_deg", dict(facing=400.0)), ("ear_deg", dict(ear=130.0)),
           ("ear_deg", dict(ear=59.0)), ("shadow", dict(shadow=1.5)), ("shadow", dict(shadow=-0.5))]
    for name, fields in bad:
        for idx in (0, 1):  # (a loaded and a fresh index)
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), room=room, head=_ihead(fields))
            assert ex.value.code == -1 and name in str(ex.value)
    for idx in (0, 1):
        with pytest.raises(ValueError):
            c.prepare_synth(idx, _isynth(synth), head=_ihead(GENERAL_HEAD))
        s = _isynth(dict(synth, rate=RATE)).to_c()
        assert c._L.mc_synth_ir_room_head(c._h, idx, 1024, C.byref(s), None, None, None, C.byref(_ihead(GENERAL_HEAD).to_c()), None, None, None, None) == -1
        assert "the head needs a room" in c._L.mc_last_error().decode()
        with pytest.raises(McError) as ex:  # (the source inside the head)
            c.prepare_synth(idx, _isynth(synth), room=_iroom(dict(order=3, source=(3.38, 2.0, 1.5), spacing=0.0)), head=_ihead({}))
        assert ex.value.code == -1 and "source_m" in str(ex.value)
    with pytest.raises(McError) as ex:  # (a bad room with a bad head: the room is named)
        c.prepare_synth(0, _isynth(synth), room=_iroom(dict(order=33)), head=_ihead(dict(ear=10.0)))
    assert ex.value.code == -1 and "order" in str(ex.value)
    with pytest.raises(McError) as ex:
        c.ir_room_head_info(1)
    assert ex.value.code == -1  # (not loaded)
    assert state() == before and c.num_irs() == 1
    # a later load without a head forgets the head; the room still answers
    c.prepare_synth(0, _isynth(synth), room=room)
    with pytest.raises(McError) as ex:
        c.ir_room_head_info(0)
    assert ex.value.code == -3 and "head" in str(ex.value)
    assert c.ir_room_info(0)["order"] == 3
    c.prepare_synth(0, _isynth(synth), room=room, head=_ihead(GENERAL_HEAD))
    assert c.ir_room_head_info(0) == before[6]
    c.close()
