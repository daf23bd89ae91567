"""Walls and air per frequency band in the room on the device (mc_synth_ir_room_bands; k_room's air instantiations, k_room_join
and k_synth_room_bands of csrc/irroom.hip.h): the stored taps against the float64 restatement (tests/ir_room_bands_np.py), the
parts of the definition that are exact (equal bands store the bits of the unbanded room, two loads store the same bits, the kept
counts stay the room's), the edges of the join's chunks and its carries across workgroups, what the feature is for (T30 per band
follows the walls and the air), the chain through ir_floor and the tail step, and the refusals.

The bar for taps is test_gpu_ir_shape._check_taps, for the reason tests/test_gpu_ir_room.py gives; the air factor adds one double
exp2 and one multiply per image and channel, and the join a recurrence in double whose chunked form is within 2e-9 relative RMS
of the sequential one.  Before every comparison of counts the restatement asserts that no delay lies where a rounding
could move its floor (ir_room_np.assert_floor_margin)."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_decay_np
import ir_room_bands_np
import ir_room_np
import ir_tail_np
from helpers import rms
from test_gpu_ir_eq import _check_sums_and_spectra
from test_gpu_ir_room import ALONE, CHAIN_BANDS, CHAIN_DAMP, CHAIN_F, CHAIN_ROOM, CHAIN_SHAPE, CROWDED, RATE, _conv, _freeze, _iroom, _isynth
from test_gpu_ir_room_mics import _imics
from test_gpu_ir_shape import _check_taps
from test_ir_room_mics_cpu import GENERAL

pytestmark = pytest.mark.gpu

# three bands, different walls per band and wall, one of them negative; no air, a little, more
GENERAL_BANDS = dict(xovers=(500.0, 2000.0), beta=((0.95, 0.9, 0.92, 0.97, 0.85, 0.9), (0.85, -0.8, 0.7, 0.9, 0.6, 0.8), (0.6, 0.5, 0.55, 0.7, 0.3, 0.45)),
                     air=(0.0, 0.005, 0.03))
NEAR = dict(source=(1.0, 1.5, 1.2), receiver=(1.3, 1.5, 1.2), spacing=0.2, gain=0.05)  # (test_lengths' receiver: the direct sound at 28 and 56 frames)


def _ibands(fields):
    from cuda_audio_amd.engine import IrRoomBands

    return IrRoomBands(**fields)


@functools.lru_cache(maxsize=None)
def _restated_cached(room, mics, bands, synth):
    room, bands, synth = dict(room), dict(bands), dict(synth)
    out, covered, info = ir_room_bands_np.frames64(room, dict(mics) if mics is not None else None, bands, RATE, **synth)
    for a in (out, covered):
        a.setflags(write=False)
    return out, covered, info


def _restated(room, mics, bands, synth):
    """(frames float64 [F, 2], covered, info with every tau) of a banded room over a synthesis, computed once."""
    return _restated_cached(_freeze(room), _freeze(mics) if mics is not None else None, _freeze(bands), _freeze(synth))


def _load_and_check(c, idx, room, mics, bands, synth, **kw):
    """Load, then the taps, the room's information and the kept counts against the restatement."""
    want, _, winfo = _restated(room, mics, bands, synth)
    ir_room_np.assert_floor_margin(winfo["tau"], winfo["last"])
    c.prepare_synth(idx, _isynth(synth), room=_iroom(room), mics=_imics(mics) if mics is not None else None, bands=_ibands(bands), **kw)
    got = c.ir_taps(idx)
    w = want[:len(got)]
    err = got.astype(np.float64) - w
    print(f"relative rms {rms(err) / rms(w):.2e}")
    _check_taps(got, w)
    info = c.ir_room_info(idx)
    assert info["order"] == winfo["order"] and info["images"] == winfo["images"] and info["last"] == winfo["last"] and info["complete"] == winfo["complete"]
    np.testing.assert_allclose(info["direct"], winfo["direct"], rtol=1e-14, atol=0)
    return got, w, winfo


def _bits(c, idx):
    return c.ir_taps(idx).tobytes(), c.ir_spectra(idx).tobytes()


@pytest.mark.parametrize("mics", [None, GENERAL], ids=["omni", "mics"])
@pytest.mark.parametrize("order", [2, 6])
def test_the_general_case_matches_the_restatement(gpu_lib, order, mics):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import room_bands_plan

    F = 4000
    synth, room = dict(ALONE, frames=F), dict(order=order)
    c = _conv()
    got, want, winfo = _load_and_check(c, 0, room, mics, GENERAL_BANDS, synth)
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    assert c.ir_room_bands_info(0) == room_bands_plan(_iroom(room), _ibands(GENERAL_BANDS), RATE, F)
    # the counts, the delays and E are the room's, whatever the bands
    c.prepare_synth(1, _isynth(synth), room=_iroom(room), mics=_imics(mics) if mics is not None else None)
    assert c.ir_room_info(1) == c.ir_room_info(0)
    assert not np.array_equal(c.ir_taps(1), got)
    with pytest.raises(McError) as ex:
        c.ir_room_bands_info(1)
    assert ex.value.code == -3
    if mics is not None:
        assert c.ir_room_mics_info(0) == c.ir_room_mics_info(1)
    c.close()


def test_equal_bands_store_the_bits_of_the_unbanded_room(gpu_lib):
    F = 4000
    beta = (0.9, -0.8, 0.7, 0.95, 0.6, 1.0)
    synth = dict(frames=F, seed=21, late_start=500, t60=3000, build_up=200, late_gain=0.02, direct=1.0, n_early=4, early_first=50, early_last=400)
    room = dict(order=4, beta=beta, last=3000)  # (frames past E + 16 hold the synthesis alone, plus the join's +0.0)
    c = _conv()
    for mics in (None, GENERAL):
        m = _imics(mics) if mics is not None else None
        c.prepare_synth(0, _isynth(synth), room=_iroom(room), mics=m)
        want = _bits(c, 0)
        # bands = NULL through the new entry point
        s, r = _isynth(dict(synth, rate=RATE)).to_c(), _iroom(room).to_c()
        mc = m.to_c() if m is not None else None
        assert c._L.mc_synth_ir_room_bands(c._h, 1, 1024, C.byref(s), C.byref(r), C.byref(mc) if mc is not None else None, None, None, None, None, None) == 0
        assert _bits(c, 1) == want
        # one band with the room's walls; three equal bands; the room's own beta is not what is rendered
        for idx, bands in ((2, dict(beta=(beta,))), (3, dict(xovers=(300.0, 3000.0), beta=(beta,) * 3))):
            c.prepare_synth(idx, _isynth(synth), room=_iroom(dict(room, beta=0.1)), mics=m, bands=_ibands(bands))
            assert _bits(c, idx) == want, (mics, bands)
            assert c.ir_info(idx) == c.ir_info(0) and c.ir_room_info(idx) == c.ir_room_info(0)
        c.prepare_synth(4, _isynth(synth), room=_iroom(room), mics=m, bands=_ibands(dict(xovers=(300.0,), beta=(beta, beta), air=(0.0, 0.01))))
        assert _bits(c, 4) != want
    c.close()


def test_two_loads_store_the_same_bits(gpu_lib):
    F = 6000
    synth = dict(ALONE, frames=F)
    c = _conv()
    a, _, _ = _load_and_check(c, 0, dict(order=5), GENERAL, GENERAL_BANDS, synth)
    c.prepare_synth(1, _isynth(synth), room=_iroom(dict(order=5)), mics=_imics(GENERAL), bands=_ibands(GENERAL_BANDS))
    assert _bits(c, 0) == _bits(c, 1) and c.ir_info(0) == c.ir_info(1)
    # the crowded cube: dozens of images on one frame, in every band
    bands = dict(xovers=(1000.0,), beta=(0.9, 0.7), air=(0.0, 0.02))
    _load_and_check(c, 2, CROWDED, None, bands, synth)
    c.prepare_synth(3, _isynth(synth), room=_iroom(CROWDED), bands=_ibands(bands))
    assert _bits(c, 2) == _bits(c, 3) and c.ir_info(2) == c.ir_info(3) and c.ir_room_info(2) == c.ir_room_info(3)
    c.close()


@pytest.mark.parametrize("F", [1, 2, 255, 256, 257, 16383, 16384, 16385])
def test_the_edges_of_the_join(gpu_lib, F):
    """A lone frame, a pair, a chunk of the join and a frame either side, a workgroup's span and a frame either side.  Order 10
    keeps the restatement quick and still has images arriving up to the last frame."""
    room = dict(NEAR, order=10)
    synth = dict(frames=F, seed=99, late_start=0, t60=500, build_up=40, late_gain=0.01, direct=0.5, n_early=3, early_first=0, early_last=max(F - 1, 0),
                 early_gain=0.25, width=0.6)
    c = _conv(32768)
    got, want, _ = _load_and_check(c, 0, room, None, dict(xovers=(200.0,), beta=(0.9, 0.6)), synth)
    assert len(got) == F and c.ir_shape_info(0)["frames"] == F
    _check_sums_and_spectra(c, 0, got, want.astype(np.float32))
    c.close()


def test_carries_across_workgroups(gpu_lib):
    """40 000 frames are three workgroups of the join and 157 chunks, runs of two in the carry pass.  The accumulators end at
    12 016: frames [16384, 20000) hold only what a 20 Hz crossover carried across a workgroup's boundary."""
    F, last = 40000, 12000
    room, bands, synth = dict(last=last, gain=0.2), dict(xovers=(20.0,), beta=(0.9, 0.6)), dict(ALONE, frames=F)
    want, _, winfo = _restated(room, None, bands, synth)
    seg = slice(16384, 20000)
    print(f"rms of the whole IR {rms(want):.3e}, of frames [16384, 20000) {rms(want[seg]):.3e}")
    assert winfo["last"] == last and rms(want[seg]) > 1e-6 * rms(want)
    c = _conv(65536)
    got, w, _ = _load_and_check(c, 0, room, None, bands, synth)
    c.close()
    assert len(got) == F
    _check_taps(got[seg], w[seg])


T30_BANDS = (160.0, 1000.0, 6000.0)  # centred below, between and above the crossovers at 500 and 2000 Hz


@pytest.mark.parametrize("bands", [dict(xovers=(500.0, 2000.0), beta=(0.8, 0.65, 0.5)), dict(xovers=(500.0, 2000.0), beta=0.8, air=(0.0, 0.15, 0.4))],
                         ids=["walls", "air"])
def test_t30_per_band_follows_the_walls_and_the_air(gpu_lib, bands):
    F = 9000
    room, synth = dict(gain=0.2), dict(ALONE, frames=F)
    want, _, _ = _restated(room, None, bands, synth)
    wd = ir_decay_np.decay(want.astype(np.float32), RATE, bands=T30_BANDS)
    ir_decay_np.assert_margins(wd)
    c = _conv()
    _load_and_check(c, 0, room, None, bands, synth)
    gd = c.ir_decay(0, bands=T30_BANDS)
    c.close()
    got = [gd["rows"][(b, "LR")]["t30"] for b in (1, 2, 3)]
    restated = [wd["rows"][(b, "LR")]["t30"] for b in (1, 2, 3)]
    print("T30 per band on the device:", got, "restated:", restated)
    assert got[0] > got[1] > got[2] > 0 and restated[0] > restated[1] > restated[2] > 0
    np.testing.assert_allclose(got, restated, rtol=1e-6, atol=0)  # (test_gpu_ir_decay.py's tolerance for times)


def test_the_chain_from_the_banded_room_through_the_floor_to_the_tail(gpu_lib):
    """test_the_chain_from_the_room_through_the_floor_to_the_tail with two bands: the floor is found per band of the same split,
    and each band of the tail continues at its own measured slope."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, tail_from_floor

    n_ref = 65536
    xovers = (1000.0,)
    # (walls at 0.8 and 0.7: tests/ir_floor_np.py finds both bands' knees inside the quarter second, near 11 500, with decay times of
    # 0.34 and 0.31 s; at 0.9 the lower band's line crosses past the last frame and that band would be left alone)
    bands = dict(xovers=xovers, beta=(0.8, 0.7), air=(0.0, 0.01))
    synth = dict(ALONE, frames=CHAIN_F)
    c = _conv(n_ref)
    _, want_room, winfo = _load_and_check(c, 0, CHAIN_ROOM, None, bands, synth)
    assert winfo["order"] == 15 and winfo["complete"] >= CHAIN_F
    floor = c.ir_floor(0, xovers=xovers, margin_db=5.0)
    tail = tail_from_floor(floor, mode="extend", fade=256, length=48000, seed=11)
    print("tail:", tail)
    assert tail.xovers == xovers and len(tail.knee) == 2 and all(k is not None and CHAIN_F // 2 < k < CHAIN_F for k in tail.knee), tail
    assert 0 < tail.t60[1] < tail.t60[0] < RATE  # (the band with the softer walls and the air decays faster)
    dx, decay, origin = CHAIN_DAMP
    c.prepare_synth(0, _isynth(synth), room=_iroom(CHAIN_ROOM), bands=_ibands(bands), tail=tail, shape=IrShape(**CHAIN_SHAPE), eq=IrEq(bands=list(CHAIN_BANDS)),
                    damp=IrDamp(xovers=dx, decay=decay, origin=origin))
    got = c.ir_taps(0)
    spec = dict(xovers=tail.xovers, knee=tail.knee, t60=tail.t60, level_db=tail.level_db, fade=256, length=48000, seed=11, width=1.0)
    y, wtinfo = ir_tail_np.tail64(want_room.astype(np.float32), RATE, "extend", **spec)
    want, _, wdinfo = ir_damp_np.damped(y.astype(np.float32), n_ref - 1024, None, RATE, dx, decay, origin, CHAIN_BANDS, **CHAIN_SHAPE)
    _check_taps(got, want.astype(np.float64))
    assert c.ir_tail_info(0) == wtinfo and wtinfo["frames"] == CHAIN_F and wtinfo["length"] == 48000
    assert c.ir_room_info(0)["images"] == winfo["images"] and c.ir_room_bands_info(0)["bands"] == 2
    assert c.ir_damp_info(0) == wdinfo and c.ir_shape_info(0)["taps"] == 48000
    c.close()


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrTail
    from cuda_audio_amd.synth import make_ir

    synth = dict(ALONE, frames=3000)
    good = dict(xovers=(800.0,), beta=(0.9, 0.7), air=(0.0, 0.01))
    c = _conv()
    c.prepare_synth(0, _isynth(synth), room=_iroom(dict(order=3)), mics=_imics(GENERAL), bands=_ibands(good))
    state = lambda: (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0), c.ir_room_info(0),
                     c.ir_room_mics_info(0), c.ir_room_bands_info(0), c.num_irs())
    before = state()
    assert c.ir_room_bands_info(0)["bands"] == 2 and c.ir_room_bands_info(0)["xovers"] == (800.0,)
    bad_bands = [("xover_hz[0]", dict(xovers=(5.0,), beta=(0.9, 0.7))), ("xover_hz[1]", dict(xovers=(800.0, 700.0), beta=0.9)),
                 ("xover_hz[0]", dict(xovers=(0.46 * RATE,), beta=0.9)), ("beta[1][0]", dict(xovers=(800.0,), beta=(0.9, 1.2))),
                 ("air_db_per_m[1]", dict(xovers=(800.0,), air=(0.0, 1.5))), ("air_db_per_m[0]", dict(air=-0.1))]
    for name, fields in bad_bands:
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), room=_iroom(dict(order=2)), bands=_ibands(fields))
            assert ex.value.code == -1 and name in str(ex.value), (name, str(ex.value))
    for kw in (dict(room=_iroom(dict(order=33))), dict(mics=_imics(dict(el=(0, 91)))), dict(tail=IrTail(mode="extend", knee=(100,), t60=(0,))), dict(nframes=16384)):
        kw.setdefault("room", _iroom(dict(order=2)))
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), bands=_ibands(good), **kw)
            assert ex.value.code == -1
    with pytest.raises(McError) as ex:
        c.ir_room_bands_info(1)
    assert ex.value.code == -1
    assert state() == before
    # a load without bands over the index forgets them
    c.prepare_synth(0, _isynth(synth), room=_iroom(dict(order=2)))
    with pytest.raises(McError) as ex:
        c.ir_room_bands_info(0)
    assert ex.value.code == -3 and c.ir_room_info(0)["order"] == 2
    c.prepare_synth(0, _isynth(synth), room=_iroom(dict(order=2)), bands=_ibands(good))
    assert c.ir_room_bands_info(0)["bands"] == 2
    c.prepare(0, make_ir(3000, seed=2, norm=0.05))
    with pytest.raises(McError) as ex:
        c.ir_room_bands_info(0)
    assert ex.value.code == -3
    c.close()
