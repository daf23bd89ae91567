"""mc_ir_room_head as ctypes sees it against what include/mcconv.h documents, the defaults field by field, every bad field
refused by name in the documented order, after the bands and before the tail and the engine, and mc_ir_room_head_plan against
the restatement (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ir_room_head_np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
RATE = 48000
NAN, INF = float("nan"), float("inf")


def _default():
    from cuda_audio_amd import _lib

    h = _lib.McIrRoomHead()
    _lib.load().mc_default_ir_room_head(C.byref(h))
    return h


def _head(**fields):
    h = _default()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(h, k)[j] = x
        else:
            setattr(h, k, v)
    return h


def test_the_struct_has_its_documented_size():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_room_head\) = (\d+)", src).group(1))
    M = _lib.McIrRoomHead
    assert C.sizeof(M) == size == _default().struct_size == 32
    offsets = dict(struct_size=0, flags=4, radius_m=8, facing_az_deg=12, ear_deg=16, shadow=20, reserved=24)
    assert {n: getattr(M, n).offset for n, _ in M._fields_} == offsets
    symbols = {"mc_default_ir_room_head", "mc_synth_ir_room_head", "mc_ir_room_head_plan", "mc_ir_room_head_info"}
    assert symbols <= set(_lib.SYMBOLS)
    for name in symbols:
        assert re.search(r"\b%s\(" % name, src), name
        getattr(_lib.load(), name)


def test_the_defaults_field_by_field():
    from cuda_audio_amd.engine import IrRoomHead

    h = _default()
    assert (h.flags, list(h.reserved)) == (0, [0, 0])
    assert (h.radius_m, h.facing_az_deg, h.ear_deg, h.shadow) == (C.c_float(0.0875).value, 0.0, 90.0, 1.0)
    assert bytes(IrRoomHead().to_c()) == bytes(h)
    assert "100" in re.search(r"float ear_deg;[^\n]*", open(HEADER).read()).group(0)  # (Brown and Duda's own placement is documented)


def _call(head, room="default", mics=None, bands=None, tail=None, plan=False, rate=RATE, frames=4000):
    """(rc, message) of mc_synth_ir_room_head with a null engine, or of mc_ir_room_head_plan."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrSynth

    L = _lib.load()
    r = IrRoom().to_c() if room == "default" else room
    ref = lambda v: C.byref(v) if v is not None else None
    if plan:
        out = (C.c_double * 12)()
        rc = L.mc_ir_room_head_plan(ref(r), ref(head), rate, frames, out)
    else:
        s = IrSynth(frames=frames, rate=rate, late_gain=0.0).to_c()
        rc = L.mc_synth_ir_room_head(None, 0, 1024, C.byref(s), ref(r), ref(mics), ref(bands), ref(head), None, None, None, ref(tail))
    return rc, L.mc_last_error().decode()


BAD_FIELDS = [("struct_size", dict(struct_size=28)), ("radius_m", dict(radius_m=0.049)), ("radius_m", dict(radius_m=0.151)), ("radius_m", dict(radius_m=NAN)),
              ("facing_az_deg", dict(facing_az_deg=360.5)), ("facing_az_deg", dict(facing_az_deg=-INF)), ("ear_deg", dict(ear_deg=59.0)),
              ("ear_deg", dict(ear_deg=121.0)), ("ear_deg", dict(ear_deg=NAN)), ("shadow", dict(shadow=-0.01)), ("shadow", dict(shadow=1.01)),
              ("shadow", dict(shadow=NAN)), ("flags", dict(flags=1)), ("reserved[0]", dict(reserved=(1,))), ("reserved[1]", dict(reserved=(0, 5)))]


@pytest.mark.parametrize("name,fields", BAD_FIELDS)
def test_every_bad_field_is_refused_by_name(name, fields):
    for plan in (False, True):
        rc, msg = _call(_head(**fields), plan=plan)
        assert rc == -1 and name in msg and "head" in msg, (name, fields, plan, rc, msg)


def test_the_order_of_the_checks():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrRoomBands, IrRoomMics, IrSynth, IrTail

    # in the documented order: of two bad fields the earlier one is named
    order = [("radius_m", dict(radius_m=1.0)), ("facing_az_deg", dict(facing_az_deg=400.0)), ("ear_deg", dict(ear_deg=10.0)), ("shadow", dict(shadow=2.0)),
             ("flags", dict(flags=2)), ("reserved[0]", dict(reserved=(7, 0))), ("reserved[1]", dict(reserved=(0, 7)))]
    for (first, a), (_, b) in zip(order, order[1:]):
        fields = dict(b)
        fields.update({k: (v[0], fields[k][1]) if isinstance(v, tuple) and k in fields else v for k, v in a.items()})
        rc, msg = _call(_head(**fields))
        assert rc == -1 and first in msg, (first, msg)
    # what follows from the fields comes after them, in this order: the corner, the distance, the order, the sum, the microphones
    fast = IrRoom(speed=1000.0, source=(3.38, 2.0, 1.5), spacing=0.0).to_c()  # (0.12 m from the centre: the room passes it, no head does)
    rc, msg = _call(_head(radius_m=0.05, reserved=(0, 1)), room=fast, rate=8000, frames=400)
    assert rc == -1 and "reserved[1]" in msg, msg
    rc, msg = _call(_head(radius_m=0.05), room=fast, rate=8000, frames=400)
    assert rc == -1 and "corner lies above the rate" in msg, msg
    rc, msg = _call(_head(radius_m=0.05), room=fast, rate=48000, frames=400)
    assert rc == -1 and "source_m" in msg and "radius_m" in msg, msg
    for plan in (False, True):
        rc, msg = _call(_head(radius_m=0.15), room=IrRoom(source=(3.3, 2.0, 1.5), spacing=0.0).to_c(), plan=plan)  # (0.2 m: the room passes it)
        assert rc == -1 and "source_m" in msg and "radius_m" in msg, msg
    rc, msg = _call(_head(radius_m=0.15), room=IrRoom(source=(3.2, 2.0, 1.5), spacing=0.0).to_c(), mics=IrRoomMics(pattern=0.5).to_c())
    assert rc == -1 and "mic_pattern[0]" in msg, msg  # (0.3 m is far enough: the microphones' patterns are looked at last)
    # the automatic order is the head's: 32 covers 26 869 frames of the default room without a head and 26 857 with this one
    room = IrRoom().to_c()
    assert _call(None, room=room, frames=26865)[1].count("null") and _call(_head(), room=room, frames=26850, plan=True)[0] == 0
    rc, msg = _call(_head(), room=room, frames=26865, plan=True)
    assert rc == -1 and "order 0 needs order 33" in msg and "head" in msg, msg
    # the sum's bound takes the head's order and the centre's distance
    # (8390 frames: order 10 without a head, 74 088 images, and 11 with one, 97 336; at 0.3 m a gain of 15 lies between the two bounds)
    near = IrRoom(source=(3.2, 2.0, 1.5), spacing=0.0, gain=15.0).to_c()
    assert _call(None, room=near, frames=8390)[1].count("null")
    rc, msg = _call(_head(), room=near, frames=8390, plan=True)
    assert rc == -1 and "gain" in msg and "97336 images" in msg, msg
    # ears are not microphones
    for pattern, name in (((0.5, 1.0), "mic_pattern[0]"), ((1.0, 0.0), "mic_pattern[1]")):
        rc, msg = _call(_head(), mics=IrRoomMics(pattern=pattern, source_pattern="cardioid").to_c())
        assert rc == -1 and name in msg and "head" in msg, msg
    rc, msg = _call(_head(), mics=IrRoomMics(source_pattern="cardioid", source_az=30.0, az=(20.0, 50.0)).to_c())
    assert rc == -1 and "null" in msg, msg
    rc, msg = _call(_head(shadow=3.0), mics=IrRoomMics(pattern=0.5).to_c())
    assert rc == -1 and "shadow" in msg, msg
    bad = _head(reserved=(9, 0))
    # the room, the microphones and the bands come before the head, the head before the tail, the synthesis before everything
    rc, msg = _call(bad, room=IrRoom(order=40).to_c())
    assert rc == -1 and "order" in msg and "head" not in msg, msg
    rc, msg = _call(bad, mics=IrRoomMics(el=(0, 91)).to_c())
    assert rc == -1 and "mic_el_deg[1]" in msg, msg
    rc, msg = _call(bad, bands=IrRoomBands(air=2.0).to_c())
    assert rc == -1 and "air_db_per_m[0]" in msg, msg
    bad_tail = IrTail(mode="extend", knee=(100,), t60=(0,)).to_c()
    rc, msg = _call(bad, tail=bad_tail)
    assert rc == -1 and "head reserved[0]" in msg, msg
    rc, msg = _call(_head(), tail=bad_tail)
    assert rc == -1 and "t60" in msg, msg
    L = _lib.load()
    s = IrSynth(frames=0, rate=RATE).to_c()
    assert L.mc_synth_ir_room_head(None, 0, 1024, C.byref(s), None, None, None, C.byref(bad), None, None, None, None) == -1
    assert "frames" in L.mc_last_error().decode()
    # a head without a room
    rc, msg = _call(_default(), room=None)
    assert rc == -1 and "the head needs a room" in msg, msg
    rc, msg = _call(_default(), room=None, bands=IrRoomBands().to_c())
    assert rc == -1 and "the bands need a room" in msg, msg
    rc, msg = _call(_default(), room=None, plan=True)
    assert rc == -1 and "null room" in msg, msg
    rc, msg = _call(None, plan=True)
    assert rc == -1 and "null head" in msg, msg
    # the spacing is still checked with a head, though it is not used
    rc, msg = _call(_default(), room=IrRoom(spacing=4.0).to_c())
    assert rc == -1 and "spacing_m" in msg and "head" not in msg, msg
    # the good edges pass the head and stop at the engine, which is null
    for fields in (dict(), dict(radius_m=0.05), dict(radius_m=0.15), dict(facing_az_deg=-360.0, ear_deg=60.0), dict(facing_az_deg=360.0, ear_deg=120.0),
                   dict(shadow=0.0)):
        rc, msg = _call(_head(**fields))
        assert rc == -1 and "null" in msg and "head" not in msg, (fields, msg)
        rc, msg = _call(_head(**fields), plan=True)
        assert rc == 0, (fields, msg)
    # without a head the call is mc_synth_ir_room_bands: its own refusals, in its own words
    rc, msg = _call(None, room=IrRoom(order=40).to_c())
    assert rc == -1 and "order" in msg, msg
    rc, msg = _call(None, bands=IrRoomBands(air=2.0).to_c())
    assert rc == -1 and "air_db_per_m[0]" in msg, msg
    rc, msg = _call(None)
    assert rc == -1 and "null" in msg, msg


def test_a_head_without_a_room_raises():
    from cuda_audio_amd.engine import Convolution, IrRoomHead, IrSynth

    with pytest.raises(ValueError) as ex:  # (before the engine is looked at: no engine is needed to see it)
        Convolution.prepare_synth(None, 0, IrSynth(frames=100, rate=RATE), head=IrRoomHead())
    assert "needs a room" in str(ex.value)


PLAN_CASES = [({}, {}, 48000, 4000), ({}, dict(facing=35.0, ear=100.0), 48000, 4000), (dict(order=6), dict(radius=0.07, facing=-140.0, ear=75.0, shadow=0.5), 44100, 3000),
              (dict(size=(9.0, 6.5, 2.8), speed=331.0, source=(2.0, 5.5, 2.2), receiver=(6.0, 1.5, 1.1)), dict(radius=0.15, facing=200.0, ear=120.0), 96000, 9000),
              (dict(gain=0.2), {}, 48000, 12000), (dict(beta=0.0), dict(radius=0.05, shadow=0.0), 8000, 500)]


@pytest.mark.parametrize("room,head,rate,F", PLAN_CASES)
def test_the_plan_against_the_restatement(room, head, rate, F):
    """The delays are a fused multiply-add and two more roundings of numbers near 500; an angle is an arc cosine away from its
    ends; a shadow factor is a cosine of it: 1e-13 relative, 1e-10 degrees and 1e-13 absolute are hundreds of ulp each."""
    from cuda_audio_amd.engine import IrRoom, IrRoomHead, room_head_plan

    got = room_head_plan(IrRoom(**room), IrRoomHead(**head), rate, F)
    want = ir_room_head_np.plan(room, head, rate, F)
    print(got, want)
    assert set(got) == set(want)
    assert got["order"] == want["order"] and got["complete"] == want["complete"]
    np.testing.assert_allclose(got["direct"], want["direct"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["itd"], want["itd"], rtol=0, atol=1e-13 * max(want["direct"]) / rate)
    np.testing.assert_allclose(got["angle"], want["angle"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(got["shadow"], want["shadow"], rtol=0, atol=1e-13)
    np.testing.assert_allclose([got["corner"], got["k"]], [want["corner"], want["k"]], rtol=1e-14, atol=0)
    assert -0.9 * ir_room_head_np.spec(**head)["shadow"] - 1e-12 <= min(got["shadow"]) and max(got["shadow"]) <= 1.0
    assert got["complete"] >= (F if not room.get("order") else 0)
