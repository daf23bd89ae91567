"""mc_ir_room_mics as ctypes sees it against what include/mcconv.h documents, the defaults field by field, and every bad field
refused by name in the struct's order, after the room and before the tail and the engine (no GPU: the library's checks touch
no device)."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
RATE = 48000
NAN, INF = float("nan"), float("inf")


def _default():
    from cuda_audio_amd import _lib

    m = _lib.McIrRoomMics()
    _lib.load().mc_default_ir_room_mics(C.byref(m))
    return m


def _mics(**fields):
    m = _default()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(m, k)[j] = x
        else:
            setattr(m, k, v)
    return m


def test_the_struct_has_its_documented_size():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_room_mics\) = (\d+)", src).group(1))
    M = _lib.McIrRoomMics
    assert C.sizeof(M) == size == _default().struct_size == 48
    offsets = dict(struct_size=0, flags=4, mic_pattern=8, mic_az_deg=16, mic_el_deg=24, src_pattern=32, src_az_deg=36, src_el_deg=40, reserved=44)
    assert {n: getattr(M, n).offset for n, _ in M._fields_} == offsets
    symbols = {"mc_default_ir_room_mics", "mc_synth_ir_room_mics", "mc_ir_room_mics_plan", "mc_ir_room_mics_info"}
    assert symbols <= set(_lib.SYMBOLS)
    for name in symbols:
        assert re.search(r"\b%s\(" % name, src), name
        getattr(_lib.load(), name)


def test_the_defaults_field_by_field():
    from cuda_audio_amd.engine import IrRoomMics

    m = _default()
    assert (m.flags, m.reserved) == (0, 0)
    assert list(m.mic_pattern) == [1.0, 1.0] and list(m.mic_az_deg) == [0.0, 0.0] and list(m.mic_el_deg) == [0.0, 0.0]
    assert (m.src_pattern, m.src_az_deg, m.src_el_deg) == (1.0, 0.0, 0.0)
    assert bytes(IrRoomMics().to_c()) == bytes(m)


def test_patterns_by_name_and_the_pair():
    from cuda_audio_amd.engine import IrRoomMics

    want = dict(omni=1.0, subcardioid=0.75, cardioid=0.5, supercardioid=0.366, hypercardioid=0.25, fig8=0.0)
    assert IrRoomMics.PATTERNS == want
    m = IrRoomMics(pattern=("cardioid", 0.3), az=(10, -20), el=5, source_pattern="fig8", source_az=7, source_el=-8).to_c()
    assert list(m.mic_pattern) == [0.5, C.c_float(0.3).value] and list(m.mic_az_deg) == [10.0, -20.0] and list(m.mic_el_deg) == [5.0, 5.0]
    assert (m.src_pattern, m.src_az_deg, m.src_el_deg) == (0.0, 7.0, -8.0)
    p = IrRoomMics.pair()  # XY: cardioids at +45 (left) and -45 (right)
    assert p.az == (45.0, -45.0) and IrRoomMics.alpha(p.pattern) == 0.5
    p = IrRoomMics.pair(facing=180.0, angle=110.0, pattern="supercardioid", source_pattern="cardioid")
    assert p.az == (235.0, 125.0) and p.source_pattern == "cardioid" and list(p.to_c().mic_pattern) == [C.c_float(0.366).value] * 2
    with pytest.raises(ValueError):
        IrRoomMics(pattern="shotgun").to_c()
    with pytest.raises(ValueError):
        IrRoomMics(az=(1, 2, 3)).to_c()


def _call(mics, room="default", tail=None, plan=False):
    """(rc, message) of mc_synth_ir_room_mics with a null engine, or of mc_ir_room_mics_plan."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrSynth

    L = _lib.load()
    r = IrRoom().to_c() if room == "default" else room
    if plan:
        out = (C.c_double * 8)()
        rc = L.mc_ir_room_mics_plan(C.byref(r) if r is not None else None, C.byref(mics) if mics is not None else None, RATE, 4000, out)
    else:
        s = IrSynth(frames=4000, rate=RATE, late_gain=0.0).to_c()
        rc = L.mc_synth_ir_room_mics(None, 0, 1024, C.byref(s), C.byref(r) if r is not None else None, C.byref(mics) if mics is not None else None, None,
                                     None, None, C.byref(tail) if tail is not None else None)
    return rc, L.mc_last_error().decode()


BAD_FIELDS = [("struct_size", dict(struct_size=44)), ("flags", dict(flags=1)), ("mic_pattern[0]", dict(mic_pattern=(-0.01,))),
              ("mic_pattern[1]", dict(mic_pattern=(1.0, 1.01))), ("mic_pattern[0]", dict(mic_pattern=(NAN,))), ("mic_az_deg[0]", dict(mic_az_deg=(361.0,))),
              ("mic_az_deg[1]", dict(mic_az_deg=(0.0, -360.5))), ("mic_az_deg[1]", dict(mic_az_deg=(0.0, INF))), ("mic_el_deg[0]", dict(mic_el_deg=(90.5,))),
              ("mic_el_deg[1]", dict(mic_el_deg=(0.0, -91.0))), ("mic_el_deg[0]", dict(mic_el_deg=(NAN,))), ("src_pattern", dict(src_pattern=1.5)),
              ("src_pattern", dict(src_pattern=NAN)), ("src_az_deg", dict(src_az_deg=400.0)), ("src_az_deg", dict(src_az_deg=-INF)),
              ("src_el_deg", dict(src_el_deg=-90.5)), ("src_el_deg", dict(src_el_deg=NAN)), ("reserved", dict(reserved=1))]


@pytest.mark.parametrize("name,fields", BAD_FIELDS)
def test_every_bad_field_is_refused_by_name(name, fields):
    for plan in (False, True):
        rc, msg = _call(_mics(**fields), plan=plan)
        assert rc == -1 and name in msg, (name, fields, plan, rc, msg)


def test_the_order_of_the_checks():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrSynth, IrTail

    # in the struct's order: of two bad fields the earlier one is named
    order = [("flags", dict(flags=2)), ("mic_pattern[0]", dict(mic_pattern=(2.0,))), ("mic_pattern[1]", dict(mic_pattern=(1.0, 2.0))),
             ("mic_az_deg[0]", dict(mic_az_deg=(999.0,))), ("mic_az_deg[1]", dict(mic_az_deg=(0.0, 999.0))), ("mic_el_deg[0]", dict(mic_el_deg=(99.0,))),
             ("mic_el_deg[1]", dict(mic_el_deg=(0.0, 99.0))), ("src_pattern", dict(src_pattern=-1.0)), ("src_az_deg", dict(src_az_deg=999.0)),
             ("src_el_deg", dict(src_el_deg=99.0)), ("reserved", dict(reserved=7))]
    for (first, a), (_, b) in zip(order, order[1:]):
        fields = dict(b)
        for k, v in a.items():  # (two entries of one array: the earlier entry's value stays)
            fields[k] = v + fields[k][len(v):] if isinstance(v, tuple) and k in fields else v
        rc, msg = _call(_mics(**fields))
        assert rc == -1 and first in msg, (first, msg)
    bad = _mics(src_el_deg=99.0)
    # the room comes before the microphones, the microphones before the tail, the synthesis before everything
    rc, msg = _call(bad, room=IrRoom(order=40).to_c())
    assert rc == -1 and "order" in msg, msg
    bad_tail = IrTail(mode="extend", knee=(100,), t60=(0,)).to_c()
    rc, msg = _call(bad, tail=bad_tail)
    assert rc == -1 and "src_el_deg" in msg, msg
    rc, msg = _call(_default(), tail=bad_tail)
    assert rc == -1 and "t60" in msg, msg
    L = _lib.load()
    s = IrSynth(frames=0, rate=RATE).to_c()
    assert L.mc_synth_ir_room_mics(None, 0, 1024, C.byref(s), None, C.byref(bad), None, None, None, None) == -1
    assert "frames" in L.mc_last_error().decode()
    # microphones without a room
    rc, msg = _call(_default(), room=None)
    assert rc == -1 and "the microphones need a room" in msg, msg
    rc, msg = _call(_default(), room=None, plan=True)
    assert rc == -1 and "null room" in msg, msg
    rc, msg = _call(None, plan=True)
    assert rc == -1 and "null mics" in msg, msg
    # the good edges pass the microphones and stop at the engine, which is null
    for fields in (dict(), dict(mic_pattern=(0.0, 1.0)), dict(mic_az_deg=(-360.0, 360.0)), dict(mic_el_deg=(-90.0, 90.0)), dict(src_pattern=0.0),
                   dict(src_az_deg=360.0, src_el_deg=90.0), dict(src_az_deg=-360.0, src_el_deg=-90.0)):
        rc, msg = _call(_mics(**fields))
        assert rc == -1 and "null" in msg and "mics" not in msg, (fields, msg)
        rc, msg = _call(_mics(**fields), plan=True)
        assert rc == 0, (fields, msg)
    # without microphones the call is mc_synth_ir_room: its own refusals, in its own words
    rc, msg = _call(None, room=IrRoom(order=40).to_c())
    assert rc == -1 and "order" in msg, msg
    rc, msg = _call(None)
    assert rc == -1 and "null" in msg, msg
