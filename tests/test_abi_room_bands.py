"""mc_ir_room_bands as ctypes sees it against what include/mcconv.h documents, the defaults field by field, every bad field
refused by name in the struct's order, after the microphones and before the tail and the engine, and mc_ir_room_bands_plan
against the restatement (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ir_room_bands_np

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
RATE = 48000
NAN, INF = float("nan"), float("inf")


def _default():
    from cuda_audio_amd import _lib

    b = _lib.McIrRoomBands()
    _lib.load().mc_default_ir_room_bands(C.byref(b))
    return b


def _bands(**fields):
    """The defaults with three crossovers at 250, 1000 and 4000 Hz (every entry of the arrays in use), then `fields`: a tuple
    sets the first entries of an array, a dict {(j, w): v} entries of beta."""
    b = _default()
    b.n_xovers = 3
    for k, hz in enumerate((250.0, 1000.0, 4000.0)):
        b.xover_hz[k] = hz
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(b, k)[j] = x
        elif isinstance(v, dict):
            for (j, w), x in v.items():
                getattr(b, k)[j][w] = x
        else:
            setattr(b, k, v)
    return b


def test_the_struct_has_its_documented_size():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_room_bands\) = (\d+)", src).group(1))
    M = _lib.McIrRoomBands
    assert C.sizeof(M) == size == _default().struct_size == 140
    offsets = dict(struct_size=0, n_xovers=4, xover_hz=8, beta=20, air_db_per_m=116, flags=132, reserved=136)
    assert {n: getattr(M, n).offset for n, _ in M._fields_} == offsets
    symbols = {"mc_default_ir_room_bands", "mc_synth_ir_room_bands", "mc_ir_room_bands_plan", "mc_ir_room_bands_info"}
    assert symbols <= set(_lib.SYMBOLS)
    for name in symbols:
        assert re.search(r"\b%s\(" % name, src), name
        getattr(_lib.load(), name)


def test_the_defaults_field_by_field():
    from cuda_audio_amd.engine import IrRoomBands

    b = _default()
    assert (b.n_xovers, b.flags, b.reserved) == (0, 0, 0)
    assert list(b.xover_hz) == [0.0] * 3 and list(b.air_db_per_m) == [0.0] * 4
    assert [list(r) for r in b.beta] == [[C.c_float(0.9).value] * 6] * 4
    assert bytes(IrRoomBands().to_c()) == bytes(b)


def _call(bands, room="default", mics=None, tail=None, plan=False, rate=RATE):
    """(rc, message) of mc_synth_ir_room_bands with a null engine, or of mc_ir_room_bands_plan."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrSynth

    L = _lib.load()
    r = IrRoom().to_c() if room == "default" else room
    ref = lambda v: C.byref(v) if v is not None else None
    if plan:
        out = (C.c_double * 16)()
        rc = L.mc_ir_room_bands_plan(ref(r), ref(bands), rate, 4000, out)
    else:
        s = IrSynth(frames=4000, rate=rate, late_gain=0.0).to_c()
        rc = L.mc_synth_ir_room_bands(None, 0, 1024, C.byref(s), ref(r), ref(mics), ref(bands), None, None, None, ref(tail))
    return rc, L.mc_last_error().decode()


BAD_FIELDS = [("struct_size", dict(struct_size=136)), ("n_xovers", dict(n_xovers=4)), ("xover_hz[0]", dict(xover_hz=(9.0,))),
              ("xover_hz[0]", dict(xover_hz=(NAN,))), ("xover_hz[1]", dict(xover_hz=(250.0, 250.0))), ("xover_hz[1]", dict(xover_hz=(250.0, 100.0))),
              ("xover_hz[2]", dict(xover_hz=(250.0, 1000.0, 0.45 * RATE + 1.0))), ("xover_hz[2]", dict(xover_hz=(250.0, 1000.0, INF))),
              ("beta[0][0]", dict(beta={(0, 0): 1.01})), ("beta[1][5]", dict(beta={(1, 5): -1.5})), ("beta[2][3]", dict(beta={(2, 3): NAN})),
              ("beta[3][1]", dict(beta={(3, 1): INF})), ("air_db_per_m[0]", dict(air_db_per_m=(-0.001,))), ("air_db_per_m[1]", dict(air_db_per_m=(0.0, 1.5))),
              ("air_db_per_m[2]", dict(air_db_per_m=(0.0, 0.0, NAN))), ("air_db_per_m[3]", dict(air_db_per_m=(0.0, 0.0, 0.0, INF))), ("flags", dict(flags=1)),
              ("reserved", dict(reserved=1))]


@pytest.mark.parametrize("name,fields", BAD_FIELDS)
def test_every_bad_field_is_refused_by_name(name, fields):
    for plan in (False, True):
        rc, msg = _call(_bands(**fields), plan=plan)
        assert rc == -1 and name in msg and "bands" in msg, (name, fields, plan, rc, msg)


def test_the_order_of_the_checks():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrRoomMics, IrSynth, IrTail

    # in the struct's order: of two bad fields the earlier one is named
    order = [("n_xovers", dict(n_xovers=7)), ("xover_hz[0]", dict(xover_hz=(1.0,))), ("xover_hz[1]", dict(xover_hz=(250.0, 2.0))),
             ("xover_hz[2]", dict(xover_hz=(250.0, 1000.0, 3.0))), ("beta[0][0]", dict(beta={(0, 0): 2.0})), ("beta[0][1]", dict(beta={(0, 1): 2.0})),
             ("beta[1][0]", dict(beta={(1, 0): 2.0})), ("beta[3][5]", dict(beta={(3, 5): 2.0})), ("air_db_per_m[0]", dict(air_db_per_m=(2.0,))),
             ("air_db_per_m[3]", dict(air_db_per_m=(0.0, 0.0, 0.0, 2.0))), ("flags", dict(flags=2)), ("reserved", dict(reserved=7))]
    for (first, a), (_, b) in zip(order, order[1:]):
        fields = dict(b)
        for k, v in a.items():  # (two entries of one array: the earlier entry's value stays)
            if isinstance(v, tuple) and k in fields:
                fields[k] = v + fields[k][len(v):]
            elif isinstance(v, dict) and k in fields:
                fields[k] = {**fields[k], **v}
            else:
                fields[k] = v
        rc, msg = _call(_bands(**fields))
        assert rc == -1 and first in msg, (first, msg)
    # entries of bands that are not in use are not looked at
    spare = _default()
    spare.n_xovers = 1
    spare.xover_hz[0], spare.xover_hz[1], spare.beta[2][0], spare.air_db_per_m[3] = 500.0, NAN, 9.0, -1.0
    rc, msg = _call(spare, plan=True)
    assert rc == 0, msg
    # the crossovers are checked against the synthesis' rate
    rc, msg = _call(_bands(xover_hz=(250.0, 1000.0, 4000.0)), plan=True, rate=8000)
    assert rc == -1 and "xover_hz[2]" in msg and "3600" in msg, msg
    bad = _bands(reserved=9)
    # the room and the microphones come before the bands, the bands before the tail, the synthesis before everything
    rc, msg = _call(bad, room=IrRoom(order=40).to_c())
    assert rc == -1 and "order" in msg, msg
    rc, msg = _call(bad, mics=IrRoomMics(el=(0, 91)).to_c())
    assert rc == -1 and "mic_el_deg[1]" in msg, msg
    bad_tail = IrTail(mode="extend", knee=(100,), t60=(0,)).to_c()
    rc, msg = _call(bad, tail=bad_tail)
    assert rc == -1 and "bands reserved" in msg, msg
    rc, msg = _call(_bands(), tail=bad_tail)
    assert rc == -1 and "t60" in msg, msg
    L = _lib.load()
    s = IrSynth(frames=0, rate=RATE).to_c()
    assert L.mc_synth_ir_room_bands(None, 0, 1024, C.byref(s), None, None, C.byref(bad), None, None, None, None) == -1
    assert "frames" in L.mc_last_error().decode()
    # bands without a room
    rc, msg = _call(_default(), room=None)
    assert rc == -1 and "the bands need a room" in msg, msg
    rc, msg = _call(_default(), room=None, mics=IrRoomMics().to_c())
    assert rc == -1 and "the microphones need a room" in msg, msg
    rc, msg = _call(_default(), room=None, plan=True)
    assert rc == -1 and "null room" in msg, msg
    rc, msg = _call(None, plan=True)
    assert rc == -1 and "null bands" in msg, msg
    # with bands the room's own beta is still checked
    rc, msg = _call(_default(), room=IrRoom(beta=1.5).to_c())
    assert rc == -1 and "beta[0]" in msg and "bands" not in msg, msg
    # the good edges pass the bands and stop at the engine, which is null
    for fields in (dict(), dict(xover_hz=(10.0, 11.0, 0.45 * RATE)), dict(beta={(0, 0): -1.0, (3, 5): 1.0}), dict(air_db_per_m=(0.0, 1.0, 0.5, 1.0))):
        rc, msg = _call(_bands(**fields))
        assert rc == -1 and "null" in msg and "bands" not in msg, (fields, msg)
        rc, msg = _call(_bands(**fields), plan=True)
        assert rc == 0, (fields, msg)
    # without bands the call is mc_synth_ir_room_mics: its own refusals, in its own words
    rc, msg = _call(None, room=IrRoom(order=40).to_c())
    assert rc == -1 and "order" in msg, msg
    rc, msg = _call(None, mics=IrRoomMics(source_pattern=2.0).to_c())
    assert rc == -1 and "src_pattern" in msg, msg
    rc, msg = _call(None)
    assert rc == -1 and "null" in msg, msg


PLAN_CASES = [({}, dict(), 48000), ({}, dict(xovers=(500.0, 2000.0), beta=(0.95, 0.85, 0.6), air=(0.0, 0.005, 0.03)), 48000),
              (dict(size=(9.0, 6.5, 2.8), speed=331.0), dict(xovers=(125.0, 1000.0, 8000.0), beta=((0.9, 0.8, 0.7, 0.95, 0.6, -0.5), 0.8, 0.99, 0.3),
                                                             air=(0.0, 0.001, 0.01, 0.1)), 96000),
              (dict(beta=0.2), dict(xovers=(3000.0,), beta=(1.0, 0.0), air=(1.0, 0.0)), 8000)]


@pytest.mark.parametrize("room,bands,rate", PLAN_CASES)
def test_the_plan_against_the_restatement(room, bands, rate):
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrRoom, IrRoomBands

    out = (C.c_double * 16)()
    assert _lib.load().mc_ir_room_bands_plan(C.byref(IrRoom(**room).to_c()), C.byref(IrRoomBands(**bands).to_c()), rate, 3000, out) == 0
    want = ir_room_bands_np.plan(room, bands, rate, 3000)
    B = want["bands"]
    assert out[0] == B and list(out[1:4]) == list(want["xovers"]) + [0.0] * (4 - B) and list(out[12:16]) == [0.0] * 4
    np.testing.assert_allclose(list(out[4:4 + B]), want["sabine"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(list(out[8:8 + B]), want["eyring"], rtol=1e-14, atol=0)
    assert list(out[4 + B:8]) == [0.0] * (4 - B) and list(out[8 + B:12]) == [0.0] * (4 - B)
