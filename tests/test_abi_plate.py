"""mc_ir_plate as ctypes sees it against what include/mcconv.h documents, the defaults field by field, every bad field refused by
name in the struct's order and before the tail and the engine, and the four symbols (no GPU: the library's checks touch no
device)."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
RATE = 48000
NAN, INF = float("nan"), float("inf")


def _default():
    from cuda_audio_amd import _lib

    p = _lib.McIrPlate()
    _lib.load().mc_default_ir_plate(C.byref(p))
    return p


def _plate(**fields):
    p = _default()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                if isinstance(x, tuple):
                    for i, y in enumerate(x):
                        getattr(p, k)[j][i] = y
                else:
                    getattr(p, k)[j] = x
        else:
            setattr(p, k, v)
    return p


def test_the_struct_has_its_documented_size_and_the_constants_match():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_plate\) = (\d+)", src).group(1))
    P = _lib.McIrPlate
    assert C.sizeof(P) == size == _default().struct_size == 88
    offsets = dict(struct_size=0, size_m=4, thickness_mm=12, young_gpa=16, density=20, poisson=24, driver_m=28, pickup_m=36, low_hz=52, high_hz=56,
                   t60_s=60, damp_hz=68, gain=72, reserved=76, last=80)
    assert {n: getattr(P, n).offset for n, _ in P._fields_} == offsets
    for name in ("MC_PLATE_MAX_MODES", "MC_PLATE_GROUP", "MC_PLATE_SLAB", "MC_PLATE_MAX_PAIRS"):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == getattr(_lib, name), name
    assert _lib.MC_PLATE_MAX_MODES == 2 ** 18 and _lib.MC_PLATE_MAX_PAIRS == 2 ** 36


def test_the_symbols():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    symbols = {"mc_default_ir_plate", "mc_synth_ir_plate", "mc_ir_plate_plan", "mc_ir_plate_modes", "mc_ir_plate_info"}
    assert symbols <= set(_lib.SYMBOLS)
    for name in symbols:
        assert re.search(r"\b%s\(" % name, src), name
        getattr(_lib.load(), name)
    assert _lib.load().mc_abi_version() == 1


def test_the_defaults_field_by_field():
    from cuda_audio_amd.engine import IrPlate

    f = lambda v: C.c_float(v).value  # noqa: E731
    p = _default()
    assert list(p.size_m) == [f(2.04), f(0.97)] and p.thickness_mm == 0.5
    assert (p.young_gpa, p.density, p.poisson) == (200.0, 7850.0, f(0.3))  # steel
    assert list(p.driver_m) == [f(0.83), f(0.41)]
    assert [list(q) for q in p.pickup_m] == [[f(0.31), f(0.67)], [f(1.57), f(0.29)]]
    assert (p.low_hz, p.high_hz) == (20.0, 0.0) and list(p.t60_s) == [4.0, 1.0] and p.damp_hz == 10000.0
    assert (p.gain, p.reserved, p.last) == (1.0, 0, 0)
    assert bytes(IrPlate().to_c()) == bytes(p)
    # the sides' squares are in no small rational ratio, and nothing sits on a low-order nodal line
    Lx, Ly = p.size_m
    for at in (p.driver_m, p.pickup_m[0], p.pickup_m[1]):
        for m in range(1, 13):
            assert abs((m * at[0] / Lx) - round(m * at[0] / Lx)) > 0.01 and abs((m * at[1] / Ly) - round(m * at[1] / Ly)) > 0.01, (list(at), m)


def test_the_python_class():
    from cuda_audio_amd.engine import IrPlate

    p = IrPlate(size=(1.5, 0.8), thickness_mm=1.0, material=(70.0, 2700.0, 0.33), driver=(0.5, 0.3), pickups=((0.2, 0.2), (1.2, 0.6)), low_hz=30, high_hz=5000,
                t60=(2.0, 0.5), damp_hz=8000, gain=0.5, last=77).to_c()
    f = lambda v: C.c_float(v).value  # noqa: E731
    assert list(p.size_m) == [1.5, f(0.8)] and (p.young_gpa, p.density, p.poisson) == (70.0, 2700.0, f(0.33))
    assert [list(q) for q in p.pickup_m] == [[f(0.2), f(0.2)], [f(1.2), f(0.6)]] and list(p.t60_s) == [2.0, 0.5]
    assert (p.low_hz, p.high_hz, p.damp_hz, p.gain, p.last, p.thickness_mm) == (30.0, 5000.0, 8000.0, 0.5, 77, 1.0)
    with pytest.raises(ValueError):
        IrPlate(material="brass").to_c()
    with pytest.raises(ValueError):
        IrPlate(pickups=((0.2, 0.2),)).to_c()


def _call(plate, tail=None, which="synth", rate=RATE, frames=4000):
    """(rc, message) of mc_synth_ir_plate with a null engine, of mc_ir_plate_plan or of mc_ir_plate_modes."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrSynth

    L = _lib.load()
    ref = C.byref(plate) if plate is not None else None
    if which == "plan":
        rc = L.mc_ir_plate_plan(ref, rate, frames, (C.c_double * 8)())
    elif which == "modes":
        rc = L.mc_ir_plate_modes(ref, rate, 0, 1, (C.c_double * 6)())
    else:
        s = IrSynth(frames=frames, rate=rate, late_gain=0.0).to_c()
        rc = L.mc_synth_ir_plate(None, 0, 1024, C.byref(s), ref, None, None, None, C.byref(tail) if tail is not None else None)
    return rc, L.mc_last_error().decode()


BAD_FIELDS = [("struct_size", dict(struct_size=84)), ("size_m[0]", dict(size_m=(0.01,))), ("size_m[1]", dict(size_m=(2.0, 11.0))), ("size_m[0]", dict(size_m=(NAN,))),
              ("thickness_mm", dict(thickness_mm=0.0)), ("thickness_mm", dict(thickness_mm=INF)), ("young_gpa", dict(young_gpa=-1.0)),
              ("density", dict(density=10.0)), ("poisson", dict(poisson=0.5)), ("poisson", dict(poisson=NAN)), ("driver_m[0]", dict(driver_m=(0.0,))),
              ("driver_m[1]", dict(driver_m=(0.5, 0.97))), ("driver_m[0]", dict(driver_m=(NAN,))), ("pickup_m[0][0]", dict(pickup_m=((2.5,),))),
              ("pickup_m[0][1]", dict(pickup_m=((0.5, -0.1),))), ("pickup_m[1][0]", dict(pickup_m=((0.5, 0.5), (0.0,)))),
              ("pickup_m[1][1]", dict(pickup_m=((0.5, 0.5), (0.5, NAN)))), ("low_hz", dict(low_hz=0.5)), ("low_hz", dict(low_hz=NAN)),
              ("high_hz", dict(high_hz=10.0)), ("high_hz", dict(high_hz=INF)), ("t60_s[0]", dict(t60_s=(-1.0,))), ("t60_s[1]", dict(t60_s=(4.0, 2000.0))),
              ("t60_s[1]", dict(t60_s=(1.0, 4.0))), ("t60_s[1]", dict(t60_s=(1.0, 0.0))), ("damp_hz", dict(damp_hz=0.0)), ("damp_hz", dict(damp_hz=NAN)),
              ("gain", dict(gain=0.0)), ("gain", dict(gain=17.0)), ("reserved", dict(reserved=1))]


@pytest.mark.parametrize("name,fields", BAD_FIELDS)
def test_every_bad_field_is_refused_by_name(name, fields):
    for which in ("synth", "plan", "modes"):
        rc, msg = _call(_plate(**fields), which=which)
        assert rc == -1 and name in msg, (name, fields, which, rc, msg)


def test_the_order_of_the_checks():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrSynth, IrTail

    # in the struct's order: of two bad fields the earlier one is named
    order = [("size_m[0]", dict(size_m=(0.0, 0.97))), ("size_m[1]", dict(size_m=(2.04, 0.0))), ("thickness_mm", dict(thickness_mm=-1.0)),
             ("young_gpa", dict(young_gpa=0.0)), ("density", dict(density=0.0)), ("poisson", dict(poisson=0.7)), ("driver_m[0]", dict(driver_m=(3.0, 0.41))),
             ("driver_m[1]", dict(driver_m=(0.83, 3.0))), ("pickup_m[0][0]", dict(pickup_m=((3.0, 0.67), (1.57, 0.29)))),
             ("pickup_m[1][1]", dict(pickup_m=((0.31, 0.67), (1.57, 3.0)))), ("low_hz", dict(low_hz=0.0)), ("high_hz", dict(high_hz=-5.0)),
             ("t60_s[0]", dict(t60_s=(-1.0, 1.0))), ("t60_s[1]", dict(t60_s=(4.0, -1.0))), ("damp_hz", dict(damp_hz=1.0)), ("gain", dict(gain=-1.0)),
             ("reserved", dict(reserved=7))]
    for i, (first, a) in enumerate(order):
        for _, b in order[i + 1:]:
            if set(a) & set(b):
                continue  # (two entries of one array: covered by BAD_FIELDS)
            rc, msg = _call(_plate(**dict(b, **a)))
            assert rc == -1 and first in msg, (first, msg)
    # the synthesis comes before the plate, the plate's fields before what follows from the rate, all of it before the tail
    bad = _plate(reserved=7)
    L = _lib.load()
    s = IrSynth(frames=0, rate=RATE).to_c()
    assert L.mc_synth_ir_plate(None, 0, 1024, C.byref(s), C.byref(bad), None, None, None, None) == -1
    assert "frames" in L.mc_last_error().decode()
    rc, msg = _call(bad, rate=0)
    assert rc == -1 and "reserved" in msg, msg
    rc, msg = _call(_default(), rate=0)
    assert rc == -1 and "the plate needs the session's rate" in msg, msg
    bad_tail = IrTail(mode="extend", knee=(100,), t60=(0,)).to_c()
    rc, msg = _call(_plate(high_hz=23999.0), tail=bad_tail, rate=44100)
    assert rc == -1 and "high_hz" in msg and "half the rate" in msg, msg
    rc, msg = _call(_plate(low_hz=20.0, high_hz=20.5), tail=bad_tail)
    assert rc == -1 and "M = 0" in msg, msg
    rc, msg = _call(_plate(size_m=(10.0, 10.0), thickness_mm=0.05), tail=bad_tail)
    assert rc == -1 and "more than 262144 modes" in msg, msg
    # (the bound on the sum, gain 4 sqrt(2 M) < 2^22, holds for every M and gain that get this far: no struct reaches its message)
    rc, msg = _call(_default(), tail=bad_tail, frames=1 << 22)
    assert rc == -1 and "pairs" in msg and "times" in msg, msg  # (25697 modes x 2^22 frames: 1.57 times the cap)
    rc, msg = _call(_default(), tail=bad_tail)
    assert rc == -1 and "t60" in msg and "pairs" not in msg, msg
    # the good edges pass the plate and stop at the engine, which is null
    for fields in (dict(), dict(t60_s=(0.0, 0.0)), dict(t60_s=(0.0, 1.0)), dict(t60_s=(2.0, 2.0)), dict(gain=16.0, high_hz=400.0), dict(size_m=(2.0, 1.0)),
                   dict(last=1 << 40), dict(poisson=0.0)):
        rc, msg = _call(_plate(**fields))
        assert rc == -1 and "null" in msg and "plate" not in msg, (fields, msg)
        rc, msg = _call(_plate(**fields), which="plan")
        assert rc == 0, (fields, msg)
    # without a plate the call is mc_synth_ir_room(room = NULL): its own refusals, in its own words
    rc, msg = _call(None)
    assert rc == -1 and "null" in msg, msg
    rc, msg = _call(None, tail=bad_tail)
    assert rc == -1 and "t60" in msg, msg
    for which in ("plan", "modes"):
        rc, msg = _call(None, which=which)
        assert rc == -1 and "null plate" in msg, msg
    assert L.mc_ir_plate_plan(C.byref(_default()), RATE, 0, (C.c_double * 8)()) == -1 and "frames" in L.mc_last_error().decode()
    assert L.mc_ir_plate_modes(C.byref(_plate(high_hz=400.0)), RATE, 470, 3, (C.c_double * 18)()) == -1 and "rows" in L.mc_last_error().decode()
