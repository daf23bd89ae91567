"""mc_ir_spring as ctypes sees it against what include/mcconv.h documents, the defaults field by field, every bad field refused by
name in the struct's order and before the tail and the engine, the derived refusals, and the five symbols (no GPU: the
library's checks touch no device)."""
import ctypes as C
import os
import re

import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
RATE = 48000
NAN, INF = float("nan"), float("inf")


def _default():
    from cuda_audio_amd import _lib

    p = _lib.McIrSpring()
    _lib.load().mc_default_ir_spring(C.byref(p))
    return p


def _spring(**fields):
    p = _default()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j in range(3):
                getattr(p, k)[j] = v[j] if j < len(v) else 0.0
        else:
            setattr(p, k, v)
    return p


def test_the_struct_has_its_documented_size_and_the_constants_match():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_spring\) = (\d+)", src).group(1))
    P = _lib.McIrSpring
    assert C.sizeof(P) == size == _default().struct_size == 80
    offsets = dict(struct_size=0, sections=4, transition_hz=8, dispersion=12, delay_ms=16, t60_s=28, damping=32, lowpass_order=36, high_gain=40,
                   high_sections=44, high_dispersion=48, high_delay=52, high_t60_s=56, stereo=60, gain=64, log2_points=68, last=72)
    assert {n: getattr(P, n).offset for n, _ in P._fields_} == offsets
    for name in ("MC_SPRING_MAX", "MC_SPRING_MAX_STRETCH", "MC_SPRING_MAX_LOG2"):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == getattr(_lib, name), name
    assert float(re.search(r"#define MC_SPRING_RADIUS (\S+)", src).group(1)) == _lib.MC_SPRING_RADIUS == 1e8


def test_the_symbols():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    symbols = {"mc_default_ir_spring", "mc_synth_ir_spring", "mc_ir_spring_plan", "mc_ir_spring_response", "mc_ir_spring_info"}
    assert symbols <= set(_lib.SYMBOLS)
    for name in symbols:
        assert re.search(r"\b%s\(" % name, src), name
        getattr(_lib.load(), name)
    assert _lib.load().mc_abi_version() == 1


def test_the_defaults_field_by_field():
    from cuda_audio_amd.engine import IrSpring

    f = lambda v: C.c_float(v).value  # noqa: E731
    p = _default()
    assert (p.sections, p.transition_hz, p.dispersion) == (100, 4300.0, f(0.62)) and list(p.delay_ms) == [66.0, 82.0, 0.0]
    assert (p.t60_s, p.damping, p.lowpass_order) == (2.5, f(0.2), 8)
    assert (p.high_gain, p.high_sections, p.high_dispersion, p.high_delay, p.high_t60_s) == (f(0.1), 200, f(-0.6), 0.5, 1.0)
    assert (p.stereo, p.gain, p.log2_points, p.last) == (f(0.03), 1.0, 0, 0)
    assert bytes(IrSpring().to_c()) == bytes(p)


def test_the_python_class():
    from cuda_audio_amd.engine import IrSpring

    f = lambda v: C.c_float(v).value  # noqa: E731
    p = IrSpring(sections=7, transition_hz=1000, dispersion=0.5, delay_ms=(30, 40, 50), t60=1.5, damping=0.1, lowpass_order=4, high_gain=0.2, high_sections=9,
                 high_dispersion=-0.3, high_delay=0.25, high_t60=0.7, stereo=0.1, gain=2, log2_points=12, last=77).to_c()
    assert (p.sections, p.transition_hz, p.dispersion, list(p.delay_ms), p.t60_s, p.damping, p.lowpass_order) == (7, 1000.0, 0.5, [30.0, 40.0, 50.0], 1.5, f(0.1), 4)
    assert (p.high_gain, p.high_sections, p.high_dispersion, p.high_delay, p.high_t60_s) == (f(0.2), 9, f(-0.3), 0.25, f(0.7))
    assert (p.stereo, p.gain, p.log2_points, p.last) == (f(0.1), 2.0, 12, 77)
    assert list(IrSpring(delay_ms=33).to_c().delay_ms) == [33.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        IrSpring(delay_ms=(1, 2, 3, 4)).to_c()


def _call(spring, tail=None, which="synth", rate=RATE, frames=4000):
    """(rc, message) of mc_synth_ir_spring with a null engine, of mc_ir_spring_plan or of mc_ir_spring_response."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrSynth

    L = _lib.load()
    ref = C.byref(spring) if spring is not None else None
    if which == "plan":
        rc = L.mc_ir_spring_plan(ref, rate, frames, (C.c_double * 24)())
    elif which == "response":
        rc = L.mc_ir_spring_response(ref, rate, (C.c_double * 1)(100.0), 1, (C.c_double * 4)())
    else:
        s = IrSynth(frames=frames, rate=rate, late_gain=0.0).to_c()
        rc = L.mc_synth_ir_spring(None, 0, 1024, C.byref(s), ref, None, None, None, C.byref(tail) if tail is not None else None)
    return rc, L.mc_last_error().decode()


BAD_FIELDS = [("struct_size", dict(struct_size=76)), ("sections", dict(sections=513)), ("transition_hz", dict(transition_hz=0.0)),
              ("transition_hz", dict(transition_hz=NAN)), ("transition_hz", dict(transition_hz=-5.0)), ("dispersion", dict(dispersion=-0.1)),
              ("dispersion", dict(dispersion=0.96)), ("dispersion", dict(dispersion=NAN)), ("delay_ms[1]", dict(delay_ms=(0.0, 82.0))), ("delay_ms[0]", dict(delay_ms=(0.0,))),
              ("delay_ms[0]", dict(delay_ms=(-1.0,))), ("delay_ms[1]", dict(delay_ms=(66.0, INF))), ("delay_ms[2]", dict(delay_ms=(66.0, 0.0, 40.0))),
              ("delay_ms[2]", dict(delay_ms=(66.0, 82.0, NAN))), ("t60_s", dict(t60_s=-1.0)), ("t60_s", dict(t60_s=2000.0)), ("t60_s", dict(t60_s=NAN)),
              ("damping", dict(damping=0.99)), ("damping", dict(damping=-0.5)), ("lowpass_order", dict(lowpass_order=3)), ("lowpass_order", dict(lowpass_order=14)),
              ("high_gain", dict(high_gain=-0.1)), ("high_gain", dict(high_gain=INF)), ("high_sections", dict(high_sections=1025)),
              ("high_dispersion", dict(high_dispersion=0.1)), ("high_dispersion", dict(high_dispersion=-0.99)), ("high_delay", dict(high_delay=0.0)),
              ("high_delay", dict(high_delay=1.5)), ("high_t60_s", dict(high_t60_s=-2.0)), ("high_t60_s", dict(high_t60_s=INF)), ("stereo", dict(stereo=0.3)),
              ("stereo", dict(stereo=-0.01)), ("gain", dict(gain=0.0)), ("gain", dict(gain=17.0)), ("log2_points", dict(log2_points=9)),
              ("log2_points", dict(log2_points=23))]


@pytest.mark.parametrize("name,fields", BAD_FIELDS)
def test_every_bad_field_is_refused_by_name(name, fields):
    for which in ("synth", "plan", "response"):
        rc, msg = _call(_spring(**fields), which=which)
        assert rc == -1 and name in msg, (name, fields, which, rc, msg)


def test_the_order_of_the_checks():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrSynth, IrTail

    # in the struct's order: of two bad fields the earlier one is named
    order = [("sections", dict(sections=1000)), ("transition_hz", dict(transition_hz=-1.0)), ("dispersion", dict(dispersion=2.0)),
             ("delay_ms[1]", dict(delay_ms=(66.0, -1.0))), ("t60_s", dict(t60_s=-1.0)), ("damping", dict(damping=2.0)), ("lowpass_order", dict(lowpass_order=5)),
             ("high_gain", dict(high_gain=-1.0)), ("high_sections", dict(high_sections=5000)), ("high_dispersion", dict(high_dispersion=0.5)),
             ("high_delay", dict(high_delay=2.0)), ("high_t60_s", dict(high_t60_s=-1.0)), ("stereo", dict(stereo=1.0)), ("gain", dict(gain=-1.0)),
             ("log2_points", dict(log2_points=5))]
    for i, (first, a) in enumerate(order):
        for _, b in order[i + 1:]:
            rc, msg = _call(_spring(**dict(b, **a)))
            assert rc == -1 and msg.startswith(first), (first, msg)
    # the synthesis comes before the spring, the spring's fields before what follows from the rate, all of it before the tail
    bad = _spring(log2_points=5)
    L = _lib.load()
    s = IrSynth(frames=0, rate=RATE).to_c()
    assert L.mc_synth_ir_spring(None, 0, 1024, C.byref(s), C.byref(bad), None, None, None, None) == -1
    assert "frames" in L.mc_last_error().decode()
    rc, msg = _call(bad, rate=0)
    assert rc == -1 and "log2_points" in msg, msg
    rc, msg = _call(_default(), rate=0)
    assert rc == -1 and "the spring needs the session's rate" in msg, msg
    bad_tail = IrTail(mode="extend", knee=(100,), t60=(0,)).to_c()
    # the derived refusals, each before the tail: transition above half the rate, K, L for channel L and for R alone, |g|, E and N
    rc, msg = _call(_spring(transition_hz=5000.0), tail=bad_tail, rate=8000)
    assert rc == -1 and "transition_hz" in msg and "half the rate" in msg, msg
    rc, msg = _call(_spring(transition_hz=300.0), tail=bad_tail)
    assert rc == -1 and "K = 80" in msg and "more than 64" in msg, msg
    # 100 sections at K = 6: the cascade's own delay is rint(600 0.38 / 1.62) = 141 frames; 2.9 ms are 139
    rc, msg = _call(_spring(delay_ms=(2.9,)), tail=bad_tail)
    assert rc == -1 and "delay_ms[0]" in msg and "shorter than the dispersion's own delay" in msg and "channel L" in msg, msg
    # (channel R's period is never the shorter one, so no struct is refused for R with L passing)
    rc, msg = _call(_spring(delay_ms=(66.0, 2.9)), tail=bad_tail)
    assert rc == -1 and "delay_ms[1]" in msg and "channel L" in msg, msg
    rc, msg = _call(_spring(delay_ms=(10.0,), t60_s=1000.0), tail=bad_tail)  # 10^(-3 0.01 / 1000) = 0.99993
    assert rc == -1 and "t60_s" in msg and "0.9999" in msg and "high" not in msg, msg
    rc, msg = _call(_spring(delay_ms=(10.0,), t60_s=0.0, high_t60_s=1000.0), tail=bad_tail)
    assert rc == -1 and "high_t60_s" in msg and "0.9999" in msg, msg
    rc, msg = _call(_spring(delay_ms=(10.0,), t60_s=0.0, high_t60_s=1000.0, high_gain=0.0), tail=bad_tail)
    assert rc == -1 and "t60" in msg and "0.9999" not in msg, msg  # (the high loop is off: its gain is not looked at; the tail is)
    rc, msg = _call(_spring(log2_points=10), tail=bad_tail, frames=513)
    assert rc == -1 and "log2_points 10" in msg and "512 frames" in msg and "set last" in msg, msg
    rc, msg = _call(_default(), tail=bad_tail, frames=(1 << 21) + 1)
    assert rc == -1 and "2^22 points" in msg and "set last" in msg, msg
    rc, msg = _call(_default(), tail=bad_tail)
    assert rc == -1 and "t60" in msg and "points" not in msg, msg
    # the good edges pass the spring and stop at the engine, which is null
    for fields in (dict(), dict(sections=0), dict(sections=512, delay_ms=(300.0,)), dict(t60_s=0.0), dict(lowpass_order=0), dict(lowpass_order=12),
                   dict(high_gain=0.0), dict(high_gain=16.0, gain=16.0), dict(high_sections=1024), dict(stereo=0.25), dict(delay_ms=(66.0, 82.0, 91.0)),
                   dict(last=1 << 40), dict(log2_points=22), dict(log2_points=13, last=4000), dict(transition_hz=24000.0), dict(delay_ms=(2.95,)),
                   dict(dispersion=0.0, damping=0.0)):
        rc, msg = _call(_spring(**fields))
        assert rc == -1 and "null" in msg and "spring" not in msg, (fields, msg)
        rc, msg = _call(_spring(**fields), which="plan")
        assert rc == 0, (fields, msg)
    rc, msg = _call(_default(), frames=1 << 21)
    assert rc == -1 and "null" in msg, msg
    # without a spring the call is mc_synth_ir_room(room = NULL): its own refusals, in its own words
    rc, msg = _call(None)
    assert rc == -1 and "null" in msg, msg
    rc, msg = _call(None, tail=bad_tail)
    assert rc == -1 and "t60" in msg, msg
    for which in ("plan", "response"):
        rc, msg = _call(None, which=which)
        assert rc == -1 and "null spring" in msg, msg
    assert L.mc_ir_spring_plan(C.byref(_default()), RATE, 0, (C.c_double * 24)()) == -1 and "frames" in L.mc_last_error().decode()


def test_the_shortest_delay_that_passes_in_both_channels():
    """R's period is never the shorter one, so no struct is refused for channel R with L passing; what can be checked is that
    both channels get their own delay: L = 1 in channel L, the least allowed, and more in R with stereo on."""
    from cuda_audio_amd import _lib

    out = (C.c_double * 24)()
    assert _lib.load().mc_ir_spring_plan(C.byref(_spring(delay_ms=(2.95,), stereo=0.25)), RATE, 1000, out) == 0
    assert (out[8], out[9]) == (1.0, 36.0)  # rint(141.6) - 141, rint(177.0) - 141
