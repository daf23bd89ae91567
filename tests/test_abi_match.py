"""mc_ir_match as ctypes sees it against what include/mcconv.h documents, the defaults field by field, and every refusal of
mc_ir_match_plan, mc_load_ir_match and mc_load_ir_sweep_match in the documented order before the engine is looked at; a step
that is off is the wrapped load, refusal for refusal (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
NAN = float("nan")
FP = C.POINTER(C.c_float)


def _match(**fields):
    from cuda_audio_amd import _lib

    m = _lib.McIrMatch()
    _lib.load().mc_default_ir_match(C.byref(m))
    m.mode = _lib.MC_MATCH_TARGET
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(m, k)[j] = x
        else:
            setattr(m, k, v)
    return m


def test_the_struct_has_its_documented_size_and_defaults():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_match\) = (\d+)", src).group(1))
    m = _lib.McIrMatch()
    _lib.load().mc_default_ir_match(C.byref(m))
    assert C.sizeof(_lib.McIrMatch) == size == m.struct_size == 80
    assert (m.mode, m.phase, m.link, m.rate, m.per_octave, m.lo_hz, m.hi_hz, m.octaves) == (_lib.MC_MATCH_OFF, _lib.MC_MATCH_MINIMUM, 1, 0, 12, 20.0, 0.0, 1.0 / 3.0)
    assert (m.amount, m.boost_db, m.cut_db, m.floor_db, m.tilt_db, m.delay, list(m.reserved)) == (1.0, 12.0, 24.0, 120.0, 0.0, 0, [0, 0])
    assert re.search(r"enum \{ MC_MATCH_OFF = 0, MC_MATCH_TARGET = 1, MC_MATCH_FLAT = 2 \};", src)
    assert re.search(r"enum \{ MC_MATCH_MINIMUM = 0, MC_MATCH_LINEAR = 1 \};", src)
    assert re.search(r"#define MC_ABI_VERSION 1\b", src)
    assert {"mc_default_ir_match", "mc_ir_match_plan", "mc_load_ir_match", "mc_load_ir_sweep_match", "mc_ir_match_info", "mc_ir_match_curve"} <= set(_lib.SYMBOLS)
    # the struct's fields in the header's order, as the refusals name them
    body = re.search(r"typedef struct \{([^}]*)\} mc_ir_match;", src).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [n for n, _ in _lib.McIrMatch._fields_]
    kernel = open(os.path.join(os.path.dirname(HEADER), "..", "cuda_audio_amd", "csrc", "irmatch.hip.h")).read()
    assert int(re.search(r"constexpr uint32_t MT_MAX_POINTS = (\d+);", kernel).group(1)) == _lib.MC_MATCH_MAX_POINTS == 1024


BAD_FIELDS = [("struct_size", dict(struct_size=76)), ("mode", dict(mode=3)), ("phase", dict(phase=2)), ("link", dict(link=2)), ("rate", dict(rate=7999)),
              ("rate", dict(rate=384001)), ("per_octave", dict(per_octave=0)), ("per_octave", dict(per_octave=97)), ("lo_hz", dict(lo_hz=0.5)),
              ("lo_hz", dict(lo_hz=NAN)), ("hi_hz", dict(hi_hz=20.0)), ("hi_hz", dict(hi_hz=NAN)), ("hi_hz", dict(hi_hz=-1.0)), ("octaves", dict(octaves=0.04)),
              ("octaves", dict(octaves=2.01)), ("octaves", dict(octaves=NAN)), ("amount", dict(amount=-0.1)), ("amount", dict(amount=1.5)),
              ("boost_db", dict(boost_db=60.5)), ("boost_db", dict(boost_db=NAN)), ("cut_db", dict(cut_db=-1.0)), ("floor_db", dict(floor_db=39.0)),
              ("floor_db", dict(floor_db=301.0)), ("tilt_db", dict(tilt_db=12.5)), ("tilt_db", dict(tilt_db=-13.0)), ("delay", dict(delay=(1 << 20) + 1)),
              ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, 1)))]
ORDER = [("mode", dict(mode=9)), ("phase", dict(phase=9)), ("link", dict(link=9)), ("rate", dict(rate=5)), ("per_octave", dict(per_octave=500)),
         ("lo_hz", dict(lo_hz=0.0)), ("hi_hz", dict(hi_hz=1e9)), ("octaves", dict(octaves=9.0)), ("amount", dict(amount=2.0)), ("boost_db", dict(boost_db=99.0)),
         ("cut_db", dict(cut_db=99.0)), ("floor_db", dict(floor_db=1.0)), ("tilt_db", dict(tilt_db=50.0)), ("delay", dict(delay=1 << 30)),
         ("reserved", dict(reserved=(7, 7)))]


def _plan(m, frames=100, target_frames=10, rate=48000, out=True):
    from cuda_audio_amd import _lib

    L = _lib.load()
    buf = (C.c_double * 6)(*([-1.0] * 6))
    rc = L.mc_ir_match_plan(C.byref(m) if m is not None else None, frames, target_frames, rate, buf if out else None)
    return rc, L.mc_last_error().decode(), list(buf)


def test_the_plan_refuses():
    rc, msg, _ = _plan(None)
    assert rc == -1 and "null match" in msg
    for name, fields in BAD_FIELDS:
        rc, msg, out = _plan(_match(**fields))
        assert rc == -1 and name in msg and out == [-1.0] * 6, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):  # (of two bad fields the earlier one is named)
        rc, msg, _ = _plan(_match(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # the limits in their order: the session's rate, hi_hz, the grid, the target's frames, the transform, the delay
    every = dict(hi_hz=30000.0, lo_hz=25000.0, phase=1, delay=1 << 20)
    rc, msg, _ = _plan(_match(**every), frames=1 << 22, target_frames=0, rate=0)
    assert rc == -1 and "session_rate is 0" in msg, msg
    rc, msg, _ = _plan(_match(**every), frames=1 << 22, target_frames=0)
    assert rc == -1 and "hi_hz" in msg and "half" in msg, msg
    rc, msg, _ = _plan(_match(**dict(every, hi_hz=0.0)), frames=1 << 22, target_frames=0)  # (hi_hz = 20000 < lo_hz)
    assert rc == -1 and "grid" in msg, msg
    rc, msg, _ = _plan(_match(**dict(every, hi_hz=0.0, lo_hz=20.0)), frames=1 << 22, target_frames=0)
    assert rc == -1 and "target_frames" in msg, msg
    rc, msg, _ = _plan(_match(**dict(every, hi_hz=0.0, lo_hz=20.0)), frames=1 << 22, target_frames=5)
    assert rc == -1 and "transform" in msg and "4194304" in msg, msg
    rc, msg, _ = _plan(_match(**dict(every, hi_hz=0.0, lo_hz=20.0)), frames=1000, target_frames=5)
    assert rc == -1 and "delay" in msg, msg
    rc, msg, out = _plan(_match(**dict(every, hi_hz=0.0, lo_hz=20.0)), frames=1 << 20, target_frames=5)
    assert rc == 0 and out[0] == float(1 << 21) and out[3] == float(1 << 21)
    rc, msg, out = _plan(_match(mode=0))  # (off is planned as a target)
    assert rc == 0 and out[:2] == [256.0, 1.0] and out[3:5] == [100.0, 120.0]
    rc, msg, _ = _plan(_match(), out=False)
    assert rc == -1 and "null out" in msg


@pytest.mark.parametrize("frames", [(1 << 22) + 1, (1 << 40) + 1, (1 << 62) + 1, (1 << 63) - 1])
def test_the_plan_refuses_any_length_beyond_the_transform(frames):
    """mc_ir_match_plan bounds `frames` by nothing but the transform: the search for its length must end at 2^22 whatever comes in
    (a power of two >= 2 frames does not exist in 64 bits from 2^62 + 1 on)."""
    rc, msg, out = _plan(_match(), frames=frames, target_frames=5)
    assert rc == -1 and msg == f"{frames} frames and 5 target frames at the session's rate need a transform of more than 2^22 points", msg
    assert out == [-1.0] * 6


def _load(m, frames=100, rates=(48000, 48000), lr=True, tlr=True, G=10, tail=None, shape=None, phase=None, filt=None, flr=True, fG=10):
    from cuda_audio_amd import _lib

    L = _lib.load()
    buf, tbuf, fbuf = (np.zeros((max(min(n, 1000), 1), 2), np.float32) for n in (frames, G, fG))
    rc = L.mc_load_ir_match(None, 0, buf.ctypes.data_as(FP) if lr else None, frames, 1024, rates[0], rates[1], shape, None, None, tail, phase, filt,
                            fbuf.ctypes.data_as(FP) if flr else None, fG, C.byref(m) if m is not None else None, tbuf.ctypes.data_as(FP) if tlr else None, G)
    return rc, L.mc_last_error().decode()


def _load_sweep(m, ir_frames=900, tail=None, phase=None, filt=None, lr=True, flr=True, tlr=True, G=10, fG=10):
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import Sweep

    L = _lib.load()
    rec = np.zeros((5000, 2), np.float32)
    tbuf, fbuf = (np.zeros((max(min(n, 1000), 1), 2), np.float32) for n in (G, fG))
    sw = Sweep(frames=4096, f1_hz=20.0, f2_hz=3000.0, rate=8000).to_c()
    rc = L.mc_load_ir_sweep_match(None, 0, rec.ctypes.data_as(FP) if lr else None, len(rec), 1024, C.byref(sw), 0, ir_frames, None, None, None, tail, phase, filt,
                                  fbuf.ctypes.data_as(FP) if flr else None, fG, C.byref(m) if m is not None else None, tbuf.ctypes.data_as(FP) if tlr else None, G)
    return rc, L.mc_last_error().decode()


def _others():
    """A bad filter, a bad phase, a bad tail and a bad shape."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    filt = _lib.McIrFilter()
    L.mc_default_ir_filter(C.byref(filt))
    filt.op, filt.reg_db = _lib.MC_FILTER_CONVOLVE, 1.0
    phase = _lib.McIrPhase()
    L.mc_default_ir_phase(C.byref(phase))
    phase.mode, phase.over_log2 = _lib.MC_PHASE_MINIMUM, 0
    tail = _lib.McIrTail()
    L.mc_default_ir_tail(C.byref(tail))
    tail.mode, tail.width = _lib.MC_TAIL_EXTEND, 7.0
    shape = _lib.McIrShape()
    L.mc_default_ir_shape(C.byref(shape))
    shape.trim_db = 5.0
    return filt, phase, tail, shape


def test_the_loads_refuse_in_the_documented_order_before_the_engine_is_looked_at():
    """No engine is passed: a call that gets past the checks ends at "null argument", the load's own first check."""
    from cuda_audio_amd import _lib

    for name, fields in BAD_FIELDS:
        for rates in ((0, 0), (8000, 8000), (1, 2)):  # (the match comes before the rates)
            rc, msg = _load(_match(**fields), rates=rates)
            assert rc == -1 and name in msg, (name, msg)
        rc, msg = _load_sweep(_match(**fields))
        assert rc == -1 and name in msg, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):
        rc, msg = _load(_match(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # the match before a bad filter, phase, tail and shape; a good match lets them speak, in the wrapped call's order
    filt, phase, tail, shape = _others()
    every = dict(rates=(8000, 8000), tail=C.byref(tail), shape=C.byref(shape), phase=C.byref(phase), filt=C.byref(filt))
    sweep_every = dict(tail=C.byref(tail), phase=C.byref(phase), filt=C.byref(filt))
    for load, kw in ((_load, every), (_load_sweep, sweep_every)):
        filt.reg_db, phase.over_log2, tail.width = 1.0, 0, 7.0
        rc, msg = load(_match(reserved=(3, 0), hi_hz=3000.0), **kw)
        assert rc == -1 and "reserved" in msg, msg
        rc, msg = load(_match(hi_hz=3000.0), **kw)
        assert rc == -1 and "reg_db" in msg, msg
        filt.reg_db = 60.0
        rc, msg = load(_match(hi_hz=3000.0), **kw)
        assert rc == -1 and "over_log2" in msg, msg
        phase.over_log2 = 3
        rc, msg = load(_match(hi_hz=3000.0), **kw)
        assert rc == -1 and "width" in msg, msg
    tail.width = 1.0
    # with a tail the steps' limits come before the shape: the phase step's, the filter step's, then the match step's
    rc, msg = _load(_match(hi_hz=5000.0), **every)
    assert rc == -1 and "hi_hz" in msg and "half" in msg, msg
    filt.frames_out = 1 << 30
    rc, msg = _load(_match(hi_hz=5000.0), **every)
    assert rc == -1 and "frames_out" in msg, msg
    filt.frames_out = 0
    rc, msg = _load(_match(hi_hz=3000.0), **every)
    assert rc == -1 and "trim_db" in msg, msg
    # without a tail a bad shape comes before them
    rc, msg = _load(_match(hi_hz=30000.0), shape=C.byref(shape))
    assert rc == -1 and "trim_db" in msg, msg
    # the limits, in their order (the plan's test walks all of them; here through the loads)
    rc, msg = _load(_match(hi_hz=30000.0, lo_hz=25000.0), rates=(0, 0), G=0)
    assert rc == -1 and "session_rate is 0" in msg, msg
    rc, msg = _load(_match(hi_hz=30000.0, lo_hz=25000.0), G=0)
    assert rc == -1 and "hi_hz" in msg, msg
    rc, msg = _load(_match(lo_hz=19500.0), G=0)
    assert rc == -1 and "grid" in msg, msg
    rc, msg = _load(_match(phase=1, delay=1000), G=0)
    assert rc == -1 and "target_frames" in msg, msg
    rc, msg = _load(_match(phase=1, delay=1000), G=(1 << 40) + 1)
    assert rc == -1 and "target_frames" in msg, msg
    rc, msg = _load(_match(phase=1, delay=1000), G=(1 << 21) + 1)
    assert rc == -1 and "transform" in msg and "2097153" in msg, msg
    rc, msg = _load(_match(phase=1, delay=157))
    assert rc == -1 and "delay" in msg, msg
    rc, msg = _load(_match(phase=1, delay=156))
    assert rc == -1 and "null argument" in msg, msg
    rc, msg = _load(_match(delay=157))  # (minimum phase does not use the delay)
    assert rc == -1 and "null argument" in msg, msg
    # the match step sees what the filter step hands on: 100 and 29 frames give 128, and a transform of 256 points
    filt.reg_db = 60.0
    rc, msg = _load(_match(phase=1, delay=129), filt=C.byref(filt), fG=29)
    assert rc == -1 and "delay" in msg and "128 frames" in msg, msg
    rc, msg = _load(_match(phase=1, delay=128), filt=C.byref(filt), fG=29)
    assert rc == -1 and "null argument" in msg, msg
    # the target's own rate: 10 frames at 8 kHz are 480 at 384 kHz
    rc, msg = _load(_match(rate=8000, phase=1, delay=545, hi_hz=20000.0), frames=480, rates=(384000, 384000), G=10)
    assert rc == -1 and "delay" in msg, msg
    rc, msg = _load(_match(rate=8000, phase=1, delay=544, hi_hz=20000.0), frames=480, rates=(384000, 384000), G=10)
    assert rc == -1 and "null argument" in msg, msg
    rc, msg = _load_sweep(_match(), ir_frames=900)  # (the session's rate is the sweep's, 8 kHz: hi_hz defaults to 4000)
    assert rc == -1 and "null argument" in msg, msg
    rc, msg = _load_sweep(_match(hi_hz=4001.0), ir_frames=900)
    assert rc == -1 and "hi_hz" in msg, msg
    # pointers last: the filter's, then the target's; a flat target needs none
    rc, msg = _load(_match(phase=1, delay=157), tlr=False)
    assert rc == -1 and "delay" in msg, msg
    rc, msg = _load(_match(), tlr=False, flr=False, filt=C.byref(filt))
    assert rc == -1 and "null filter_lr" in msg, msg
    rc, msg = _load(_match(), tlr=False, filt=C.byref(filt))
    assert rc == -1 and "null target_lr" in msg, msg
    rc, msg = _load_sweep(_match(), tlr=False, flr=False, filt=C.byref(filt))
    assert rc == -1 and "null filter_lr" in msg, msg
    rc, msg = _load_sweep(_match(), tlr=False)
    assert rc == -1 and "null target_lr" in msg, msg
    rc, msg = _load_sweep(_match(), lr=False, tlr=False)
    assert rc == -1 and "null lr" in msg, msg
    for rc, msg in (_load(_match(mode=_lib.MC_MATCH_FLAT), tlr=False, G=0), _load(_match(), lr=False), _load_sweep(_match(mode=_lib.MC_MATCH_FLAT), tlr=False, G=0)):
        assert rc == -1 and "null argument" in msg, msg


def test_a_step_that_is_off_refuses_what_the_wrapped_load_refuses_message_for_message():
    """MC_MATCH_OFF with nonsense in every other field, and NULL: mc_load_ir_filter's and mc_load_ir_sweep_filter's own refusals."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    off = _match(mode=0, struct_size=3, phase=9, link=9, rate=1, per_octave=0, lo_hz=NAN, hi_hz=-1.0, octaves=NAN, amount=NAN, boost_db=NAN, cut_db=NAN,
                 floor_db=NAN, tilt_db=NAN, delay=1 << 31, reserved=(5, 5))
    filt, phase, tail, shape = _others()
    buf = np.zeros((100, 2), np.float32)
    rec = np.zeros((5000, 2), np.float32)
    from cuda_audio_amd.engine import Sweep

    sw = Sweep(frames=4096, f1_hz=20.0, f2_hz=3000.0, rate=8000).to_c()
    cases = []
    for f, p, t, s, rates, flr, frames in ((filt, phase, tail, shape, (8000, 8000), True, 100), (None, phase, tail, shape, (8000, 8000), True, 100),
                                           (None, None, tail, shape, (8000, 8000), True, 100), (None, None, None, shape, (0, 0), True, 100),
                                           (None, None, None, None, (1, 2), True, 100), (None, None, None, None, (0, 0), True, 0),
                                           (None, None, None, None, (0, 0), True, 100)):
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        args = (None, 0, buf.ctypes.data_as(FP), frames, 1024, rates[0], rates[1], ref(s), None, None, ref(t), ref(p), ref(f), buf.ctypes.data_as(FP) if flr else None, 10)
        sargs = (None, 0, rec.ctypes.data_as(FP), len(rec), 1024, C.byref(sw), 0, 900, None, None, None, ref(t), ref(p), ref(f), buf.ctypes.data_as(FP), 10)
        cases.append((L.mc_load_ir_filter, L.mc_load_ir_match, args))
        cases.append((L.mc_load_ir_sweep_filter, L.mc_load_ir_sweep_match, sargs))
    for wrapped, load, args in cases:
        rc0 = wrapped(*args)
        want = L.mc_last_error().decode()
        for m in (None, C.byref(off)):
            assert load(*args, m, None, 0) == rc0 == -1 and L.mc_last_error().decode() == want, want
    print(sorted({c[0].__name__ for c in cases}), "refusals compared")
