"""The order in which the IR load entry points that no other file pins refuse their arguments, through the library with a null
engine (every check comes before the engine is looked at): mc_load_ir_tail, mc_load_ir_sweep_tail, mc_load_ir_damped, and what
the six mc_ir_*_info getters say without a loaded IR.  One call gets several bad arguments at once; they are repaired one at a
time, and each time the message names the next one in the documented order.  tests/test_ir_room_cpu.py, test_ir_sweep_cpu.py
and test_ir_synth_cpu.py do the same for their entry points."""
import ctypes as C

import numpy as np
import pytest

from cuda_audio_amd import _lib
from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, IrTail, Sweep

RATE = 48000
FRAMES = 1000


def _ref(x):
    return C.byref(x) if x is not None else None


def _bad():
    """a damping, an eq and a shape that are each refused, by xover_hz, freq_hz and trim_db"""
    return IrDamp(xovers=(400, 300), decay=(0, 1, 2)).to_c(), IrEq(bands=[("peak", 5.0, 3.0)]).to_c(), IrShape(trim_db=1.0).to_c()


def _good():
    return IrDamp().to_c(), IrEq(bands=[("peak", 500.0, 3.0)]).to_c(), IrShape(trim_db=-40.0).to_c()


def _tail(**kw):
    return IrTail(**dict(dict(mode="extend", knee=(500,), t60=(2000,), level_db=((-60.0, -60.0),), fade=40), **kw)).to_c()


def _msg(L):
    return L.mc_last_error().decode()


def _lr(frames=FRAMES):
    lr = np.zeros((frames, 2), np.float32)
    return lr, lr.ctypes.data_as(C.POINTER(C.c_float))


def _file_tail(L, tail, frames=FRAMES, rates=(RATE, RATE), lr=None, shape=None, eq=None, damp=None):
    return L.mc_load_ir_tail(None, 0, lr, frames, 1024, rates[0], rates[1], _ref(shape), _ref(eq), _ref(damp), _ref(tail))


def _damped(L, frames=FRAMES, rates=(RATE, RATE), lr=None, shape=None, eq=None, damp=None):
    return L.mc_load_ir_damped(None, 0, lr, frames, 1024, rates[0], rates[1], _ref(shape), _ref(eq), _ref(damp))


def test_file_load_with_a_tail_refuses_in_the_documented_order():
    """the tail, the session's rate, the IR's rate, the frames, F', damping, eq, shape, and only then the pointers"""
    L = _lib.load()
    damp, eq, shape = _bad()
    every = dict(shape=shape, eq=eq, damp=damp)
    tail = _tail(width=2.0)
    big = (1 << 24) + 1  # (with length 0 the step would hand on more frames than it may)
    assert _file_tail(L, tail, big, (384001, 7999), **every) == -1 and "width" in _msg(L)
    tail.width = 1.0
    assert _file_tail(L, tail, big, (384001, 7999), **every) == -1
    assert "session_rate 7999" in _msg(L) and "the tail step needs the session's rate" in _msg(L)
    assert _file_tail(L, tail, big, (384001, RATE), **every) == -1
    assert "ir_rate 384001" in _msg(L) and "the tail step needs the session's rate" in _msg(L)
    assert _file_tail(L, tail, (1 << 40) + 1, (RATE, RATE), **every) == -1 and _msg(L) == f"IR of {(1 << 40) + 1} frames"
    assert _file_tail(L, tail, big, (RATE, RATE), **every) == -1 and _msg(L).startswith(f"length 0 takes the IR's {big} frames")
    # (F' is judged at the session's rate: 2^23 + 1 frames at 24 kHz are more than 2^24 at 48 kHz)
    assert _file_tail(L, tail, (1 << 23) + 1, (24000, RATE), **every) == -1 and _msg(L).startswith("length 0 takes the IR's")
    assert _file_tail(L, tail, **every) == -1 and "xover_hz" in _msg(L)
    assert _file_tail(L, tail, shape=shape, eq=eq) == -1 and "freq_hz" in _msg(L)
    assert _file_tail(L, tail, shape=shape) == -1 and "trim_db" in _msg(L)
    assert _file_tail(L, tail) == -1 and _msg(L) == "null argument"
    gd, ge, gs = _good()
    _, p = _lr()
    assert _file_tail(L, tail, lr=p, shape=gs, eq=ge, damp=gd) == -1 and _msg(L) == "null argument"
    # a band or a damping that is on needs the session's rate, as in mc_load_ir_damped: the tail's own rate check comes first
    assert _file_tail(L, tail, rates=(0, 0), damp=gd) == -1 and "the tail step needs the session's rate" in _msg(L)


@pytest.mark.parametrize("off", [None, "off"])
def test_file_load_with_the_tail_off_is_mc_load_ir_damped(off):
    """whatever else is wrong, and with a tail struct that would be refused were it on"""
    L = _lib.load()
    tail = None
    if off == "off":
        tail = _tail(mode="off")
        tail.width, tail.n_xovers = 9.0, 17
    bd, be, bs = _bad()
    gd, ge, gs = _good()
    _, p = _lr()
    cases = [
        dict(shape=bs, eq=be, damp=bd), dict(shape=bs, eq=be), dict(shape=bs), dict(), dict(lr=p), dict(shape=gs, eq=ge, damp=gd),
        dict(shape=gs, eq=ge, damp=gd, frames=(1 << 40) + 1), dict(damp=gd, rates=(0, 0)), dict(eq=ge, rates=(0, 0)), dict(shape=gs, rates=(0, 0)),
        dict(shape=gs, rates=(7999, RATE)), dict(rates=(44100, RATE), frames=(1 << 40) + 1), dict(rates=(44100, 7999)),
    ]
    for kw in cases:
        assert _damped(L, **kw) == -1
        want = _msg(L)
        assert _file_tail(L, tail, **kw) == -1 and _msg(L) == want, (kw, want, _msg(L))


def test_damped_load_refuses_damping_eq_shape_and_then_the_frames():
    L = _lib.load()
    damp, eq, shape = _bad()
    gd, ge, gs = _good()
    huge = (1 << 40) + 1
    assert _damped(L, huge, shape=shape, eq=eq, damp=damp) == -1 and "xover_hz" in _msg(L)
    assert _damped(L, huge, shape=shape, eq=eq, damp=gd) == -1 and "freq_hz" in _msg(L)
    assert _damped(L, huge, shape=shape, eq=ge, damp=gd) == -1 and "trim_db" in _msg(L)
    assert _damped(L, huge, shape=shape, damp=gd) == -1 and "trim_db" in _msg(L)  # (no eq: the default, which has no band)
    assert _damped(L, huge, shape=gs, eq=ge, damp=gd) == -1 and _msg(L) == f"IR of {huge} frames"
    assert _damped(L, huge, damp=gd) == -1 and _msg(L) == f"IR of {huge} frames"  # (no shape: the default)
    assert _damped(L, 1 << 40, shape=gs, eq=ge, damp=gd) == -1 and _msg(L) == "null argument"
    assert _damped(L, damp=gd) == -1 and _msg(L) == "null argument"


SWEEP = dict(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=RATE)


def _sweep_tail(L, tail, sweep, M=5000, offset=0, F=FRAMES, lr=None, shape=None, eq=None, damp=None):
    return L.mc_load_ir_sweep_tail(None, 0, lr, M, 1024, _ref(sweep), offset, F, _ref(shape), _ref(eq), _ref(damp), _ref(tail))


def _sweep_load(L, sweep, M=5000, offset=0, F=FRAMES, lr=None, shape=None, eq=None, damp=None):
    return L.mc_load_ir_sweep(None, 0, lr, M, 1024, _ref(sweep), offset, F, _ref(shape), _ref(eq), _ref(damp))


def test_sweep_load_with_a_tail_refuses_in_the_documented_order():
    """The tail, the sweep, the lengths, damping, eq, shape, the recording, the engine.  F' cannot be refused on this path: the
    lengths keep ir_frames inside [1, 2^24], which is F's own range, and a length above it is the tail's own refusal."""
    L = _lib.load()
    damp, eq, shape = _bad()
    every = dict(shape=shape, eq=eq, damp=damp)
    tail = _tail(width=2.0)
    sw = Sweep(**dict(SWEEP, rate=100)).to_c()
    assert _sweep_tail(L, tail, None, M=0, F=0, **every) == -1 and "width" in _msg(L)
    assert _sweep_tail(L, tail, sw, M=0, F=0, **every) == -1 and "width" in _msg(L)
    tail.width = 1.0
    assert _sweep_tail(L, tail, None, M=0, F=0, **every) == -1 and "null sweep" in _msg(L)
    assert _sweep_tail(L, tail, sw, M=0, F=0, **every) == -1 and "rate" in _msg(L)
    sw.rate = RATE
    assert _sweep_tail(L, tail, sw, M=0, F=0, **every) == -1 and "recording" in _msg(L)
    assert _sweep_tail(L, tail, sw, F=0, **every) == -1 and "ir_frames" in _msg(L)
    assert _sweep_tail(L, tail, sw, F=(1 << 24) + 1, **every) == -1 and "ir_frames" in _msg(L)
    tail.length = (1 << 24) + 1
    assert _sweep_tail(L, tail, sw, **every) == -1 and "length" in _msg(L)
    tail.length = 1 << 24
    assert _sweep_tail(L, tail, sw, **every) == -1 and "xover_hz" in _msg(L)
    assert _sweep_tail(L, tail, sw, shape=shape, eq=eq) == -1 and "freq_hz" in _msg(L)
    assert _sweep_tail(L, tail, sw, shape=shape) == -1 and "trim_db" in _msg(L)
    assert _sweep_tail(L, tail, sw) == -1 and _msg(L) == "null lr"
    gd, ge, gs = _good()
    assert _sweep_tail(L, tail, sw, shape=gs, eq=ge, damp=gd) == -1 and _msg(L) == "null lr"
    _, p = _lr(5000)
    assert _sweep_tail(L, tail, sw, lr=p, shape=gs, eq=ge, damp=gd) == -1 and _msg(L) == "null argument"


@pytest.mark.parametrize("off", [None, "off"])
def test_sweep_load_with_the_tail_off_is_mc_load_ir_sweep(off):
    L = _lib.load()
    tail = None
    if off == "off":
        tail = _tail(mode="off")
        tail.width, tail.n_xovers = 9.0, 17
    bd, be, bs = _bad()
    gd, ge, gs = _good()
    _, p = _lr(5000)
    sw, slow = Sweep(**SWEEP).to_c(), Sweep(**dict(SWEEP, rate=100)).to_c()
    for sweep, kw in ((None, {}), (slow, dict(M=0)), (sw, dict(M=0, F=0)), (sw, dict(F=0)), (sw, dict(shape=bs, eq=be, damp=bd)),
                      (sw, dict(shape=bs, eq=be)), (sw, dict(shape=bs)), (sw, {}), (sw, dict(lr=p)), (sw, dict(lr=p, shape=gs, eq=ge, damp=gd))):
        assert _sweep_load(L, sweep, **kw) == -1
        want = _msg(L)
        assert _sweep_tail(L, tail, sweep, **kw) == -1 and _msg(L) == want, (kw, want, _msg(L))


GETTERS = [("mc_ir_shape_info", 8), ("mc_ir_damp_info", 4), ("mc_ir_synth_info", 4), ("mc_ir_sweep_info", 4), ("mc_ir_tail_info", 4), ("mc_ir_room_info", 8)]


@pytest.mark.parametrize("name,count", GETTERS)
@pytest.mark.parametrize("idx", [0, 5, 1 << 40, (1 << 64) - 1])
def test_an_info_getter_without_an_engine_says_not_loaded(name, count, idx):
    """-1 (MC_ERR_ARG) and the index in the message, inside the engine's range of indices and outside it; out is not written"""
    L = _lib.load()
    out = (C.c_double * count)(*([7.0] * count))
    assert getattr(L, name)(None, idx, out) == -1 and _msg(L) == f"IR {idx} not loaded"
    assert list(out) == [7.0] * count
