"""The float64 restatement of the filter step (tests/ir_filter_np.py) against np.convolve and an exact round trip, and
mc_ir_filter with mc_ir_filter_plan and every refusal through the ABI (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ir_filter_np as FN

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")


# -- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,G", [(9, 8), (1, 1), (2000, 49), (2000, 50), (5000, 300), (300000, 20000)])
def test_convolution_agrees_with_np_convolve(F, G):
    """1e-14 of the peak: both are float64, the direct sum has F + G terms at most and the FFT log2(Nfft) stages."""
    a, b = FN.decaying_noise(F, 1), FN.decaying_noise(G, 2, right=1.0 / 3.0)
    y, info = FN.filter64(a, b)
    want = np.stack([np.convolve(a[:, ch].astype(np.float64), b[:, ch].astype(np.float64)) for ch in range(2)], axis=1)
    dev = np.abs(y - want).max() / np.abs(want).max()
    print(f"F {F}, G {G}: {dev:.2e} of the peak")
    assert y.shape == (F + G - 1, 2) and dev <= 1e-14
    assert info["frames_out"] == F + G - 1 and info["nfft"] == FN.nfft_of(F, G) and info["regularised"] == (0, 0)
    assert info["energy_rest"] <= 1e-28 * info["energy_out"]


def test_the_channel_maps():
    a, b = FN.decaying_noise(300, 1), FN.decaying_noise(40, 2, right=1.0 / 3.0)
    for channels, one in (("left", b[:, 0].astype(np.float64)), ("mid", 0.5 * (b[:, 0].astype(np.float64) + b[:, 1]))):
        y, info = FN.filter64(a, b, channels=channels)
        for ch in range(2):
            want = np.convolve(a[:, ch].astype(np.float64), one)
            assert np.abs(y[:, ch] - want).max() <= 1e-14 * np.abs(want).max()
        assert abs(info["energy_filter"] - 2.0 * float((one * one).sum())) <= 1e-15 * info["energy_filter"]


@pytest.mark.parametrize("n,G", [(10, 4), (2000, 40), (60000, 5), (500000, 4)])
def test_the_integer_round_trip_is_exact(n, G):
    """a = h * b in integers, exact in float32; b = 8 and small values has |B| >= 5 everywhere, so with reg_db 200 the quotient is h
    to parts in 1e-12 against a half ulp of 6e-8 (|h| >= 1): it rounds to h bit for bit."""
    a, b, h = FN.integer_round_trip(n, G)
    assert a.shape == (n + G - 1, 2) and (np.abs(h) >= 1.0).all() and (a.astype(np.float64) == np.round(a)).all()
    y64, info = FN.filter64(a, b, op="deconvolve", reg_db=200.0, frames_out=n)
    err = np.abs(y64 - h).max()
    print(f"n {n}, G {G}: largest error {err:.2e}, min p / pm {min(info['condition']):.3f}")
    assert err <= 1e-10 and (y64.astype(np.float32) == h).all()
    assert info["frames_out"] == n and info["regularised"] == (0, 0)


def test_deconvolution_of_a_zero_filter_channel_and_of_a_comb():
    a = FN.decaying_noise(2000, 1)
    b = FN.decaying_noise(100, 2).copy()
    b[:, 1] = 0.0
    y, info = FN.filter64(a, b, op="deconvolve")
    assert not y[:, 1].any() and y[:, 0].any() and info["regularised"][1] == 0 and y.shape == (2000, 2)
    N = 4096
    y, info = FN.filter64(a, FN.comb(N), op="deconvolve", reg_db=20.0)
    assert info["nfft"] == N and info["regularised"] == (N // 4, N // 4) and np.isfinite(y).all()


# -- plan and ABI -----------------------------------------------------------------------------------------------------
def _filter(**fields):
    from cuda_audio_amd import _lib

    f = _lib.McIrFilter()
    _lib.load().mc_default_ir_filter(C.byref(f))
    f.op = _lib.MC_FILTER_CONVOLVE
    for k, v in fields.items():
        setattr(f, k, v)
    return f


def test_the_struct_has_its_documented_size_and_defaults():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_filter\) = (\d+)", src).group(1))
    f = _lib.McIrFilter()
    _lib.load().mc_default_ir_filter(C.byref(f))
    assert C.sizeof(_lib.McIrFilter) == size == f.struct_size == 32
    assert (f.op, f.channels, f.rate, f.reg_db, f.reserved, f.frames_out) == (_lib.MC_FILTER_OFF, _lib.MC_FILTER_STEREO, 0, 60.0, 0, 0)
    assert re.search(r"enum \{ MC_FILTER_OFF = 0, MC_FILTER_CONVOLVE = 1, MC_FILTER_DECONVOLVE = 2 \};", src)
    assert re.search(r"enum \{ MC_FILTER_STEREO = 0, MC_FILTER_LEFT = 1, MC_FILTER_MID = 2 \};", src)
    assert re.search(r"#define MC_ABI_VERSION 1\b", src)
    assert {"mc_default_ir_filter", "mc_ir_filter_plan", "mc_load_ir_filter", "mc_load_ir_sweep_filter", "mc_ir_filter_info"} <= set(_lib.SYMBOLS)


def test_the_python_dataclass():
    from cuda_audio_amd.engine import IrFilter

    ir = np.zeros((5, 2), np.float32)
    f = IrFilter(ir=ir).to_c()
    assert (f.struct_size, f.op, f.channels, f.rate, f.reg_db, f.reserved, f.frames_out) == (32, 1, 0, 0, 60.0, 0, 0)
    f = IrFilter(ir=ir, op="deconvolve", channels="mid", rate=44100, reg_db=90.0, frames_out=77).to_c()
    assert (f.op, f.channels, f.rate, f.reg_db, f.frames_out) == (2, 2, 44100, 90.0, 77)
    assert IrFilter(ir=ir, op="off", channels="left").to_c().channels == 1

    class Wav:
        buffer, sampleRate = ir, 96000

    assert IrFilter(ir=Wav()).to_c().rate == 96000 and IrFilter(ir=Wav(), rate=48000).to_c().rate == 48000
    assert IrFilter(ir=Wav()).frames().shape == (5, 2)
    for bad in (dict(op="multiply"), dict(channels="right")):
        with pytest.raises(ValueError):
            IrFilter(ir=ir, **bad).to_c()


def _plan(f, frames, filter_frames, out=True):
    from cuda_audio_amd import _lib

    L = _lib.load()
    buf = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    rc = L.mc_ir_filter_plan(C.byref(f) if f is not None else None, frames, filter_frames, buf if out else None)
    return rc, L.mc_last_error().decode(), list(buf)


def test_the_plan():
    from cuda_audio_amd.engine import IrFilter, filter_plan

    for F, G in ((1, 1), (9, 8), (10, 8), (2000, 49), (2000, 50), (5000, 300), (60000, 5537), (60000, 5538), (1 << 21, 1 << 21), ((1 << 22) - 1, 2)):
        for op in ("convolve", "deconvolve"):
            N = FN.nfft_of(F, G)
            got = filter_plan(IrFilter(ir=np.zeros((G, 2), np.float32), op=op), F)
            passes = 1 if N <= 2048 else 2
            assert got["nfft"] == N and got["passes"] == passes and got["frames_out"] == FN.frames_out_of(F, G, op), (F, G, op, got)
            # the filter's G float2, two buffers of Nfft double2, a third with two passes, 16 bytes of partials per 256 points
            assert got["device_bytes"] == 8 * G + (passes + 1) * 16 * N + 16 * ((N + 255) // 256), (F, G, op, got)
    # a filter at another rate is planned over its frames at the session's: ceil(441 * 160 / 147) = 480
    got = filter_plan(IrFilter(ir=np.zeros((441, 2), np.float32), rate=44100), 1000, session_rate=48000)
    assert got["frames_out"] == 1000 + 480 - 1
    rc, _, out = _plan(_filter(op=0), 1000, 25)  # (off is planned as a convolution)
    assert rc == 0 and out == [1024.0, 1.0, 8.0 * 25 + 2.0 * 16 * 1024 + 16 * 4, 1024.0]
    rc, _, out = _plan(_filter(op=2, frames_out=4096), 2000, 2000)
    assert rc == 0 and out[0] == 4096.0 and out[3] == 4096.0
    rc, _, out = _plan(_filter(frames_out=3), 2000, 2000)
    assert rc == 0 and out[3] == 3.0


BAD_FIELDS = [("struct_size", dict(struct_size=28)), ("op", dict(op=3)), ("channels", dict(channels=3)), ("rate", dict(rate=7999)), ("rate", dict(rate=384001)),
              ("reg_db", dict(reg_db=19.9)), ("reg_db", dict(reg_db=200.5)), ("reg_db", dict(reg_db=float("nan"))), ("reserved", dict(reserved=1))]
ORDER = [("op", dict(op=9)), ("channels", dict(channels=9)), ("rate", dict(rate=5)), ("reg_db", dict(reg_db=1.0)), ("reserved", dict(reserved=7))]


def test_the_plan_refuses():
    rc, msg, _ = _plan(None, 100, 10)
    assert rc == -1 and "null filter" in msg
    for name, fields in BAD_FIELDS:
        rc, msg, out = _plan(_filter(**fields), 100, 10)
        assert rc == -1 and name in msg and out == [-1.0] * 4, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):  # (of two bad fields the earlier one is named)
        rc, msg, _ = _plan(_filter(**dict(a, **b)), 100, 10)
        assert rc == -1 and first in msg, (first, msg)
    rc, msg, _ = _plan(_filter(), 0, 10)
    assert rc == -1 and "empty IR" in msg
    rc, msg, _ = _plan(_filter(), 10, 0)
    assert rc == -1 and "filter_frames" in msg
    rc, msg, _ = _plan(_filter(), (1 << 21) + 1, 1 << 21)
    assert rc == 0
    rc, msg, _ = _plan(_filter(), (1 << 21) + 2, 1 << 21)
    assert rc == -1 and "frames" in msg and "2097154" in msg and "2097152" in msg, msg
    rc, msg, _ = _plan(_filter(frames_out=2050), 2000, 50)
    assert rc == -1 and "frames_out" in msg and "2049" in msg, msg
    rc, msg, _ = _plan(_filter(op=2, frames_out=4097), 2000, 50)
    assert rc == -1 and "frames_out" in msg and "4096" in msg, msg
    rc, msg, _ = _plan(_filter(), 100, 10, out=False)
    assert rc == -1 and "null out" in msg


def _load(f, frames=100, rates=(0, 0), lr=True, flr=True, G=10, engine=None, tail=None, shape=None, phase=None):
    from cuda_audio_amd import _lib

    L = _lib.load()
    buf = np.zeros((max(min(frames, 1000), 1), 2), np.float32)
    fbuf = np.zeros((max(min(G, 1000), 1), 2), np.float32)
    fp = C.POINTER(C.c_float)
    rc = L.mc_load_ir_filter(engine, 0, buf.ctypes.data_as(fp) if lr else None, frames, 1024, rates[0], rates[1], shape, None, None, tail, phase,
                             C.byref(f) if f is not None else None, fbuf.ctypes.data_as(fp) if flr else None, G)
    return rc, L.mc_last_error().decode()


def _load_sweep(f, ir_frames=900, tail=None, phase=None, lr=True, flr=True, G=10):
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import Sweep

    L = _lib.load()
    rec = np.zeros((5000, 2), np.float32)
    fbuf = np.zeros((max(min(G, 1000), 1), 2), np.float32)
    sw = Sweep(frames=4096, f1_hz=20.0, f2_hz=3000.0, rate=8000).to_c()
    fp = C.POINTER(C.c_float)
    rc = L.mc_load_ir_sweep_filter(None, 0, rec.ctypes.data_as(fp) if lr else None, len(rec), 1024, C.byref(sw), 0, ir_frames, None, None, None, tail, phase,
                                   C.byref(f) if f is not None else None, fbuf.ctypes.data_as(fp) if flr else None, G)
    return rc, L.mc_last_error().decode()


def test_the_loads_refuse_in_the_documented_order_before_the_engine_is_looked_at():
    """No engine is passed: a call that gets past the checks ends at "null argument", the load's own first check."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    for name, fields in BAD_FIELDS:
        for rates in ((0, 0), (8000, 8000), (1, 2)):  # (the filter comes before the rates)
            rc, msg = _load(_filter(**fields), rates=rates)
            assert rc == -1 and name in msg, (name, msg)
        rc, msg = _load_sweep(_filter(**fields))
        assert rc == -1 and name in msg, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):
        rc, msg = _load(_filter(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # the filter before a bad phase, a bad tail and a bad shape; a good filter lets them speak, in that order
    phase = _lib.McIrPhase()
    L.mc_default_ir_phase(C.byref(phase))
    phase.mode, phase.over_log2 = _lib.MC_PHASE_MINIMUM, 0
    tail = _lib.McIrTail()
    L.mc_default_ir_tail(C.byref(tail))
    tail.mode, tail.width = _lib.MC_TAIL_EXTEND, 7.0
    shape = _lib.McIrShape()
    L.mc_default_ir_shape(C.byref(shape))
    shape.trim_db = 5.0
    every = dict(rates=(8000, 8000), tail=C.byref(tail), shape=C.byref(shape), phase=C.byref(phase))
    rc, msg = _load(_filter(reserved=3), **every)
    assert rc == -1 and "reserved" in msg
    rc, msg = _load(_filter(), **every)
    assert rc == -1 and "over_log2" in msg
    rc, msg = _load_sweep(_filter(reserved=3), tail=C.byref(tail), phase=C.byref(phase))
    assert rc == -1 and "reserved" in msg
    rc, msg = _load_sweep(_filter(), tail=C.byref(tail), phase=C.byref(phase))
    assert rc == -1 and "over_log2" in msg
    phase.over_log2 = 3
    rc, msg = _load(_filter(), **every)
    assert rc == -1 and "width" in msg
    rc, msg = _load_sweep(_filter(), tail=C.byref(tail), phase=C.byref(phase))
    assert rc == -1 and "width" in msg
    rc, msg = _load(_filter(), shape=C.byref(shape), phase=C.byref(phase))
    assert rc == -1 and "trim_db" in msg
    phase.mode = _lib.MC_PHASE_OFF  # (a phase that is off is not looked at)
    phase.over_log2 = 0
    rc, msg = _load(_filter(), shape=C.byref(shape), phase=C.byref(phase))
    assert rc == -1 and "trim_db" in msg
    # the step's limits after the phase step's, as soon as F is known; a bad shape comes before them without a tail, after them with one
    phase.mode, phase.over_log2 = _lib.MC_PHASE_MINIMUM, 3
    rc, msg = _load(_filter(), frames=(1 << 21) + 1, G=1 << 21, phase=C.byref(phase))
    assert rc == -1 and "the phase step" in msg, msg
    rc, msg = _load(_filter(), frames=(1 << 21) + 2, G=1 << 21)
    assert rc == -1 and "transform" in msg and "2097154" in msg, msg
    rc, msg = _load(_filter(), frames=(1 << 21) + 2, G=1 << 21, shape=C.byref(shape))
    assert rc == -1 and "trim_db" in msg, msg
    tail.width = 1.0
    rc, msg = _load(_filter(frames_out=200), frames=100, G=10, rates=(8000, 8000), tail=C.byref(tail), shape=C.byref(shape))
    assert rc == -1 and "frames_out" in msg, msg
    rc, msg = _load(_filter(), G=0)
    assert rc == -1 and "filter_frames" in msg, msg
    rc, msg = _load(_filter(), G=(1 << 40) + 1)
    assert rc == -1 and "filter_frames" in msg, msg
    rc, msg = _load(_filter(frames_out=110), frames=100, G=10)
    assert rc == -1 and "frames_out" in msg and "109" in msg, msg
    rc, msg = _load(_filter(op=2, frames_out=129), frames=100, G=10)
    assert rc == -1 and "frames_out" in msg and "128" in msg, msg
    rc, msg = _load(_filter(op=2, frames_out=128), frames=100, G=10)
    assert rc == -1 and "null argument" in msg, msg
    # the filter's own rate: converted lengths count (10 frames at 8 kHz are 480 at 384 kHz), and it needs a session rate
    rc, msg = _load(_filter(rate=8000, frames_out=580), frames=100, G=10, rates=(384000, 384000))
    assert rc == -1 and "frames_out" in msg and "579" in msg, msg
    rc, msg = _load(_filter(rate=8000, frames_out=579), frames=100, G=10, rates=(384000, 384000))
    assert rc == -1 and "null argument" in msg, msg
    rc, msg = _load(_filter(rate=8000), rates=(0, 0))
    assert rc == -1 and "session" in msg and "rate" in msg, msg
    rc, msg = _load(_filter(rate=8000), rates=(8000, 7999))
    assert rc == -1 and "session_rate" in msg, msg
    rc, msg = _load_sweep(_filter(frames_out=910), ir_frames=900, G=10)
    assert rc == -1 and "frames_out" in msg and "909" in msg, msg
    rc, msg = _load_sweep(_filter(rate=16000, frames_out=905), ir_frames=900, G=10)  # (the session's rate is the sweep's: G = 5)
    assert rc == -1 and "frames_out" in msg and "904" in msg, msg
    # pointers last
    rc, msg = _load(_filter(frames_out=110), flr=False)
    assert rc == -1 and "frames_out" in msg, msg
    rc, msg = _load(_filter(), flr=False)
    assert rc == -1 and "null filter_lr" in msg, msg
    rc, msg = _load_sweep(_filter(), flr=False)
    assert rc == -1 and "null filter_lr" in msg, msg
    rc, msg = _load_sweep(_filter(), lr=False, flr=False)
    assert rc == -1 and "null lr" in msg, msg
    for rc, msg in (_load(_filter()), _load(_filter(), lr=False), _load_sweep(_filter())):
        assert rc == -1 and "null argument" in msg, msg
    # off and null: the wrapped load itself, which does not look at the filter's frames and here ends at its own null engine
    off = _filter(op=0, struct_size=3, channels=9, rate=1, reg_db=float("nan"), reserved=5)
    for f in (None, off):
        rc, msg = _load(f, flr=False, G=0)
        assert rc == -1 and "null argument" in msg, msg
        rc, msg = _load_sweep(f, flr=False, G=0)
        assert rc == -1 and "null argument" in msg, msg
