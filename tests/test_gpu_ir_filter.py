"""The filter step of an IR load on the device (mc_load_ir_filter, mc_load_ir_sweep_filter; csrc/irfilter.hip.h over
csrc/fft64.hip.h): the stored taps and mc_ir_filter_info against the float64 restatement (tests/ir_filter_np.py, numpy's FFT, one
channel at a time), the parts of the definition that are exact (an integer round trip, a step that is off, repeated loads,
refused loads), a filter at another rate, a sweep capture, and the chain with the phase step, shape, EQ and damping into the
engine's output.

The bound per tap is |got - want| <= 2^-23 |want| + 1e-12 peak, that of tests/test_gpu_ir_phase.py and for its reason: both
pipelines are double and differ by parts in 1e-15 of the peak, and the rounding to float then differs by at most one ulp, at a
tie.  `peak` is the larger channel's: the device carries both channels through one complex transform, so its rounding error is
relative to that one.  The filter's right channel is different noise at a third of the left's level, so a sign error at a
mirrored bin shows as crosstalk.  profiles/irfilter.md has what an MI355X showed: never more than 8.1e-17 of the peak above one ulp."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_filter_np as FN
import ir_phase_np
from helpers import BASE, RMS_TOL, apply_params, rms
from test_gpu_ir_shape import _check_taps

pytestmark = pytest.mark.gpu

RATE = 48000


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irfilter", n_ref, sample_rate=rate, **kw)


def _filter(ir, **kw):
    from cuda_audio_amd.engine import IrFilter

    return IrFilter(ir=ir, **kw)


def _n_ref(F):
    n = 16384
    while n < F + 1024 + 1:
        n *= 2
    return n


@functools.lru_cache(maxsize=None)
def _inputs(F, G, lift=0.0, db=60.0):
    """(frames, filter frames), made once per size and never written to; lift is added to the filter's first frame (both
    channels), which keeps its spectrum away from zero for a deconvolution."""
    a, b = FN.decaying_noise(F, 1, db=db), FN.decaying_noise(G, 2, right=1.0 / 3.0, db=db).copy()
    b[0] += np.float32(lift)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def _check_bound(got, want32, peak=None):
    w = want32.astype(np.float64)
    err = np.abs(got.astype(np.float64) - w)
    peak = np.abs(w).max() if peak is None else peak
    slack = err - 2.0 ** -23 * np.abs(w)
    print(f"taps: largest deviation {err.max():.3e} (peak {peak:.3e}), largest excess over one ulp {slack.max() / peak:.3e} of the peak, "
          f"{np.count_nonzero(got != want32)} of {got.size} values differ")
    assert got.shape == want32.shape
    assert (slack <= 1e-12 * peak).all(), f"excess {slack.max() / peak:.3e} of the peak at {np.unravel_index(slack.argmax(), slack.shape)}"


def _check_info(got, want):
    print("filter info:", got, "restated:", {k: v for k, v in want.items() if k != "condition"})
    for k in ("frames", "filter_frames", "frames_out", "nfft"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert tuple(got["regularised"]) == tuple(want["regularised"])
    for k in ("energy_in", "energy_filter", "energy_out"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert abs(got["energy_rest"] - want["energy_rest"]) <= 1e-12 * (want["energy_out"] + want["energy_rest"])


def _load_and_check(a, b, **kw):
    """One load of a with the filter b on a fresh engine: taps and info against the restatement; the taps come back."""
    want, winfo = FN.filtered(a, b, **kw)
    c = _conv(_n_ref(want.shape[0]))
    c.prepare(0, a, filter=_filter(b, **kw))
    got, info, sinfo = c.ir_taps(0), c.ir_filter_info(0), c.ir_shape_info(0)
    c.close()
    assert sinfo["frames"] == sinfo["taps"] == want.shape[0] and sinfo["gain"] == 1.0
    _check_bound(got, want)
    _check_info(info, winfo)
    return got, winfo


# Nfft = 16 (the smallest, and single frames), 2048 (the last with one pass), 4096 (the first with two), 8192, 2^16 and 2^18
@pytest.mark.parametrize("F,G,nfft", [(9, 8, 16), (1, 1, 16), (2000, 49, 2048), (2000, 50, 4096), (5000, 300, 8192), (40000, 20000, 1 << 16),
                                      (200000, 50000, 1 << 18)])
def test_convolved_taps_match_the_restatement(gpu_lib, F, G, nfft):
    assert FN.nfft_of(F, G) == nfft
    _load_and_check(*_inputs(F, G))


def test_the_largest_transform(gpu_lib):
    """F = G = 2^21: Nfft = 2^22 = 2048 x 2048.  The shape keeps a window of 4096 of the 2^22 - 1 frames, in the middle where both
    halves of the padding meet, so that n_ref stays 16384; noise that decays by 20 dB keeps the window near the peak's level."""
    from cuda_audio_amd.engine import IrShape

    F = G = 1 << 21
    a, b = _inputs(F, G, db=20.0)
    start, length = F - 2048, 4096
    assert FN.nfft_of(F, G) == FN.MAX_NFFT
    want, winfo = FN.filtered(a, b)
    c = _conv(16384)
    c.prepare(0, a, shape=IrShape(start=start, length=length), filter=_filter(b))
    got, info, sinfo = c.ir_taps(0), c.ir_filter_info(0), c.ir_shape_info(0)
    c.close()
    assert sinfo["frames"] == 2 * F - 1 and sinfo["taps"] == length and sinfo["gain"] == 1.0
    _check_bound(got, want[start:start + length])
    _check_info(info, winfo)


@pytest.mark.parametrize("op,lift", [("convolve", 0.0), ("deconvolve", 4.0)])
@pytest.mark.parametrize("channels", ["stereo", "left", "mid"])
def test_the_channel_maps(gpu_lib, op, lift, channels):
    """All three maps at a two-pass size, for both operations."""
    a, b = _inputs(5000, 300, lift)
    _, winfo = _load_and_check(a, b, op=op, channels=channels, reg_db=80.0)
    assert winfo["regularised"] == (0, 0)


# -- deconvolution ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G", [(10, 4), (2000, 40), (60000, 5)])
def test_the_integer_round_trip_is_bit_for_bit(gpu_lib, n, G):
    """a = h * b in integers that float32 holds exactly; dividing b out with reg_db 200 and frames_out = len(h) stores h itself."""
    a, b, h = FN.integer_round_trip(n, G)
    c = _conv(_n_ref(n))
    c.prepare(0, a, filter=_filter(b, op="deconvolve", reg_db=200.0, frames_out=n))
    got, info = c.ir_taps(0), c.ir_filter_info(0)
    c.close()
    print(f"n {n}, G {G}: {np.count_nonzero(got != h)} of {h.size} values differ, largest deviation {np.abs(got - h).max():.3e}")
    assert got.shape == h.shape and got.tobytes() == h.tobytes()
    assert info["frames"] == n + G - 1 and info["frames_out"] == n and info["regularised"] == (0, 0)


@pytest.mark.parametrize("reg_db", [60.0, 120.0])
def test_a_well_conditioned_filter(gpu_lib, reg_db):
    a, b = _inputs(1500, 400, 4.0)
    _, winfo = _load_and_check(a, b, op="deconvolve", reg_db=reg_db)
    print("min p / pm:", winfo["condition"])
    assert min(winfo["condition"]) >= 1e-4 and winfo["regularised"] == (0, 0)


def test_a_regularised_comb(gpu_lib):
    """delta[0] - delta[Nfft / 4]: |B|^2 is 0, 2 or 4, so with reg_db 20 (eps pm = 0.04) exactly the Nfft / 4 bins at its zeros are regularised."""
    N = 4096
    a = _inputs(2000, 50)[0]
    b = FN.comb(N)
    assert FN.nfft_of(len(a), len(b)) == N
    c = _conv(16384)
    c.prepare(0, a, filter=_filter(b, op="deconvolve", reg_db=20.0))
    got, info = c.ir_taps(0), c.ir_filter_info(0)
    c.close()
    want, winfo = FN.filtered(a, b, op="deconvolve", reg_db=20.0)
    assert info["regularised"] == (N // 4, N // 4) == winfo["regularised"]
    _check_bound(got, want)
    _check_info(info, winfo)


def test_an_all_zero_filter_channel_stores_zeros(gpu_lib):
    a, b = _inputs(2000, 50, 4.0)
    for channel in (0, 1):
        z = b.copy()
        z[:, channel] = 0.0
        got, winfo = _load_and_check(a, z, op="deconvolve")
        assert not got[:, channel].any() and got[:, 1 - channel].any() and winfo["regularised"][channel] == 0
    z = np.zeros_like(b)
    z[:, 1] = b[:, 0]  # (left: the one signal is all zeros)
    c = _conv(16384)
    c.prepare(0, a, filter=_filter(z, op="deconvolve", channels="left"))
    taps, info = c.ir_taps(0), c.ir_filter_info(0)
    c.close()
    assert taps.shape == (2000, 2) and not taps.any() and info["energy_out"] == 0.0 and info["regularised"] == (0, 0)


# -- the exact parts --------------------------------------------------------------------------------------------------
def _off_filter():
    """MC_FILTER_OFF with nonsense in every other field."""
    from cuda_audio_amd import _lib

    f = _lib.McIrFilter()
    f.struct_size, f.op, f.channels, f.rate, f.reg_db, f.reserved, f.frames_out = 7, _lib.MC_FILTER_OFF, 9, 1, float("nan"), 5, 1 << 60
    return f


def test_a_filter_that_is_off_is_the_wrapped_load_bit_for_bit(gpu_lib):
    """filter = None (Python and C) and MC_FILTER_OFF against prepare(phase=...) and prepare_sweep(phase=...) without one."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrPhase, IrShape, IrTail, _fp
    from test_gpu_ir_sweep import _recorded, _sw

    ir = np.ascontiguousarray(ir_phase_np.delayed_noise(5000))
    other = np.ascontiguousarray(_inputs(5000, 300)[1])
    fields, rec = _recorded("A")
    rec = np.ascontiguousarray(rec)
    shape = IrShape(fade_out=100, normalize="peak", target=0.05)
    tail = IrTail(mode="cut", xovers=(1000,), knee=(3000, 2500), fade=64)
    phase = IrPhase()
    outs = []
    for how in ("without", "none", "off", "c_null", "c_off"):
        c = _conv(16384)
        L, off = c._L, _off_filter()
        if how in ("without", "none", "off"):
            kw = {} if how == "without" else dict(filter=None if how == "none" else _filter(other, op="off"))
            c.prepare(0, ir, ir_rate=44100, shape=shape, tail=tail, phase=phase, **kw)
            c.prepare(1, ir, **kw)
            c.prepare_sweep(2, rec, _sw(fields), offset=-64, ir_frames=1024, shape=shape, phase=phase, **kw)
        else:
            f = None if how == "c_null" else C.byref(off)
            s, t, p, sw = shape.to_c(), tail.to_c(), phase.to_c(), _sw(fields).to_c()
            sw.rate = RATE
            assert L.mc_load_ir_filter(c._h, 0, _fp(ir), len(ir), 1024, 44100, RATE, C.byref(s), None, None, C.byref(t), C.byref(p), f, None, 0) == 0
            assert L.mc_load_ir_filter(c._h, 1, _fp(ir), len(ir), 1024, 0, 0, None, None, None, None, None, f, None, 0) == 0
            assert L.mc_load_ir_sweep_filter(c._h, 2, _fp(rec), len(rec), 1024, C.byref(sw), -64, 1024, C.byref(s), None, None, None, C.byref(p), f, None, 0) == 0
        for idx in range(3):
            with pytest.raises(McError) as ex:
                c.ir_filter_info(idx)
            assert ex.value.code == -3
        assert c.ir_phase_info(0)["frames"] > 0 and c.ir_phase_info(2)["frames"] == 1024
        outs.append([c.ir_taps(i) for i in range(3)] + [c.ir_spectra(i) for i in range(3)] + [c.ir_info(i) for i in range(3)])
        c.close()
    for other_out in outs[1:]:
        for x, y in zip(outs[0], other_out):
            if isinstance(x, dict):
                assert x == y
            else:
                assert x.tobytes() == y.tobytes()


def test_the_same_load_stores_the_same_bits(gpu_lib):
    """Twice on one engine and once on another: one pass (F = 200) and two (F = 5000), every spectral kernel."""
    for F, G, kw in ((200, 30, dict()), (200, 30, dict(op="deconvolve")), (5000, 300, dict()), (5000, 300, dict(op="deconvolve")),
                     (5000, 300, dict(channels="mid")), (5000, 300, dict(op="deconvolve", channels="left"))):
        a, b = _inputs(F, G, 4.0)
        taps = []
        for engine in range(2):
            c = _conv(16384)
            for idx in range(2 - engine):
                c.prepare(idx, a, filter=_filter(b, **kw))
                taps.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_filter_info(idx)))
            c.close()
        for t, s, i in taps[1:]:
            assert t.tobytes() == taps[0][0].tobytes() and s.tobytes() == taps[0][1].tobytes() and i == taps[0][2], (F, G, kw)


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd import _lib
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, IrPhase, IrShape, _fp

    a, b = (np.ascontiguousarray(v) for v in _inputs(5000, 300))
    c = _conv(16384)
    c.prepare(0, a, shape=IrShape(fade_out=100), phase=IrPhase(), filter=_filter(b))

    def state():
        return (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_phase_info(0), c.ir_filter_info(0), c.num_irs())

    before = state()
    L = c._L
    good = _lib.McIrFilter()
    L.mc_default_ir_filter(C.byref(good))
    good.op = _lib.MC_FILTER_CONVOLVE
    for field, value in (("struct_size", 36), ("op", 3), ("channels", 3), ("rate", 100), ("reg_db", 10.0), ("reserved", 1), ("frames_out", 5300)):
        f = _lib.McIrFilter.from_buffer_copy(good)
        setattr(f, field, value)
        for idx in (0, 1):
            assert L.mc_load_ir_filter(c._h, idx, _fp(a), len(a), 1024, RATE, RATE, None, None, None, None, None, C.byref(f), _fp(b), len(b)) == -1
            assert field in L.mc_last_error().decode()
    for idx in (0, 1):
        assert L.mc_load_ir_filter(c._h, idx, _fp(a), len(a), 1024, RATE, RATE, None, None, None, None, None, C.byref(good), None, len(b)) == -1
        assert "filter_lr" in L.mc_last_error().decode()
        assert L.mc_load_ir_filter(c._h, idx, _fp(a), len(a), 1024, RATE, RATE, None, None, None, None, None, C.byref(good), _fp(b), 1 << 22) == -1
        assert "frames" in L.mc_last_error().decode()
        assert L.mc_load_ir_filter(c._h, idx, _fp(a), len(a), 1024, 0, 0, None, None, None, None, None, C.byref(good), _fp(b), 0) == -1
        assert "filter_frames" in L.mc_last_error().decode()
    small = np.ascontiguousarray(_inputs(2000, 50)[0])
    for kw in (dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=6000)), dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(ir_rate=7999),
               dict(nframes=16384), dict(phase=IrPhase(floor_db=1.0))):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, small, filter=_filter(b), **kw)
            assert ex.value.code == -1, kw
    with pytest.raises(McError) as ex:
        c.ir_filter_info(1)
    assert ex.value.code == -1
    assert state() == before
    # a plain load over a filtered one leaves no filter information behind
    c.prepare(0, small)
    with pytest.raises(McError) as ex:
        c.ir_filter_info(0)
    assert ex.value.code == -3
    c.close()


# -- with the other sources and steps ---------------------------------------------------------------------------------
def test_a_sweep_capture_with_a_filter(gpu_lib):
    """prepare_sweep(filter=): the step acts on the deconvolved frames, which the plain capture stores.  Here it divides a
    short loop-back response out of them."""
    from test_gpu_ir_sweep import _recorded, _sw

    fields, rec = _recorded("A")
    F = 1024
    b = _inputs(2000, 50, 4.0)[1]
    c = _conv(16384)
    c.prepare_sweep(0, rec, _sw(fields), offset=-64, ir_frames=F)
    frames = c.ir_taps(0)
    for idx, kw in ((1, dict(op="deconvolve", reg_db=80.0)), (2, dict(channels="mid"))):
        want, winfo = FN.filtered(frames, b, **kw)
        c.prepare_sweep(idx, rec, _sw(fields), offset=-64, ir_frames=F, filter=_filter(b, **kw))
        got, info = c.ir_taps(idx), c.ir_filter_info(idx)
        assert c.ir_sweep_info(idx)["frames"] == F and c.ir_shape_info(idx)["frames"] == want.shape[0]
        _check_bound(got, want)
        _check_info(info, winfo)
    c.close()


def test_a_filter_at_another_rate(gpu_lib):
    """A filter at 44.1 kHz in a 48 kHz session: the step against the restatement fed the frames that a plain resampled load of
    that filter stores; rate comes from the struct, from a WAV object's sampleRate, or is the session's."""
    a, b = _inputs(5000, 300, 4.0)
    c = _conv(16384)
    c.prepare(0, b, ir_rate=44100)
    b48 = c.ir_taps(0)
    G = -(-300 * 160 // 147)
    assert b48.shape == (G, 2)

    class Wav:
        buffer, sampleRate = b, 44100

    for idx, f in ((1, _filter(b, rate=44100)), (2, _filter(Wav())), (3, _filter(Wav(), op="deconvolve", channels="left", reg_db=40.0))):
        kw = dict(op=f.op, channels=f.channels, reg_db=f.reg_db)
        want, winfo = FN.filtered(a, b48, **kw)
        c.prepare(idx, a, filter=f)
        assert c.ir_filter_info(idx)["filter_frames"] == G
        _check_bound(c.ir_taps(idx), want)
        _check_info(c.ir_filter_info(idx), winfo)
    want, winfo = FN.filtered(a, b)
    c.prepare(4, a, filter=_filter(b, rate=RATE))
    _check_bound(c.ir_taps(4), want)
    _check_info(c.ir_filter_info(4), winfo)
    c.close()


def test_the_chain_into_the_output(oracle_mod, gpu_lib):
    """Minimum phase, then the filter, then a shape that normalises, damping and an EQ band: the stored taps against the float64
    restatements chained in the documented order (1b, 1c, then 2 .. 8), and 8 periods and one batch against the oracle fed the
    restated taps."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrPhase, IrShape
    from cuda_audio_amd.synth import make_input

    n_ref, F, G = 16384, 1500, 4500
    cab = ir_phase_np.delayed_noise(F)
    room = FN.decaying_noise(G, 3, right=0.7)
    xovers, decay, origin = (400, 1600), (0, 4800, 1600), 10
    bands = [("peak", 1000.0, 4.0, 1.0)]
    fields = dict(fade_out=200, normalize="peak", target=0.05)
    y32 = ir_phase_np.min_phase(cab)[0]
    z32, finfo = FN.filtered(y32, room)
    want, winfo, wdinfo = ir_damp_np.damp64(z32, n_ref - 1024, RATE, RATE, xovers, decay, origin, bands, **fields)
    c = _conv(n_ref, max_batch=32)
    c.prepare(0, cab, shape=IrShape(**fields), eq=IrEq(bands=bands), damp=IrDamp(xovers=xovers, decay=decay, origin=origin), phase=IrPhase(),
              filter=_filter(room))
    c.prepare(1, cab)
    got = c.ir_taps(0)
    _check_taps(got, want)
    sinfo = c.ir_shape_info(0)
    assert sinfo["frames"] == F + G - 1 and sinfo["taps"] == winfo["taps"] and abs(sinfo["gain"] - winfo["gain"]) <= 1e-6 * winfo["gain"]
    assert c.ir_damp_info(0) == wdinfo and c.ir_phase_info(0)["frames"] == F
    _check_info(c.ir_filter_info(0), finfo)
    assert abs(np.abs(got).max() - 0.05) <= 1e-6 * 0.05
    taps = [want.astype(np.float32), cab[:n_ref - 1024]]
    p1 = dict(BASE, select=1, level=0.8)
    xin = make_input(40 * 256)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, BASE, p1, True)
    out = ref.process(xin[0], xin[1])
    assert rms(out) > 0.01
    apply_params(c, BASE, p1, False)
    mine = [np.stack(c.onProcess(xin[0, k * 256:(k + 1) * 256], xin[1, k * 256:(k + 1) * 256])) for k in range(8)]
    mine.append(c.process(xin[0, 8 * 256:], xin[1, 8 * 256:]))
    c.close()
    assert rms(np.concatenate(mine, axis=1) - out) <= RMS_TOL


def test_the_single_transform_form_takes_a_filter(gpu_lib):
    """It keeps no taps, but a load with the step works there: the same output as the partitioned engine's."""
    from cuda_audio_amd.synth import make_input

    a, b = _inputs(2000, 50)
    a = a * np.float32(0.1)
    xin = make_input(16 * 256)
    outs = []
    for form in ("partitioned", "single"):
        c = _conv(16384, form=form)
        c.prepare(0, a, filter=_filter(b))
        assert c.ir_filter_info(0)["frames_out"] == 2049 and c.ir_shape_info(0)["frames"] == 2049
        outs.append(np.concatenate([np.stack(c.onProcess(xin[0, k * 256:(k + 1) * 256], xin[1, k * 256:(k + 1) * 256])) for k in range(16)], axis=1))
        c.close()
    assert rms(outs[0]) > 0.005 and rms(outs[0] - outs[1]) <= RMS_TOL
