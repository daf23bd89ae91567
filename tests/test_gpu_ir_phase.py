"""The phase step of an IR load on the device (mc_load_ir_phase, mc_load_ir_sweep_phase; csrc/irphase.hip.h over csrc/fft64.hip.h):
the stored taps and mc_ir_phase_info against the float64 restatement (tests/ir_phase_np.py, numpy's FFT, one channel at a time),
against analysis, the parts of the definition that are exact (a step that is off, repeated loads, refused loads), the chain with
shape, EQ and damping into the engine's output, and the measured response of the converted IR.

The bound per tap is |got - want| <= 2^-23 |want| + 1e-12 peak: both pipelines are double and differ by parts in 1e-15 of the
peak on these inputs (two FFT libraries on the CPU differ by as much), and the rounding to float then differs by at most one
ulp, at a tie.  `peak` is the larger channel's: the device carries both channels through one complex transform, so its rounding
error is relative to that one.  profiles/irphase.md has what an MI355X showed: never more than 7e-17 of the peak above one ulp."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_phase_np as P
from helpers import BASE, RMS_TOL, apply_params, rms
from test_gpu_ir_shape import _check_taps

pytestmark = pytest.mark.gpu

RATE = 48000


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irphase", n_ref, sample_rate=rate, **kw)


def _phase(**kw):
    from cuda_audio_amd.engine import IrPhase

    return IrPhase(**kw)


def _n_ref(F):
    n = 16384
    while n < F + 1024 + 1:
        n *= 2
    return n


@functools.lru_cache(maxsize=None)
def _case(F):
    """(frames, restated float32 taps, restated info), computed once per length and never written to."""
    x = P.delayed_noise(F)
    want, info = P.min_phase(x)
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want, info


def _check_bound(got, want32):
    w = want32.astype(np.float64)
    err = np.abs(got.astype(np.float64) - w)
    peak = np.abs(w).max()
    slack = err - 2.0 ** -23 * np.abs(w)
    print(f"taps: largest deviation {err.max():.3e} (peak {peak:.3e}), largest excess over one ulp {slack.max() / peak:.3e} of the peak, "
          f"{np.count_nonzero(got != want32)} of {got.size} values differ")
    assert got.shape == want32.shape
    assert (slack <= 1e-12 * peak).all(), f"excess {slack.max() / peak:.3e} of the peak at {np.unravel_index(slack.argmax(), slack.shape)}"


def _check_info(got, want):
    print("phase info:", got, "restated:", want)
    assert got["frames"] == want["frames"] and got["nfft"] == want["nfft"] and tuple(got["clamped"]) == tuple(want["clamped"])
    for k in ("energy_in", "energy_out", "centre_in", "centre_out"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])


def _load_and_check(F, oversample=8):
    x, want, winfo = _case(F)
    c = _conv(_n_ref(F))
    c.prepare(0, x, phase=_phase(oversample=oversample))
    got, info, sinfo = c.ir_taps(0), c.ir_phase_info(0), c.ir_shape_info(0)
    c.close()
    assert sinfo["frames"] == sinfo["taps"] == F and sinfo["gain"] == 1.0
    _check_bound(got, want)
    _check_info(info, winfo)
    return got


# oversample 8 and F = 2^(k - 3): Nfft = 2^4 .. 2^18, one pass up to 2^11 and two from 2^12 on, every tile shape of fft64.hip.h
@pytest.mark.parametrize("k", list(range(4, 19)))
def test_stored_taps_match_the_restatement(gpu_lib, k):
    F = 1 << (k - 3)
    assert P.nfft_of(F) == 1 << k
    _load_and_check(F)


# lengths that pad: Nfft = 16, 32, 1024, 65536, 524288
@pytest.mark.parametrize("F", [1, 3, 127, 5000, 40000])
def test_lengths_that_pad(gpu_lib, F):
    _load_and_check(F)


def test_the_longest_transform(gpu_lib):
    """F = 2^19: Nfft = 2^22 = 2048 x 2048, the largest the step takes."""
    F = 1 << 19
    assert P.nfft_of(F) == P.MAX_NFFT
    got = _load_and_check(F)
    assert np.abs(got[:, 0]).argmax() == 0


@pytest.mark.parametrize("K,r_max", [(16, 0.9), (40, 0.95)])
def test_reflected_zeros_come_back_inside(gpu_lib, K, r_max):
    """float32 input: the bound is twice the restatement's own deviation from the analytic product for that same input, plus
    1e-6 of the peak.  The right channel is another product at a third of the level."""
    xl, wl = P.quadratic_product(K, r_max)
    xr, wr = P.quadratic_product(K, r_max, seed=5)
    x = np.stack([xl, xr / 3.0], axis=1).astype(np.float32)
    want = np.stack([wl, wr / 3.0], axis=1)
    c = _conv(16384)
    c.prepare(0, x, phase=_phase(oversample=64))
    got = c.ir_taps(0).astype(np.float64)
    c.close()
    restated = P.min_phase64(x, 64)[0]
    for ch in range(2):
        peak = np.abs(want[:, ch]).max()
        own = np.abs(restated[:, ch] - want[:, ch]).max()
        dev = np.abs(got[:, ch] - want[:, ch]).max()
        print(f"channel {ch}: device {dev / peak:.3e}, restatement {own / peak:.3e} of the peak")
        assert dev <= 2.0 * own + 1e-6 * peak


def _off_phase():
    """MC_PHASE_OFF with nonsense in every other field."""
    from cuda_audio_amd import _lib

    p = _lib.McIrPhase()
    p.struct_size, p.mode, p.floor_db, p.over_log2 = 7, _lib.MC_PHASE_OFF, float("nan"), 99
    return p


def test_a_phase_that_is_off_is_the_wrapped_load_bit_for_bit(gpu_lib):
    """phase = None (Python and C) and MC_PHASE_OFF against prepare(tail=...) and prepare_sweep() without one."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrShape, IrTail, _fp
    from test_gpu_ir_sweep import _recorded, _sw

    ir = np.ascontiguousarray(_case(5000)[0])
    fields, rec = _recorded("A")
    rec = np.ascontiguousarray(rec)
    shape = IrShape(fade_out=100, normalize="peak", target=0.05)
    tail = IrTail(mode="cut", xovers=(1000,), knee=(3000, 2500), fade=64)
    outs = []
    for how in ("without", "none", "off", "c_null", "c_off"):
        c = _conv(16384)
        L, off = c._L, _off_phase()
        if how in ("without", "none", "off"):
            kw = {} if how == "without" else dict(phase=None if how == "none" else _phase(mode="off"))
            c.prepare(0, ir, ir_rate=44100, shape=shape, tail=tail, **kw)
            c.prepare(1, ir, **kw)
            c.prepare_sweep(2, rec, _sw(fields), offset=-64, ir_frames=1024, shape=shape, **kw)
        else:
            p = None if how == "c_null" else C.byref(off)
            s, t, sw = shape.to_c(), tail.to_c(), _sw(fields).to_c()
            sw.rate = RATE
            assert L.mc_load_ir_phase(c._h, 0, _fp(ir), len(ir), 1024, 44100, RATE, C.byref(s), None, None, C.byref(t), p) == 0
            assert L.mc_load_ir_phase(c._h, 1, _fp(ir), len(ir), 1024, 0, 0, None, None, None, None, p) == 0
            assert L.mc_load_ir_sweep_phase(c._h, 2, _fp(rec), len(rec), 1024, C.byref(sw), -64, 1024, C.byref(s), None, None, None, p) == 0
        for idx in range(3):
            with pytest.raises(McError) as ex:
                c.ir_phase_info(idx)
            assert ex.value.code == -3
        outs.append([c.ir_taps(i) for i in range(3)] + [c.ir_spectra(i) for i in range(3)] + [c.ir_info(i) for i in range(3)])
        c.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            if isinstance(a, dict):
                assert a == b
            else:
                assert a.tobytes() == b.tobytes()


def test_the_same_load_stores_the_same_bits(gpu_lib):
    """Twice on one engine and once on another, one pass (F = 200) and two (F = 40000)."""
    for F in (200, 40000):
        x = _case(F)[0]
        taps = []
        for engine in range(2):
            c = _conv(_n_ref(F))
            for idx in range(2 - engine):
                c.prepare(idx, x, phase=_phase())
                taps.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_phase_info(idx)))
            c.close()
        for t, s, i in taps[1:]:
            assert t.tobytes() == taps[0][0].tobytes() and s.tobytes() == taps[0][1].tobytes() and i == taps[0][2]


def test_a_sweep_capture_with_a_phase(gpu_lib):
    """prepare_sweep(phase=): the step acts on the deconvolved frames, which the plain capture stores."""
    from test_gpu_ir_sweep import _recorded, _sw

    fields, rec = _recorded("A")
    F = 1024
    c = _conv(16384)
    c.prepare_sweep(0, rec, _sw(fields), offset=-64, ir_frames=F)
    frames = c.ir_taps(0)
    want, winfo = P.min_phase(frames)
    c.prepare_sweep(1, rec, _sw(fields), offset=-64, ir_frames=F, phase=_phase())
    got, info = c.ir_taps(1), c.ir_phase_info(1)
    assert c.ir_sweep_info(1)["frames"] == F and c.ir_shape_info(1)["frames"] == F
    c.close()
    _check_bound(got, want)
    _check_info(info, winfo)
    assert info["centre_in"] - info["centre_out"] > 32.0  # (the capture's pre-roll of 64 frames is gone)


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd import _lib
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, IrShape, IrTail, _fp

    ir = np.ascontiguousarray(_case(5000)[0])
    c = _conv(16384)
    tail = IrTail(mode="cut", xovers=(1000,), knee=(3000, 2500), fade=64)
    c.prepare(0, ir, shape=IrShape(fade_out=100), tail=tail, phase=_phase())

    def state():
        return (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_tail_info(0), c.ir_phase_info(0), c.num_irs())

    before = state()
    L = c._L
    bad = _lib.McIrPhase()
    L.mc_default_ir_phase(C.byref(bad))
    bad.mode = _lib.MC_PHASE_MINIMUM
    for field, value in (("struct_size", 20), ("mode", 2), ("floor_db", 10.0), ("over_log2", 7)):
        p = _lib.McIrPhase.from_buffer_copy(bad)
        setattr(p, field, value)
        for idx in (0, 1):
            assert L.mc_load_ir_phase(c._h, idx, _fp(ir), len(ir), 1024, RATE, RATE, None, None, None, None, C.byref(p)) == -1
            assert field in L.mc_last_error().decode()
    p = _lib.McIrPhase.from_buffer_copy(bad)
    p.over_log2 = 6
    long_ir = np.zeros((70000, 2), np.float32)
    long_ir[0] = 1.0
    for idx in (0, 1):
        assert L.mc_load_ir_phase(c._h, idx, _fp(long_ir), len(long_ir), 1024, 0, 0, None, None, None, None, C.byref(p)) == -1
        assert "over_log2" in L.mc_last_error().decode()
    other = np.ascontiguousarray(_case(4096)[0])
    for kw in (dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=5000)), dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(ir_rate=7999, tail=tail),
               dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, phase=_phase(), **kw)
            assert ex.value.code == -1, kw
    with pytest.raises(McError) as ex:
        c.ir_phase_info(1)
    assert ex.value.code == -1
    assert state() == before
    # a plain load over a converted one leaves no phase information behind
    c.prepare(0, other)
    with pytest.raises(McError) as ex:
        c.ir_phase_info(0)
    assert ex.value.code == -3
    c.close()


def test_the_chain_into_the_output(oracle_mod, gpu_lib):
    """Minimum phase, then a shape that normalises, damping and an EQ band: the stored taps against the float64 restatements
    chained in the documented order (1b before 2 .. 8), and 8 periods and one batch against the oracle fed the restated taps."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape
    from cuda_audio_amd.synth import make_input

    n_ref, F = 16384, 6000
    x = P.delayed_noise(F)
    xovers, decay, origin = (400, 1600), (0, 4800, 1600), 10
    bands = [("peak", 1000.0, 4.0, 1.0)]
    fields = dict(fade_out=200, normalize="peak", target=0.05)
    y32 = P.min_phase(x)[0]
    want, winfo, wdinfo = ir_damp_np.damp64(y32, n_ref - 1024, RATE, RATE, xovers, decay, origin, bands, **fields)
    c = _conv(n_ref, max_batch=32)
    c.prepare(0, x, shape=IrShape(**fields), eq=IrEq(bands=bands), damp=IrDamp(xovers=xovers, decay=decay, origin=origin), phase=_phase())
    c.prepare(1, x)
    got = c.ir_taps(0)
    _check_taps(got, want)
    sinfo = c.ir_shape_info(0)
    assert sinfo["frames"] == F and sinfo["taps"] == winfo["taps"] and abs(sinfo["gain"] - winfo["gain"]) <= 1e-6 * winfo["gain"]
    assert c.ir_damp_info(0) == wdinfo and c.ir_phase_info(0)["frames"] == F
    assert np.abs(got).max(axis=0).argmax() in (0, 1) and abs(np.abs(got).max() - 0.05) <= 1e-6 * 0.05
    taps = [want.astype(np.float32), x[:n_ref - 1024]]
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


def test_the_single_transform_form_takes_a_phase(gpu_lib):
    """It keeps no taps, but a load with the step works there: the same output as the partitioned engine's."""
    from cuda_audio_amd.synth import make_input

    x = P.delayed_noise(3000) * np.float32(0.1)
    xin = make_input(16 * 256)
    outs = []
    for form in ("partitioned", "single"):
        c = _conv(16384, form=form)
        c.prepare(0, x, phase=_phase())
        assert c.ir_phase_info(0)["frames"] == 3000 and c.ir_shape_info(0)["frames"] == 3000
        outs.append(np.concatenate([np.stack(c.onProcess(xin[0, k * 256:(k + 1) * 256], xin[1, k * 256:(k + 1) * 256])) for k in range(16)], axis=1))
        c.close()
    assert rms(outs[0]) > 0.005 and rms(outs[0] - outs[1]) <= RMS_TOL


def test_the_measured_response_keeps_its_magnitude_and_loses_its_delay(gpu_lib):
    """ir_response of the converted IR against the original's: the magnitudes agree as far as the restatement's own do on the
    same grid (the truncation to F frames and the cepstrum's aliasing), plus 10 %; the group delay at the eight strongest
    frequencies, counted from frame 0, is lower."""
    from ir_response_np import response

    F = 2000
    x = P.delayed_noise(F, delay=250)
    hz = np.array([200.0 * 2.0 ** (i / 3.0) for i in range(20)], np.float32)
    c = _conv(16384)
    c.prepare(0, x)
    c.prepare(1, x, phase=_phase())
    a, b = c.ir_response(0, hz=hz), c.ir_response(1, hz=hz)
    conv = c.ir_taps(1)
    c.close()
    ra, rb = response(x, RATE, hz), response(P.min_phase(x)[0], RATE, hz)
    for ch in range(2):
        top = np.abs(a["h"][0, ch]).max()
        dev = np.abs(np.abs(b["h"][0, ch]) - np.abs(a["h"][0, ch])).max() / top
        own = np.abs(np.abs(rb["h"][0, ch]) - np.abs(ra["h"][0, ch])).max() / np.abs(ra["h"][0, ch]).max()
        print(f"channel {ch}: magnitudes differ by {dev:.3e} of the largest, the restatement's by {own:.3e}")
        assert dev <= 1.1 * own
        strongest = np.argsort(np.abs(a["h"][0, ch]))[-8:]
        before, after = a["origin"] + a["delay"][0, ch, strongest], b["origin"] + b["delay"][0, ch, strongest]
        print(f"channel {ch}: group delay {before.round(1)} -> {after.round(1)} frames")
        assert (after < before - 200.0).all()
    assert np.abs(conv[:, 0]).argmax() == 0
