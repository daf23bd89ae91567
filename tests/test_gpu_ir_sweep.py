"""Capture of an IR from a recorded sine sweep on the device (mc_load_ir_sweep, csrc/irsweep.hip.h): the stored taps, the shape
information, the sums and the spectra against the float64 restatement (tests/ir_sweep_np.py), the parts of the definition that
are exact (zeros where the window misses the recording, a silent channel, swapped channels, repeated loads), every length at
which the kernel's walk changes, the chain through shaping, damping and EQ, the engine's paths against the oracle fed the
restated taps, and the flat band of a sweep deconvolved with itself.  Tolerances are test_gpu_ir_shape.py's: device double
arithmetic (sin, expm1, exp a few ulp of a double from numpy's, the sum in another order of rounding) rounded to float32."""
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_sweep_np
from helpers import BASE, RMS_TOL, _dry, apply_params, rms
from ir_shape_np import assert_onset_margin, shape
from test_gpu_ir_eq import CASCADE8, _check_sums_and_spectra
from test_gpu_ir_shape import COMBINED_A, FP16_REL_TOL, OS_P, P0, P1, _check_level, _check_taps, _os_want, _settled_batches
from test_ir_sweep_cpu import CASE_A, CASE_B

pytestmark = pytest.mark.gpu

T = 2048  # outputs per workgroup of k_sweep_corr: 256 threads, 8 consecutive outputs each (SWP_T)
J = 256   # weights per LDS tile (SWP_J)
H0 = {0: (1.0, 0.6), 37: (-0.5, 0.7), 300: (0.25, -0.3), 599: (0.125, 0.2)}  # the room: tap -> (L, R)


def _conv(n_ref, rate, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    return Convolution("irsweep", n_ref, sample_rate=rate, **kw)


def _sw(fields):
    from cuda_audio_amd.engine import Sweep

    return Sweep(**fields)


@functools.lru_cache(maxsize=None)
def _recorded(name, tail=700):
    """The float32 sweep of a case played through H0 (float64 convolution, rounded to float32) and `tail` frames of room."""
    fields = dict(A=CASE_A, B=CASE_B)[name]
    s = ir_sweep_np.sweep(**fields).astype(np.float32).astype(np.float64)
    rec = np.zeros((len(s) + tail, 2))
    for tap, gains in H0.items():
        for ch in range(2):
            rec[tap:tap + len(s), ch] += gains[ch] * s
    rec = rec.astype(np.float32)
    rec.setflags(write=False)
    return fields, rec


@functools.lru_cache(maxsize=None)
def _restated(name, offset, F):
    fields, rec = _recorded(name)
    h = ir_sweep_np.deconvolve(rec, fields, offset, F)
    h.setflags(write=False)
    return h


def _check_plain(c, idx, want64, F):
    """Taps, shape information, sums and spectra of a deconvolved IR with shape, EQ and damping off."""
    want = want64.astype(np.float32)
    got = c.ir_taps(idx)
    if np.abs(want).max() > 0:
        _check_taps(got, want64)
    else:
        np.testing.assert_array_equal(got, want)
    info = c.ir_shape_info(idx)
    for k, v in dict(frames=F, onset=0, first=0, taps=len(want)).items():
        assert info[k] == v, k
    assert info["gain"] == 1.0 and info["eq_bands"] == 0
    assert abs(info["peak"] - np.abs(want).max()) <= 1e-6 * np.abs(want).max()
    _check_sums_and_spectra(c, idx, got, want)
    return got


@pytest.mark.parametrize("name,offset,F", [("A", -64, 1024), ("B", -100, 900)])
def test_a_recorded_sweep_matches_the_restatement(gpu_lib, name, offset, F):
    fields, rec = _recorded(name)
    want = _restated(name, offset, F)
    c = _conv(16384, fields["rate"], max_batch=8)
    c.prepare_sweep(0, rec, _sw(dict(fields, rate=0)), offset=offset, ir_frames=F)  # (the rate comes from the engine)
    got = _check_plain(c, 0, want, F)
    assert c.ir_sweep_info(0) == dict(sweep_frames=fields["frames"], recording_frames=len(rec), frames=F, offset=offset)
    # the room comes back: every tap of H0 stands at its place at 0.81 of its level, the peak of the band-limited unit impulse
    # (test_ir_sweep_cpu.py), to 5 % (the restatement is within 2.2 %: the neighbours' side lobes)
    for tap, gains in H0.items():
        for ch in range(2):
            assert abs(got[tap - offset, ch] / 0.81 - gains[ch]) < 0.05 * abs(gains[ch]), (tap, ch, got[tap - offset, ch])
    c.close()


def test_ir_frames_defaults_to_what_the_recording_holds_past_the_sweep(gpu_lib):
    fields, rec = _recorded("A")
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_sweep(0, rec, _sw(fields))
    assert c.ir_sweep_info(0) == dict(sweep_frames=4096, recording_frames=4796, frames=701, offset=0)
    c.prepare_sweep(1, rec, _sw(fields), offset=-50)
    assert c.ir_sweep_info(1)["frames"] == 751 and c.ir_shape_info(1)["frames"] == 751
    _check_taps(c.ir_taps(1), _restated("A", -50, 751))
    c.prepare_sweep(1, rec, _sw(fields), offset=5000)
    assert c.ir_sweep_info(1)["frames"] == 1
    c.close()


# -- exact parts --------------------------------------------------------------------------------------------------------------
def test_outputs_whose_window_misses_the_recording_are_exact_zeros(gpu_lib):
    fields, rec = _recorded("B")
    rec = rec[:fields["frames"] + 500]  # (cut inside the room's tail: the last frames are not silent)
    M, N, F = len(rec), fields["frames"], 3000
    assert np.count_nonzero(rec[-100:]) > 190
    c = _conv(16384, 44100, max_batch=8)
    for idx, offset in enumerate((M, M + 12345, -(N + F), -(1 << 24), 1 << 24)):
        c.prepare_sweep(idx, rec, _sw(fields), offset=offset, ir_frames=F)
        got = c.ir_taps(idx)
        assert got.shape == (F, 2) and not got.any() and not np.signbit(got).any()
        assert c.ir_shape_info(idx)["peak"] == 0.0
    # part of the outputs: frames from M - offset on lie past the recording's end, frames before -(N - 1) - offset before its start
    c.prepare_sweep(0, rec, _sw(fields), offset=M - 100, ir_frames=F)
    got = c.ir_taps(0)
    assert not got[100:].any() and np.count_nonzero(got[:100]) > 150
    c.prepare_sweep(0, rec, _sw(fields), offset=-(N + 99), ir_frames=F)
    got = c.ir_taps(0)
    assert not got[:100].any() and np.count_nonzero(got[100:]) > 5000
    c.close()


def test_channels_are_independent_and_loads_repeat_bit_for_bit(gpu_lib):
    fields, rec = _recorded("A")
    F, offset = 1500, -300
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_sweep(0, rec, _sw(fields), offset=offset, ir_frames=F)
    base = c.ir_taps(0)
    assert np.abs(base[:, 0]).max() > 0.5 and np.abs(base[:, 1]).max() > 0.3
    silent = rec.copy()
    silent[:, 1] = 0.0
    c.prepare_sweep(1, silent, _sw(fields), offset=offset, ir_frames=F)
    got = c.ir_taps(1)
    assert not got[:, 1].any()
    np.testing.assert_array_equal(got[:, 0], base[:, 0])
    c.prepare_sweep(2, rec[:, ::-1], _sw(fields), offset=offset, ir_frames=F)
    np.testing.assert_array_equal(c.ir_taps(2), base[:, ::-1])
    c.prepare_sweep(3, rec, _sw(fields), offset=offset, ir_frames=F)
    np.testing.assert_array_equal(c.ir_taps(3), base)
    np.testing.assert_array_equal(c.ir_spectra(3), c.ir_spectra(0))
    assert c.ir_info(3) == c.ir_info(0) and c.ir_shape_info(3) == c.ir_shape_info(0)
    # a longer load holds the shorter one: a frame does not depend on the grid
    c.prepare_sweep(3, rec, _sw(fields), offset=offset, ir_frames=2 * T + 77)
    np.testing.assert_array_equal(c.ir_taps(3)[:F], base)
    c.close()


# -- edges of the kernel's walk -----------------------------------------------------------------------------------------------
# F around one workgroup's outputs and past two; N around one tile of weights and past two; the recording long, shorter than
# the sweep, and longer than everything; offsets that leave the first tile half before the recording's start (-1100 of its
# 2304 frames), the last one half past its end (M - 1000), and the window wholly inside.  Every (F, N) once, the rest in turn.
EDGE_F = (1, 2, T - 1, T, T + 1, 2 * T + 3)
EDGE_N = (2, J - 1, J, J + 1, 2 * J + 5)


def _edge_cases():
    cases, k = [], 0
    for F in EDGE_F:
        for N in EDGE_N:
            M = (3000, max(1, N // 2), 5000 + N)[k % 3]
            offset = ((0, -1100, M - 1000, -(N // 2)) if F > 2 else (0, -(N - 1), M - 1, -(N // 2)))[k % 4]  # (one or two outputs: on the recording)
            cases.append((F, N, M, offset))
            k += 1
    # by hand: a recording of one frame; both ends outside within one tile; the last workgroup's window ending at the last frame
    return cases + [(T + 1, J + 1, 1, -700), (2 * T + 3, 2 * J + 5, 1200, -1100), (2 * T + 3, 2 * J + 5, 2 * T + 3 + 2 * J + 4, 0)]


@pytest.fixture(scope="module")
def edge_engine(gpu_lib):
    c = _conv(16384, 48000, max_batch=8)
    yield c
    c.close()


@pytest.mark.parametrize("F,N,M,offset", _edge_cases())
def test_edges_of_the_kernels_walk(edge_engine, F, N, M, offset):
    fields = dict(frames=N, f1_hz=300.0, f2_hz=12000.0, rate=48000, amplitude=0.5, fade_in=min(5, N // 2), fade_out=min(3, N // 2))
    rec = (0.1 * np.random.default_rng(1000 * F + N).standard_normal((M, 2))).astype(np.float32)
    want = ir_sweep_np.deconvolve(rec, fields, offset, F)
    c = edge_engine
    c.prepare_sweep(0, rec, _sw(fields), offset=offset, ir_frames=F)
    got = _check_plain(c, 0, want, F)
    assert got.shape == (F, 2)
    np.testing.assert_array_equal((got == 0).all(axis=1), (want == 0).all(axis=1))
    assert c.ir_sweep_info(0) == dict(sweep_frames=N, recording_frames=M, frames=F, offset=offset)


# -- the chain ----------------------------------------------------------------------------------------------------------------
CHAIN_DAMP = ((250, 2000, 8000), (20000, 0, 6000, 2500), 700)


def test_the_chain_of_shape_damping_and_eq(gpu_lib):
    """The deconvolved frames stand where a WAV's do: loading them back as a WAV with a shape, an EQ cascade and damping stores
    the bits mc_load_ir_sweep stores with the same three."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    fields, rec = _recorded("A")
    F, offset, n_ref = 3000, -200, 16384
    assert F <= n_ref - 1024
    xovers, decay, origin = CHAIN_DAMP
    three = dict(shape=IrShape(**COMBINED_A), eq=IrEq(bands=list(CASCADE8)), damp=IrDamp(xovers=xovers, decay=decay, origin=origin))
    c = _conv(n_ref, 48000, max_batch=8)
    c.prepare_sweep(0, rec, _sw(fields), offset=offset, ir_frames=F)
    frames = c.ir_taps(0)
    assert frames.shape == (F, 2)
    assert_onset_margin(_restated("A", offset, F).astype(np.float32), 0, COMBINED_A["trim_db"])
    c.prepare(1, frames, **three)
    c.prepare_sweep(2, rec, _sw(fields), offset=offset, ir_frames=F, **three)
    got, want = c.ir_taps(2), c.ir_taps(1)
    assert len(want) < F and np.abs(want).max() > 0  # (the trim took the pre-roll)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(c.ir_spectra(2), c.ir_spectra(1))
    assert c.ir_shape_info(2) == c.ir_shape_info(1) and c.ir_damp_info(2) == c.ir_damp_info(1) and c.ir_info(2) == c.ir_info(1)
    assert c.ir_shape_info(2)["frames"] == F and c.ir_shape_info(2)["eq_bands"] == 8
    # and against the restatement of all of it
    restated = ir_damp_np.damped(_restated("A", offset, F).astype(np.float32), n_ref - 1024, None, 48000, xovers, decay, origin, CASCADE8, **COMBINED_A)[0]
    _check_taps(got, restated.astype(np.float64))
    c.close()


# -- the engine plays the captured IRs ----------------------------------------------------------------------------------------
IR_A = dict(case="A", offset=-64, F=1024, bands=(("lowcut", 120), ("peak", 2500, 6.0, 1.5)), damp=((400, 1600), (0, 4800, 1600), 37),
            fields=dict(fade_out=512, normalize="energy", target=0.25))
IR_B = dict(case="B", offset=-100, F=900, bands=(), damp=None, fields=dict(start=100, length=700, normalize="peak", target=0.02))


@functools.lru_cache(maxsize=None)
def _pair(n_ref=16384, nframes=1024):
    """The two captured IRs and their restated taps (computed once)."""
    taps = []
    for s in (IR_A, IR_B):
        rate = _recorded(s["case"])[0]["rate"]
        frames = _restated(s["case"], s["offset"], s["F"]).astype(np.float32)
        if s["damp"] or s["bands"]:
            t = ir_damp_np.damped(frames, n_ref - nframes, None, rate, *(s["damp"] or ((), (), 0)), s["bands"], **s["fields"])[0]
        else:
            t = shape(frames, n_ref - nframes, None, rate, **s["fields"])[0]
        t.setflags(write=False)
        taps.append(t)
    return (IR_A, IR_B), taps


def _prepare_pair(c, irs):
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    for i, s in enumerate(irs):
        fields, rec = _recorded(s["case"])
        damp = IrDamp(xovers=s["damp"][0], decay=s["damp"][1], origin=s["damp"][2]) if s["damp"] else None
        c.prepare_sweep(i, rec, _sw(fields), offset=s["offset"], ir_frames=s["F"], shape=IrShape(**s["fields"]),
                        eq=IrEq(bands=list(s["bands"])) if s["bands"] else None, damp=damp)


def test_jack_period_matches_the_oracle(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, period, ncalls = 16384, 256, 420
    irs, taps = _pair(n_ref)
    x = make_input(ncalls * period)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, P0, P1, True)
    want = ref.process(x[0], x[1], block=period)
    _check_level(want, x, P0, P1)
    c = _conv(n_ref, None, max_batch=16, period=period)  # (each sweep carries its own rate)
    _prepare_pair(c, irs)
    for i, t in enumerate(taps):
        _check_taps(c.ir_taps(i), t.astype(np.float64))
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period]))
                          for k in range(ncalls)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_overlap_save_batch(oracle_mod, gpu_lib):
    """A settled batch of 12288 blocks takes the overlap-save form (os_stats) with the captured IRs."""
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 12288
    irs, taps = _pair(n_ref)
    xx = make_input(2 * nb * 256)
    c = _conv(n_ref, None, max_batch=nb)
    _prepare_pair(c, irs)
    for h in (0, 1):
        c.cc[h].value.update(**OS_P)
    out = _settled_batches(c, xx, nb)
    took = c.os_stats()["batches"]
    c.close()
    assert took >= 1
    b0, n = nb + 4000, 96
    want = _os_want(oracle_mod, n_ref, taps, xx, b0, n)
    got = out[:, b0 * 256:(b0 + n) * 256].cpu().numpy()
    assert rms(got - want) <= RMS_TOL


def test_fp16_storage(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 96
    irs, taps = _pair(n_ref)
    x = make_input(nb * 256)
    o = oracle_mod.Upols(n_ref, True)
    for i, t in enumerate(taps):
        o.prepare(i, t)
    p1 = dict(BASE, select=1)
    apply_params(o, BASE, p1, True)
    want = o.process(x[0], x[1])
    _check_level(want, x, BASE, p1)
    c = _conv(n_ref, None, max_batch=32, precision="fp16")
    _prepare_pair(c, irs)
    apply_params(c, BASE, p1, False)
    got = c.process(x[0], x[1])
    c.close()
    wet = want - _dry(x, BASE, p1)
    assert rms(got - want) <= FP16_REL_TOL * rms(wet)


def test_single_transform_form(oracle_mod, gpu_lib):
    """form = 1 builds its spectrum from the deconvolved, shaped taps left on the device (it keeps none)."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 64
    irs, taps = _pair(n_ref)
    x = make_input(nb * 256)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, P0, P1, True)
    want = ref.process(x[0], x[1])
    _check_level(want, x, P0, P1)
    c = _conv(n_ref, None, max_batch=32, form="single")
    _prepare_pair(c, irs)
    for i, s in enumerate(irs):
        info = c.ir_info(i)
        assert info["taps"] == len(taps[i]) and c.ir_shape_info(i)["frames"] == s["F"]
        np.testing.assert_allclose(info["sigma"], taps[i].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
        assert c.ir_sweep_info(i)["frames"] == s["F"] and c.ir_sweep_info(i)["offset"] == s["offset"]
    with pytest.raises(McError) as ex:
        c.ir_taps(0)
    assert ex.value.code == -3
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


# -- meaning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("amplitude", [0.5, 0.25])
def test_a_sweep_deconvolved_with_itself_is_flat_in_its_band(gpu_lib, amplitude):
    """Case A through the engine: within +-0.25 dB of 0 dB between 4 f1 and f2 / 2, the peak at frame -offset, at either
    amplitude (test_ir_sweep_cpu.py has the same of the restatement)."""
    from cuda_audio_amd.engine import sweep_frames

    sw = dict(CASE_A, amplitude=amplitude)
    s = sweep_frames(_sw(sw))
    rec = np.zeros((4096 + 1024, 2), np.float32)
    rec[:4096, 0] = rec[:4096, 1] = s
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_sweep(0, rec, _sw(sw), offset=-512, ir_frames=1024)
    h = c.ir_taps(0)
    c.close()
    lo, hi = ir_sweep_np.band_db(h[:, 0].astype(np.float64), sw)
    k = int(np.abs(h[:, 0]).argmax())
    print(f"amplitude {amplitude}: band {lo:+.3f} / {hi:+.3f} dB, peak {h[k, 0]:.4f} at frame {k}")
    assert -0.25 <= lo and hi <= 0.25
    assert k == 512 and 0.7 < h[512, 0] < 0.9
    np.testing.assert_array_equal(h[:, 0], h[:, 1])


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, IrShape
    from cuda_audio_amd.synth import make_ir

    fields, rec = _recorded("A")
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_sweep(0, rec, _sw(fields), offset=-64, ir_frames=1024, shape=IrShape(fade_out=100, normalize="peak", target=0.02), eq=IrEq(bands=[("lowcut", 120)]))
    taps, spec, info, sinfo, winfo = c.ir_taps(0), c.ir_spectra(0), c.ir_info(0), c.ir_shape_info(0), c.ir_sweep_info(0)
    for change in (dict(frames=1), dict(f2_hz=30000.0), dict(amplitude=0.0), dict(fade_in=4096, fade_out=1)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_sweep(idx, rec, _sw(dict(fields, **change)), ir_frames=500)
            assert ex.value.code == -1
    for kw in (dict(ir_frames=0), dict(offset=(1 << 24) + 1), dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=500)),
               dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_sweep(idx, rec, _sw(fields), **dict(dict(ir_frames=500), **kw))
            assert ex.value.code == -1
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    np.testing.assert_array_equal(c.ir_spectra(0), spec)
    assert c.ir_info(0) == info and c.ir_shape_info(0) == sinfo and c.ir_sweep_info(0) == winfo and c.num_irs() == 1
    # a WAV load over a captured index forgets the capture
    c.prepare(0, make_ir(3000, seed=2, norm=0.05))
    with pytest.raises(McError) as ex:
        c.ir_sweep_info(0)
    assert ex.value.code == -3
    c.close()
