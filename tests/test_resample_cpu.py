"""IR sample-rate conversion (mc_load_ir_resampled): the float64 restatement's properties and the C entry point's
argument checks.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from resample_np import geometry, out_frames, resample

RATIOS = [(44100, 48000), (48000, 44100), (44100, 96000), (96000, 44100), (32000, 44100)]


def _tone_amp(y, f, fs, lo, hi):
    """Least-squares amplitude of a tone of f Hz in y[lo:hi] sampled at fs."""
    t = np.arange(lo, hi) / fs
    A = np.stack([np.sin(2 * np.pi * f * t), np.cos(2 * np.pi * f * t)], axis=1)
    c, *_ = np.linalg.lstsq(A, y[lo:hi], rcond=None)
    return float(np.hypot(*c))


def _H(h, f, fs):
    return float(np.abs(np.exp(-2j * np.pi * f * np.arange(len(h)) / fs) @ h))


@pytest.mark.parametrize("src,dst", RATIOS)
def test_passband_is_flat(src, dst):
    """A tone from 1 kHz up to 18 kHz (or 0.45 of the lower rate) keeps its level within 0.001 dB once the src / dst tap
    scale is taken out (the converted IR has dst / src times as many taps: per tap it is src / dst as loud)."""
    fmax = min(18000.0, 0.45 * min(src, dst))
    for f in np.linspace(1000.0, fmax, 9):
        x = np.sin(2 * np.pi * f * np.arange(3000) / src)
        y = resample(x, src, dst)
        a = _tone_amp(y, f, dst, 600, len(y) - 600) * dst / src
        assert abs(20 * np.log10(a)) <= 0.001, f"{src}->{dst}, {f:.0f} Hz: {20 * np.log10(a):.5f} dB"


@pytest.mark.parametrize("src,dst", [(48000, 44100), (96000, 44100)])
def test_alias_rejection(src, dst):
    """A 23.55 kHz tone (above the 22.05 kHz Nyquist frequency of the session) folds back at no more than -90 dB."""
    f = 23550.0
    x = np.sin(2 * np.pi * f * np.arange(6000) / src)
    y = resample(x, src, dst)
    a = _tone_amp(y, dst - f, dst, 600, len(y) - 600) * dst / src
    assert 20 * np.log10(a + 1e-30) <= -90.0


@pytest.mark.parametrize("src,dst", RATIOS + [(44100, 47999)])
def test_sum_and_tone_gain_of_an_ir_are_kept(src, dst):
    """An IR whose direct sound is not at frame 0 keeps sum h (within 1e-4 of sum |h| ~ 1e2: here 1e-5 absolute) and its
    response at 100, 500, 2000 and 8000 Hz (within 0.001 dB): the src / dst scale is what keeps the reverb's loudness."""
    from cuda_audio_amd.synth import make_ir

    ir = np.concatenate([np.zeros((300, 2), np.float32), make_ir(30000)])
    y = resample(ir, src, dst)
    np.testing.assert_allclose(y.sum(axis=0), ir.astype(np.float64).sum(axis=0), atol=2e-5)
    for c in range(2):
        for f in (100, 500, 2000, 8000):
            g = 20 * np.log10(_H(y[:, c], f, dst) / _H(ir[:, c].astype(np.float64), f, src))
            assert abs(g) <= 0.001, f"{src}->{dst}, channel {c}, {f} Hz: {g:.5f} dB"


@pytest.mark.parametrize("src,dst", [(44100, 48000), (48000, 44100)])
def test_tone_gain_with_the_direct_sound_at_frame_0(src, dst):
    """synth.make_ir starts at full level at frame 0: the pre-ringing dropped before output frame 0 (about half of the first
    frames' share) is all that moves, within 0.1 dB at 100 - 8000 Hz and 3e-3 on sum h."""
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(30000)
    y = resample(ir, src, dst)
    assert np.abs(y.sum(axis=0) - ir.astype(np.float64).sum(axis=0)).max() <= 3e-3
    for c in range(2):
        for f in (100, 500, 2000, 8000):
            g = 20 * np.log10(_H(y[:, c], f, dst) / _H(ir[:, c].astype(np.float64), f, src))
            assert abs(g) <= 0.1


def test_equal_rates_are_the_identity():
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(1000, seed=3)
    np.testing.assert_array_equal(resample(ir, 48000, 48000), ir.astype(np.float64))


@pytest.mark.parametrize("src,dst", RATIOS + [(44100, 47999), (8000, 384000), (384000, 8000)])
@pytest.mark.parametrize("frames", [1, 2, 147, 1000, 30001])
def test_output_length(src, dst, frames):
    g = geometry(src, dst)
    want = -(-frames * g["p"] // g["q"])
    assert out_frames(frames, src, dst) == want
    assert want == int(np.ceil(frames * dst / src - 1e-9))
    if frames <= 1000 and src != 384000:
        assert resample(np.ones(frames), src, dst).shape == (want,)


def test_geometry_constants():
    g = geometry(44100, 48000)
    assert (g["p"], g["q"], g["W"], g["L"]) == (160, 147, 64.0, 128)
    g = geometry(48000, 44100)
    assert (g["p"], g["q"], g["Wi"]) == (147, 160, 70) and abs(g["W"] - 64 * 48000 / 44100) < 1e-12


def test_entry_point_checks_its_arguments():
    """mc_load_ir_resampled is exported and refuses a null engine or a rate outside [8000, 384000] with MC_ERR_ARG and a
    message, before any HIP call (no GPU needed)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    lr = (C.c_float * 4)()
    assert L.mc_load_ir_resampled(None, 0, lr, 2, 1024, 44100, 48000) == -1
    assert L.mc_last_error()
    for a, b in ((7999, 48000), (44100, 384001), (0, 0)):
        assert L.mc_load_ir_resampled(None, 0, lr, 2, 1024, a, b) == -1
        assert b"rate" in L.mc_last_error()
