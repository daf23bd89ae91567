"""IR sample-rate conversion on the device (mc_load_ir_resampled, csrc/resample.hip.h): the stored taps against the float64
restatement (tests/resample_np.py), then every path of the engine against the oracle fed the restated taps."""
import numpy as np
import pytest

from helpers import BASE, RMS_TOL, apply_params, rms
from resample_np import out_frames, resample

pytestmark = pytest.mark.gpu

RATIOS = [(44100, 48000), (48000, 44100), (44100, 96000), (96000, 44100), (32000, 44100), (44100, 47999)]
FP16_REL_TOL = 2e-3  # the bar of the existing fp16 tests (test_gpu_parity.py)


def _conv(n_ref, rate, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    return Convolution("resample", n_ref, sample_rate=rate, **kw)


def _restated(ir, src, dst, n_ref, nframes=1024):
    """What the engine should hold: the converted IR truncated at n_ref - nframes, as float32 frames."""
    return resample(ir, src, dst, n=n_ref - nframes).astype(np.float32)


def _check_taps(got, want64):
    err = got.astype(np.float64) - want64
    assert got.shape == want64.shape
    assert rms(err) <= 1e-6 * rms(want64), f"rms {rms(err):.3e} vs {rms(want64):.3e}"
    assert np.abs(err).max() <= 1e-5 * np.abs(want64).max()


@pytest.mark.parametrize("src,dst", RATIOS)
def test_taps_info_and_spectra_match_the_restatement(gpu_lib, src, dst):
    from cuda_audio_amd.synth import make_ir

    n_ref = 65536
    ir = make_ir(20000, seed=31, norm=0.05)
    c = _conv(n_ref, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src)
    want = resample(ir, src, dst, n=n_ref - 1024)
    n = out_frames(20000, src, dst)
    assert want.shape[0] == n
    got = c.ir_taps(0)
    _check_taps(got, want)
    info = c.ir_info(0)
    assert info["taps"] == n and info["partitions"] == (n + 255) // 256
    g64 = got.astype(np.float64)
    sg = np.where(np.arange(n) % 2, -1.0, 1.0)
    np.testing.assert_allclose(info["sigma"], g64.sum(axis=0), rtol=0, atol=1e-9)
    np.testing.assert_allclose(info["alpha"], (sg[:, None] * g64).sum(axis=0), rtol=0, atol=1e-9)
    # per-partition 512-point spectra against numpy's rfft of the restated taps (as test_ir_spectra_match_numpy)
    H = c.ir_spectra(0)
    for ch in range(2):
        for p in (0, 1, info["partitions"] // 2, info["partitions"] - 1):
            seg = np.zeros(512)
            part = want[p * 256:(p + 1) * 256, ch]
            seg[:len(part)] = part
            ref = np.fft.rfft(seg)
            assert abs(H[ch, p][0].real - ref[0].real) < 2e-5 and abs(H[ch, p][0].imag - ref[256].real) < 2e-5
            assert np.abs(H[ch, p][1:] - ref[1:256]).max() < 2e-5
    c.close()


@pytest.mark.parametrize("src,dst", [(44100, 48000), (96000, 44100), (44100, 47999)])
def test_edges_one_frame_and_truncation(gpu_lib, src, dst):
    """A 1-frame IR gives ceil(p / q) taps; an IR whose converted length crosses n_ref - nframes stops there."""
    from cuda_audio_amd.synth import make_ir

    c = _conv(16384, dst, max_batch=8)
    one = np.array([[0.3, -0.2]], np.float32)
    c.prepare(0, one, ir_rate=src)
    _check_taps(c.ir_taps(0), resample(one, src, dst))
    assert c.ir_info(0)["taps"] == out_frames(1, src, dst)
    ir = make_ir(36000, seed=4, norm=0.05)  # (at 96 -> 44.1 kHz still past n_ref - 1024)
    for nframes in (1024, 4096):  # (the engine holds n_ref - 1024 taps at most)
        c.prepare(1, ir, nframes=nframes, ir_rate=src)
        assert c.ir_info(1)["taps"] == 16384 - nframes < out_frames(36000, src, dst)
        _check_taps(c.ir_taps(1), resample(ir, src, dst, n=16384 - nframes))
    c.close()


def test_refused_rates_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(3000, seed=2, norm=0.05)
    c = _conv(16384, 48000, max_batch=8)
    c.prepare(0, ir, ir_rate=44100)
    taps = c.ir_taps(0)
    for bad in (7999, 384001):
        with pytest.raises(McError):
            c.prepare(0, make_ir(5000, seed=3), ir_rate=bad)
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    assert c.num_irs() == 1
    c.close()


def test_equal_rates_are_mc_load_ir_bit_for_bit(gpu_lib):
    from cuda_audio_amd.synth import make_input, make_ir

    ir = make_ir(9000, seed=6, norm=0.05)
    x = make_input(64 * 256)
    outs = []
    for kind in ("plain", "equal"):
        c = _conv(16384, 44100 if kind == "equal" else None, max_batch=32)
        c.prepare(0, ir, ir_rate=44100)
        if kind == "equal":  # the entry point itself, not just the Python shortcut
            from cuda_audio_amd.engine import _fp

            lr = np.ascontiguousarray(ir, np.float32)
            assert c._L.mc_load_ir_resampled(c._h, 1, _fp(lr), lr.shape[0], 1024, 48000, 48000) == 0
        else:
            c.prepare(1, ir)
        outs.append((c.ir_taps(0), c.ir_spectra(0), c.ir_taps(1), c.ir_spectra(1), c.process(x[0], x[1])))
        c.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def _pair(n_ref, nframes=1024):
    from cuda_audio_amd.synth import make_ir

    irs = [(make_ir(7000, seed=11, norm=0.05), 44100), (make_ir(9000, seed=22, norm=0.05), 96000)]
    return irs, [_restated(ir, src, 48000, n_ref, nframes) for ir, src in irs]


P0 = dict(BASE, predelay=300, wet=0.7, panWet=0.25, vsteps=9)
P1 = dict(BASE, select=1, level=0.8)


@pytest.mark.parametrize("period", [256, 512])
def test_jack_periods_match_the_oracle(oracle_mod, gpu_lib, period):
    """One period per mc_process call (past the cold-start ramp: parked periods included)."""
    from cuda_audio_amd.synth import make_input

    n_ref, ncalls = 16384, 420 * 256 // period
    irs, taps = _pair(n_ref)
    x = make_input(ncalls * period)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, P0, P1, True)
    want = ref.process(x[0], x[1], block=period)
    c = _conv(n_ref, 48000, max_batch=16, period=period)
    for i, (ir, src) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src)
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period]))
                          for k in range(ncalls)], axis=1)
    c.close()
    assert rms(want) > 0.05
    assert rms(got - want) <= RMS_TOL


@pytest.mark.parametrize("compat", [True, False])
def test_short_batch_matches_the_oracle(oracle_mod, gpu_lib, compat):
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 96
    irs, taps = _pair(n_ref)
    x = make_input(nb * 256)
    o = oracle_mod.Upols(n_ref, compat)
    for i, t in enumerate(taps):
        o.prepare(i, t)
    apply_params(o, P0, P1, True)
    want = o.process(x[0], x[1])
    c = _conv(n_ref, 48000, max_batch=32, compat=compat)
    for i, (ir, src) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src)
    apply_params(c, P0, P1, False)
    got = c.process(x[0], x[1])
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_single_transform_form(oracle_mod, gpu_lib):
    """form = 1 builds its spectrum from the device-converted taps (it keeps none: item 17 is MC_ERR_STATE)."""
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
    c = _conv(n_ref, 48000, max_batch=32, form="single")
    for i, (ir, src) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src)
    info = c.ir_info(1)
    assert info["taps"] == len(taps[1])
    np.testing.assert_allclose(info["sigma"], taps[1].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
    with pytest.raises(McError) as ex:
        c.ir_taps(0)
    assert ex.value.code == -3
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_overlap_save_batch(oracle_mod, gpu_lib):
    """A settled batch of 12288 blocks takes the overlap-save form (os_stats) with the converted IRs."""
    import torch

    from cuda_audio_amd.synth import make_input

    n_ref, T = 16384, 12288
    irs, taps = _pair(n_ref)
    xx = make_input(2 * T * 256)
    c = _conv(n_ref, 48000, max_batch=T)
    for i, (ir, src) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src)
    p = dict(BASE, select=1, wet=0.6, panWet=-0.25)
    for h in (0, 1):
        c.cc[h].value.update(**p)
    dx = torch.from_numpy(xx).to("cuda:0")
    out = torch.zeros(2, 2 * T * 256, device="cuda:0")
    for k in range(2):
        o = k * T * 256
        c.process_device(dx[0, o:].data_ptr(), dx[1, o:].data_ptr(), out[0, o:].data_ptr(), out[1, o:].data_ptr(), T)
    c.sync()
    took = c.os_stats()["batches"]
    c.close()
    assert took >= 1
    u = oracle_mod.Upols(n_ref, True)
    for i, t in enumerate(taps):
        u.prepare(i, t)
    for h in (0, 1):
        u.set(h, **p)
    b0, n = T + 4000, 96
    want = u.range(xx[0], xx[1], b0, n)
    u.close()
    got = out[:, b0 * 256:(b0 + n) * 256].cpu().numpy()
    assert rms(want) > 0.01
    assert rms(got - want) <= RMS_TOL


def test_shipped_tail_drop_regime(oracle_mod, gpu_lib):
    """n_ref 131072, predelay 1024, an IR whose converted length runs past n_ref - 1024 (Q8: the reference cuts what its
    shift pushes past n_ref; the cut terms come from the stored taps)."""
    from cuda_audio_amd.synth import make_input, make_ir

    n_ref, nb = 131072, 48
    ir = make_ir(125000, seed=7, norm=0.02)
    taps = _restated(ir, 44100, 48000, n_ref)
    assert len(taps) == n_ref - 1024
    x = make_input(nb * 256)
    p = dict(BASE, predelay=1024)
    ref = oracle_mod.RefCompat(n_ref, True)
    ref.prepare(0, taps)
    apply_params(ref, p, p, True)
    want = ref.process(x[0], x[1])
    c = _conv(n_ref, 48000, max_batch=16)
    c.prepare(0, ir, ir_rate=44100)
    apply_params(c, p, p, False)
    got = c.process(x[0], x[1])
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_fp16_storage(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 96
    irs, taps = _pair(n_ref)
    x = make_input(nb * 256)
    o = oracle_mod.Upols(n_ref, True)
    for i, t in enumerate(taps):
        o.prepare(i, t)
    o.set(1, select=1)
    want = o.process(x[0], x[1])
    c = _conv(n_ref, 48000, max_batch=32, precision="fp16")
    for i, (ir, src) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src)
    c.cc[1].value.select = 1
    got = c.process(x[0], x[1])
    c.close()
    wet = want - 0.5 * (x[0] + x[1])
    assert rms(got - want) <= FP16_REL_TOL * rms(wet)


def test_loudness_is_kept(gpu_lib):
    """The steady wet level of a 500 Hz tone through a 48 kHz engine with the converted IR is that of a 44.1 kHz engine with
    the original IR, within 0.1 dB."""
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(6000, seed=9, norm=0.05)

    def level(rate, ir_rate):
        nb = 200
        t = np.arange(nb * 256) / rate
        x = (0.25 * np.sin(2 * np.pi * 500.0 * t)).astype(np.float32)
        c = _conv(16384, rate, max_batch=40)
        c.prepare(0, ir, ir_rate=ir_rate)
        for h in (0, 1):
            c.cc[h].value.update(dry=0.0, wet=1.0, vsteps=0)
        y = c.process(x, np.zeros_like(x))[0].astype(np.float64)
        c.close()
        lo = 100 * 256  # past the IR's length and the gain ramp
        A = np.stack([np.sin(2 * np.pi * 500.0 * t[lo:]), np.cos(2 * np.pi * 500.0 * t[lo:])], axis=1)
        cf, *_ = np.linalg.lstsq(A, y[lo:], rcond=None)
        return float(np.hypot(*cf))

    a441, a48 = level(44100, 44100), level(48000, 44100)
    assert a441 > 1e-3
    assert abs(20 * np.log10(a48 / a441)) <= 0.1
