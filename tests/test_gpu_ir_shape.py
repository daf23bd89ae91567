"""IR shaping on load on the device (mc_load_ir_shaped, csrc/irshape.hip.h): the stored taps, the shape information and
the spectra against the float64 restatement (tests/ir_shape_np.py), then every path of the engine against the oracle fed the
restated taps.  Every test that trims first asserts, on the restatement, that the onset stands clear of the threshold
(ir_shape_np.assert_onset_margin); every oracle comparison that the wet sum stays far inside the reference's clamp."""
import ctypes as C

import numpy as np
import pytest

from helpers import BASE, RMS_TOL, _dry, apply_params, rms
from ir_shape_np import assert_onset_margin, quiet_lead_ir, session_frames, shape

pytestmark = pytest.mark.gpu

FP16_REL_TOL = 2e-3  # the bar of the existing fp16 tests (test_gpu_parity.py)
RATES = [(44100, 44100), (44100, 48000), (96000, 44100)]
COMBINED_A = dict(trim_db=-20, pre_roll=16, reverse=True, decay_t60=6000, fade_out=512, normalize="energy", target=0.25)
COMBINED_B = dict(start=100, length=5000, normalize="peak", target=0.02)
SHAPES = {
    "start": dict(start=100),
    "trim20": dict(trim_db=-20),
    "trim16_preroll": dict(trim_db=-16, pre_roll=16),
    "length": dict(length=5000),
    "reverse": dict(reverse=True),
    "decay": dict(decay_t60=6000),
    "fade": dict(fade_out=512),
    "peak": dict(normalize="peak", target=0.02),
    "energy": dict(normalize="energy", target=0.25),
    "combined_a": COMBINED_A,
    "combined_b": COMBINED_B,
}
# (-40 dB holds the onset margin at equal rates only, -60 dB lies under the lead-in's noise: onset 0, nothing trimmed)
CASES = [(name, src, dst) for name in SHAPES for src, dst in RATES] + [("trim40", 44100, 44100), ("trim60", 44100, 44100)]
SHAPES_EQUAL_ONLY = {"trim40": dict(trim_db=-40), "trim60": dict(trim_db=-60)}
SELECT_ONLY = {"start", "trim20", "trim16_preroll", "length", "reverse", "trim40", "trim60"}  # frames moved, none changed


def _conv(n_ref, rate, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    return Convolution("irshape", n_ref, sample_rate=rate, **kw)


def _ishape(fields):
    from cuda_audio_amd.engine import IrShape

    return IrShape(**fields)


def _margin(ir, src, dst, fields):
    if fields.get("trim_db", 0) < 0:
        assert_onset_margin(session_frames(ir, src, dst), fields.get("start", 0), fields["trim_db"])


def _check_taps(got, want64):
    """The bar of test_gpu_resample.py::_check_taps: device double arithmetic rounded to float32."""
    err = got.astype(np.float64) - want64
    assert got.shape == want64.shape
    print(f"taps: rms err {rms(err):.3e} of {rms(want64):.3e}, max err {np.abs(err).max():.3e} of {np.abs(want64).max():.3e}")
    assert rms(err) <= 1e-6 * rms(want64), f"rms {rms(err):.3e} vs {rms(want64):.3e}"
    assert np.abs(err).max() <= 1e-5 * np.abs(want64).max()


def _check_info(got, want):
    print("shape info:", got, "restated:", want)
    for k in ("frames", "onset", "first", "taps"):
        assert got[k] == want[k], k
    for k in ("gain", "peak", "energy"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), k


def _check_level(want, x, p0, p1):
    """Q4 (the reference clamps its wet sum at +-1, the partitioned engine does not) must not enter a comparison."""
    wet = want - _dry(x, p0, p1)
    print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert np.abs(wet).max() < 0.5
    assert rms(want) > 0.01


@pytest.mark.parametrize("name,src,dst", CASES)
def test_taps_info_and_spectra_match_the_restatement(gpu_lib, name, src, dst):
    fields = SHAPES.get(name) or SHAPES_EQUAL_ONLY[name]
    n_ref = 65536
    ir = quiet_lead_ir()
    _margin(ir, src, dst, fields)
    want, winfo = shape(ir, n_ref - 1024, src, dst, **fields)
    if name == "trim60":
        assert winfo["onset"] == 0 and winfo["first"] == 0 and winfo["taps"] == len(ir)
    c = _conv(n_ref, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src, shape=_ishape(fields))
    got = c.ir_taps(0)
    n = winfo["taps"]
    if src == dst and name in SELECT_ONLY:
        np.testing.assert_array_equal(got, want)
    _check_taps(got, want.astype(np.float64))
    _check_info(c.ir_shape_info(0), winfo)
    info = c.ir_info(0)
    assert info["taps"] == n and info["partitions"] == (n + 255) // 256
    g64 = got.astype(np.float64)
    sg = np.where(np.arange(n) % 2, -1.0, 1.0)
    np.testing.assert_allclose(info["sigma"], g64.sum(axis=0), rtol=0, atol=1e-9)
    np.testing.assert_allclose(info["alpha"], (sg[:, None] * g64).sum(axis=0), rtol=0, atol=1e-9)
    # per-partition 512-point spectra against numpy's rfft of the restated taps (as test_gpu_resample.py)
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


@pytest.mark.parametrize("src,dst", [(44100, 44100), (44100, 48000)])
def test_truncation_comes_before_the_fade_and_the_gain(gpu_lib, src, dst):
    """An IR longer than n_ref - nframes after trimming is cut there; the fade ends at the last stored tap and the
    normalisation measures what is stored."""
    n_ref = 16384
    ir = quiet_lead_ir(36000, seed=4)
    fields = dict(trim_db=-16, pre_roll=16, fade_out=512, normalize="energy", target=0.25)  # (-20 dB fails the margin at 48 kHz)
    _margin(ir, src, dst, fields)
    c = _conv(n_ref, dst, max_batch=8)
    for nframes in (1024, 4096):
        want, winfo = shape(ir, n_ref - nframes, src, dst, **fields)
        c.prepare(1, ir, nframes=nframes, ir_rate=src, shape=_ishape(fields))
        assert c.ir_info(1)["taps"] == n_ref - nframes == winfo["taps"] < winfo["frames"] - winfo["first"]
        got = c.ir_taps(1)
        _check_taps(got, want.astype(np.float64))
        _check_info(c.ir_shape_info(1), winfo)
        # the last stored tap carries the fade's last factor (about 1e-5 of what it was), the tap before the fade none
        assert np.abs(got[-1]).max() < 1e-3 * np.abs(got[-513]).max()
    c.close()


def test_everything_off_is_the_plain_and_the_resampled_load_bit_for_bit(gpu_lib):
    from cuda_audio_amd._lib import McError, McIrShape
    from cuda_audio_amd.engine import _fp
    from cuda_audio_amd.synth import make_input, make_ir

    ir = make_ir(9000, seed=6, norm=0.05)
    lr = np.ascontiguousarray(ir, np.float32)
    x = make_input(64 * 256)
    outs = []
    for kind in ("plain", "shaped"):
        c = _conv(16384, 48000, max_batch=32)
        if kind == "shaped":  # the entry point itself, with the shape mc_default_ir_shape gives
            off = McIrShape()
            c._L.mc_default_ir_shape(C.byref(off))
            assert c._L.mc_load_ir_shaped(c._h, 0, _fp(lr), lr.shape[0], 1024, 0, 0, C.byref(off)) == 0
            assert c._L.mc_load_ir_shaped(c._h, 1, _fp(lr), lr.shape[0], 1024, 44100, 48000, C.byref(off)) == 0
            assert c._L.mc_load_ir_shaped(c._h, 2, _fp(lr), lr.shape[0], 1024, 48000, 48000, C.byref(off)) == 0
            for i in range(3):  # (the plain loads themselves: no shape information is left)
                with pytest.raises(McError) as ex:
                    c.ir_shape_info(i)
                assert ex.value.code == -3
        else:
            c.prepare(0, ir)
            c.prepare(1, ir, ir_rate=44100)
            c.prepare(2, ir, ir_rate=48000)
        c.cc[1].value.select = 1
        outs.append([c.ir_taps(i) for i in range(3)] + [c.ir_spectra(i) for i in range(3)] + [c.process(x[0], x[1])])
        c.close()
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrShape
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(3000, seed=2, norm=0.05)
    c = _conv(16384, 48000, max_batch=8)
    c.prepare(0, ir, ir_rate=44100, shape=IrShape(fade_out=100, normalize="peak", target=0.02))
    taps, info, sinfo = c.ir_taps(0), c.ir_info(0), c.ir_shape_info(0)
    other = make_ir(5000, seed=3)
    bad = [IrShape(start=5000), IrShape(start=1 << 40), IrShape(trim_db=1.0), IrShape(trim_db=-121.0), IrShape(trim_db=float("nan")),
           IrShape(normalize="peak", target=0.0), IrShape(normalize="energy", target=float("inf")), IrShape(fade_out=10, start=5000)]
    for s in bad:
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, shape=s)
            assert ex.value.code == -1
    with pytest.raises(McError):  # (converted: 5000 frames at 44.1 kHz are 5443 at 48 kHz)
        c.prepare(0, other, ir_rate=44100, shape=IrShape(start=5443))
    with pytest.raises(McError):
        c.prepare(0, other, ir_rate=7999, shape=IrShape(fade_out=10))
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    assert c.ir_info(0) == info and c.ir_shape_info(0) == sinfo
    assert c.num_irs() == 1
    c.prepare(0, other, ir_rate=44100, shape=IrShape(start=5442))  # the last frame alone is a load
    assert c.ir_info(0)["taps"] == 1
    c.close()


@pytest.mark.parametrize("src,dst", [(44100, 44100), (44100, 48000)])
def test_the_same_load_twice_gives_the_same_bits(gpu_lib, src, dst):
    ir = quiet_lead_ir()
    _margin(ir, src, dst, COMBINED_A)
    c = _conv(65536, dst, max_batch=8)
    res = []
    for idx in (0, 1, 0):
        c.prepare(idx, ir, ir_rate=src, shape=_ishape(COMBINED_A))
        res.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_info(idx), c.ir_shape_info(idx)))
    c.close()
    for r in res[1:]:
        np.testing.assert_array_equal(r[0], res[0][0])
        np.testing.assert_array_equal(r[1], res[0][1])
        assert r[2] == res[0][2] and r[3] == res[0][3]


# -- every path plays the shaped IR ------------------------------------------------------------------------------------
SESSION = 48000


def _pair(n_ref, nframes=1024):
    """Two shaped IRs, the first of them converted: [(frames, rate, shape fields)] and their restated taps."""
    irs = [(quiet_lead_ir(7000, seed=11), 44100, COMBINED_A), (quiet_lead_ir(9000, seed=22), SESSION, COMBINED_B)]
    for ir, src, fields in irs:
        _margin(ir, src, SESSION, fields)
    return irs, [shape(ir, n_ref - nframes, src, SESSION, **fields)[0] for ir, src, fields in irs]


def _prepare_pair(c, irs):
    for i, (ir, src, fields) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src, shape=_ishape(fields))


P0 = dict(BASE, predelay=300, wet=0.7, panWet=0.25, vsteps=9)
P1 = dict(BASE, select=1, level=0.8)


@pytest.mark.parametrize("period", [256, 512])
def test_jack_periods_match_the_oracle(oracle_mod, gpu_lib, period):
    from cuda_audio_amd.synth import make_input

    n_ref, ncalls = 16384, 420 * 256 // period
    irs, taps = _pair(n_ref)
    x = make_input(ncalls * period)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, P0, P1, True)
    want = ref.process(x[0], x[1], block=period)
    _check_level(want, x, P0, P1)
    c = _conv(n_ref, SESSION, max_batch=16, period=period)
    _prepare_pair(c, irs)
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period]))
                          for k in range(ncalls)], axis=1)
    c.close()
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
    _check_level(want, x, P0, P1)
    c = _conv(n_ref, SESSION, max_batch=32, compat=compat)
    _prepare_pair(c, irs)
    apply_params(c, P0, P1, False)
    got = c.process(x[0], x[1])
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_single_transform_form(oracle_mod, gpu_lib):
    """form = 1 builds its spectrum from the shaped taps left on the device (it keeps none: item 17 is MC_ERR_STATE)."""
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
    c = _conv(n_ref, SESSION, max_batch=32, form="single")
    _prepare_pair(c, irs)
    for i, (ir, src, fields) in enumerate(irs):
        info = c.ir_info(i)
        assert info["taps"] == len(taps[i])
        np.testing.assert_allclose(info["sigma"], taps[i].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
        _check_info(c.ir_shape_info(i), shape(ir, n_ref - 1024, src, SESSION, **fields)[1])
    with pytest.raises(McError) as ex:
        c.ir_taps(0)
    assert ex.value.code == -3
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


OS_P = dict(BASE, select=1, wet=0.6, panWet=-0.25)


def _settled_batches(c, xx, T):
    """Two settled batches of T blocks through the device-buffer call; returns the output [2, 2 T 256] (torch, on the device)."""
    import torch

    dx = torch.from_numpy(xx).to("cuda:0")
    out = torch.zeros(2, 2 * T * 256, device="cuda:0")
    for k in range(2):
        o = k * T * 256
        c.process_device(dx[0, o:].data_ptr(), dx[1, o:].data_ptr(), out[0, o:].data_ptr(), out[1, o:].data_ptr(), T)
    c.sync()
    return out


def _os_want(oracle_mod, n_ref, taps, xx, b0, n):
    u = oracle_mod.Upols(n_ref, True)
    for i, t in enumerate(taps):
        u.prepare(i, t)
    for h in (0, 1):
        u.set(h, **OS_P)
    want = u.range(xx[0], xx[1], b0, n)
    u.close()
    _check_level(want, xx[:, b0 * 256:(b0 + n) * 256], OS_P, OS_P)
    return want


def test_overlap_save_batch(oracle_mod, gpu_lib):
    """A settled batch of 12288 blocks takes the overlap-save form (os_stats) with the shaped IRs."""
    from cuda_audio_amd.synth import make_input

    n_ref, T = 16384, 12288
    irs, taps = _pair(n_ref)
    xx = make_input(2 * T * 256)
    c = _conv(n_ref, SESSION, max_batch=T)
    _prepare_pair(c, irs)
    for h in (0, 1):
        c.cc[h].value.update(**OS_P)
    out = _settled_batches(c, xx, T)
    took = c.os_stats()["batches"]
    c.close()
    assert took >= 1
    b0, n = T + 4000, 96
    want = _os_want(oracle_mod, n_ref, taps, xx, b0, n)
    got = out[:, b0 * 256:(b0 + n) * 256].cpu().numpy()
    assert rms(got - want) <= RMS_TOL


def test_a_shaped_reload_over_a_used_index(oracle_mod, gpu_lib):
    """Index 1 has played unshaped through two settled batches (its overlap-save spectra and the other derived copies exist);
    it is loaded again with a shape, the engine is reset and plays the same batches: the output is the shaped IR's."""
    from cuda_audio_amd.synth import make_input

    n_ref, T = 16384, 12288
    irs, taps = _pair(n_ref)
    xx = make_input(2 * T * 256)
    c = _conv(n_ref, SESSION, max_batch=T)
    for i, (ir, src, _) in enumerate(irs):
        c.prepare(i, ir, ir_rate=src)
    for h in (0, 1):
        c.cc[h].value.update(**OS_P)
    _settled_batches(c, xx, T)
    before = c.os_stats()
    assert before["batches"] >= 1 and before["spectra_builds"] >= 1
    _prepare_pair(c, irs)
    c.reset()
    out = _settled_batches(c, xx, T)
    after = c.os_stats()
    c.close()
    assert after["batches"] > before["batches"] and after["spectra_builds"] > before["spectra_builds"]
    b0, n = T + 4000, 96
    want = _os_want(oracle_mod, n_ref, taps, xx, b0, n)
    got = out[:, b0 * 256:(b0 + n) * 256].cpu().numpy()
    assert rms(got - want) <= RMS_TOL


def test_shipped_tail_drop_regime(oracle_mod, gpu_lib):
    """n_ref 131072, predelay 1024, a trimmed, faded and normalised IR that still reaches n_ref - 1024 taps (Q8: the reference
    cuts what its shift pushes past n_ref; the cut terms come from the stored, shaped taps)."""
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 131072, 48
    ir = quiet_lead_ir(125000, seed=10, norm=0.02)
    fields = dict(trim_db=-20, pre_roll=16, fade_out=2048, normalize="energy", target=0.25)
    _margin(ir, 44100, SESSION, fields)
    taps, winfo = shape(ir, n_ref - 1024, 44100, SESSION, **fields)
    assert len(taps) == n_ref - 1024 and winfo["first"] > 0
    x = make_input(nb * 256)
    p = dict(BASE, predelay=1024)
    ref = oracle_mod.RefCompat(n_ref, True)
    ref.prepare(0, taps)
    apply_params(ref, p, p, True)
    want = ref.process(x[0], x[1])
    _check_level(want, x, p, p)
    c = _conv(n_ref, SESSION, max_batch=16)
    c.prepare(0, ir, ir_rate=44100, shape=_ishape(fields))
    _check_info(c.ir_shape_info(0), winfo)
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
    p1 = dict(BASE, select=1)
    apply_params(o, BASE, p1, True)
    want = o.process(x[0], x[1])
    _check_level(want, x, BASE, p1)
    c = _conv(n_ref, SESSION, max_batch=32, precision="fp16")
    _prepare_pair(c, irs)
    apply_params(c, BASE, p1, False)
    got = c.process(x[0], x[1])
    c.close()
    wet = want - _dry(x, BASE, p1)
    assert rms(got - want) <= FP16_REL_TOL * rms(wet)
