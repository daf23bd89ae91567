"""Equalisation of an IR on load on the device (mc_load_ir_eq, csrc/ireq.hip.h): the stored taps, the shape information and the
spectra against the float64 restatement (tests/ir_eq_np.py, a sequential recurrence), a unit impulse against the analytic
response (no recurrence), then every path of the engine against the oracle fed the restated taps.  The tolerances are those of
test_gpu_ir_shape.py: device double arithmetic rounded to float32 (at this module's lengths, 64 512 taps and fewer, the chunked
recurrence differs from the sequential one by 1.4e-9 relative RMS at worst; the float rounding of a stored tap is 2.5e-8).
Longer IRs and the worst-conditioned bands the limits allow, where that difference grows, are test_gpu_ir_long_carry.py's,
which has the figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_eq_np
from helpers import BASE, RMS_TOL, _dry, apply_params, rms
from ir_shape_np import assert_onset_margin, quiet_lead_ir, session_frames, shape
from test_gpu_ir_shape import (COMBINED_A, FP16_REL_TOL, OS_P, P0, P1, _check_info, _check_level, _check_taps, _os_want,
                               _settled_batches)

pytestmark = pytest.mark.gpu

CASCADE8 = (("lowcut", 60, 0, 1.0), ("lowshelf", 200, 6.0), ("peak", 400, -12.0, 4.0), ("peak", 1000, 6.0, 2.0), ("peak", 2500, 3.5, 0.3),
            ("peak", 5200, -18.0, 16.0), ("highshelf", 6000, -9.0, 0.5), ("highcut", 15000, 0, 0.9))
BANDS = {
    "lowcut": (("lowcut", 120),),
    "highcut": (("highcut", 9000),),
    "lowshelf": (("lowshelf", 200, 6.0),),
    "highshelf": (("highshelf", 6000, -9.0),),
    "peak": (("peak", 2500, 6.0, 1.5),),
    "cascade8": CASCADE8,
}
RATES = [(44100, 44100), (44100, 48000)]
# (name of the bands, IR rate, session rate, shape fields); the last is the ill-conditioned one: poles 2.3e-4 inside the circle
CASES = [(name, src, dst, None) for name in BANDS for src, dst in RATES] + [("cascade8", 44100, 48000, "combined_a"), ("lowcut20", 384000, 384000, None)]
BANDS_MORE = {"lowcut20": (("lowcut", 20),)}
LENGTH_BANDS = (("lowcut", 120), ("peak", 2500, 6.0, 1.5))


def _conv(n_ref, rate, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    return Convolution("ireq", n_ref, sample_rate=rate, **kw)


def _ieq(bands):
    from cuda_audio_amd.engine import IrEq

    return IrEq(bands=list(bands))


def _ishape(fields):
    from cuda_audio_amd.engine import IrShape

    return IrShape(**fields) if fields else None


def _margin(ir, src, dst, fields):
    if fields and fields.get("trim_db", 0) < 0:
        assert_onset_margin(session_frames(ir, src, dst), fields.get("start", 0), fields["trim_db"])


def _check_eq_info(got, want):
    _check_info(got, want)
    assert got["eq_bands"] == want["eq_bands"]


def _check_sums_and_spectra(c, idx, got, want):
    """mc_ir_info's sums against the stored taps and four partitions' 512-point spectra against the restated taps
    (as test_gpu_ir_shape.py)."""
    n = len(want)
    info = c.ir_info(idx)
    assert info["taps"] == n and info["partitions"] == (n + 255) // 256
    g64 = got.astype(np.float64)
    sg = np.where(np.arange(n) % 2, -1.0, 1.0)
    np.testing.assert_allclose(info["sigma"], g64.sum(axis=0), rtol=0, atol=1e-9)
    np.testing.assert_allclose(info["alpha"], (sg[:, None] * g64).sum(axis=0), rtol=0, atol=1e-9)
    H = c.ir_spectra(idx)
    for ch in range(2):
        for p in sorted({0, min(1, info["partitions"] - 1), info["partitions"] // 2, info["partitions"] - 1}):
            seg = np.zeros(512)
            part = want[p * 256:(p + 1) * 256, ch]
            seg[:len(part)] = part
            ref = np.fft.rfft(seg)
            assert abs(H[ch, p][0].real - ref[0].real) < 2e-5 and abs(H[ch, p][0].imag - ref[256].real) < 2e-5
            assert np.abs(H[ch, p][1:] - ref[1:256]).max() < 2e-5


@pytest.mark.parametrize("name,src,dst,shaped", CASES)
def test_taps_info_and_spectra_match_the_restatement(gpu_lib, name, src, dst, shaped):
    bands = BANDS.get(name) or BANDS_MORE[name]
    fields = COMBINED_A if shaped else {}
    n_ref = 65536
    ir = quiet_lead_ir()
    _margin(ir, src, dst, fields)
    want, winfo = ir_eq_np.eq(ir, n_ref - 1024, src, dst, bands, **fields)
    c = _conv(n_ref, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src, shape=_ishape(fields), eq=_ieq(bands))
    got = c.ir_taps(0)
    _check_taps(got, want.astype(np.float64))
    _check_eq_info(c.ir_shape_info(0), winfo)
    _check_sums_and_spectra(c, 0, got, want)
    c.close()


@functools.lru_cache(maxsize=None)
def _length_ir():
    return quiet_lead_ir(45000, seed=5)


# 1 .. 3: shorter than the recurrence's order; 255 .. 257: one chunk of ireq.hip.h (and one workgroup of its map kernels) and a tap
# either side; 4095 .. 4097: sixteen chunks and a tap either side; 16383 .. 16385: one workgroup's span of the chunk pass; 32768 / 32769: one chunk per
# run of the carry pass and two; 40000: three workgroups of the chunk pass, 157 of the others, two chunks per run
LENGTHS_16K = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097]
LENGTHS_64K = [16383, 16384, 16385, 32768, 32769, 40000]


@pytest.mark.parametrize("n_ref,length", [(16384, n) for n in LENGTHS_16K] + [(65536, n) for n in LENGTHS_64K])
def test_lengths(gpu_lib, n_ref, length):
    ir = _length_ir()
    fields = dict(start=700, length=length)
    want, winfo = ir_eq_np.eq(ir, n_ref - 1024, None, 48000, LENGTH_BANDS, **fields)
    assert winfo["taps"] == length
    c = _conv(n_ref, 48000, max_batch=8)
    c.prepare(0, ir, shape=_ishape(fields), eq=_ieq(LENGTH_BANDS))
    got = c.ir_taps(0)
    _check_taps(got, want.astype(np.float64))
    _check_eq_info(c.ir_shape_info(0), winfo)
    _check_sums_and_spectra(c, 0, got, want)
    c.close()


def test_unit_impulse_has_the_analytic_response(gpu_lib):
    """Independent of the restatement's recurrence: the device's 32768 stored taps of a unit impulse transform to H(e^{jw})."""
    rate, n = 48000, 32768
    bands = (("lowcut", 80), ("peak", 1000, 6.0, 2.0), ("highcut", 8000))
    ir = np.zeros((n, 2), np.float32)
    ir[0] = 1.0
    c = _conv(65536, rate, max_batch=8)
    c.prepare(0, ir, eq=_ieq(bands))
    got = c.ir_taps(0)
    c.close()
    assert got.shape == (n, 2) and got.dtype == np.float32
    want = ir_eq_np.response(bands, rate, np.arange(n // 2 + 1) * rate / n)
    for ch in range(2):
        err = np.abs(np.fft.rfft(got[:, ch].astype(np.float64)) - want).max()
        print(f"channel {ch}: max |rfft - H| {err:.2e}, max |H| {np.abs(want).max():.3f}")
        assert err <= 1e-6


def test_order_of_operations(gpu_lib):
    """The bands act on the faded taps and the normalisation on the bands' output: max |stored tap| is the target, the
    reported peak and gain are the equalised taps', and the fade's zero at the end is filled by the bands' ringing."""
    n_ref = 16384
    ir = quiet_lead_ir(9000, seed=8)
    fields = dict(fade_out=512, normalize="peak", target=0.02)
    bands = (("peak", 1000, 12.0),)
    want, winfo = ir_eq_np.eq(ir, n_ref - 1024, None, 48000, bands, **fields)
    plain, pinfo = shape(ir, n_ref - 1024, **fields)
    assert winfo["peak"] > 1.05 * pinfo["peak"]  # (the boost shows in what is measured)
    # on the restatement: the un-equalised last tap carries the fade's last factor, the equalised one does not
    assert np.abs(plain[-1]).max() < 1e-3 * np.abs(plain[-513]).max()
    assert np.abs(want[-1]).max() > 30 * np.abs(plain[-1]).max()
    c = _conv(n_ref, 48000, max_batch=8)
    c.prepare(0, ir, shape=_ishape(fields), eq=_ieq(bands))
    got = c.ir_taps(0)
    sinfo = c.ir_shape_info(0)
    c.close()
    _check_taps(got, want.astype(np.float64))
    _check_eq_info(sinfo, winfo)
    assert abs(float(np.abs(got).max()) / float(np.float32(0.02)) - 1) <= 1e-6
    assert np.abs(got[-1]).max() > 30 * np.abs(plain[-1]).max()
    assert np.abs(got[-1] - want[-1]).max() <= 1e-5 * np.abs(want).max()


def test_no_band_on_is_the_other_loads_bit_for_bit(gpu_lib):
    """mc_load_ir_eq with every band off against mc_load_ir, mc_load_ir_resampled and mc_load_ir_shaped."""
    from cuda_audio_amd._lib import McError, McIrEq, McIrShape
    from cuda_audio_amd.engine import IrShape, _fp
    from cuda_audio_amd.synth import make_input, make_ir

    ir = make_ir(9000, seed=6, norm=0.05)
    lr = np.ascontiguousarray(ir, np.float32)
    x = make_input(64 * 256)
    on = IrShape(**COMBINED_A)
    outs = []
    for kind in ("others", "eq"):
        c = _conv(16384, 48000, max_batch=32)
        if kind == "eq":  # the entry point itself, with the eq mc_default_ir_eq gives (and one whose off bands hold nonsense)
            off = McIrEq()
            c._L.mc_default_ir_eq(C.byref(off))
            junk = McIrEq()
            c._L.mc_default_ir_eq(C.byref(junk))
            junk.band[3].freq_hz, junk.band[3].q, junk.band[3].gain_db = 1.0, 0.0, 99.0
            sh_off = McIrShape()
            c._L.mc_default_ir_shape(C.byref(sh_off))
            assert c._L.mc_load_ir_eq(c._h, 0, _fp(lr), lr.shape[0], 1024, 0, 0, None, C.byref(off)) == 0
            assert c._L.mc_load_ir_eq(c._h, 1, _fp(lr), lr.shape[0], 1024, 44100, 48000, C.byref(sh_off), C.byref(junk)) == 0
            assert c._L.mc_load_ir_eq(c._h, 2, _fp(lr), lr.shape[0], 1024, 48000, 48000, None, C.byref(off)) == 0
            assert c._L.mc_load_ir_eq(c._h, 3, _fp(lr), lr.shape[0], 1024, 44100, 48000, C.byref(on.to_c()), C.byref(off)) == 0
        else:
            c.prepare(0, ir)
            c.prepare(1, ir, ir_rate=44100)
            c.prepare(2, ir, ir_rate=48000)
            c.prepare(3, ir, ir_rate=44100, shape=on)
        for i in range(3):  # (the plain loads themselves: no shape information is left)
            with pytest.raises(McError) as ex:
                c.ir_shape_info(i)
            assert ex.value.code == -3
        assert c.ir_shape_info(3)["eq_bands"] == 0
        res = [c.ir_taps(i) for i in range(4)] + [c.ir_spectra(i) for i in range(4)] + [c.ir_shape_info(3), c.ir_info(3)]
        for sel in ((0, 1), (2, 3)):
            c.reset()
            c.cc[0].value.select, c.cc[1].value.select = sel
            res.append(c.process(x[0], x[1]))
        outs.append(res)
        c.close()
    for a, b in zip(*outs):
        if isinstance(a, dict):
            assert a == b
        else:
            np.testing.assert_array_equal(a, b)


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, IrShape
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(3000, seed=2, norm=0.05)
    c = _conv(16384, 48000, max_batch=8)
    good = IrEq(bands=[("lowcut", 120), ("peak", 2500, 6.0, 1.5)])
    c.prepare(0, ir, ir_rate=44100, shape=IrShape(fade_out=100, normalize="peak", target=0.02), eq=good)
    taps, spec, info, sinfo = c.ir_taps(0), c.ir_spectra(0), c.ir_info(0), c.ir_shape_info(0)
    assert sinfo["eq_bands"] == 2
    other = make_ir(5000, seed=3)
    bad = [IrEq(bands=[("peak", 9.0, 3.0)]), IrEq(bands=[("peak", 0.46 * 48000, 3.0)]), IrEq(bands=[("lowcut", float("nan"))]),
           IrEq(bands=[("peak", 1000, 25.0)]), IrEq(bands=[("lowshelf", 1000, -37.0)]), IrEq(bands=[("highcut", 1000, 0, 0.05)]),
           IrEq(bands=[("off", 1000), ("peak", 1000, 3.0, 33.0)]), IrEq(bands=[("peak", 1000, 3.0, float("inf"))])]
    for eq in bad:
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, eq=eq)
            assert ex.value.code == -1
    for kw in (dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=5000)), dict(ir_rate=7999), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, eq=good, **kw)
            assert ex.value.code == -1
    nosr = _conv(16384, None, max_batch=8)  # (an engine without a session rate: 0 / 0 with a band on)
    with pytest.raises(McError) as ex:
        nosr.prepare(0, other, eq=good)
    assert ex.value.code == -1 and nosr.num_irs() == 0
    nosr.close()
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    np.testing.assert_array_equal(c.ir_spectra(0), spec)
    assert c.ir_info(0) == info and c.ir_shape_info(0) == sinfo
    assert c.num_irs() == 1
    c.close()


@pytest.mark.parametrize("src,dst", RATES)
def test_the_same_load_twice_gives_the_same_bits(gpu_lib, src, dst):
    ir = quiet_lead_ir()
    _margin(ir, src, dst, COMBINED_A)
    c = _conv(65536, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src)  # (index 0 is a used one: the first equalised load replaces a plain one)
    res = []
    for idx in (0, 1, 0):
        c.prepare(idx, ir, ir_rate=src, shape=_ishape(COMBINED_A), eq=_ieq(CASCADE8))
        res.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_info(idx), c.ir_shape_info(idx)))
    c.close()
    for r in res[1:]:
        np.testing.assert_array_equal(r[0], res[0][0])
        np.testing.assert_array_equal(r[1], res[0][1])
        assert r[2] == res[0][2] and r[3] == res[0][3]


# -- every path plays the equalised IRs ----------------------------------------------------------------------------------
SESSION = 48000
IR_A = dict(frames=7000, seed=11, rate=44100, bands=(("lowcut", 120), ("peak", 2500, 6.0, 1.5), ("highcut", 9000)),
            fields=dict(trim_db=-20, pre_roll=16, reverse=True, decay_t60=6000, fade_out=512, normalize="energy", target=0.25))
IR_B = dict(frames=9000, seed=22, rate=SESSION, bands=(("lowshelf", 200, 6.0), ("highshelf", 6000, -9.0)),
            fields=dict(start=100, length=5000, normalize="peak", target=0.02))


@functools.lru_cache(maxsize=None)
def _pair(n_ref=16384, nframes=1024):
    """The two equalised IRs, the first of them converted: [(frames, spec)] and their restated taps (computed once)."""
    irs = [(quiet_lead_ir(s["frames"], seed=s["seed"]), s) for s in (IR_A, IR_B)]
    taps = []
    for ir, s in irs:
        _margin(ir, s["rate"], SESSION, s["fields"])
        t = ir_eq_np.eq(ir, n_ref - nframes, s["rate"], SESSION, s["bands"], **s["fields"])[0]
        t.setflags(write=False)
        taps.append(t)
    return irs, taps


def _prepare_pair(c, irs):
    for i, (ir, s) in enumerate(irs):
        c.prepare(i, ir, ir_rate=s["rate"], shape=_ishape(s["fields"]), eq=_ieq(s["bands"]))


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
    """form = 1 builds its spectrum from the equalised taps left on the device."""
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
    for i, (ir, s) in enumerate(irs):
        info = c.ir_info(i)
        assert info["taps"] == len(taps[i])
        np.testing.assert_allclose(info["sigma"], taps[i].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
        _check_eq_info(c.ir_shape_info(i), ir_eq_np.eq(ir, n_ref - 1024, s["rate"], SESSION, s["bands"], **s["fields"])[1])
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_overlap_save_batch(oracle_mod, gpu_lib):
    """A settled batch of 12288 blocks takes the overlap-save form (os_stats) with the equalised IRs."""
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
