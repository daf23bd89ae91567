"""Synthesis of an IR on the device from a seed (mc_synth_ir, csrc/irsynth.hip.h): the stored taps, the shape information, the
sums and the spectra against the float64 restatement (tests/ir_synth_np.py), the parts of the definition that are exact (which
frames are zero, where the reflections land, equal channels at width 0), every length at which the kernel's walk changes, the
chain through shaping, damping and EQ, the decay mc_ir_decay then reads, and the engine's paths against the oracle fed the
restated taps.  Tolerances are test_gpu_ir_shape.py's: device double arithmetic (log, cos, exp2 a few ulp of a double from
numpy's) rounded to float32."""
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_decay_np
import ir_synth_np
from helpers import BASE, RMS_TOL, _dry, apply_params, rms
from ir_shape_np import assert_onset_margin, shape
from test_gpu_ir_eq import CASCADE8, _check_eq_info, _check_sums_and_spectra
from test_gpu_ir_shape import COMBINED_A, FP16_REL_TOL, OS_P, P0, P1, _check_level, _check_taps, _os_want, _settled_batches

pytestmark = pytest.mark.gpu

SPAN = 512  # frames per workgroup of k_synth: 256 threads, two frames each
FULL = dict(frames=45000, seed=(0x1234 << 32) | 7, late_start=1500, t60=20000, build_up=2000, late_gain=0.05, direct=1.0, n_early=12,
            early_first=100, early_last=1400, early_gain=0.5, width=0.7)


def _conv(n_ref, rate, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    return Convolution("irsynth", n_ref, sample_rate=rate, **kw)


def _isynth(p):
    from cuda_audio_amd.engine import IrSynth

    return IrSynth(**p)


def _plain_info(F, n):
    """What mc_ir_shape_info reports of a synthesised IR with the shape off: F frames, n stored, gain 1."""
    return dict(frames=F, onset=0, first=0, taps=n)


def _check_plain(c, idx, p, cap):
    """Taps, shape information, sums and spectra of a synthesised IR with shape, EQ and damping off."""
    want = ir_synth_np.frames(**p)[:cap]
    got = c.ir_taps(idx)
    if np.abs(want).max() > 0:
        _check_taps(got, want.astype(np.float64))
    else:
        np.testing.assert_array_equal(got, want)
    info = c.ir_shape_info(idx)
    for k, v in _plain_info(p["frames"], len(want)).items():
        assert info[k] == v, k
    assert info["gain"] == 1.0 and info["eq_bands"] == 0
    assert abs(info["peak"] - np.abs(want).max()) <= 1e-6 * np.abs(want).max()
    _check_sums_and_spectra(c, idx, got, want)
    return got, want


@pytest.mark.parametrize("rate", [44100, 48000])
def test_everything_on_matches_the_restatement(gpu_lib, rate):
    c = _conv(65536, rate, max_batch=8)
    c.prepare_synth(0, _isynth(FULL))
    got, want = _check_plain(c, 0, FULL, 65536 - 1024)
    assert c.ir_synth_info(0) == dict(frames=45000, reflections=12, late_start=1500)
    # the exact parts: which frames of the build-up are empty, and that nothing sounds between the reflections before it
    zero_got, zero_want = (got == 0).all(axis=1), (want == 0).all(axis=1)
    assert 1000 < zero_want[1500:3500].sum() < 1900
    np.testing.assert_array_equal(zero_got, zero_want)
    c.close()


def test_reflection_positions_are_exact(gpu_lib):
    p = dict(FULL, late_gain=0.0, direct=0.0, n_early=64, early_last=60000)  # (some past F: dropped)
    tab = ir_synth_np.table(p)
    assert 0 < len(tab) < 64
    c = _conv(65536, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(p))
    got, want = _check_plain(c, 0, p, 65536 - 1024)
    np.testing.assert_array_equal(np.flatnonzero(np.abs(got).sum(axis=1)), sorted({pos for pos, _, _ in tab}))
    assert c.ir_synth_info(0)["reflections"] == len(tab)
    c.close()


def test_width_zero_gives_equal_channels(gpu_lib):
    p = dict(FULL, width=0.0, frames=6000)
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(p))
    got, _ = _check_plain(c, 0, p, 16384 - 1024)
    np.testing.assert_array_equal(got[:, 0], got[:, 1])
    assert np.count_nonzero(got[:, 0]) > 3000
    c.close()


def test_two_reflections_on_one_frame_are_added_in_order(gpu_lib):
    p = dict(frames=300, seed=5, late_start=300, n_early=2, early_first=77, early_last=77, early_gain=0.5, width=1.0)
    tab = ir_synth_np.table(p)
    assert [pos for pos, _, _ in tab] == [77, 77]
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(p))
    got = c.ir_taps(0)
    want = np.zeros((300, 2))
    for _, gL, gR in tab:
        want[77] += (gL, gR)
    assert np.abs(want[77]).min() > 0  # (the two do not cancel)
    np.testing.assert_array_equal(got, want.astype(np.float32))
    c.close()


# 1, 2, 3: the tail frame alone, one pair, a pair and the tail; SPAN and 2 SPAN with a frame either side: one workgroup's span
# and a multiple; 777: odd; 20000 at n_ref 16384: more generated than stored
LENGTHS = [1, 2, 3, SPAN - 1, SPAN, SPAN + 1, 777, 2 * SPAN - 1, 2 * SPAN, 2 * SPAN + 1, 20000]


@pytest.mark.parametrize("F", LENGTHS)
def test_lengths(gpu_lib, F):
    p = dict(frames=F, seed=99, late_start=0, t60=500, build_up=40, late_gain=0.1, direct=0.5, n_early=3, early_first=0, early_last=max(F - 1, 0),
             early_gain=0.25, width=0.6)
    n_ref = 16384
    c = _conv(n_ref, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(p))
    got, want = _check_plain(c, 0, p, n_ref - 1024)
    assert len(got) == min(F, n_ref - 1024) and c.ir_shape_info(0)["frames"] == F
    c.close()


@pytest.mark.parametrize("change", [dict(late_start=3000), dict(late_start=2 ** 40), dict(t60=0), dict(build_up=1), dict(build_up=65535, frames=70000, t60=0)])
def test_edges_of_the_late_field(gpu_lib, change):
    p = dict(frames=3000, seed=4, late_start=10, t60=900, build_up=100, late_gain=0.1, direct=1.0, width=0.3)
    p.update(change)
    n_ref = 131072 if p["frames"] > 60000 else 16384
    c = _conv(n_ref, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(p))
    got, want = _check_plain(c, 0, p, n_ref - 1024)
    np.testing.assert_array_equal((got == 0).all(axis=1), (want == 0).all(axis=1))
    if p["late_start"] >= p["frames"]:
        assert np.count_nonzero(got) == 2  # the direct sound alone
    if p["build_up"] == 1:
        assert (got[10:] != 0).all()
    if p["build_up"] == 65535:
        occ, prob = ir_synth_np.occupancy(p)
        assert not occ[:60000].all() and prob[65534] == 1.0 and prob[65533] < 1.0
    c.close()


def test_seeds(gpu_lib):
    p = dict(FULL, frames=5000, late_start=100, early_last=90, early_first=10)
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(p))
    c.prepare_synth(1, _isynth(dict(p, seed=p["seed"] ^ (1 << 40))))  # the high word alone differs
    c.prepare_synth(2, _isynth(p))
    a, b, again = c.ir_taps(0), c.ir_taps(1), c.ir_taps(2)
    assert not np.array_equal(a, b)
    _check_taps(b, ir_synth_np.frames(**dict(p, seed=p["seed"] ^ (1 << 40))).astype(np.float64))
    np.testing.assert_array_equal(a, again)
    np.testing.assert_array_equal(c.ir_spectra(0), c.ir_spectra(2))
    assert c.ir_info(0) == c.ir_info(2) and c.ir_shape_info(0) == c.ir_shape_info(2)
    c.close()


CHAIN_DAMP = ((250, 2000, 8000), (20000, 0, 6000, 2500), 700)


@pytest.mark.parametrize("rate", [44100, 48000])
def test_the_chain_of_shape_damping_and_eq(gpu_lib, rate):
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    xovers, decay, origin = CHAIN_DAMP
    n_ref = 65536
    frames = ir_synth_np.frames(**FULL)
    assert_onset_margin(frames, 0, COMBINED_A["trim_db"])
    want, winfo, wdinfo = ir_damp_np.damped(frames, n_ref - 1024, None, rate, xovers, decay, origin, CASCADE8, **COMBINED_A)
    assert winfo["frames"] == FULL["frames"] and winfo["eq_bands"] == 8
    c = _conv(n_ref, rate, max_batch=8)
    c.prepare_synth(0, _isynth(FULL), shape=IrShape(**COMBINED_A), eq=IrEq(bands=list(CASCADE8)), damp=IrDamp(xovers=xovers, decay=decay, origin=origin))
    got = c.ir_taps(0)
    _check_taps(got, want.astype(np.float64))
    _check_eq_info(c.ir_shape_info(0), winfo)
    assert c.ir_damp_info(0) == wdinfo
    _check_sums_and_spectra(c, 0, got, want)
    c.close()


DECAY_SYNTH = dict(frames=12000, seed=2, t60=4000, late_start=120, late_gain=0.3, direct=1.0, n_early=8, early_first=20, early_last=110, early_gain=0.5,
                   build_up=400, width=1.0)
DECAY_DAMP = dict(rate=8000, xovers=(400, 1600), decay=(0, 4800, 1600), origin=120, bands=(125, 800, 3200))


def test_the_measured_decay_of_a_synthesised_damped_ir(gpu_lib):
    from cuda_audio_amd.engine import IrDamp

    d = DECAY_DAMP
    frames = ir_synth_np.frames(**DECAY_SYNTH)
    restated = ir_damp_np.damped(frames, 16384 - 1024, None, d["rate"], d["xovers"], d["decay"], d["origin"])[0]
    want = ir_decay_np.decay(restated, d["rate"], bands=d["bands"])
    ir_decay_np.assert_margins(want)
    c = _conv(16384, d["rate"], max_batch=8)
    c.prepare_synth(0, _isynth(DECAY_SYNTH), damp=IrDamp(xovers=d["xovers"], decay=d["decay"], origin=d["origin"]))
    _check_taps(c.ir_taps(0), restated.astype(np.float64))
    got = c.ir_decay(0, bands=d["bands"])
    c.close()
    for b, hz in enumerate(d["bands"], start=1):
        print(f"{hz} Hz: T30 {got['rows'][(b, 'LR')]['t30']:.4f} s on the device, {want['rows'][(b, 'LR')]['t30']:.4f} s restated")
    ir_decay_np.check_against(got, want)
    assert got["rows"][(3, "LR")]["t30"] < got["rows"][(1, "LR")]["t30"]


# -- the engine plays the synthesised IRs -----------------------------------------------------------------------------------
SESSION = 48000
IR_A = dict(synth=dict(frames=7000, seed=11, late_start=400, t60=5000, build_up=600, late_gain=0.05, direct=1.0, n_early=10, early_first=30,
                       early_last=390, early_gain=0.5, width=0.7),
            bands=(("lowcut", 120), ("peak", 2500, 6.0, 1.5)), damp=((400, 1600), (0, 4800, 1600), 37), fields=dict(fade_out=512, normalize="energy", target=0.25))
IR_B = dict(synth=dict(frames=9000, seed=(9 << 32) | 22, late_start=0, t60=6000, late_gain=0.1, width=1.0),
            bands=(), damp=None, fields=dict(start=100, length=5000, normalize="peak", target=0.02))


@functools.lru_cache(maxsize=None)
def _pair(n_ref=16384, nframes=1024):
    """The two synthesised IRs and their restated taps (computed once)."""
    taps = []
    for s in (IR_A, IR_B):
        frames = ir_synth_np.frames(**s["synth"])
        if s["damp"] or s["bands"]:
            t = ir_damp_np.damped(frames, n_ref - nframes, None, SESSION, *(s["damp"] or ((), (), 0)), s["bands"], **s["fields"])[0]
        else:
            t = shape(frames, n_ref - nframes, None, SESSION, **s["fields"])[0]
        t.setflags(write=False)
        taps.append(t)
    return (IR_A, IR_B), taps


def _prepare_pair(c, irs):
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    for i, s in enumerate(irs):
        damp = IrDamp(xovers=s["damp"][0], decay=s["damp"][1], origin=s["damp"][2]) if s["damp"] else None
        c.prepare_synth(i, _isynth(s["synth"]), shape=IrShape(**s["fields"]), eq=IrEq(bands=list(s["bands"])) if s["bands"] else None, damp=damp)


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
    for i, t in enumerate(taps):
        _check_taps(c.ir_taps(i), t.astype(np.float64))
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period]))
                          for k in range(ncalls)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_overlap_save_batch(oracle_mod, gpu_lib):
    """A settled batch of 12288 blocks takes the overlap-save form (os_stats) with the synthesised IRs."""
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


def test_single_transform_form(oracle_mod, gpu_lib):
    """form = 1 builds its spectrum from the synthesised, shaped taps left on the device (it keeps none)."""
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
    for i, s in enumerate(irs):
        info = c.ir_info(i)
        assert info["taps"] == len(taps[i]) and c.ir_shape_info(i)["frames"] == s["synth"]["frames"]
        np.testing.assert_allclose(info["sigma"], taps[i].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
        assert c.ir_synth_info(i)["frames"] == s["synth"]["frames"]
    with pytest.raises(McError) as ex:
        c.ir_taps(0)
    assert ex.value.code == -3
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape
    from cuda_audio_amd.synth import make_ir

    good = dict(FULL, frames=5000, late_start=100, early_first=10, early_last=90)
    c = _conv(16384, 48000, max_batch=8)
    c.prepare_synth(0, _isynth(good), shape=IrShape(fade_out=100, normalize="peak", target=0.02), eq=IrEq(bands=[("lowcut", 120)]))
    taps, spec, info, sinfo, yinfo = c.ir_taps(0), c.ir_spectra(0), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0)
    assert sinfo["frames"] == 5000 and sinfo["eq_bands"] == 1
    bad = [dict(frames=0), dict(frames=(1 << 24) + 1), dict(n_early=65), dict(build_up=65536), dict(late_gain=-1.0), dict(direct=float("nan")),
           dict(early_gain=float("inf")), dict(width=1.01), dict(rate=100), dict(early_first=200, early_last=100), dict(early_last=1 << 24)]
    other = dict(good, seed=1)
    for change in bad:
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(other, **change)))
            assert ex.value.code == -1
    for kw in (dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=5000)), dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])),
               dict(damp=IrDamp(xovers=(1600, 400), decay=(0, 1, 2))), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(other), **kw)
            assert ex.value.code == -1
    nosr = _conv(16384, None, max_batch=8)  # (an engine without a session rate: EQ and damping need one, synthesis alone does not)
    with pytest.raises(McError) as ex:
        nosr.prepare_synth(0, _isynth(other), eq=IrEq(bands=[("lowcut", 120)]))
    assert ex.value.code == -1 and nosr.num_irs() == 0
    nosr.prepare_synth(0, _isynth(other))
    assert nosr.num_irs() == 1
    nosr.close()
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    np.testing.assert_array_equal(c.ir_spectra(0), spec)
    assert c.ir_info(0) == info and c.ir_shape_info(0) == sinfo and c.ir_synth_info(0) == yinfo
    assert c.num_irs() == 1
    # a WAV load over a synthesised index forgets the synthesis
    c.prepare(0, make_ir(3000, seed=2, norm=0.05))
    with pytest.raises(McError) as ex:
        c.ir_synth_info(0)
    assert ex.value.code == -3
    c.close()
