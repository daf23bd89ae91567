"""Damping of an IR on load on the device (mc_load_ir_damped, csrc/irdamp.hip.h): the stored taps, the shape and damping
information and the spectra against the float64 restatement (tests/ir_damp_np.py, sequential recurrences), the properties the
header states (equal decays are the broadband envelope, no decay and a late origin change nothing, damping off is mc_load_ir_eq),
the decay the damped taps then measure, and the engine's paths against the oracle fed the restated taps.  The tolerances are
those of test_gpu_ir_eq.py: device double arithmetic rounded to float32 (the chunked recurrence differs from the sequential one
by 2e-9 relative RMS at worst; the float rounding of a stored tap is 2.5e-8)."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_decay_np
from helpers import BASE, RMS_TOL, _dry, apply_params, rms
from ir_shape_np import assert_onset_margin, quiet_lead_ir, session_frames, shape64
from test_gpu_ir_eq import CASCADE8, _check_eq_info, _check_sums_and_spectra
from test_gpu_ir_shape import COMBINED_A, FP16_REL_TOL, OS_P, P0, P1, _check_level, _check_taps, _os_want, _settled_batches

pytestmark = pytest.mark.gpu

# (crossovers, decays low to high, origin) for X = 1, 2, 3
DAMPS = {
    1: ((1000,), (0, 6000), 300),
    2: ((400, 1600), (0, 4800, 1600), 37),
    3: ((250, 2000, 8000), (20000, 0, 6000, 2500), 700),
}
RATES = [(44100, 44100), (44100, 48000)]
LENGTH_DAMP = ((250, 2000, 8000), (20000, 9000, 6000, 2500))


def _conv(n_ref, rate, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    return Convolution("irdamp", n_ref, sample_rate=rate, **kw)


def _idamp(xovers, decay, origin=0):
    from cuda_audio_amd.engine import IrDamp

    return IrDamp(xovers=tuple(xovers), decay=tuple(decay), origin=origin)


def _ieq(bands):
    from cuda_audio_amd.engine import IrEq

    return IrEq(bands=list(bands)) if bands else None


def _ishape(fields):
    from cuda_audio_amd.engine import IrShape

    return IrShape(**fields) if fields else None


def _margin(ir, src, dst, fields):
    if fields and fields.get("trim_db", 0) < 0:
        assert_onset_margin(session_frames(ir, src, dst), fields.get("start", 0), fields["trim_db"])


def _check_all(c, idx, want, winfo, wdinfo):
    got = c.ir_taps(idx)
    _check_taps(got, want.astype(np.float64))
    _check_eq_info(c.ir_shape_info(idx), winfo)
    assert c.ir_damp_info(idx) == wdinfo
    _check_sums_and_spectra(c, idx, got, want)
    return got


@pytest.mark.parametrize("src,dst", RATES)
@pytest.mark.parametrize("X", [1, 2, 3])
def test_damping_alone_matches_the_restatement(gpu_lib, X, src, dst):
    xovers, decay, origin = DAMPS[X]
    n_ref = 65536
    ir = quiet_lead_ir()
    want, winfo, wdinfo = ir_damp_np.damped(ir, n_ref - 1024, src, dst, xovers, decay, origin)
    assert wdinfo["xovers"] == X and winfo["eq_bands"] == 0
    c = _conv(n_ref, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src, damp=_idamp(xovers, decay, origin))
    _check_all(c, 0, want, winfo, wdinfo)
    c.close()


@pytest.mark.parametrize("src,dst", RATES)
@pytest.mark.parametrize("X", [1, 2, 3])
def test_the_order_is_fade_damping_eq_normalisation(gpu_lib, X, src, dst):
    """Damping under COMBINED_A (trim, reverse, decay, fade, energy target) and the 8-band cascade.  The restatement with 6a and 6b
    swapped differs from the device by far more than the tolerance, which is asserted before the right order is compared."""
    xovers, decay, origin = DAMPS[X]
    n_ref = 65536
    ir = quiet_lead_ir()
    _margin(ir, src, dst, COMBINED_A)
    want, winfo, wdinfo = ir_damp_np.damped(ir, n_ref - 1024, src, dst, xovers, decay, origin, CASCADE8, **COMBINED_A)
    swapped = ir_damp_np.damp64(ir, n_ref - 1024, src, dst, xovers, decay, origin, CASCADE8, eq_first=True, **COMBINED_A)[0]
    assert winfo["eq_bands"] == 8
    c = _conv(n_ref, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src, shape=_ishape(COMBINED_A), eq=_ieq(CASCADE8), damp=_idamp(xovers, decay, origin))
    got = c.ir_taps(0)
    far = rms(got.astype(np.float64) - swapped) / rms(swapped)
    print(f"EQ before damping would differ by {far:.2e} relative RMS")
    assert far >= 100 * 1e-6
    _check_all(c, 0, want, winfo, wdinfo)
    c.close()


@functools.lru_cache(maxsize=None)
def _length_ir():
    return quiet_lead_ir(45000, seed=5)


# 1 .. 5: around the cascade's order of four; 255 .. 257: one chunk of irdamp.hip.h and a tap either side; 4095 .. 4097: sixteen
# chunks; 16383 .. 16385: one workgroup's span of the chunk passes; 32768 / 32769: one chunk per run of the carry pass and two;
# 40000: three workgroups, two chunks per run
LENGTHS_16K = [1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097]
LENGTHS_64K = [16383, 16384, 16385, 32768, 32769, 40000]


@pytest.mark.parametrize("n_ref,length", [(16384, n) for n in LENGTHS_16K] + [(65536, n) for n in LENGTHS_64K])
def test_lengths(gpu_lib, n_ref, length):
    xovers, decay = LENGTH_DAMP
    ir = _length_ir()
    fields = dict(start=700, length=length)
    want, winfo, wdinfo = ir_damp_np.damped(ir, n_ref - 1024, None, 48000, xovers, decay, 100, **fields)
    assert winfo["taps"] == length and wdinfo == dict(xovers=3, origin=min(100, length), damped_bands=4)
    c = _conv(n_ref, 48000, max_batch=8)
    c.prepare(0, ir, shape=_ishape(fields), damp=_idamp(xovers, decay, 100))
    _check_all(c, 0, want, winfo, wdinfo)
    c.close()


ORIGIN_N = 40000
ORIGIN_FIELDS = dict(start=700, length=ORIGIN_N)


@functools.lru_cache(maxsize=None)
def _origin_parts():
    """The 40000 selected taps as double and their three low-passes, computed once for every origin."""
    x = shape64(_length_ir(), 65536 - 1024, None, 48000, **ORIGIN_FIELDS)[0]
    P = ir_damp_np.lowpasses(x, LENGTH_DAMP[0], 48000)
    for a in [x] + P:
        a.setflags(write=False)
    return x, P


# 0; a chunk edge; a workgroup edge; the last tap; n and past n, which leave nothing to damp
@pytest.mark.parametrize("origin", [0, 255, 256, 257, 16384, ORIGIN_N - 1, ORIGIN_N, ORIGIN_N + 5])
def test_origins(gpu_lib, origin):
    xovers, decay = LENGTH_DAMP
    x, P = _origin_parts()
    want = ir_damp_np.combine(x, P, decay, origin)
    c = _conv(65536, 48000, max_batch=8)
    c.prepare(0, _length_ir(), shape=_ishape(ORIGIN_FIELDS), damp=_idamp(xovers, decay, origin))
    got = c.ir_taps(0)
    assert c.ir_damp_info(0) == dict(xovers=3, origin=min(origin, ORIGIN_N), damped_bands=4)
    _check_taps(got, want)
    if origin >= ORIGIN_N:
        c.prepare(1, _length_ir(), shape=_ishape(ORIGIN_FIELDS))
        assert np.array_equal(got, c.ir_taps(1))
    else:
        assert np.array_equal(got[:origin + 1], x[:origin + 1].astype(np.float32))  # (t = 0 up to and at the origin)
        if origin < ORIGIN_N - 1:
            assert not np.array_equal(got[origin + 1:], x[origin + 1:].astype(np.float32))
    c.close()


def test_equal_decays_are_the_broadband_envelope(gpu_lib):
    from cuda_audio_amd.engine import IrShape

    ir = quiet_lead_ir(30000, seed=9)
    d = 9000
    c = _conv(65536, 48000, max_batch=8)
    c.prepare(0, ir, damp=_idamp((250, 2000, 8000), (d,) * 4, 0))
    c.prepare(1, ir, shape=IrShape(decay_t60=d))
    got, plain = c.ir_taps(0), c.ir_taps(1)
    assert c.ir_damp_info(0) == dict(xovers=3, origin=0, damped_bands=4)
    c.close()
    _check_taps(got, plain.astype(np.float64))


def test_no_decay_changes_nothing(gpu_lib):
    ir = quiet_lead_ir(30000, seed=9)
    c = _conv(65536, 48000, max_batch=8)
    c.prepare(0, ir, damp=_idamp((250, 2000, 8000), (0, 0, 0, 0), 5))
    c.prepare(1, ir)
    assert c.ir_damp_info(0) == dict(xovers=3, origin=5, damped_bands=0)
    assert np.array_equal(c.ir_taps(0), c.ir_taps(1))
    assert np.array_equal(c.ir_taps(0), ir[:len(c.ir_taps(0))])
    c.close()


def test_damping_off_is_mc_load_ir_eq_bit_for_bit(gpu_lib):
    """n_xovers = 0 with nonsense in every other field against mc_load_ir_eq: plain, resampled, shaped and equalised loads."""
    from cuda_audio_amd._lib import McError, McIrDamp, McIrEq
    from cuda_audio_amd.engine import IrEq, IrShape, _fp
    from cuda_audio_amd.synth import make_input, make_ir

    ir = make_ir(9000, seed=6, norm=0.05)
    lr = np.ascontiguousarray(ir, np.float32)
    x = make_input(64 * 256)
    on = IrShape(**COMBINED_A).to_c()
    bands = IrEq(bands=[("lowcut", 120), ("peak", 2500, 6.0, 1.5)]).to_c()
    off = McIrEq()
    outs = []
    for kind in ("eq", "damped"):
        c = _conv(16384, 48000, max_batch=32)
        c._L.mc_default_ir_eq(C.byref(off))
        junk = McIrDamp()
        junk.struct_size, junk.n_xovers, junk.reserved, junk.origin = 3, 0, 9, 1 << 60
        junk.xover_hz[0], junk.xover_hz[1], junk.xover_hz[2] = float("nan"), -5.0, 1.0
        junk.decay_t60[0] = junk.decay_t60[3] = 77
        loads = [(0, 0, 0, None, off), (1, 44100, 48000, None, off), (2, 44100, 48000, on, off), (3, 44100, 48000, on, bands)]
        for idx, src, dst, sh, eq in loads:
            args = (c._h, idx, _fp(lr), lr.shape[0], 1024, src, dst, C.byref(sh) if sh is not None else None, C.byref(eq))
            rc = c._L.mc_load_ir_damped(*args, C.byref(junk)) if kind == "damped" else c._L.mc_load_ir_eq(*args)
            assert rc == 0
        if kind == "damped":  # (a null mc_ir_damp and null eq are off too)
            assert c._L.mc_load_ir_damped(c._h, 0, _fp(lr), lr.shape[0], 1024, 0, 0, None, None, None) == 0
        for i in range(4):
            with pytest.raises(McError) as ex:
                c.ir_damp_info(i)
            assert ex.value.code == -3
        for i in (0, 1):
            with pytest.raises(McError) as ex:
                c.ir_shape_info(i)
            assert ex.value.code == -3
        res = [c.ir_taps(i) for i in range(4)] + [c.ir_spectra(i) for i in range(4)] + [c.ir_info(i) for i in range(4)]
        res += [c.ir_shape_info(2), c.ir_shape_info(3)]
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


@pytest.mark.parametrize("src,dst", RATES)
def test_the_same_load_twice_gives_the_same_bits(gpu_lib, src, dst):
    xovers, decay, origin = DAMPS[3]
    ir = quiet_lead_ir()
    _margin(ir, src, dst, COMBINED_A)
    c = _conv(65536, dst, max_batch=8)
    c.prepare(0, ir, ir_rate=src)  # (index 0 is a used one: the first damped load replaces a plain one)
    res = []
    for idx in (0, 1, 0):
        c.prepare(idx, ir, ir_rate=src, shape=_ishape(COMBINED_A), eq=_ieq(CASCADE8), damp=_idamp(xovers, decay, origin))
        res.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_info(idx), c.ir_shape_info(idx), c.ir_damp_info(idx)))
    c.close()
    for r in res[1:]:
        np.testing.assert_array_equal(r[0], res[0][0])
        np.testing.assert_array_equal(r[1], res[0][1])
        assert r[2:] == res[0][2:]


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, IrShape
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(3000, seed=2, norm=0.05)
    c = _conv(16384, 48000, max_batch=8)
    good = _idamp((400, 1600), (0, 4800, 1600), 10)
    c.prepare(0, ir, ir_rate=44100, shape=IrShape(fade_out=100, normalize="peak", target=0.02), eq=IrEq(bands=[("lowcut", 120)]), damp=good)
    taps, spec, info, sinfo, dinfo = c.ir_taps(0), c.ir_spectra(0), c.ir_info(0), c.ir_shape_info(0), c.ir_damp_info(0)
    assert sinfo["eq_bands"] == 1 and dinfo == dict(xovers=2, origin=10, damped_bands=2)
    other = make_ir(5000, seed=3)
    bad = [_idamp((9.0,), (0, 100)), _idamp((0.46 * 48000,), (0, 100)), _idamp((float("nan"),), (0, 100)), _idamp((400, 400), (0, 1, 2)),
           _idamp((1600, 400), (0, 1, 2)), _idamp((400, 1600, 1000), (0, 1, 2, 3))]
    for d in bad:
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, damp=d)
            assert ex.value.code == -1
    for kw in (dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=5000)), dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(ir_rate=7999),
               dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, damp=good, **kw)
            assert ex.value.code == -1
    nosr = _conv(16384, None, max_batch=8)  # (an engine without a session rate: 0 / 0 with damping on)
    with pytest.raises(McError) as ex:
        nosr.prepare(0, other, damp=good)
    assert ex.value.code == -1 and nosr.num_irs() == 0
    nosr.close()
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    np.testing.assert_array_equal(c.ir_spectra(0), spec)
    assert c.ir_info(0) == info and c.ir_shape_info(0) == sinfo and c.ir_damp_info(0) == dinfo
    assert c.num_irs() == 1
    c.close()


def test_the_damped_taps_measure_the_decay_the_restatement_measures(gpu_lib):
    """Closing the loop: the aiming case of test_ir_damp_cpu.py loaded on the device and read back by mc_ir_decay in the three
    octave bands, against ir_decay_np.decay of the restated taps."""
    aim = ir_damp_np.AIM
    ir, restated, _, want = ir_damp_np.aim_case()
    ir_decay_np.assert_margins(want)
    c = _conv(16384, aim["rate"], max_batch=8)
    c.prepare(0, ir, damp=_idamp(aim["xovers"], aim["decay"], aim["origin"]))
    _check_taps(c.ir_taps(0), restated.astype(np.float64))
    got = c.ir_decay(0, bands=aim["bands"])
    c.close()
    for b, hz in enumerate(aim["bands"], start=1):
        print(f"{hz} Hz: T30 {got['rows'][(b, 'LR')]['t30']:.4f} s on the device, {want['rows'][(b, 'LR')]['t30']:.4f} s restated")
    ir_decay_np.check_against(got, want)


# -- the engine plays the damped IRs -------------------------------------------------------------------------------------
SESSION = 48000
IR_A = dict(frames=7000, seed=11, rate=44100, bands=(("lowcut", 120), ("peak", 2500, 6.0, 1.5)), damp=((400, 1600), (0, 4800, 1600), 37),
            fields=dict(trim_db=-20, pre_roll=16, reverse=True, decay_t60=6000, fade_out=512, normalize="energy", target=0.25))
IR_B = dict(frames=9000, seed=22, rate=SESSION, bands=(), damp=((250, 2000, 8000), (0, 9000, 3000, 1500), 200),
            fields=dict(start=100, length=5000, normalize="peak", target=0.02))


@functools.lru_cache(maxsize=None)
def _pair(n_ref=16384, nframes=1024):
    """The two damped IRs, the first of them converted and equalised: [(frames, spec)] and their restated taps (computed once)."""
    irs = [(quiet_lead_ir(s["frames"], seed=s["seed"]), s) for s in (IR_A, IR_B)]
    taps = []
    for ir, s in irs:
        _margin(ir, s["rate"], SESSION, s["fields"])
        t = ir_damp_np.damped(ir, n_ref - nframes, s["rate"], SESSION, *s["damp"], s["bands"], **s["fields"])[0]
        t.setflags(write=False)
        taps.append(t)
    return irs, taps


def _prepare_pair(c, irs):
    for i, (ir, s) in enumerate(irs):
        c.prepare(i, ir, ir_rate=s["rate"], shape=_ishape(s["fields"]), eq=_ieq(s["bands"]), damp=_idamp(*s["damp"]))


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


def test_overlap_save_batch(oracle_mod, gpu_lib):
    """A settled batch of 12288 blocks takes the overlap-save form (os_stats) with the damped IRs."""
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
