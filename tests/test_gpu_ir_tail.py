"""The tail step of an IR load on the device (mc_load_ir_tail, mc_load_ir_sweep_tail, csrc/irtail.hip.h): the stored taps against
the float64 restatement (tests/ir_tail_np.py, sequential recurrences) applied to the same frames, the parts of the definition
that are exact (frames before the first touched one, knees past the end, repeated loads, a tail that is off), the chain from
ir_floor through tail_from_floor to the engine's output against the oracle fed the restated taps, and the refusals.

The tolerance is test_gpu_ir_damp.py's (test_gpu_ir_shape._check_taps: 1e-6 relative RMS, 1e-5 of the peak), on its grounds: the
same chunked recurrence, which differs from the sequential one by 2e-9 relative RMS at worst, in double, plus one rounding to
float32 (2.5e-8); the noise adds device log, cos, sin and exp2 a few ulp of a double from numpy's."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_floor_np
import ir_tail_np
from helpers import BASE, RMS_TOL, apply_params, rms
from test_gpu_ir_shape import _check_taps

pytestmark = pytest.mark.gpu

RATE = 8000
XOVERS = {0: (), 1: (1000,), 3: (250, 1000, 3000)}


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irtail", n_ref, sample_rate=rate, **kw)


def _itail(mode, spec):
    from cuda_audio_amd.engine import IrTail

    return IrTail(mode=mode, **spec)


@functools.lru_cache(maxsize=None)
def _ir(n):
    """n frames: 37 of silence, then noise that decays by 60 dB over the rest, on a floor 45 dB down."""
    ir = ir_floor_np.noisy_ir(n - 37, 37, RATE, t60=(n - 37) / RATE, floor_db=-45.0, seed=3 + n % 5, noise_seed=17 + n % 3)
    ir.setflags(write=False)
    return ir


def _spec(X, n, fade=32, length=0, seed=12345, width=0.75):
    """Knees a little apart around the middle of n frames, a decay and two levels per band."""
    bands = X + 1
    return dict(xovers=XOVERS[X], knee=tuple(n // 2 + 7 * j for j in range(bands)), t60=tuple(max(n // 2 - 11 * j, 1) for j in range(bands)),
                level_db=tuple((-42.0 - 3.0 * j, -44.5 + 2.0 * j) for j in range(bands)), fade=fade, length=length, seed=seed, width=width)


def _load_and_check(c, idx, ir, mode, spec):
    want, winfo = ir_tail_np.tail64(ir, RATE, mode, **spec)
    c.prepare(idx, ir, tail=_itail(mode, spec))
    got = c.ir_taps(idx)
    assert c.ir_tail_info(idx) == winfo, (c.ir_tail_info(idx), winfo)
    sinfo = c.ir_shape_info(idx)
    assert sinfo["frames"] == winfo["length"] and sinfo["taps"] == len(got) == winfo["length"] and sinfo["gain"] == 1.0
    _check_taps(got, want)
    first = winfo["first"]
    np.testing.assert_array_equal(got[:first], ir[:first])  # (frames before the first touched one: the input's)
    return got, want, winfo


# 255 .. 257: one chunk of irtail.hip.h and a frame either side; 16385: one workgroup's span of the chunk passes and a frame; 40000:
# three workgroups and 157 chunks, more than the 128 runs of the carry pass
@pytest.mark.parametrize("n", [255, 256, 257, 16385, 40000])
@pytest.mark.parametrize("X", [0, 1, 3])
@pytest.mark.parametrize("mode", ["extend", "cut"])
def test_stored_taps_match_the_restatement(gpu_lib, mode, X, n):
    c = _conv(65536 if n > 15000 else 16384)
    got, want, winfo = _load_and_check(c, 0, _ir(n), mode, _spec(X, n))
    c.close()
    assert winfo == dict(bands=X + 1, frames=n, length=n, first=n // 2 - 32)
    assert not np.array_equal(got[winfo["first"]:], _ir(n)[winfo["first"]:])
    if mode == "cut" and X == 0:
        assert not got[n // 2:].any()


def test_the_extension_runs_past_the_recording(gpu_lib):
    """length > F: the frames past the recording read as zero and the noise carries on alone; length < F cuts."""
    n = 3000
    c = _conv(16384)
    for idx, (length, X) in enumerate([(6000, 3), (6000, 0), (2000, 1)]):
        spec = _spec(X, n, length=length)
        if length < n:
            spec["knee"] = (900, 1200)
        got, want, winfo = _load_and_check(c, idx, _ir(n), "extend", spec)
        assert winfo["frames"] == n and winfo["length"] == length and len(got) == length
        if length > n:
            assert np.count_nonzero(got[n:]) > 2 * (length - n) - 10
    c.close()


def test_a_fade_longer_than_the_knee_is_clamped(gpu_lib):
    """A knee in mid-chunk (300) with fade = 1000: W = 300 and the fade starts at frame 0."""
    n = 4000
    c = _conv(16384)
    for idx, mode in enumerate(("extend", "cut")):
        spec = dict(_spec(1, n, fade=1000), knee=(300, 1500))
        _, _, winfo = _load_and_check(c, idx, _ir(n), mode, spec)
        assert winfo == dict(bands=2, frames=n, length=n, first=0)
    c.close()


def test_knees_past_the_end_leave_the_ir_alone(gpu_lib):
    n = 4000
    ir = _ir(n)
    c = _conv(16384)
    c.prepare(0, ir)
    plain = c.ir_taps(0)
    for idx, knee in enumerate([(n, n + 5, 1 << 40, None), (None,) * 4], start=1):
        c.prepare(idx, ir, tail=_itail("extend", dict(_spec(3, n), knee=knee)))
        assert c.ir_tail_info(idx) == dict(bands=0, frames=n, length=n, first=n)
        np.testing.assert_array_equal(c.ir_taps(idx), plain)
    np.testing.assert_array_equal(plain, ir)
    # one band touched, the others alone: only that band changes, and only from its fade on
    spec = dict(_spec(3, n), knee=(None, None, 2000, None))
    _, _, winfo = _load_and_check(c, 3, ir, "extend", spec)
    assert winfo == dict(bands=1, frames=n, length=n, first=2000 - 32)
    c.close()


def test_the_same_load_stores_the_same_bits_and_the_seed_matters(gpu_lib):
    n = 20000
    c = _conv(65536)
    spec = _spec(3, n)
    for idx, s in enumerate((spec, spec, dict(spec, seed=spec["seed"] + 1))):
        c.prepare(idx, _ir(n), tail=_itail("extend", s))
    a, b, other = c.ir_taps(0), c.ir_taps(1), c.ir_taps(2)
    c.close()
    assert a.tobytes() == b.tobytes()
    first = n // 2 - 32
    assert np.array_equal(a[:first], other[:first]) and not np.array_equal(a[first:], other[first:])


def _off_tail():
    """MC_TAIL_OFF with nonsense in every other field."""
    from cuda_audio_amd import _lib

    t = _lib.McIrTail()
    t.struct_size, t.mode, t.n_xovers, t.width, t.length = 7, _lib.MC_TAIL_OFF, 9, 5.0, 1 << 60
    t.xover_hz[0] = float("nan")
    return t


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_a_tail_that_is_off_is_the_wrapped_load_bit_for_bit(gpu_lib, precision):
    """tail = None (Python and C) and MC_TAIL_OFF against prepare() and prepare_sweep() without one."""
    from cuda_audio_amd.engine import IrDamp, IrShape, IrTail, _fp
    from cuda_audio_amd.synth import make_input
    from test_gpu_ir_sweep import _recorded, _sw

    ir = np.ascontiguousarray(_ir(5000))
    x = make_input(32 * 256)
    fields, rec = _recorded("A")
    rec = np.ascontiguousarray(rec)
    shape, damp = IrShape(fade_out=100, normalize="peak", target=0.05), IrDamp(xovers=(400, 1600), decay=(0, 4800, 1600), origin=37)
    outs = []
    for how in ("without", "none", "off", "c_null", "c_off"):
        c = _conv(16384, 48000, max_batch=32, precision=precision)
        L, off = c._L, _off_tail()
        if how in ("without", "none", "off"):
            kw = {} if how == "without" else dict(tail=None if how == "none" else IrTail(mode="off"))
            c.prepare(0, ir, ir_rate=44100, shape=shape, damp=damp, **kw)
            c.prepare(1, ir, **kw)
            c.prepare_sweep(2, rec, _sw(fields), offset=-64, ir_frames=1024, shape=shape, **kw)
        else:
            t = None if how == "c_null" else C.byref(off)
            s, d, sw = shape.to_c(), damp.to_c(), _sw(fields).to_c()
            sw.rate = 48000
            assert L.mc_load_ir_tail(c._h, 0, _fp(ir), len(ir), 1024, 44100, 48000, C.byref(s), None, C.byref(d), t) == 0
            assert L.mc_load_ir_tail(c._h, 1, _fp(ir), len(ir), 1024, 0, 0, None, None, None, t) == 0
            assert L.mc_load_ir_sweep_tail(c._h, 2, _fp(rec), len(rec), 1024, C.byref(sw), -64, 1024, C.byref(s), None, None, t) == 0
        c.cc[1].value.select = 2
        from cuda_audio_amd._lib import McError
        for idx in range(3):
            with pytest.raises(McError) as ex:
                c.ir_tail_info(idx)
            assert ex.value.code == -3
        outs.append([c.ir_taps(i) for i in range(3)] + [c.ir_spectra(i) for i in range(3)] + [c.ir_info(i) for i in range(3)] + [c.process(x[0], x[1])])
        c.close()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            if isinstance(a, dict):
                assert a == b
            else:
                assert a.tobytes() == b.tobytes()


def test_a_sweep_capture_with_a_tail(gpu_lib):
    """prepare_sweep(tail=): the step acts on the deconvolved frames, which the plain capture stores."""
    from test_gpu_ir_sweep import _recorded, _sw

    fields, rec = _recorded("A")
    F = 1024
    c = _conv(16384, 48000)
    c.prepare_sweep(0, rec, _sw(fields), offset=-64, ir_frames=F)
    frames = c.ir_taps(0)
    spec = dict(xovers=(500, 4000), knee=(700, 650, 600), t60=(3000, 2000, 1000), level_db=((-60.0, -61.0), (-62.0, -60.5), (-66.0, -64.0)), fade=48,
                length=2048, seed=99, width=1.0)
    want, winfo = ir_tail_np.tail64(frames, 48000, "extend", **spec)
    c.prepare_sweep(1, rec, _sw(fields), offset=-64, ir_frames=F, tail=_itail("extend", spec))
    got = c.ir_taps(1)
    assert c.ir_tail_info(1) == winfo == dict(bands=3, frames=F, length=2048, first=552)
    assert c.ir_sweep_info(1)["frames"] == F and c.ir_shape_info(1)["frames"] == 2048
    c.close()
    _check_taps(got, want)
    np.testing.assert_array_equal(got[:552], frames[:552])


def test_floor_to_tail_to_output(oracle_mod, gpu_lib):
    """prepare, ir_floor, tail_from_floor, prepare(tail=): the floor is gone (peak to noise at least 20 dB up), the stored taps are
    the restatement's, and 8 periods and one batch match the oracle fed the restated taps."""
    from cuda_audio_amd.engine import IrShape, tail_from_floor
    from cuda_audio_amd.synth import make_input

    n_ref, n = 16384, 6000
    ir = ir_floor_np.noisy_ir(n, 37, RATE, 0.25, floor_db=-50.0) * np.float32(0.02)
    c = _conv(n_ref, max_batch=32)
    c.prepare(0, ir)
    before = c.ir_floor(0, xovers=(400, 1600))
    tail = tail_from_floor(before, mode="extend", fade=64, length=n, seed=7)
    assert all(k is not None and 1500 < k < 2100 for k in tail.knee), tail
    shape = IrShape(fade_out=200)
    c.prepare(0, ir, shape=shape, tail=tail)
    c.prepare(1, ir)
    after = c.ir_floor(0)
    print("peak to noise before", before["rows"][(0, "LR")]["peak_to_noise_db"], "after", after["rows"][(0, "LR")]["peak_to_noise_db"])
    assert after["rows"][(0, "LR")]["peak_to_noise_db"] >= before["rows"][(0, "LR")]["peak_to_noise_db"] + 20.0
    spec = dict(xovers=tail.xovers, knee=tail.knee, t60=tail.t60, level_db=tail.level_db, fade=64, length=n, seed=7, width=1.0)
    y, winfo = ir_tail_np.tail64(ir, RATE, "extend", **spec)
    assert c.ir_tail_info(0) == winfo
    fade = np.ones(n)
    fade[n - 200:] = (1.0 + np.cos(np.pi * (np.arange(200) + 1.0) / 201.0)) / 2.0
    restated = (y.astype(np.float32).astype(np.float64) * fade[:, None])
    _check_taps(c.ir_taps(0), restated)
    taps = [restated.astype(np.float32), ir[:n_ref - 1024]]
    p1 = dict(BASE, select=1, level=0.8)
    x = make_input(40 * 256)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, BASE, p1, True)
    want = ref.process(x[0], x[1])
    assert rms(want) > 0.01
    apply_params(c, BASE, p1, False)
    got = [np.stack(c.onProcess(x[0, k * 256:(k + 1) * 256], x[1, k * 256:(k + 1) * 256])) for k in range(8)]
    got.append(c.process(x[0, 8 * 256:], x[1, 8 * 256:]))
    c.close()
    assert rms(np.concatenate(got, axis=1) - want) <= RMS_TOL


def test_the_single_transform_form_takes_a_tail(gpu_lib):
    """It keeps no taps (ir_floor: MC_ERR_STATE), but a tail load works there: the same output as the partitioned engine's."""
    from cuda_audio_amd.synth import make_input

    n = 6000
    ir = _ir(n) * np.float32(0.02)
    x = make_input(16 * 256)
    spec = _spec(3, n)
    outs = []
    for form in ("partitioned", "single"):
        c = _conv(16384, form=form)
        c.prepare(0, ir, tail=_itail("extend", spec))
        assert c.ir_tail_info(0) == dict(bands=4, frames=n, length=n, first=n // 2 - 32) and c.ir_shape_info(0)["frames"] == n
        outs.append(np.concatenate([np.stack(c.onProcess(x[0, k * 256:(k + 1) * 256], x[1, k * 256:(k + 1) * 256])) for k in range(16)], axis=1))
        c.close()
    assert rms(outs[0]) > 0.005 and rms(outs[0] - outs[1]) <= RMS_TOL


def _raw_tail(**fields):
    from cuda_audio_amd import _lib

    t = _lib.McIrTail()
    _lib.load().mc_default_ir_tail(C.byref(t))
    t.mode = _lib.MC_TAIL_EXTEND
    t.knee[0] = 1000
    for k, v in fields.items():
        if k in ("xover_hz", "knee", "t60"):
            for i, e in enumerate(v):
                getattr(t, k)[i] = e
        elif k == "level_db":
            for i, (a, b) in enumerate(v):
                t.level_db[i][0], t.level_db[i][1] = a, b
        else:
            setattr(t, k, v)
    return t


BAD_TAILS = [("struct_size", dict(struct_size=140)), ("mode", dict(mode=3)), ("n_xovers", dict(n_xovers=4)), ("xover_hz[0]", dict(n_xovers=1, xover_hz=(9.0,))),
             ("xover_hz[0]", dict(n_xovers=1, xover_hz=(float("inf"),))), ("xover_hz[1]", dict(n_xovers=2, xover_hz=(400.0, 0.46 * RATE))),
             ("xover_hz[1]", dict(n_xovers=2, xover_hz=(400.0, 300.0))), ("width", dict(width=1.5)), ("width", dict(width=float("nan"))),
             ("length", dict(length=(1 << 24) + 1)), ("t60[0]", dict(t60=(0,))), ("t60[1]", dict(n_xovers=1, t60=(5, 0))),
             ("level_db[0][1]", dict(level_db=((0.0, float("inf")),))), ("level_db[1][0]", dict(n_xovers=1, level_db=((0.0, 0.0), (float("nan"), 0.0))))]


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, IrShape, Sweep, _fp

    ir = np.ascontiguousarray(_ir(3000))
    c = _conv(16384)
    good = _itail("extend", _spec(1, 3000))
    c.prepare(0, ir, shape=IrShape(fade_out=100), tail=good)
    taps, spec, info, sinfo, tinfo = c.ir_taps(0), c.ir_spectra(0), c.ir_info(0), c.ir_shape_info(0), c.ir_tail_info(0)
    L = c._L
    rec = np.zeros((5000, 2), np.float32)
    sw = Sweep(frames=4096, f1_hz=20.0, f2_hz=3000.0, rate=RATE).to_c()
    for name, fields in BAD_TAILS:
        t = _raw_tail(**fields)
        for idx in (0, 1):
            for rates in ((RATE, RATE), (0, 0)):  # (the tail comes before the rates)
                assert L.mc_load_ir_tail(c._h, idx, _fp(ir), len(ir), 1024, *rates, None, None, None, C.byref(t)) == -1
                msg = L.mc_last_error().decode()
                # (without a session rate a crossover has no upper bound to miss: the rates are refused in its place)
                assert name in msg or (rates == (0, 0) and 0.46 * RATE in fields.get("xover_hz", ()) and "session_rate" in msg), (name, msg)
            assert L.mc_load_ir_sweep_tail(c._h, idx, _fp(rec), len(rec), 1024, C.byref(sw), 0, 900, None, None, None, C.byref(t)) == -1
            assert name in L.mc_last_error().decode(), (name, L.mc_last_error())
    ok = _raw_tail()
    for rates, name in (((0, 0), "session_rate"), ((RATE, 0), "session_rate"), ((7999, RATE), "ir_rate"), ((RATE, 384001), "session_rate")):
        assert L.mc_load_ir_tail(c._h, 1, _fp(ir), len(ir), 1024, *rates, None, None, None, C.byref(ok)) == -1
        assert name in L.mc_last_error().decode(), (rates, L.mc_last_error())
    other = np.ascontiguousarray(_ir(4000))
    for kw in (dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=5000)), dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(ir_rate=7999), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, other, tail=good, **kw)
            assert ex.value.code == -1
    nosr = _conv(16384, None)  # (an engine without a session rate: 0 / 0 with a tail on)
    with pytest.raises(McError) as ex:
        nosr.prepare(0, other, tail=good)
    assert ex.value.code == -1 and nosr.num_irs() == 0
    nosr.close()
    with pytest.raises(McError) as ex:
        c.ir_tail_info(1)
    assert ex.value.code == -1
    np.testing.assert_array_equal(c.ir_taps(0), taps)
    np.testing.assert_array_equal(c.ir_spectra(0), spec)
    assert c.ir_info(0) == info and c.ir_shape_info(0) == sinfo and c.ir_tail_info(0) == tinfo and c.num_irs() == 1
    c.close()
