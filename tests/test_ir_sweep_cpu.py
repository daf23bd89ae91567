"""Capture of an IR from a recorded sine sweep without a GPU: mc_sweep_generate (host arithmetic) against the float64
restatement (tests/ir_sweep_np.py), where the sweep's frequency ends, what the normalisation of the deconvolution weights
means (the sweep deconvolved with itself is a band-limited unit impulse, whatever the amplitude), and every argument check of
mc_load_ir_sweep through the library with a null engine, in the documented order (they come before the engine is looked at)."""
import ctypes as C

import numpy as np
import pytest

import ir_sweep_np
from cuda_audio_amd import _lib

CASE_A = dict(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=48000, amplitude=0.5, fade_in=64, fade_out=32)
CASE_B = dict(frames=2048, f1_hz=200.0, f2_hz=18000.0, rate=44100, amplitude=0.5, fade_in=0, fade_out=0)


def _sweep(**fields):
    L = _lib.load()
    s = _lib.McSweep()
    L.mc_default_sweep(C.byref(s))
    for k, v in fields.items():
        setattr(s, k, v)
    return L, s


def _generate(fields, first=0, count=None):
    L, s = _sweep(**fields)
    count = s.frames - first if count is None else count
    out = np.full(count, np.nan, np.float32)
    assert L.mc_sweep_generate(C.byref(s), out.ctypes.data_as(C.POINTER(C.c_float)), first, count) == 0, L.mc_last_error()
    return out


def test_struct_size_and_defaults():
    L, s = _sweep()
    assert C.sizeof(_lib.McSweep) == 40 and s.struct_size == 40
    assert _lib.McSweep.frames.offset == 8 and _lib.McSweep.f1_hz.offset == 16 and _lib.McSweep.reserved.offset == 36
    assert (s.rate, s.frames, s.f1_hz, s.f2_hz, s.amplitude, s.fade_in, s.fade_out, s.reserved) == (44100, 0, 20.0, 20000.0, 0.5, 0, 0, 0)
    from cuda_audio_amd.engine import Sweep

    c = Sweep(frames=4096, f1_hz=100.0, f2_hz=15000.0, amplitude=0.25, fade_in=7, fade_out=9, rate=48000).to_c()
    assert (c.struct_size, c.rate, c.frames, c.f1_hz, c.f2_hz, c.amplitude, c.fade_in, c.fade_out, c.reserved) == (40, 48000, 4096, 100.0, 15000.0, 0.25, 7, 9, 0)
    assert Sweep(frames=10).to_c().rate == 44100


@pytest.mark.parametrize("fields", [CASE_A, CASE_B, dict(CASE_A, amplitude=0.25), dict(frames=2, f1_hz=1.0, f2_hz=4000.0, rate=8000, fade_in=1, fade_out=1),
                                    dict(frames=1 << 18, f1_hz=20.0, f2_hz=20000.0, rate=44100, fade_in=1000, fade_out=500),
                                    dict(frames=333, f1_hz=50.0, f2_hz=60.0, rate=384000, fade_in=333, fade_out=0)])
def test_generate_matches_the_restatement(fields):
    """To 2^-23 * amplitude per sample: one float ulp at full scale.  The phase of a double is good to about phi * 2^-52, with
    phi up to some 1e7 rad at N = 2^22, far below that."""
    got = _generate(fields)
    want = ir_sweep_np.sweep(**fields)
    amp = float(np.float32(fields.get("amplitude", 0.5)))
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"max err {err:.3e}, bound {2.0 ** -23 * amp:.3e}, peak {np.abs(want).max():.4f}")
    assert err <= 2.0 ** -23 * amp
    if fields["frames"] >= 2048:
        assert np.abs(want).max() > 0.99 * amp


def test_windows_are_slices_of_the_whole_sweep_bit_for_bit():
    whole = _generate(CASE_A)
    for first, count in ((0, 1), (0, 64), (63, 2), (1000, 1234), (4095, 1), (4064, 32), (4096, 0), (0, 0)):
        np.testing.assert_array_equal(_generate(CASE_A, first, count), whole[first:first + count])
    from cuda_audio_amd.engine import Sweep, sweep_frames

    np.testing.assert_array_equal(sweep_frames(Sweep(**CASE_A)), whole)


def test_a_window_past_the_end_is_refused():
    L, s = _sweep(**CASE_A)
    out = np.zeros(8, np.float32)
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    for first, count in ((4090, 7), (4097, 0), (0, 4097), (2 ** 64 - 1, 2)):
        assert L.mc_sweep_generate(C.byref(s), p, first, count) == -1 and "first" in L.mc_last_error().decode()
    assert L.mc_sweep_generate(C.byref(s), None, 0, 1) == -1 and "null out" in L.mc_last_error().decode()
    assert L.mc_sweep_generate(None, p, 0, 1) == -1 and "null sweep" in L.mc_last_error().decode()
    s.amplitude = 0.0
    assert L.mc_sweep_generate(C.byref(s), p, 0, 1) == -1 and "amplitude" in L.mc_last_error().decode()


@pytest.mark.parametrize("fields", [CASE_A, CASE_B, dict(frames=1 << 16, f1_hz=20.0, f2_hz=20000.0, rate=44100)])
def test_the_instantaneous_frequency_ends_at_f2(fields):
    """phi(N - 1) - phi(N - 2) against 2 pi f2 / rate.  The last step is the frequency's mean over the last interval, which
    in exact arithmetic is 2 pi f2 / rate * Ls (1 - exp(-1 / Ls)): 1 / (2 Ls) = ln(f2 / f1) / (2 (N - 1)) below the end
    value.  That is held to 1e-9 everywhere, and the end value itself to 1e-3 wherever the definition puts it inside that
    (1 / (2 Ls) < 1e-3: case A at 6.5e-4, the 2^16 sweep at 5.3e-5; case B, N 2048 over 6.5 octaves, lies 1.1e-3 below by the
    definition itself and has the first statement alone)."""
    assert fields["frames"] >= 2048
    phi = ir_sweep_np.phase(**fields)
    assert phi[0] == 0.0
    Ls = (fields["frames"] - 1) / np.log(fields["f2_hz"] / fields["f1_hz"])
    step, want = phi[-1] - phi[-2], 2.0 * np.pi * fields["f2_hz"] / fields["rate"]
    print(f"last phase step {step:.6f} rad, 2 pi f2 / rate {want:.6f}, 1 / (2 Ls) {0.5 / Ls:.2e}")
    assert abs(step - want * Ls * -np.expm1(-1.0 / Ls)) <= 1e-9 * want
    if 0.5 / Ls < 1e-3:
        assert abs(step - want) <= 1e-3 * want
    else:
        assert fields is CASE_B
    first = phi[1] - phi[0]
    assert abs(first - 2.0 * np.pi * fields["f1_hz"] / fields["rate"]) <= 1e-2 * first


@pytest.mark.parametrize("amplitude", [0.5, 0.25])
def test_the_normalisation_means_what_the_header_says(amplitude):
    """Case A deconvolved with itself, by the restatement alone: flat within +-0.25 dB of 0 dB between 4 f1 and f2 / 2 over an
    8192-point transform (-0.101 / +0.087 dB), the largest |sample| at frame -offset (0.81), at either amplitude."""
    sw = dict(CASE_A, amplitude=amplitude)
    s = ir_sweep_np.sweep(**sw).astype(np.float32)
    rec = np.zeros((4096 + 1024, 2), np.float32)
    rec[:4096, 0] = rec[:4096, 1] = s
    h = ir_sweep_np.deconvolve(rec, sw, -512, 1024)
    lo, hi = ir_sweep_np.band_db(h[:, 0], sw)
    k = int(np.abs(h[:, 0]).argmax())
    print(f"amplitude {amplitude}: band {lo:+.3f} / {hi:+.3f} dB, peak {h[k, 0]:.4f} at frame {k}")
    assert -0.25 <= lo and hi <= 0.25
    assert k == 512 and 0.7 < h[512, 0] < 0.9
    np.testing.assert_array_equal(h[:, 0], h[:, 1])


# -- arguments ----------------------------------------------------------------------------------------------------------------
GOOD = dict(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=48000)
LOAD = dict(M=5000, offset=0, F=1000)
REFUSALS = [
    (dict(struct_size=36), {}, "struct_size"),
    (dict(rate=7999), {}, "rate"),
    (dict(rate=384001), {}, "rate"),
    (dict(frames=1), {}, "frames"),
    (dict(frames=(1 << 22) + 1), {}, "frames"),
    (dict(f1_hz=0.5), {}, "f1_hz"),
    (dict(f1_hz=float("nan")), {}, "f1_hz"),
    (dict(f2_hz=100.0), {}, "f2_hz"),
    (dict(f2_hz=50.0), {}, "f2_hz"),
    (dict(f2_hz=24000.5), {}, "f2_hz"),
    (dict(f2_hz=float("inf")), {}, "f2_hz"),
    (dict(amplitude=0.0), {}, "amplitude"),
    (dict(amplitude=-0.5), {}, "amplitude"),
    (dict(amplitude=float("nan")), {}, "amplitude"),
    (dict(fade_in=4000, fade_out=97), {}, "fade_in"),
    (dict(fade_in=2 ** 32 - 1, fade_out=2 ** 32 - 1), {}, "fade_in"),
    (dict(reserved=1), {}, "reserved"),
    ({}, dict(M=0), "recording"),
    ({}, dict(M=(1 << 24) + 1), "recording"),
    ({}, dict(F=0), "ir_frames"),
    ({}, dict(F=(1 << 24) + 1), "ir_frames"),
    ({}, dict(offset=-(1 << 24) - 1), "offset"),
    ({}, dict(offset=(1 << 24) + 1), "offset"),
    (dict(frames=1 << 22), dict(F=(1 << 18) + 1), "sweep frames"),
]


def _load(L, s, lr=None, e=None, shape=None, eq=None, damp=None, nframes=1024, **kw):
    a = dict(LOAD, **kw)
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    return L.mc_load_ir_sweep(e, 0, lr, a["M"], nframes, C.byref(s) if s is not None else None, a["offset"], a["F"], ref(shape), ref(eq), ref(damp))


@pytest.mark.parametrize("fields,load,name", REFUSALS)
def test_a_bad_argument_is_refused_before_the_engine_is_looked_at(fields, load, name):
    L, s = _sweep(**dict(GOOD, **fields))
    assert _load(L, s, **load) == -1
    msg = L.mc_last_error().decode()
    assert name in msg and "null" not in msg, msg
    if not load:  # (mc_sweep_generate checks the struct by the same function)
        out = np.zeros(1, np.float32)
        assert L.mc_sweep_generate(C.byref(s), out.ctypes.data_as(C.POINTER(C.c_float)), 0, 1) == -1 and name in L.mc_last_error().decode()


def test_the_edges_of_the_ranges_pass_the_checks():
    """The largest and smallest of everything get as far as the null recording."""
    for fields, load in ((dict(rate=8000, f2_hz=4000.0), {}), (dict(rate=384000, f2_hz=192000.0), {}), (dict(frames=2), {}), (dict(f1_hz=1.0), {}),
                         (dict(fade_in=4000, fade_out=96), {}), ({}, dict(M=1, F=1)), ({}, dict(M=1 << 24, F=1 << 24, offset=1 << 24)),
                         ({}, dict(offset=-(1 << 24))), (dict(frames=1 << 22), dict(F=1 << 18))):
        L, s = _sweep(**dict(GOOD, **fields))
        assert _load(L, s, **load) == -1
        assert "null lr" in L.mc_last_error().decode(), (fields, load, L.mc_last_error())


def test_checks_come_in_the_documented_order():
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    L = _lib.load()
    bad_damp, bad_eq, bad_shape = IrDamp(xovers=(400, 300), decay=(0, 1, 2)).to_c(), IrEq(bands=[("peak", 5.0, 3.0)]).to_c(), IrShape(trim_db=1.0).to_c()
    lr = np.zeros((LOAD["M"], 2), np.float32)
    p = lr.ctypes.data_as(C.POINTER(C.c_float))
    every = dict(shape=bad_shape, eq=bad_eq, damp=bad_damp)
    msg = lambda: L.mc_last_error().decode()  # noqa: E731
    assert _load(L, None, **every) == -1 and "null sweep" in msg()
    # the struct in field order: each field is bad, and the first one named is the first in the struct
    order = [("struct_size", 44), ("rate", 100), ("frames", 0), ("f1_hz", 0.0), ("f2_hz", 1e6), ("amplitude", -1.0), ("fade_in", 2 ** 31), ("reserved", 7)]
    _, s = _sweep(**dict(order))
    for k, _ in order:
        assert _load(L, s, M=0, F=0, offset=1 << 30, **every) == -1 and k in msg(), (k, msg())
        setattr(s, k, dict(GOOD, struct_size=40, amplitude=0.5, fade_in=0, reserved=0)[k])
    # then M, F, offset and F * N
    s.frames = 1 << 22
    assert _load(L, s, M=0, F=0, offset=1 << 30, **every) == -1 and "recording" in msg()
    assert _load(L, s, F=0, offset=1 << 30, **every) == -1 and "ir_frames" in msg()
    assert _load(L, s, F=1 << 20, offset=1 << 30, **every) == -1 and "offset" in msg()
    assert _load(L, s, F=1 << 20, **every) == -1 and "sweep frames" in msg()
    s.frames = 4096
    # then damp, eq and shape, at the sweep's rate
    assert _load(L, s, **every) == -1 and "xover_hz" in msg()
    assert _load(L, s, shape=bad_shape, eq=bad_eq) == -1 and "freq_hz" in msg()
    assert _load(L, s, shape=bad_shape) == -1 and "trim_db" in msg()
    above = IrEq(bands=[("peak", 21000.0, 3.0)]).to_c()  # (inside the band range at 48000, above it at 44100)
    assert _load(L, s, lr=p, eq=above) == -1 and "null argument" in msg()
    s.rate, s.f2_hz = 44100, 20000.0
    assert _load(L, s, lr=p, eq=above) == -1 and "freq_hz" in msg()
    s.rate = 48000
    # only then the recording and the engine
    assert _load(L, s) == -1 and "null lr" in msg()
    assert _load(L, s, lr=p) == -1 and "null argument" in msg()
    assert L.mc_ir_sweep_info(None, 0, (C.c_double * 4)()) == -1
