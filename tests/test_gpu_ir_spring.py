"""A spring tank's IR on the device (mc_synth_ir_spring, csrc/irspring.hip.h): spike trains against their closed form within the
plan's alias bound, dispersive loads against the float64 restatement (a) of tests/ir_spring_np.py, the radius against the alias
identity summed from the time recursion (b), the bits, the first echo's group delay, the decay time, the synthesis' own terms
and the measurements on the result, the engine's paths against the oracle fed the restated taps, and the refusals.

The bar for taps is test_gpu_ir_shape._check_taps (1e-6 relative RMS, 1e-5 of the peak): a frame differs from numpy's by the
transform's rounding times rho^t <= 1e4 and by the M ulp of the powers, far below a quantum of 2^-40 times the taps' level before
the one rounding to float32, which is the situation that bar was set for."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_decay_np
import ir_response_np
import ir_spring_np as sp
import ir_synth_np
from helpers import RMS_TOL, apply_params, rms
from test_gpu_ir_shape import P0, P1, _check_level, _check_taps
from test_ir_spring_cpu import DECAY_FIELDS, DECAY_FRAMES, DECAY_MARGIN, GROUP_DELAY_MARGIN

pytestmark = pytest.mark.gpu

RATE = 8000
ALONE = dict(late_gain=0.0, direct=0.0)  # the synthesis' own terms off: the spring alone
QUANTUM = 2.0 ** -40


def _conv(n_ref=16384, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irspring", n_ref, sample_rate=rate, **kw)


def _ispring(fields):
    from cuda_audio_amd.engine import IrSpring

    return IrSpring(**fields)


def _isynth(fields):
    from cuda_audio_amd.engine import IrSynth

    return IrSynth(**fields)


def _freeze(v):
    return tuple(sorted((k, _freeze(x)) for k, x in v.items())) if isinstance(v, dict) else v


@functools.lru_cache(maxsize=None)
def _restated_cached(spring, frames, rate):
    out, plan = sp.spring64(rate, frames, **dict(spring))
    out.setflags(write=False)
    return out, plan


def _restated(spring, frames, rate=RATE):
    """(the spring's term float64 [F, 2], plan) by restatement (a), computed once."""
    return _restated_cached(_freeze(spring), frames, rate)


def _check_info(info, plan):
    from cuda_audio_amd.engine import _spring_numbers

    want = _spring_numbers(sp.plan_numbers(plan))
    print("spring info:", info)
    for k in ("points", "stretch", "transition", "springs", "sections", "lowpass", "last", "delay"):
        assert info[k] == want[k], (k, info[k], want[k])
    np.testing.assert_allclose(np.array(info["loop_gain"]), np.array(want["loop_gain"]), rtol=1e-14)
    assert abs(info["alias_db"] - want["alias_db"]) <= 1e-9 * abs(want["alias_db"])


def _load_and_check(c, idx, spring, frames, rate=RATE, **kw):
    """Load the spring alone, then the taps and the plan against restatement (a)."""
    want, plan = _restated(spring, frames, rate)
    c.prepare_synth(idx, _isynth(dict(ALONE, frames=frames)), spring=_ispring(spring), **kw)
    got = c.ir_taps(idx)
    assert len(got) == len(want)
    _check_taps(got, want)
    _check_info(c.ir_spring_info(idx), plan)
    return got, want, plan


# -- 1. spike trains -------------------------------------------------------------------------------------------------------
def _spikes(F, L, g, gain=1.0):
    want = np.zeros(F)
    k = np.arange(1, F // L + 1) if L <= F else np.arange(0)
    k = k[k * L < F]
    want[k * L] = gain * g ** (k - 1.0) if k.size else 0.0
    return want


def _check_spikes(got, want, plan):
    """Within the plan's alias bound plus one rounding to float32."""
    err = np.abs(got.astype(np.float64) - want)
    tol = plan["alias"] + 2.0 ** -24 * np.abs(want)
    print(f"spikes: {np.count_nonzero(want)} of {len(want)}, alias bound {plan['alias']:.2e}, worst error {err.max():.2e}, worst error over bound {(err / tol).max():.3f}")
    assert (err <= tol).all()


def _spike_fields(L, g, **kw):
    return sp.loop_fields(RATE, 1, 0, 0.0, L, g, **kw)


@pytest.mark.parametrize("F", [1, 7, 511, 512, 513, 1024, 1025, 4097])
def test_spike_trains_over_the_lengths(gpu_lib, F):
    """N goes from 1024 to 2048 at 513 frames and the transform from one pass to two at 1025 (N = 4096).  The loop hardly decays
    (|g| = 0.999 every 3 frames), so the alias bound is what the radius alone leaves: 1e-8 and less."""
    fields = _spike_fields(3, -0.999)
    plan = sp.spring_plan64(RATE, F, **fields)
    assert plan["N"] == max(1024, 1 << (2 * F - 1).bit_length()) and plan["L"][0] == [3, 3] and 1e-12 < plan["alias"] <= 1e-8
    g = plan["g"][0][0]
    c = _conv()
    c.prepare_synth(0, _isynth(dict(ALONE, frames=F)), spring=_ispring(fields))
    got = c.ir_taps(0)
    _check_info(c.ir_spring_info(0), plan)
    c.close()
    assert got.shape == (F, 2)
    for ch in range(2):
        _check_spikes(got[:, ch], _spikes(F, 3, g), plan)
    if F >= 7:
        assert abs(got[3, 0] - 1.0) < 1e-6 and abs(got[6, 0] - g) < 1e-6


def test_spike_trains_of_one_frame_beyond_the_end_and_apart_in_the_channels(gpu_lib):
    c = _conv()
    # L = 1: every frame from the first on
    fields = _spike_fields(1, -0.999)
    plan = sp.spring_plan64(RATE, 513, **fields)
    assert plan["L"][0] == [1, 1]
    c.prepare_synth(0, _isynth(dict(ALONE, frames=513)), spring=_ispring(fields))
    _check_spikes(c.ir_taps(0)[:, 0], _spikes(513, 1, plan["g"][0][0]), plan)
    # L > E: the first echo lies past the last frame, inside the transform; nothing is heard of it
    fields = _spike_fields(600, -0.9)
    plan = sp.spring_plan64(RATE, 511, **fields)
    assert plan["L"][0] == [600, 600] and plan["N"] == 1024 and plan["alias"] == 1e-8
    c.prepare_synth(1, _isynth(dict(ALONE, frames=511)), spring=_ispring(fields))
    _check_spikes(c.ir_taps(1)[:, 0], np.zeros(511), plan)
    # ... and past the transform as well
    fields = _spike_fields(3000, -0.9)
    plan = sp.spring_plan64(RATE, 511, **fields)
    c.prepare_synth(1, _isynth(dict(ALONE, frames=511)), spring=_ispring(fields))
    _check_spikes(c.ir_taps(1)[:, 1], np.zeros(511), plan)
    # stereo: R's spikes every 10 frames, L's every 8, half as loud
    fields = _spike_fields(8, -0.999, stereo=0.25, gain=0.5)
    plan = sp.spring_plan64(RATE, 1000, **fields)
    assert plan["L"][0] == [8, 10]
    c.prepare_synth(2, _isynth(dict(ALONE, frames=1000)), spring=_ispring(fields))
    got = c.ir_taps(2)
    c.close()
    for ch in range(2):
        _check_spikes(got[:, ch], _spikes(1000, plan["L"][0][ch], plan["g"][0][ch], 0.5), plan)
    assert got[8, 0] > 0.4 and abs(got[8, 1]) < 1e-7 and got[10, 1] > 0.4 and abs(got[10, 0]) < 1e-7


# -- 2. dispersive loads against (a) -------------------------------------------------------------------------------------
HIGH = dict(high_gain=0.2, high_sections=37, high_dispersion=-0.6, high_delay=0.5, high_t60=0.3)
DISPERSIVE = {
    "M 1, K 1": (RATE, 1500, sp.loop_fields(RATE, 1, 1, 0.62, 50, -0.8, damping=0.2, lowpass_order=8)),  # (K = 1 leaves the low-pass out)
    "M 2, K 5, low-pass 2, high": (RATE, 1500, sp.loop_fields(RATE, 5, 2, 0.62, 60, -0.8, damping=0.3, lowpass_order=2, **HIGH)),
    "M 3, K 5, three springs, low-pass 8, last": (RATE, 1500, dict(sp.loop_fields(RATE, 5, 3, 0.5, 60, -0.8, damping=0.2, lowpass_order=8, stereo=0.05),
                                                                   delay_ms=(9.0, 11.5, 14.25), last=1000)),
    "M 100, K 5, three springs, high": (RATE, 3000, dict(sections=100, transition_hz=800.0, delay_ms=(33.0, 41.0, 47.5), t60=0.8, **HIGH)),
    "the default tank at 48 kHz": (48000, 6000, {}),
}


@pytest.mark.parametrize("name", list(DISPERSIVE))
def test_dispersive_loads_match_the_restatement(gpu_lib, name):
    rate, F, fields = DISPERSIVE[name]
    plan = sp.spring_plan64(rate, F, **fields)
    if name.startswith("M "):
        assert (plan["M"], plan["K"]) == tuple(int(v) for v in name.replace(",", "").split()[1:4:2])
    assert plan["S"] == (3 if "three" in name else 1 if name.startswith("M ") else 2) and plan["high"] == ("high" in name or not fields)
    assert len(plan["bq"]) == (1 if "low-pass 2" in name else 0 if "K 1" in name else 4)
    c = _conv(rate=rate)
    got, want, _ = _load_and_check(c, 0, fields, F, rate)
    c.close()
    E = plan["E"]
    assert (E < F) == ("last" in name) and not got[E:].any() and np.abs(got[:E]).max() > 0.01


# -- 3. the radius -------------------------------------------------------------------------------------------------------------
def test_a_forced_transform_size_wraps_as_the_alias_identity_says(gpu_lib):
    """N = 1024 and a loop that has hardly decayed by then: the device's frames are sum_m h[t + 1024 m] 1e-8^m with h from the
    time recursion (b).  Where h itself is zero, before the first echo, the wrapped part stands alone: 1e-8 of h[t + 1024], held to
    a quantum of 2^-40 and 1e-12 (the transform's rounding there is u log2(N) |X| rho^t, about 1e-14)."""
    fields = dict(sp.loop_fields(RATE, 3, 7, 0.62, 40, -0.97, damping=0.1, stereo=0.1), log2_points=10)
    F = 500
    h = sp.recursion64(RATE, 4096, **fields)
    folded = sum(h[1024 * m:1024 * m + F] * 1e-8 ** m for m in range(4))
    c = _conv()
    got, _, plan = _load_and_check(c, 0, fields, F)
    c.close()
    assert plan["N"] == 1024 and plan["L"][0][0] == 40 <= plan["L"][0][1]
    _check_taps(got, folded)
    quiet = slice(0, 40)
    assert not h[quiet].any() and np.abs(folded[quiet]).max() > 100 * (QUANTUM + 1e-12)  # (the wrapped part is there to be seen)
    err = np.abs(got[quiet].astype(np.float64) - folded[quiet])
    print(f"before the first echo: wrapped part up to {np.abs(folded[quiet]).max():.2e}, device off by {err.max():.2e}")
    assert (err <= QUANTUM + 1e-12 + 2.0 ** -24 * np.abs(folded[quiet])).all()


# -- 4. bits ------------------------------------------------------------------------------------------------------------------
def test_the_same_struct_stores_the_same_bits(gpu_lib):
    rate, F, fields = DISPERSIVE["M 100, K 5, three springs, high"]
    c = _conv()
    a, _, _ = _load_and_check(c, 0, fields, F)
    b, _, _ = _load_and_check(c, 3, fields, F)
    assert a.tobytes() == b.tobytes() and c.ir_spectra(0).tobytes() == c.ir_spectra(3).tobytes()
    assert c.ir_info(0) == c.ir_info(3) and c.ir_spring_info(0) == c.ir_spring_info(3)
    c.close()
    c = _conv()
    c.prepare_synth(1, _isynth(dict(ALONE, frames=700)), spring=_ispring(DISPERSIVE["M 1, K 1"][2]))  # (something else first)
    d, _, _ = _load_and_check(c, 2, fields, F)
    assert d.tobytes() == a.tobytes()
    # with the transform's size fixed, a frame does not depend on the length
    fixed = dict(fields, log2_points=12)
    short, _, _ = _load_and_check(c, 0, fixed, 1000)
    long_, _, _ = _load_and_check(c, 1, fixed, 2048)
    assert short.tobytes() == long_[:1000].tobytes()
    # the high loop switched off is really off: its other fields change nothing
    off, _, _ = _load_and_check(c, 0, dict(fields, high_gain=0.0), F)
    other, _, _ = _load_and_check(c, 1, dict(fields, high_gain=0.0, high_sections=3, high_dispersion=-0.1, high_delay=1.0, high_t60=0.0), F)
    assert off.tobytes() == other.tobytes() and off.tobytes() != a.tobytes()
    c.close()


FULL = dict(frames=5000, seed=(0x1234 << 32) | 7, late_start=1500, t60=20000, build_up=2000, late_gain=0.05, direct=1.0, n_early=12, early_first=100,
            early_last=1400, early_gain=0.5, width=0.7)


def test_without_a_spring_the_call_is_mc_synth_ir_room_without_a_room(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, IrTail

    shape, eq, damp = IrShape(fade_out=100, normalize="peak", target=0.05), IrEq(bands=[("lowcut", 120)]), IrDamp(xovers=(400, 1600), decay=(0, 4800, 1600), origin=37)
    tail = IrTail(mode="cut", knee=(3000,), fade=64)
    c = _conv()
    L = c._L
    s, sh, q, d, t = _isynth(dict(FULL, rate=RATE)).to_c(), shape.to_c(), eq.to_c(), damp.to_c(), tail.to_c()
    assert L.mc_synth_ir_room(c._h, 0, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), None) == 0
    assert L.mc_synth_ir_spring(c._h, 1, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), None) == 0
    assert L.mc_synth_ir_room(c._h, 2, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), C.byref(t)) == 0
    assert L.mc_synth_ir_spring(c._h, 3, 1024, C.byref(s), None, C.byref(sh), C.byref(q), C.byref(d), C.byref(t)) == 0
    c.prepare_synth(4, _isynth(FULL), shape=shape, eq=eq, damp=damp, spring=None)
    for a, b in ((0, 1), (2, 3), (0, 4)):
        assert c.ir_taps(a).tobytes() == c.ir_taps(b).tobytes() and c.ir_spectra(a).tobytes() == c.ir_spectra(b).tobytes()
        assert c.ir_info(a) == c.ir_info(b) and c.ir_shape_info(a) == c.ir_shape_info(b) and c.ir_synth_info(a) == c.ir_synth_info(b)
    assert c.ir_taps(0).tobytes() != c.ir_taps(2).tobytes() and c.ir_tail_info(3) == c.ir_tail_info(2)
    for idx in range(5):
        with pytest.raises(McError) as ex:
            c.ir_spring_info(idx)
        assert ex.value.code == -3
    c.close()


# -- 5. group delay -----------------------------------------------------------------------------------------------------------
def test_the_group_delay_of_the_first_echo(gpu_lib):
    """M = 20, K = 2, a = 0.5, L = 400, g = 0: one echo over frames 413 .. 520.  ir_response's delay over the window [300, 700)
    against the restatement of that measurement on the stored taps at its own bar, the stored taps against (a), and the delay
    against the closed form within the margin tests/test_ir_spring_cpu.py measured on (a)."""
    M, K, a, L = 20, 2, 0.5, 400
    fields = sp.loop_fields(RATE, K, M, a, L, 0.0)
    c = _conv()
    got, want, plan = _load_and_check(c, 0, fields, 1024)
    assert plan["L"][0] == [L, L] and plan["g"][0] == [0.0, 0.0] and not got[:L].any()
    hz = np.array([100.0, 300.0, 600.0, 900.0, 1200.0, 1500.0, 1800.0], np.float32)
    query = dict(hz=hz, windows=[(300, 400, 0, 0)], onset_db=0.0)
    measured = c.ir_response(0, **query)
    c.close()
    ir_response_np.check_against(measured, ir_response_np.response(got, RATE, **query))
    closed = sp.group_delay_closed(2 * np.pi * hz.astype(np.float64) / RATE, L, M, K, sp.f32(a))
    on_a = ir_response_np.response(want.astype(np.float32), RATE, **query)["delay"][0, 0]
    delay = measured["delay"][0, 0]
    print("closed form", np.round(closed, 3), "device - closed", delay - closed, "device - numpy on (a)", delay - on_a)
    assert np.abs(delay - closed).max() <= GROUP_DELAY_MARGIN
    assert np.abs(delay - on_a).max() <= GROUP_DELAY_MARGIN


# -- 6. decay -----------------------------------------------------------------------------------------------------------------
def test_the_decay_time(gpu_lib):
    """One spring, no damping, t60 2 s, 4 s at 8 kHz: T30 within DECAY_MARGIN of 2 s (tests/test_ir_spring_cpu.py has where the
    margin comes from), and ir_decay on the stored taps against its restatement."""
    c = _conv(65536)
    got, _, plan = _load_and_check(c, 0, DECAY_FIELDS, DECAY_FRAMES)
    assert len(got) == DECAY_FRAMES == 4 * RATE
    res = c.ir_decay(0)
    c.close()
    ir_decay_np.check_against(res, ir_decay_np.decay(got, RATE))
    t30 = res["rows"][(0, "L")]["t30"]
    print(f"T30 {t30:.4f} s, loop gain {plan['g'][0][0]:.4f} every {plan['L'][0][0]} frames and the cascade")
    assert abs(t30 - 2.0) <= DECAY_MARGIN


# -- 7. composition ---------------------------------------------------------------------------------------------------------
COMP = dict(sp.loop_fields(RATE, 4, 12, 0.6, 150, -0.85, damping=0.2, lowpass_order=4, stereo=0.04, gain=0.3, **HIGH), last=4000)


def test_spring_late_field_direct_and_reflections_round_once(gpu_lib):
    import ir_density_np
    import ir_tail_np
    from cuda_audio_amd.engine import IrTail

    term, plan = _restated(COMP, FULL["frames"])
    want = ir_synth_np.frames64(**FULL) + term
    c = _conv()
    c.prepare_synth(0, _isynth(FULL), spring=_ispring(COMP))
    got = c.ir_taps(0)
    _check_taps(got, want)
    _check_info(c.ir_spring_info(0), plan)
    assert c.ir_synth_info(0) == dict(frames=5000, reflections=12, late_start=1500)
    # the spring is a fourth term: without it the frames are mc_synth_ir's, and from E on they are with it
    c.prepare_synth(1, _isynth(FULL))
    plain = c.ir_taps(1)
    assert not np.array_equal(got[:4000], plain[:4000])
    np.testing.assert_array_equal(got[4000:], plain[4000:])
    # the measurements read the result
    dens = c.ir_density(0, profile=True)
    ir_density_np.check_against(dens, ir_density_np.density(got, RATE))
    # the tail step runs on the generated frames
    spec = dict(xovers=(1000,), knee=(3000, 2500), fade=64)
    c.prepare_synth(2, _isynth(FULL), spring=_ispring(COMP), tail=IrTail(mode="cut", **spec))
    cut = c.ir_taps(2)
    y, tinfo = ir_tail_np.tail64(want.astype(np.float32), RATE, "cut", **spec)
    _check_taps(cut, y)
    assert c.ir_tail_info(2) == tinfo and c.ir_spring_info(2) == c.ir_spring_info(0) and not cut[3000:].any()
    c.close()


# -- the engine plays a spring ---------------------------------------------------------------------------------------------
PLAY_SPRING = dict(sections=40, transition_hz=2000.0, delay_ms=(41.0, 53.0), t60=0.6, gain=0.02, high_gain=0.1, high_sections=50, high_t60=0.3)
PLAY_FRAMES = 7000
PLAY_OTHER = dict(frames=5000, seed=3, late_start=0, t60=4000, late_gain=0.01, width=1.0)


def _play_taps(n_ref):
    a = _restated(PLAY_SPRING, PLAY_FRAMES)[0].astype(np.float32)[:n_ref - 1024]
    return [a, ir_synth_np.frames(**PLAY_OTHER)[:n_ref - 1024]]


def _prepare_play(c):
    c.prepare_synth(0, _isynth(dict(ALONE, frames=PLAY_FRAMES)), spring=_ispring(PLAY_SPRING))
    c.prepare_synth(1, _isynth(PLAY_OTHER))


def _oracle_want(oracle_mod, n_ref, taps, x, **kw):
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, P0, P1, True)
    want = ref.process(x[0], x[1], **kw)
    _check_level(want, x, P0, P1)
    return want


def test_jack_period_matches_the_oracle(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, period, ncalls = 16384, 256, 160
    taps = _play_taps(n_ref)
    x = make_input(ncalls * period)
    want = _oracle_want(oracle_mod, n_ref, taps, x, block=period)
    c = _conv(n_ref, max_batch=16, period=period)
    _prepare_play(c)
    _check_taps(c.ir_taps(0), taps[0].astype(np.float64))
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period])) for k in range(ncalls)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


def test_single_transform_form(oracle_mod, gpu_lib):
    from cuda_audio_amd.synth import make_input

    n_ref, nb = 16384, 64
    taps = _play_taps(n_ref)
    x = make_input(nb * 256)
    want = _oracle_want(oracle_mod, n_ref, taps, x)
    c = _conv(n_ref, max_batch=32, form="single")
    _prepare_play(c)
    _check_info(c.ir_spring_info(0), _restated(PLAY_SPRING, PLAY_FRAMES)[1])
    assert c.ir_info(0)["taps"] == len(taps[0])
    np.testing.assert_allclose(c.ir_info(0)["sigma"], taps[0].astype(np.float64).sum(axis=0), rtol=0, atol=1e-5)
    apply_params(c, P0, P1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    c.close()
    assert rms(got - want) <= RMS_TOL


# -- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, IrEq, IrPlate, IrRoom, IrShape, IrTail
    from cuda_audio_amd.synth import make_ir

    synth = dict(ALONE, frames=3000)
    good_fields = DISPERSIVE["M 2, K 5, low-pass 2, high"][2]
    good = _ispring(good_fields)
    tail = IrTail(mode="cut", knee=(2000,), fade=64)
    c = _conv()
    c.prepare_synth(0, _isynth(synth), spring=good, tail=tail, shape=IrShape(fade_out=100))
    c.prepare_synth(1, _isynth(dict(synth, late_gain=0.01, seed=5)))  # a second IR, without a spring
    state = lambda: (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_synth_info(0), c.ir_spring_info(0),  # noqa: E731
                     c.ir_tail_info(0), c.ir_taps(1).tobytes(), c.ir_info(1), c.num_irs())
    before = state()
    assert c.ir_spring_info(0)["sections"] == 2
    bad = [(dict(sections=513), "sections"), (dict(transition_hz=0.0), "transition_hz"), (dict(dispersion=0.99), "dispersion"), (dict(delay_ms=(0.0,)), "delay_ms[0]"),
           (dict(delay_ms=(20.0, -1.0)), "delay_ms[1]"), (dict(t60=-1.0), "t60_s"), (dict(damping=1.0), "damping"), (dict(lowpass_order=3), "lowpass_order"),
           (dict(high_gain=-1.0), "high_gain"), (dict(high_sections=2000), "high_sections"), (dict(high_dispersion=0.2), "high_dispersion"),
           (dict(high_delay=0.0), "high_delay"), (dict(high_t60=-1.0), "high_t60_s"), (dict(stereo=0.5), "stereo"), (dict(gain=0.0), "gain"),
           (dict(log2_points=9), "log2_points"), (dict(transition_hz=5000.0), "half the rate"), (dict(transition_hz=50.0), "K = 80"),
           (dict(sections=100, delay_ms=(5.0,)), "shorter than the dispersion's own delay"), (dict(delay_ms=(1.0,), t60=1000.0), "0.9999"),
           (dict(log2_points=10), "set last")]
    for fields, word in bad:
        for idx in (0, 1, 2):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), spring=_ispring(dict(good_fields, **fields)))
            assert ex.value.code == -1 and word in str(ex.value), (fields, str(ex.value))
    with pytest.raises(McError) as ex:
        c.prepare_synth(0, _isynth(dict(ALONE, frames=(1 << 21) + 1)), spring=good)
    assert ex.value.code == -1 and "set last" in str(ex.value)
    # a spring together with a room or a plate is not offered
    for kw in (dict(room=IrRoom(order=2)), dict(plate=IrPlate())):
        with pytest.raises(ValueError):
            c.prepare_synth(0, _isynth(synth), spring=good, **kw)
    for kw in (dict(tail=IrTail(mode="extend", knee=(100,), t60=(0,))), dict(shape=IrShape(trim_db=1.0)), dict(shape=IrShape(start=3000)),
               dict(eq=IrEq(bands=[("peak", 5.0, 3.0)])), dict(damp=IrDamp(xovers=(1600, 400), decay=(0, 1, 2))), dict(nframes=16384)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare_synth(idx, _isynth(dict(synth, seed=1)), spring=good, **kw)
            assert ex.value.code == -1
    with pytest.raises(McError) as ex:
        c.prepare_synth(1, _isynth(dict(synth, frames=0)), spring=good)
    assert ex.value.code == -1
    nosr = _conv(16384, None)  # (an engine without a session rate: the spring needs one)
    with pytest.raises(McError) as ex:
        nosr.prepare_synth(0, _isynth(synth), spring=good)
    assert ex.value.code == -1 and "the spring needs the session's rate" in str(ex.value) and nosr.num_irs() == 0
    nosr.close()
    with pytest.raises(McError) as ex:
        c.ir_spring_info(1)
    assert ex.value.code == -3 and "was not loaded with a spring" in str(ex.value)
    with pytest.raises(McError) as ex:
        c.ir_spring_info(2)
    assert ex.value.code == -1
    assert state() == before
    # a WAV load over the index forgets the spring, and so does a synthesis without one
    c.prepare(0, make_ir(3000, seed=2, norm=0.05))
    with pytest.raises(McError) as ex:
        c.ir_spring_info(0)
    assert ex.value.code == -3
    c.prepare_synth(0, _isynth(synth), spring=good)
    assert c.ir_spring_info(0)["sections"] == 2
    c.prepare_synth(0, _isynth(dict(synth, direct=1.0)))
    with pytest.raises(McError) as ex:
        c.ir_spring_info(0)
    assert ex.value.code == -3
    c.close()
