"""Synthesis of an IR from a seed without a GPU: the Philox known answers of the restatement (tests/ir_synth_np.py), the argument
checks of mc_synth_ir through the library with a null engine (they come before the engine is looked at), and the properties
the definition promises, on the restatement: equal channels at width 0, exact zeros where the build-up leaves a frame out, the
share of occupied frames, the channel correlation, and the decay time that was asked for."""
import ctypes as C
import math

import numpy as np
import pytest

import ir_decay_np
import ir_synth_np
from cuda_audio_amd import _lib

KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = ir_synth_np.philox(counter, key)
    assert " ".join(f"{int(w[0]):08x}" for w in got) == want


def test_philox_over_arrays_is_philox_of_each():
    i = np.array([0, 1, 77, 2 ** 24 - 1])
    got = ir_synth_np.words((5 << 32) | 9, i, 2)
    for k, v in enumerate(i):
        one = ir_synth_np.philox((int(v), 0, 2, 0), (9, 5))
        assert [int(w[k]) for w in got] == [int(w[0]) for w in one]


def test_u_is_exact_and_inside_the_open_interval():
    w = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    u = ir_synth_np.u(w)
    assert u[0] == 2.0 ** -33 and u[-1] == 1.0 - 2.0 ** -33
    assert np.array_equal(u * 4294967296.0 - 0.5, w.astype(np.float64))


# -- arguments ----------------------------------------------------------------------------------------------------------------
def _default():
    L = _lib.load()
    s = _lib.McIrSynth()
    L.mc_default_ir_synth(C.byref(s))
    return L, s


def test_struct_size_and_defaults():
    L, s = _default()
    assert C.sizeof(_lib.McIrSynth) == 80 and s.struct_size == 80
    assert _lib.McIrSynth.rate.offset == 60 and _lib.McIrSynth.early_first.offset == 64
    assert (s.n_early, s.seed, s.frames, s.late_start, s.t60, s.build_up) == (0, 0, 0, 0, 0, 0)
    assert (s.late_gain, s.direct, s.early_gain, s.width, s.rate, s.early_first, s.early_last) == (1.0, 0.0, 1.0, 1.0, 0, 0, 0)
    from cuda_audio_amd.engine import IrSynth

    c = IrSynth(frames=1000, seed=(7 << 32) | 3, late_start=5, t60=300, build_up=20, late_gain=0.5, direct=0.25, n_early=4, early_first=2,
                early_last=90, early_gain=-0.5, width=0.75, rate=48000).to_c()
    assert (c.struct_size, c.frames, c.seed, c.late_start, c.t60, c.build_up) == (80, 1000, (7 << 32) | 3, 5, 300, 20)
    assert (c.late_gain, c.direct, c.n_early, c.early_first, c.early_last, c.early_gain, c.width, c.rate) == (0.5, 0.25, 4, 2, 90, -0.5, 0.75, 48000)


REFUSALS = [
    (dict(struct_size=76), "struct_size"),
    (dict(n_early=65), "n_early"),
    (dict(frames=0), "frames"),
    (dict(frames=(1 << 24) + 1), "frames"),
    (dict(build_up=65536), "build_up"),
    (dict(late_gain=-0.1), "late_gain"),
    (dict(late_gain=float("nan")), "late_gain"),
    (dict(direct=float("inf")), "direct"),
    (dict(early_gain=float("nan")), "early_gain"),
    (dict(width=1.5), "width"),
    (dict(width=-0.01), "width"),
    (dict(width=float("nan")), "width"),
    (dict(rate=7999), "rate"),
    (dict(rate=384001), "rate"),
    (dict(n_early=1, early_first=10, early_last=9), "early_first"),
    (dict(n_early=1, early_first=10, early_last=1 << 24), "early_last"),
]


@pytest.mark.parametrize("fields,name", REFUSALS)
def test_a_bad_field_is_refused_before_the_engine_is_looked_at(fields, name):
    L, s = _default()
    s.frames = 1000
    for k, v in fields.items():
        setattr(s, k, v)
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, None, None) == -1
    msg = L.mc_last_error().decode()
    assert name in msg and "null" not in msg, msg


def test_fields_are_checked_in_order_and_then_damp_eq_shape_and_the_engine():
    L, s = _default()
    s.frames, s.n_early, s.width = 0, 99, 7.0
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, None, None) == -1 and "n_early" in L.mc_last_error().decode()
    s.n_early = 0
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, None, None) == -1 and "frames" in L.mc_last_error().decode()
    s.frames = 1000
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, None, None) == -1 and "width" in L.mc_last_error().decode()
    s.width = 0.5
    assert L.mc_synth_ir(None, 0, 1024, None, None, None, None) == -1 and "null synth" in L.mc_last_error().decode()
    # early_first and early_last are not looked at without reflections; seed, late_start and t60 take any value
    s.early_first, s.early_last, s.seed, s.late_start, s.t60 = 9, 3, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, None, None) == -1 and "null argument" in L.mc_last_error().decode()
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    damp, eq, shape = IrDamp(xovers=(400, 300), decay=(0, 1, 2)).to_c(), IrEq(bands=[("peak", 5.0, 3.0)]).to_c(), IrShape(trim_db=1.0).to_c()
    s.rate = 48000
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), C.byref(shape), C.byref(eq), C.byref(damp)) == -1
    assert "xover_hz" in L.mc_last_error().decode()
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), C.byref(shape), C.byref(eq), None) == -1 and "freq_hz" in L.mc_last_error().decode()
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), C.byref(shape), None, None) == -1 and "trim_db" in L.mc_last_error().decode()
    # a band or a damping that is on needs the session's rate
    s.rate = 0
    good = IrEq(bands=[("peak", 500.0, 3.0)]).to_c()
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, C.byref(good), None) == -1 and "session_rate" in L.mc_last_error().decode()
    gd = IrDamp().to_c()
    assert L.mc_synth_ir(None, 0, 1024, C.byref(s), None, None, C.byref(gd)) == -1 and "session_rate" in L.mc_last_error().decode()
    assert L.mc_ir_synth_info(None, 0, (C.c_double * 4)()) == -1


# -- properties of the restatement --------------------------------------------------------------------------------------------
def test_width_zero_gives_equal_channels_bit_for_bit():
    f = ir_synth_np.frames(frames=5000, seed=3, late_start=40, t60=2000, build_up=300, late_gain=0.3, direct=1.0, n_early=6, early_first=3,
                           early_last=35, early_gain=0.5, width=0.0)
    assert np.array_equal(f[:, 0], f[:, 1]) and np.count_nonzero(f[:, 0]) > 4000


def test_unoccupied_frames_are_exact_zeros_and_the_occupied_share_is_the_mean_of_p():
    B = 400
    p = dict(frames=3000, seed=11, late_start=100, t60=0, build_up=B, late_gain=1.0, width=1.0)
    f64 = ir_synth_np.frames64(**p)
    occ, prob = ir_synth_np.occupancy(p)
    late = f64[100:]
    assert np.all(late[~occ] == 0.0) and np.all(late[occ] != 0.0)
    assert occ[B - 1:].all() and np.all(prob[B - 1:] == 1.0) and not occ[:B].all()
    t1 = np.arange(1, B + 1, dtype=np.float64)
    want_p = np.minimum(1.0, np.maximum(1.0 / 16.0, (t1 / B) ** 2))
    assert np.array_equal(prob[:B], want_p)
    share, mean = occ[:B].mean(), want_p.mean()
    sd = math.sqrt((want_p * (1.0 - want_p)).sum()) / B  # of a sum of independent Bernoulli draws
    print(f"occupied share {share:.4f}, mean p {mean:.4f}, sd {sd:.4f}")
    assert abs(share - mean) <= 3.0 * sd
    # an occupied frame carries 1 / sqrt(p): the first ones are scaled by 4
    first = np.flatnonzero(occ)[0]
    assert prob[first] == 1.0 / 16.0
    dense = ir_synth_np.frames64(**dict(p, build_up=0))
    assert late[first, 0] == dense[100 + first, 0] * 4.0


def test_the_channel_correlation_follows_the_width():
    f = ir_synth_np.frames64(frames=4000, seed=1, late_start=0, t60=0, late_gain=1.0, width=0.5)
    r = float(np.corrcoef(f[:, 0], f[:, 1])[0, 1])
    print(f"correlation {r:.4f} at width 0.5 over 4000 frames")
    assert abs(r - 0.5) <= 0.05
    assert abs(float(f.std()) - 1.0) < 0.05  # late_gain is the standard deviation


def test_reflections_direct_sound_and_dropped_positions():
    p = dict(frames=200, seed=21, late_start=10 ** 6, direct=0.75, n_early=16, early_first=20, early_last=400, early_gain=0.5, width=1.0)
    tab = ir_synth_np.table(p)
    assert 0 < len(tab) < 16 and all(20 <= pos < 200 for pos, _, _ in tab)  # those at or past F are dropped
    f = ir_synth_np.frames64(**p)
    assert f[0, 0] == f[0, 1] == 0.75
    assert set(np.flatnonzero(np.abs(f).sum(axis=1))) == {0} | {pos for pos, _, _ in tab}
    for pos, gL, gR in tab:
        assert max(abs(gL), abs(gR)) == pytest.approx(0.5 * 21 / (pos + 1), rel=1e-12)  # the louder channel is g: 1 / distance
        assert min(abs(gL), abs(gR)) <= max(abs(gL), abs(gR))


DECAY_CASE = dict(frames=12000, t60=2000, late_start=120, late_gain=0.3, direct=1.0, n_early=8, early_first=20, early_last=110, early_gain=0.5, width=1.0)


@pytest.mark.parametrize("build_up", [0, 400])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_decay_is_the_one_asked_for(seed, build_up):
    """Rate 8000, t60 = 2000 frames = 0.25 s: the T30 of the broadband LR row within 5 % of it."""
    f = ir_synth_np.frames(**dict(DECAY_CASE, seed=seed, build_up=build_up))
    d = ir_decay_np.decay(f, 8000, onset_db=0, end=9000)
    t30 = d["rows"][(0, "LR")]["t30"]
    print(f"seed {seed}, build_up {build_up}: T30 {t30:.4f} s")
    assert abs(t30 - 0.25) <= 0.05 * 0.25
