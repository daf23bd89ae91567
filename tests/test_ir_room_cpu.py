"""The room of mc_synth_ir_room without a GPU: the struct's layout and defaults, every refusal through the library with a null
engine (the checks come before the engine is looked at), mc_ir_room_plan against the restatement's plan(), and the properties
of the definition on the float64 restatement (tests/ir_room_np.py) that need no device."""
import ctypes as C

import numpy as np
import pytest

import ir_room_np
from cuda_audio_amd import _lib
from cuda_audio_amd.engine import IrRoom, IrSynth, IrTail, room_plan

RATE = 48000
WHOLE = dict(size=(10.0, 10.0, 10.0), source=(2.0, 5.0, 5.0), receiver=(3.0, 5.0, 5.0), spacing=0.0, speed=480.0, beta=0.0, gain=0.5)


def _room(**fields):
    r = _lib.McIrRoom()
    _lib.load().mc_default_ir_room(C.byref(r))
    for k, v in fields.items():
        if k in ("size_m", "source_m", "receiver_m", "beta"):
            for i, e in v.items():
                getattr(r, k)[i] = e
        else:
            setattr(r, k, v)
    return r


def test_struct_layout_and_defaults():
    R = _lib.McIrRoom
    assert C.sizeof(R) == 96
    offsets = dict(struct_size=0, order=4, size_m=8, source_m=20, receiver_m=32, beta=44, spacing_m=68, axis=72, speed=76, gain=80, reserved=84, last=88)
    assert {n: getattr(R, n).offset for n, _ in R._fields_} == offsets
    r = _room()
    assert (r.struct_size, r.order, r.axis, r.reserved, r.last) == (96, 0, 0, 0, 0)
    assert tuple(r.size_m) == (5.0, 4.0, 3.0) and tuple(r.source_m) == (1.0, 1.5, np.float32(1.2)) and tuple(r.receiver_m) == (3.5, 2.0, 1.5)
    assert tuple(r.beta) == (np.float32(0.9),) * 6 and r.spacing_m == np.float32(0.2) and r.speed == 343.0 and r.gain == 1.0
    assert _lib.MC_ROOM_MAX_ORDER == ir_room_np.MAX_ORDER == 32
    c = IrRoom().to_c()
    assert bytes(c) == bytes(r)
    assert IrRoom(axis="z", beta=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6)).to_c().axis == 2


# (the field the message must name, the fields changed, the session's rate, F)
BAD_ROOMS = [
    ("struct_size", dict(struct_size=92), RATE, 4000),
    ("order", dict(order=33), RATE, 4000),
    ("size_m[0]", dict(size_m={0: 0.4}), RATE, 4000),
    ("size_m[2]", dict(size_m={2: 201.0}), RATE, 4000),
    ("size_m[1]", dict(size_m={1: float("nan")}), RATE, 4000),
    ("source_m[0]", dict(source_m={0: 0.0}), RATE, 4000),
    ("source_m[1]", dict(source_m={1: 4.0}), RATE, 4000),
    ("source_m[2]", dict(source_m={2: float("nan")}), RATE, 4000),
    ("receiver_m[0]", dict(receiver_m={0: 5.0}), RATE, 4000),
    ("receiver_m[2]", dict(receiver_m={2: -0.1}), RATE, 4000),
    ("beta[0]", dict(beta={0: 1.01}), RATE, 4000),
    ("beta[5]", dict(beta={5: -1.5}), RATE, 4000),
    ("beta[3]", dict(beta={3: float("nan")}), RATE, 4000),
    ("spacing_m", dict(spacing_m=-0.1), RATE, 4000),
    ("spacing_m", dict(spacing_m=float("inf")), RATE, 4000),
    ("axis", dict(axis=3), RATE, 4000),
    ("spacing_m", dict(spacing_m=3.0), RATE, 4000),            # the right receiver at 3.5 + 1.5 = 5: on the wall
    ("spacing_m", dict(spacing_m=3.5, axis=2), RATE, 4000),    # the left receiver below the floor
    ("speed", dict(speed=99.0), RATE, 4000),
    ("speed", dict(speed=float("nan")), RATE, 4000),
    ("gain", dict(gain=0.0), RATE, 4000),
    ("gain", dict(gain=16.5), RATE, 4000),
    ("reserved", dict(reserved=1), RATE, 4000),
    ("session's rate", dict(), 0, 4000),
    ("apart", dict(source_m={0: 3.45, 1: 2.0, 2: 1.5}, spacing_m=0.0), RATE, 4000),       # 0.05 m from both receivers
    ("apart", dict(source_m={0: 3.45, 1: 2.0, 2: 1.5}), RATE, 4000),                      # 0.05 m from the left one
    ("order", dict(), RATE, 48000),                                                        # order 0 would need 58
    ("gain", dict(order=32, gain=8.0), RATE, 4000),                                        # 8 * 65^3 * 8 / 2.4 m >= 2^22
]


@pytest.mark.parametrize("name,fields,rate,F", BAD_ROOMS)
def test_refusals_name_the_field(name, fields, rate, F):
    L = _lib.load()
    r = _room(**fields)
    s = IrSynth(frames=F, rate=rate, late_gain=0.0).to_c()
    assert L.mc_synth_ir_room(None, 0, 1024, C.byref(s), C.byref(r), None, None, None, None) == -1
    msg = L.mc_last_error().decode()
    assert name in msg, (name, msg)
    if rate:
        out = (C.c_double * 8)()
        assert L.mc_ir_room_plan(C.byref(r), rate, F, out) == -1
        assert name in L.mc_last_error().decode(), (name, L.mc_last_error())


def test_the_order_of_the_checks():
    """synth, then room, then tail (F' after F), then damp, eq and shape, then the engine."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape

    L = _lib.load()
    good, bad_room = _room(), _room(order=40)
    s = IrSynth(frames=4000, rate=RATE, late_gain=0.0).to_c()
    bad_s = IrSynth(frames=0, rate=RATE).to_c()
    tail = IrTail(mode="extend", knee=(100,), t60=(100,)).to_c()
    bad_tail = IrTail(mode="extend", knee=(100,), t60=(0,)).to_c()
    bad_damp = IrDamp(xovers=(1600, 400), decay=(0, 1, 2)).to_c()
    bad_eq = IrEq(bands=[("peak", 5.0, 3.0)]).to_c()
    bad_shape = IrShape(trim_db=1.0).to_c()

    def call(synth=s, room=good, shape=None, eq=None, damp=None, tail=None):
        rc = L.mc_synth_ir_room(None, 0, 1024, C.byref(synth), C.byref(room) if room is not None else None, C.byref(shape) if shape is not None else None,
                                C.byref(eq) if eq is not None else None, C.byref(damp) if damp is not None else None,
                                C.byref(tail) if tail is not None else None)
        return rc, L.mc_last_error().decode()

    assert "frames" in call(synth=bad_s, room=bad_room, tail=bad_tail)[1]
    assert "order" in call(room=bad_room, tail=bad_tail, damp=bad_damp)[1]
    assert "t60[0]" in call(tail=bad_tail, damp=bad_damp, eq=bad_eq)[1]
    assert "t60[0]" in call(room=None, tail=bad_tail, damp=bad_damp)[1]  # (a tail without a room)
    rc, msg = call(tail=tail, damp=bad_damp, eq=bad_eq, shape=bad_shape)
    assert rc == -1 and "xover" in msg, msg
    rc, msg = call(tail=tail, eq=bad_eq, shape=bad_shape)
    assert rc == -1 and ("freq" in msg or "band" in msg), msg
    rc, msg = call(tail=tail, shape=bad_shape)
    assert rc == -1 and "trim_db" in msg, msg
    norate = IrSynth(frames=4000, rate=0, late_gain=0.0).to_c()
    rc, msg = call(synth=norate, room=None, tail=tail)
    assert rc == -1 and "session's rate" in msg, msg
    rc, msg = call(tail=tail)
    assert rc == -1 and "null" in msg, msg  # everything is good: the engine is looked at last
    rc, msg = call(room=None)  # neither a room nor a tail: mc_synth_ir itself
    assert rc == -1 and "null" in msg, msg


@pytest.mark.parametrize("fields,rate,F", [({}, 48000, 4000), (dict(order=7, last=1000), 44100, 30000), (dict(beta=1.0, size=(8.0, 3.0, 2.5)), 96000, 9000),
                                           (dict(beta=0.0, spacing=0.0), 8000, 500), (dict(beta=(0.9, -0.8, 0.5, 0.7, 0.2, 1.0), axis="y"), 48000, 12000)])
def test_the_plan_matches_the_restatement(fields, rate, F):
    got = room_plan(IrRoom(**fields), rate, F)
    want = ir_room_np.plan(dict(fields, axis=IrRoom.AXES.get(fields.get("axis", 0), fields.get("axis", 0))), rate, F)
    print(got, want)
    for k in ("order", "images", "complete"):
        assert got[k] == want[k], k
    for k in ("direct", "volume", "sabine", "eyring"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0)
    if fields.get("beta") == 1.0:
        assert got["sabine"] == 0.0 and got["eyring"] == 0.0
    if fields.get("beta") == 0.0:
        assert got["eyring"] == 0.0 and got["sabine"] > 0.0


def test_the_plan_needs_a_rate_and_frames():
    L = _lib.load()
    out = (C.c_double * 8)()
    r = _room()
    for rate, F, name in ((0, 4000, "rate"), (7999, 4000, "rate"), (48000, 0, "frames"), (48000, (1 << 24) + 1, "frames")):
        assert L.mc_ir_room_plan(C.byref(r), rate, F, out) == -1
        assert name in L.mc_last_error().decode()
    assert L.mc_ir_room_plan(None, 48000, 4000, out) == -1 and L.mc_ir_room_plan(C.byref(r), 48000, 4000, None) == -1


def test_a_whole_frame_delay_is_exactly_one_tap():
    """The source 1 m from the receiver at c = 480 and 48 kHz: 100 frames exactly; beta 0 silences every other image."""
    im = ir_room_np.images(WHOLE, RATE, 300)
    ir_room_np.assert_floor_margin(im["tau"][im["a"] != 0], 300, exact=2)
    out, covered, info = ir_room_np.frames64(WHOLE, RATE, frames=300, late_gain=0.0)
    want = np.zeros((300, 2))
    want[100] = 0.5
    np.testing.assert_array_equal(out, want)
    assert covered.sum() == 2 and info["direct"] == (100.0, 100.0)


def test_spacing_zero_gives_equal_channels():
    acc, _, info = ir_room_np.render(dict(spacing=0.0, order=3), RATE, 3000)
    np.testing.assert_array_equal(acc[:, 0], acc[:, 1])
    assert info["images"][0] == info["images"][1] > 300 and np.count_nonzero(acc[:, 0]) > 1000


def test_the_direct_path_is_the_shortest_image():
    for fields in ({}, dict(axis=2, spacing=0.5), dict(source=(4.9, 0.1, 2.9), receiver=(0.2, 3.9, 0.2))):
        im = ir_room_np.images(fields, RATE, 4000, N=3)
        direct = (np.abs(im["n"]).sum(axis=1) == 0) & (im["u"].sum(axis=1) == 0)
        assert direct.sum() == 1
        for ch in range(2):
            assert im["d"][direct, ch][0] < im["d"][~direct, ch].min()


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_the_lattice_is_complete_up_to_its_bound(N):
    """Every image nearer than 2 N min(L) lies inside the lattice of order N: a lattice two orders larger holds no more of them."""
    bound = 2 * N * 3.0
    inner, outer = ir_room_np.images({}, RATE, 1, N=N), ir_room_np.images({}, RATE, 1, N=N + 2)
    assert (inner["d"] < bound).sum(axis=0).tolist() == (outer["d"] < bound).sum(axis=0).tolist()
    assert (inner["d"] < bound).sum() > 8
    # and order 0 picks the smallest such N for E frames
    E = ir_room_np.complete({}, RATE, N)
    assert ir_room_np.order({}, RATE, E) == N and ir_room_np.order({}, RATE, E + 2) == N + 1


def test_reciprocity():
    """Source and receiver swapped (spacing 0): the same response, within the bar the device's taps are held to."""
    from helpers import rms

    a = dict(spacing=0.0, order=4, beta=(0.9, 0.8, 0.7, 0.95, 0.6, 0.85))
    b = dict(a, source=ir_room_np.DEFAULTS["receiver"], receiver=ir_room_np.DEFAULTS["source"])
    fa, fb = (ir_room_np.frames64(p, RATE, frames=5000, late_gain=0.0)[0] for p in (a, b))
    err = fa - fb
    print(f"reciprocity: rms err {rms(err):.3e} of {rms(fa):.3e}, max {np.abs(err).max() * 2 ** 40:.1f} quanta")
    assert rms(fa) > 1e-3
    assert rms(err) <= 1e-6 * rms(fa) and np.abs(err).max() <= 1e-5 * np.abs(fa).max()
