"""The binaural listener in the room (mc_synth_ir_room_head) without a GPU, on the restatement (tests/ir_room_head_np.py): the
closed forms of the delays and of the interaural time difference for a lateral source, the shelf's magnitudes read from the
rendered taps against |1 + h HP(e^jw)| and against Brown and Duda's figures, |h| <= 1 on every image, and the exact statements
the GPU tests rely on: no delay of their geometries lies where a rounding could move its floor."""
import numpy as np
import pytest

import ir_room_head_np
import ir_room_np
from ir_room_np import Q

RATE = 48000
CROWDED = dict(size=(4.0, 4.0, 4.0), source=(2.0, 2.0, 2.0), receiver=(2.5, 2.0, 2.0), order=8)  # test_gpu_ir_room's
ROOM_S = dict(size=(6.0, 4.0, 3.0), source=(1.5, 2.0, 1.2), receiver=(4.0, 2.0, 1.6), beta=(0.9, 0.8, 0.85, 0.85, 0.7, 0.95), spacing=0.0, axis=1, order=3)
CHAIN_ROOM = dict(gain=0.2)
# a source straight to the left of a listener who looks along +x: at the left ear's axis, and straight behind the right ear
LATERAL = dict(size=(6.0, 8.0, 3.0), source=(3.0, 6.0, 1.5), receiver=(3.0, 3.0, 1.5), beta=0.0, spacing=0.0, order=1)
GENERAL_HEAD = dict(facing=35.0, ear=100.0)
HEADS = [dict(facing=35.0), dict(ear=100.0), {}]
# every geometry the GPU tests render: (room, F, heads)
GPU_GEOMETRIES = [(dict(order=2), 4000, HEADS + [GENERAL_HEAD]), (dict(order=6), 4000, HEADS + [GENERAL_HEAD]), (CROWDED, 6000, HEADS + [GENERAL_HEAD]),
                  (ROOM_S, 3000, HEADS), (CHAIN_ROOM, 12000, HEADS + [GENERAL_HEAD]), (dict(order=3), 3000, [GENERAL_HEAD]),
                  (dict(last=3000, order=4, source=(3.0, 1.8, 1.4)), 40000, [GENERAL_HEAD]), (dict(beta=0.0, gain=2.0), 1000, [GENERAL_HEAD, dict(facing=150.0)]),
                  (LATERAL, 1000, [{}, dict(shadow=0.0)])]


def test_a_lateral_source_has_the_closed_forms():
    L, s, r, _, c, _ = ir_room_np.geometry(LATERAL)
    a, d = float(np.float32(0.0875)), 3.0
    plan = ir_room_head_np.plan(LATERAL, {}, RATE, 1000)
    print(plan)
    np.testing.assert_allclose(plan["direct"], ((d - a) * RATE / c, (d + a * np.pi / 2) * RATE / c), rtol=1e-14, atol=0)
    np.testing.assert_allclose(plan["itd"], a * (1.0 + np.pi / 2) / c, rtol=1e-12, atol=0)
    assert abs(plan["itd"] * 1e3 - 0.6558) < 5e-5 and abs(plan["itd"] * RATE - 31.48) < 5e-3
    assert plan["angle"] == (0.0, 180.0) and plan["shadow"][0] == 1.0
    np.testing.assert_allclose(plan["shadow"][1], 0.95 * np.cos(np.radians(216.0)) + 0.05, rtol=1e-14, atol=0)
    # the delay is continuous at 90 degrees and the shadow spans [-0.9, 1]
    th = np.radians(np.array([0.0, 89.999999, 90.0, 90.000001, 150.0, 180.0]))
    pos = np.stack([np.sin(th), np.cos(th), np.zeros_like(th)], axis=1)  # (from e_L = +y)
    _, g, h = ir_room_head_np.ears(pos, np.ones(len(th)), {})
    np.testing.assert_allclose(g[:, 0], [-1.0, -1.7453e-8, 0.0, 1.7453e-8, np.pi / 3, np.pi / 2], rtol=0, atol=1e-11)
    np.testing.assert_allclose(h[:, 0], [1.0, 0.95 * np.cos(1.2 * th[1]) + 0.05, 0.95 * np.cos(0.6 * np.pi) + 0.05, 0.95 * np.cos(1.2 * th[3]) + 0.05, -0.9, 0.95 * np.cos(1.2 * np.pi) + 0.05],
                               rtol=0, atol=1e-12)


def _ear_db(head, hz):
    """20 log10 of |r's spectrum / the plain accumulator's spectrum| per ear at hz, from the rendered direct sound."""
    F = 4096
    accP, accS, _, info = ir_room_head_np.render_band(LATERAL, None, head, None, 0.0, RATE, F)
    r = ir_room_head_np.highpass(accS.astype(np.float64) / Q, LATERAL, head, RATE) + accP.astype(np.float64) / Q
    w = np.exp(-2j * np.pi * np.outer(np.asarray(hz, np.float64) / RATE, np.arange(F)))
    return 20.0 * np.log10(np.abs(w @ r) / np.abs(w @ (accP.astype(np.float64) / Q))), info


def test_the_shelf_has_brown_and_dudas_magnitudes():
    hz = np.array([100.0, 10000.0])
    db, info = _ear_db({}, hz)
    print(db)
    hp = ir_room_head_np.hp_response(LATERAL, {}, RATE, hz)
    h_far = 0.95 * np.cos(np.radians(216.0)) + 0.05
    want = np.stack([20.0 * np.log10(np.abs(1.0 + hp)), 20.0 * np.log10(np.abs(1.0 + h_far * hp))], axis=1)
    # (the taps carry the formula up to the 2^-40 quantum of each of 32 taps and the recurrence's ringing cut at F)
    np.testing.assert_allclose(db, want, rtol=0, atol=1e-6)
    assert abs(want[0, 0] - 0.08) < 0.005 and abs(want[1, 0] - 5.98) < 0.005 and abs(want[1, 1] - -10.48) < 0.005
    dc = ir_room_head_np.hp_response(LATERAL, {}, RATE, 0.0)
    assert abs(dc) < 1e-15  # (unity at DC, whatever h)
    # shadow 0: nothing but the delays
    db0, _ = _ear_db(dict(shadow=0.0), hz)
    assert (db0 == 0.0).all()
    # at the darkest angle, 150 degrees, the shelf bottoms out near -20 dB at the top of the band
    worst = 20.0 * np.log10(np.abs(1.0 - 0.9 * ir_room_head_np.hp_response(LATERAL, {}, RATE, 20000.0)))
    assert -20.0 < worst < -17.0, worst


@pytest.mark.parametrize("room,F,heads", GPU_GEOMETRIES)
def test_the_gpu_geometries_keep_their_floors_and_bound_the_shadow(room, F, heads):
    for head in heads:
        im = ir_room_head_np.images(room, head, RATE, F)
        E = ir_room_np.last(room, F)
        ir_room_np.assert_floor_margin(im["tau"], E)
        shadow = ir_room_head_np.spec(**head)["shadow"]
        assert np.abs(im["h"]).max() <= shadow and im["h"].min() >= -0.9 * shadow - 1e-15
        # an ear's delay lies within the head of the centre's: at most a / c earlier and a pi / (2 c) later
        centre = ir_room_np.images(ir_room_head_np.centred(room), RATE, F, im["order"])["tau"]
        a_frames = float(np.float32(ir_room_head_np.spec(**head)["radius"])) * RATE / ir_room_np.geometry(room)[4]
        assert ((im["tau"] - centre) >= -a_frames - 1e-9).all() and ((im["tau"] - centre) <= a_frames * np.pi / 2 + 1e-9).all()  # (1e-9: the subtraction's rounding)
        if not ir_room_np.spec(**room)["order"]:
            N = im["order"]
            assert ir_room_head_np.complete(room, head, RATE, N) >= E and (N == 1 or ir_room_head_np.complete(room, head, RATE, N - 1) < E)


def test_a_mirrored_setup_has_equal_ears():
    """Room S, facing along the axis of symmetry: to the integer, for ears on the axis through the head and behind it."""
    for ear in (90.0, 100.0):
        accP, accS, _, info = ir_room_head_np.render_band(ROOM_S, None, dict(ear=ear), None, 0.0, RATE, 3000)
        assert (accP[:, 0] == accP[:, 1]).all() and (accS[:, 0] == accS[:, 1]).all() and np.count_nonzero(accS[:, 0]) > 1000
        assert info["images"][0] == info["images"][1]


def test_equal_bands_are_the_unbanded_head_and_shadow_zero_is_the_delays():
    F, room = 1500, dict(order=2)
    r, _, _ = ir_room_head_np.term(room, None, None, GENERAL_HEAD, RATE, F)
    rb, _, _ = ir_room_head_np.term(room, None, dict(xovers=(500.0, 2000.0)), GENERAL_HEAD, RATE, F)
    assert r.tobytes() == rb.tobytes()
    accP, accS, _, _ = ir_room_head_np.render_band(room, None, dict(GENERAL_HEAD, shadow=0.0), None, 0.0, RATE, F)
    r0, _, _ = ir_room_head_np.term(room, None, None, dict(GENERAL_HEAD, shadow=0.0), RATE, F)
    assert not accS.any() and r0.tobytes() == (accP.astype(np.float64) / Q).tobytes()
