"""Directional microphones and a directional source in the room (mc_synth_ir_room_mics) without a GPU: mc_ir_room_mics_plan
against the restatement (tests/ir_room_mics_np.py), and the properties of the definition on the restatement alone: omni
everywhere is the room itself to the integer, a cardioid's direct sound against the closed forms, the mirrored aim of an image
source, and the exact statements the GPU tests rely on (a figure-of-eight's null plane, equal channels of a mirrored setup)."""
import numpy as np
import pytest

import ir_room_mics_np
import ir_room_np

RATE = 48000
ROOM_Z = dict(size=(5.0, 4.0, 3.0), source=(2.5, 1.0, 1.2), receiver=(2.5, 3.0, 1.5), beta=(0.0, 0.0, 0.9, 0.9, 0.9, 0.9), spacing=0.2, axis=1, order=3)
ROOM_S = dict(size=(6.0, 4.0, 3.0), source=(1.5, 2.0, 1.2), receiver=(4.0, 2.0, 1.6), beta=(0.9, 0.8, 0.85, 0.85, 0.7, 0.95), spacing=0.0, axis=1, order=3)
GENERAL = dict(pattern=(0.5, 0.25), az=(30.0, -100.0), el=(10.0, -35.0), source_pattern=0.366, source_az=200.0, source_el=-15.0)
# (the microphones of the mirrored setups of room S: spacing, then the fields)
MIRRORED = [(0.0, dict(pattern=0.5, az=(45.0, -45.0))), (0.0, dict(pattern=0.0, az=(45.0, -45.0))),
            (0.0, dict(pattern=0.25, az=(45.0, -45.0), source_pattern=0.5, source_az=0.0)), (0.17, dict(pattern=0.5, az=(-55.0, 55.0)))]

PLAN_CASES = [({}, GENERAL, 48000, 4000), (dict(axis="y", spacing=0.3), dict(pattern="cardioid", az=(45, -45)), 44100, 3000),
              (dict(spacing=0.0), dict(pattern=("fig8", "omni"), az=90, el=(45, -45), source_pattern="hypercardioid", source_az=-170, source_el=20), 96000, 9000),
              (ROOM_Z, dict(pattern=(0.0, 1.0)), 48000, 3000), (ROOM_S, MIRRORED[2][1], 48000, 3000),
              (dict(beta=0.0), dict(pattern="supercardioid", az=(360, -360), el=(90, -90), source_pattern="subcardioid", source_az=180), 8000, 500)]


@pytest.mark.parametrize("room,mics,rate,F", PLAN_CASES)
def test_the_plan_matches_the_restatement(room, mics, rate, F):
    """A factor is a handful of double roundings of numbers of magnitude at most 1 (the library fuses the dot products' adds,
    numpy does not): 1e-14 absolute is a hundred ulp of 1."""
    from cuda_audio_amd.engine import IrRoom, IrRoomMics, room_mics_plan

    got = room_mics_plan(IrRoom(**room), IrRoomMics(**mics), rate, F)
    want = ir_room_mics_np.plan(dict(room, axis=IrRoom.AXES.get(room.get("axis", 0), room.get("axis", 0))), mics, rate, F)
    print(got, want)
    assert set(got) == set(want) == {"source", "receiver", "factor"}
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-14)
    assert max(abs(v) for k in got for v in got[k]) <= 1.0


def test_the_plan_refuses_what_the_room_plan_refuses():
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrRoom, IrRoomMics, room_mics_plan

    for room, mics, F, name in ((IrRoom(order=33), IrRoomMics(), 4000, "order"), (IrRoom(), IrRoomMics(), 0, "frames"), (IrRoom(), IrRoomMics(), 48000, "order"),
                                (IrRoom(), IrRoomMics(el=(0, 91)), 4000, "mic_el_deg[1]"), (IrRoom(), IrRoomMics(source_pattern=1.5), 4000, "src_pattern")):
        with pytest.raises(McError) as ex:
            room_mics_plan(room, mics, RATE, F)
        assert ex.value.code == -1 and name in str(ex.value)


def test_mics_without_a_room_raise():
    from cuda_audio_amd.engine import Convolution, IrRoomMics, IrSynth

    with pytest.raises(ValueError) as ex:  # (before the engine is looked at: no engine is needed to see it)
        Convolution.prepare_synth(None, 0, IrSynth(frames=100, rate=RATE), mics=IrRoomMics())
    assert "need a room" in str(ex.value)


# -- on the restatement alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("room,F", [(dict(order=2), 4000), (ROOM_Z, 3000), (dict(ROOM_S, spacing=0.17), 3000)])
def test_all_omni_is_the_room_to_the_integer(room, F):
    want, wcov, winfo = ir_room_np.render(room, RATE, F)
    got, cov, info = ir_room_mics_np.render(room, dict(az=(123.0, -77.0), el=(40.0, -80.0), source_az=211.0, source_el=33.0), RATE, F)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cov, wcov)
    assert {k: info[k] for k in winfo} == winfo
    assert info["mics"] == dict(source=(1.0, 1.0), receiver=(1.0, 1.0), factor=(1.0, 1.0)) and info["negative"] == 0.0


def test_a_cardioids_direct_sound_against_the_closed_forms():
    """Beta 0: the direct sound alone.  The source at +x of the coincident pair; a cardioid facing it has factor 1, facing away
    0, at 90 degrees 0.5, and the taps are those of the room times the factor."""
    room = dict(size=(8.0, 6.0, 3.0), source=(6.0, 3.0, 1.5), receiver=(2.0, 3.0, 1.5), spacing=0.0, beta=0.0, order=1)
    F = 1000
    plain, _, _ = ir_room_np.render(room, RATE, F)
    assert np.count_nonzero(plain[:, 0]) == 32
    for az, factor in ((0.0, 1.0), (180.0, 0.0), (90.0, 0.5), (-90.0, 0.5)):
        acc, _, info = ir_room_mics_np.render(room, dict(pattern=(0.5, 1.0), az=az), RATE, F)
        assert abs(info["mics"]["receiver"][0] - factor) <= 1e-15 and info["mics"]["factor"][1] == 1.0
        np.testing.assert_array_equal(acc[:, 1], plain[:, 1])
        assert np.abs(acc[:, 0] - factor * plain[:, 0]).max() <= 1 + 1e-15 * ir_room_np.Q  # (a quantum: the one rounding to an integer)
    # and the same for the source: a cardioid source aimed at the receivers, away from them, across
    for az, factor in ((180.0, 1.0), (0.0, 0.0), (90.0, 0.5)):
        _, _, info = ir_room_mics_np.render(room, dict(source_pattern=0.5, source_az=az), RATE, F)
        np.testing.assert_allclose(info["mics"]["source"], (factor, factor), rtol=0, atol=1e-15)
    # elevation: a cardioid pointing straight up hears the horizontal arrival at 0.5
    _, _, info = ir_room_mics_np.render(room, dict(pattern=0.5, az=0.0, el=90.0), RATE, F)
    np.testing.assert_allclose(info["mics"]["receiver"], (0.5, 0.5), rtol=0, atol=1e-15)


def test_the_image_of_a_source_aims_where_its_mirror_does():
    """One wall at beta 1 (x = 0), the others at 0: two images sound, the direct one and the mirror behind that wall.  A
    cardioid source aimed at the wall (-x), the receiver on the source's other side (+x): the direct sound leaves off axis
    (factor 0), the reflection on axis (factor 1), because the image aims along +x.  A source whose image kept the real aim
    would have it the other way round."""
    room = dict(size=(8.0, 6.0, 3.0), source=(2.0, 3.0, 1.5), receiver=(6.0, 3.0, 1.5), spacing=0.0, beta=(1.0, 0.0, 0.0, 0.0, 0.0, 0.0), order=1)
    F = 2000
    im = ir_room_np.images(room, RATE, F)
    sounding = np.flatnonzero(im["a"][:, 0] != 0.0)
    assert len(sounding) == 2
    gs, gr = ir_room_mics_np.factors(room, dict(source_pattern=0.5, source_az=180.0), im)
    for i in sounding:
        mirrored = bool(im["u"][i, 0])
        assert tuple(im["n"][i]) == (0, 0, 0) and tuple(im["u"][i, 1:]) == (0, 0)
        assert abs(gs[i, 0] - (1.0 if mirrored else 0.0)) <= 1e-15 and gr[i, 0] == 1.0
    plain, _, _ = ir_room_np.render(room, RATE, F)
    acc, _, info = ir_room_mics_np.render(room, dict(source_pattern=0.5, source_az=180.0), RATE, F)
    d0, d1 = sorted(im["tau"][sounding, 0])
    assert d1 - d0 > 64  # (the two windows do not overlap)
    k0, k1 = int(d0), int(d1)
    assert np.abs(acc[k0 - 15:k0 + 17, 0]).max() <= 1e-15 * ir_room_np.Q and np.abs(plain[k0 - 15:k0 + 17, 0]).max() > 1e-3 * ir_room_np.Q
    assert np.abs(acc[k1 - 15:k1 + 17, 0] - plain[k1 - 15:k1 + 17, 0]).max() <= 1 + 1e-15 * ir_room_np.Q
    assert abs(info["mics"]["source"][0]) <= 1e-15


def test_a_figure_of_eight_is_deaf_in_its_plane():
    """Room Z: the walls at x = 0 and x = Lx absorb everything, source and receivers share x: every image that carries
    amplitude lies at p_x = 0, in the null plane of a figure-of-eight aimed along x."""
    F = 3000
    im = ir_room_np.images(ROOM_Z, RATE, F)
    ir_room_np.assert_floor_margin(im["tau"], F)
    plain, _, pinfo = ir_room_np.render(ROOM_Z, RATE, F)
    acc, _, info = ir_room_mics_np.render(ROOM_Z, dict(pattern=(0.0, 1.0), az=0.0), RATE, F)
    assert np.count_nonzero(plain[:, 0]) == 1936 and not acc[:, 0].any()
    np.testing.assert_array_equal(acc[:, 1], plain[:, 1])
    assert info["images"] == pinfo["images"] and min(info["images"]) > 0


@pytest.mark.parametrize("spacing,mics", MIRRORED)
def test_a_mirrored_setup_has_equal_channels(spacing, mics):
    """Room S mirrors in y and so do these microphones: the definition's fixed order of operations makes the channels equal to
    the integer."""
    F = 3000
    room = dict(ROOM_S, spacing=spacing)
    ir_room_np.assert_floor_margin(ir_room_np.images(room, RATE, F)["tau"], F)
    acc, _, info = ir_room_mics_np.render(room, mics, RATE, F)
    np.testing.assert_array_equal(acc[:, 0], acc[:, 1])
    assert np.count_nonzero(acc[:, 0]) > 1000 and info["images"][0] == info["images"][1]
    assert info["mics"]["factor"][0] == info["mics"]["factor"][1]


def test_the_general_case_has_rear_lobes():
    for order in (2, 6):
        _, _, info = ir_room_mics_np.render(dict(order=order), GENERAL, RATE, 4000)
        print(order, info["negative"], info["mics"])
        assert 0.3 <= info["negative"] <= 0.5
