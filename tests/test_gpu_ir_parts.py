"""The parts step of an IR load on the device (mc_load_ir_parts, mc_load_ir_sweep_parts; csrc/irparts.hip.h): the stored taps and
mc_ir_parts_info against the float64 restatement (tests/ir_parts_np.py), the parts of the definition that are exact (unity
parts, a delayed tail, width 0, swapped channels, a step that is off, repeated loads), a sweep capture, the chain with the filter
step and the shape, and the boundaries that a density measurement gives.

The bound per value is |got - want| <= 2^-23 |want| + 1e-12 peak, that of tests/test_gpu_ir_filter.py: both sides are double
pipelines that differ in the cosine's last bits, so the rounding to float differs by at most one ulp, at a tie.  Energies to
1e-12 relative; counts, Fo and the clamped boundaries exactly.  The right channel is different noise at a third of the left's
level, so a crossed coefficient shows.  profiles/irparts.md has what an MI355X showed."""
import functools

import numpy as np
import pytest

import ir_filter_np
import ir_parts_np as PN
import ir_shape_np

pytestmark = pytest.mark.gpu

RATE = 48000


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irparts", n_ref, sample_rate=rate, **kw)


def _parts(**kw):
    from cuda_audio_amd.engine import IrParts

    return IrParts(**kw)


def _n_ref(F):
    n = 16384
    while n < F + 1024 + 1:
        n *= 2
    return n


@functools.lru_cache(maxsize=None)
def _input(F, seed=1):
    x = PN.noise(F, seed)
    x.setflags(write=False)
    return x


def _check_bound(got, want32):
    w = want32.astype(np.float64)
    err = np.abs(got.astype(np.float64) - w)
    peak = max(np.abs(w).max(), 1e-30)
    slack = err - 2.0 ** -23 * np.abs(w)
    print(f"taps: largest deviation {err.max():.3e} (peak {peak:.3e}), largest excess over one ulp {slack.max() / peak:.3e} of the peak, "
          f"{np.count_nonzero(got != want32)} of {got.size} values differ")
    assert got.shape == want32.shape
    assert (slack <= 1e-12 * peak).all(), f"excess {slack.max() / peak:.3e} of the peak at {np.unravel_index(slack.argmax(), slack.shape)}"


def _check_info(got, want):
    print("parts info:", got, "restated:", want)
    for k in ("frames", "frames_out", "direct_end", "early_end", "lost"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("energy_direct", "energy_early", "energy_late", "energy_out", "energy_lost"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    if want["drr_db"] is not None:
        assert abs(got["drr_db"] - want["drr_db"]) <= 1e-9


def _load_and_check(x, c=None, idx=0, **kw):
    """One load of x with the parts kw: taps and info against the restatement; (taps, restated info) come back."""
    want, winfo = PN.parted(x, **kw)
    own = c is None
    if own:
        c = _conv(_n_ref(want.shape[0]))
    c.prepare(idx, x, parts=_parts(**kw))
    got, info, sinfo = c.ir_taps(idx), c.ir_parts_info(idx), c.ir_shape_info(idx)
    if own:
        c.close()
    assert sinfo["frames"] == sinfo["taps"] == want.shape[0] and sinfo["gain"] == 1.0
    _check_bound(got, want)
    _check_info(info, winfo)
    return got, winfo


EVERYTHING = dict(delay=(0, 5, -9), gain_db=(-3.0, -4.0, 2.0), width=(1.0, 0.3, 1.7), balance=(0.0, 0.4, -0.4))


# F = 1, one workgroup less a frame, exactly one, one more, and many (the partials)
@pytest.mark.parametrize("F", [1, 255, 256, 257, 300001])
def test_the_sizes(gpu_lib, F):
    x = _input(F)
    b0, b1 = F // 10, F // 3
    xf = (min(2 * b0, 15), min(b1 - b0, 64))
    kw = dict(EVERYTHING, delay=0) if F == 1 else dict(EVERYTHING, frames_out=F - 20)  # (the late part's last 11 frames are dropped)
    _, winfo = _load_and_check(x, direct_end=b0, early_end=b1, xfade=xf, **kw)
    assert winfo["lost"] == (0 if F == 1 else 11)


# x_k = 0, 1, odd, even, in both places
@pytest.mark.parametrize("xfade", [(0, 0), (1, 1), (0, 7), (7, 0), (8, 33), (33, 8), (1, 100)])
def test_the_cross_fades(gpu_lib, xfade):
    _load_and_check(_input(700), direct_end=60, early_end=300, xfade=xfade, **EVERYTHING)


@pytest.mark.parametrize("b0,b1,xfade", [(0, 0, (0, 0)), (0, 100, (0, 9)), (0, 5, (0, 10)), (50, 700, (4, 0)), (50, 700, (4, 30)), (50, 900, (4, 30)), (700, 700, (0, 0)),
                                         (900, 1000, (6, 6)), (100, 100, (0, 0)), (100, 110, (0, 20))])
def test_the_boundaries(gpu_lib, b0, b1, xfade):
    """b_0 = 0 (with and without a fade that begins at frame 0), b_1 = F, b_1 > F, both past F, no early part, and an early part that is all cross-fade."""
    _, winfo = _load_and_check(_input(700), direct_end=b0, early_end=b1, xfade=xfade, gain_db=(-3.0, -4.0, 2.0), width=(1.0, 0.3, 1.7))
    assert (winfo["direct_end"], winfo["early_end"]) == (min(b0, 700), min(b1, 700))


def test_delays_of_both_signs(gpu_lib):
    x = _input(1000)
    layout = dict(direct_end=100, early_end=400, xfade=(10, 40))
    # the tail 150 frames early: it lands on the early part, two parts summed in one frame
    got, winfo = _load_and_check(x, delay=(0, 0, -150), gain_db=(0.0, -6.0, -2.0), **layout)
    assert winfo["frames_out"] == 850 and winfo["lost"] == 0
    # the direct part 30 frames early: its first 30 frames are dropped
    _, winfo = _load_and_check(x, delay=(-30, 0, 40), **layout)
    assert winfo["frames_out"] == 1040 and winfo["lost"] == 30 and winfo["energy_lost"] > 0
    # every part late by another amount; and a late part alone that leaves at frame 0
    _, winfo = _load_and_check(x, delay=(7, 300, 1), **layout)
    assert winfo["frames_out"] == 1001
    _, winfo = _load_and_check(x, delay=(0, 0, -380), mute=("direct", "early"), **layout)
    assert winfo["frames_out"] == 620 and winfo["lost"] == 0


def test_frames_out_shorter_and_longer_than_automatic(gpu_lib):
    x = _input(1000)
    layout = dict(direct_end=100, early_end=400, xfade=(10, 40), delay=(0, 0, 25), gain_db=(0.0, -4.0, 1.0))
    got, winfo = _load_and_check(x, frames_out=600, **layout)
    assert winfo["lost"] == 1025 - 600 and got.shape[0] == 600
    got, winfo = _load_and_check(x, frames_out=3000, **layout)
    assert winfo["lost"] == 0 and got.shape[0] == 3000 and not got[1025:].any() and got[1024].any()


@pytest.mark.parametrize("flag", ["mute", "swap", "invert"])
@pytest.mark.parametrize("part", PN.PARTS)
def test_each_flag(gpu_lib, flag, part):
    _, winfo = _load_and_check(_input(700), direct_end=60, early_end=300, xfade=(8, 33), **{flag: (part,)}, **EVERYTHING)
    assert winfo["energy_direct"] > 0 and winfo["energy_early"] > 0 and winfo["energy_late"] > 0  # (a muted part is still measured)


def test_all_flags_together(gpu_lib):
    _load_and_check(_input(700), direct_end=60, early_end=300, xfade=(8, 33), mute=("early",), swap=("direct", "late"), invert=("direct", "early", "late"), **EVERYTHING)


# -- exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [dict(), dict(direct_end=60, early_end=300, xfade=(8, 33)), dict(direct_end=120, early_end=5000, xfade=(240, 1001))])
def test_unity_parts_store_the_input(gpu_lib, layout):
    x = _input(2000)
    c = _conv(16384)
    c.prepare(0, x, parts=_parts(**layout))
    got, info = c.ir_taps(0), c.ir_parts_info(0)
    c.close()
    print(f"{layout}: {np.count_nonzero(got != x)} of {x.size} values differ")
    assert np.array_equal(got, x) and info["frames_out"] == 2000 and info["lost"] == 0


def test_a_late_part_alone_is_the_input_delayed(gpu_lib):
    x, D = _input(2000), 333
    c = _conv(16384)
    c.prepare(0, x, parts=_parts(mute=("direct", "early"), delay=(0, 0, D)))
    got = c.ir_taps(0)
    c.close()
    assert got.shape == (2000 + D, 2) and not got[:D].any() and np.array_equal(got[D:], x)


def test_width_zero_stores_equal_channels_byte_for_byte(gpu_lib):
    x = _input(2000)
    got, _ = _load_and_check(x, direct_end=60, early_end=300, xfade=(8, 33), width=0.0, gain_db=(0.0, -4.0, 3.0), delay=(0, 0, -100))
    assert got[:, 0].tobytes() == got[:, 1].tobytes() and got.any()


def test_swap_at_unity_exchanges_the_channels(gpu_lib):
    x = _input(2000)
    c = _conv(16384)
    c.prepare(0, x, parts=_parts(direct_end=60, early_end=300, xfade=(8, 33), swap=PN.PARTS))
    got = c.ir_taps(0)
    c.close()
    assert np.array_equal(got, x[:, ::-1])


def test_a_step_that_is_off_is_the_match_load_byte_for_byte(gpu_lib):
    """Through the new entry point itself, with NULL and with MC_PARTS_OFF: the match entry point's taps and spectra."""
    import ctypes as C

    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrMatch, IrShape, _fp

    x = np.ascontiguousarray(_input(2000))
    c = _conv(16384)
    L = c._L
    off = _lib.McIrParts()
    C.memset(C.byref(off), 0xA5, C.sizeof(off))
    off.mode = _lib.MC_PARTS_OFF
    for case, (shape, match) in enumerate(((None, None), (IrShape(fade_out=100), None), (IrShape(fade_out=100), IrMatch(tilt_db=-3.0)))):
        sh = C.byref(shape.to_c()) if shape is not None else None
        m = C.byref(match.to_c()) if match is not None else None
        args = (_fp(x), len(x), 1024, RATE, RATE, sh, None, None, None, None, None, None, 0, m, None, 0)
        assert L.mc_load_ir_match(c._h, 0, *args) == 0
        for idx, p in ((1, None), (2, C.byref(off))):
            assert L.mc_load_ir_parts(c._h, idx, *args, p) == 0
            assert c.ir_taps(idx).tobytes() == c.ir_taps(0).tobytes() and c.ir_spectra(idx).tobytes() == c.ir_spectra(0).tobytes(), case
            assert c.ir_info(idx) == c.ir_info(0)
            with pytest.raises(_lib.McError) as ex:
                c.ir_parts_info(idx)
            assert ex.value.code == -3
    c.close()


def test_the_same_load_stores_the_same_bytes(gpu_lib):
    """Twice on one engine and once on another: one workgroup and many."""
    for F in (200, 70001):
        x = _input(F)
        parts = _parts(direct_end=F // 10, early_end=F // 3, xfade=(8, 33), **EVERYTHING)
        outs = []
        for engine in range(2):
            c = _conv(_n_ref(F))
            for idx in range(2 - engine):
                c.prepare(idx, x, parts=parts)
                outs.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_parts_info(idx)))
            c.close()
        for t, s, i in outs[1:]:
            assert t.tobytes() == outs[0][0].tobytes() and s.tobytes() == outs[0][1].tobytes() and i == outs[0][2], F


# -- with the other sources and steps --------------------------------------------------------------------------------------
def test_a_sweep_capture_with_parts(gpu_lib):
    """prepare_sweep(parts=): the step acts on the deconvolved frames, which the plain capture stores."""
    from test_gpu_ir_sweep import _recorded, _sw

    fields, rec = _recorded("A")
    F = 1024
    kw = dict(direct_end=80, early_end=400, xfade=(16, 64), mute=("direct",), **EVERYTHING)
    c = _conv(16384)
    c.prepare_sweep(0, rec, _sw(fields), offset=-64, ir_frames=F)
    frames = c.ir_taps(0)
    want, winfo = PN.parted(frames, **kw)
    c.prepare_sweep(1, rec, _sw(fields), offset=-64, ir_frames=F, parts=_parts(**kw))
    got, info = c.ir_taps(1), c.ir_parts_info(1)
    assert c.ir_sweep_info(1)["frames"] == F and c.ir_shape_info(1)["frames"] == want.shape[0]
    c.close()
    _check_bound(got, want)
    _check_info(info, winfo)


def test_the_chain_with_the_filter_and_the_shape(gpu_lib):
    """Filter, parts with the direct part muted, then a shape that trims and normalises: the stored taps against the float64
    restatements chained in the documented order (1c, 1e, then 2 .. 8).  The trim finds the first reflection: the direct sound is
    gone when the onset search runs."""
    from cuda_audio_amd.engine import IrFilter, IrShape
    from test_gpu_ir_shape import _check_taps

    n_ref, F, G = 16384, 3000, 200
    x = np.zeros((F, 2), np.float32)
    x[40] = (0.9, 0.8)  # the direct sound
    x[500:] = PN.noise(F - 500, 5, level=0.2)  # the first reflection and what follows, 460 frames later
    b = ir_filter_np.decaying_noise(G, 2, right=1.0 / 3.0).copy()
    b[0] += np.float32(4.0)
    kw = dict(direct_end=40 + G + 20, early_end=1500, xfade=(16, 200), mute=("direct",), gain_db=(0.0, -4.0, 0.0), delay=(0, 0, 96))
    fields = dict(trim_db=-30.0, pre_roll=4, fade_out=300, normalize="peak", target=0.05)
    z32, _ = ir_filter_np.filtered(x, b)
    y32, pinfo = PN.parted(z32, **kw)
    ir_shape_np.assert_onset_margin(y32, trim_db=fields["trim_db"])
    want, winfo = ir_shape_np.shape64(y32, n_ref - 1024, **fields)
    assert winfo["onset"] >= 500  # (with the direct part it would be 40)
    c = _conv(n_ref)
    c.prepare(0, x, shape=IrShape(**fields), filter=IrFilter(ir=b), parts=_parts(**kw))
    got, sinfo, info = c.ir_taps(0), c.ir_shape_info(0), c.ir_parts_info(0)
    c.close()
    _check_taps(got, want)
    assert sinfo["frames"] == pinfo["frames_out"] == F + G - 1 + 96 and sinfo["onset"] == winfo["onset"] and sinfo["taps"] == winfo["taps"]
    assert abs(sinfo["gain"] - winfo["gain"]) <= 1e-6 * winfo["gain"]
    _check_info(info, pinfo)


def test_the_boundaries_from_a_density_measurement(gpu_lib):
    from cuda_audio_amd.engine import parts_from_density
    from ir_decay_np import noise_ir

    rate = 8000
    x = noise_ir(4000, 300, rate, 0.25, seed=7)
    c = _conv(16384, rate=rate)
    c.prepare(0, x)
    d = c.ir_density(0, half=80, hop=16)
    row = d["rows"]["LR"]
    assert row["status"] == 0 and d["origin"] == 300
    first = 11
    parts = parts_from_density(_parts(xfade=(0, 16), gain_db=(0.0, -4.0, 0.0)), d, first=first)
    assert parts.early_end == first + int(row["mix"]) and parts.direct_end == min(first + 300 + 20, parts.early_end) and parts.xfade == (0, 16)
    c.prepare(1, x, parts=parts)
    info = c.ir_parts_info(1)
    c.close()
    assert (info["direct_end"], info["early_end"]) == (parts.direct_end, parts.early_end)


def test_the_single_transform_form_takes_parts(gpu_lib):
    """It keeps no taps, but a load with the step works there: the same output as the partitioned engine's."""
    from cuda_audio_amd.synth import make_input
    from helpers import RMS_TOL, rms

    x = _input(2000) * np.float32(0.1)
    xin = make_input(16 * 256)
    outs = []
    for form in ("partitioned", "single"):
        c = _conv(16384, form=form)
        c.prepare(0, x, parts=_parts(direct_end=60, early_end=300, xfade=(8, 33), **EVERYTHING))
        assert c.ir_parts_info(0)["frames_out"] == 1991 and c.ir_shape_info(0)["frames"] == 1991
        outs.append(np.concatenate([np.stack(c.onProcess(xin[0, k * 256:(k + 1) * 256], xin[1, k * 256:(k + 1) * 256])) for k in range(16)], axis=1))
        c.close()
    assert rms(outs[0]) > 1e-3 and rms(outs[0] - outs[1]) <= RMS_TOL
