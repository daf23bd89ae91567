"""The float64 restatement of the match step (tests/ir_match_np.py): the cases that are exact, that the step does match a
coloured source to a white target, and that no window edge of the default grid lies where C++ and numpy could disagree; then
IrMatch and match_plan against the restatement's arithmetic (no GPU: the plan is host arithmetic)."""
import math

import numpy as np
import pytest

import ir_match_np as MN

RATE = 48000


# -- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 2000, 40000])
def test_the_exact_cases(F):
    """An IR matched to itself has raw = 0 at every point, so the curve, L and the cepstrum are zeros, C = 1 and y = IFFT(FFT(a)),
    which rounds to a.  A target four times as loud has raw = 10 log10(16) at every point, which the mean takes out; amount 0
    multiplies whatever the curve is by zero."""
    a = MN.decaying_noise(F, 1)
    other = MN.decaying_noise(F // 2 + 1, 2)
    for t, kw, flat_before in ((a, {}, True), (a * np.float32(4.0), {}, True), (other, dict(amount=0.0), False), (a, dict(link=False), True),
                               (a, dict(phase="linear", delay=0), True)):
        y, info, crv = MN.matched(a, t, **kw)
        assert y.shape == a.shape and y.tobytes() == a.tobytes(), (F, kw)
        assert not crv["gain_db"].any() and info["clamped"] == 0
        assert flat_before == (not crv["before_db"].any())
    D = min(100, MN.nfft_of(F, F) - F)  # (F + D <= Nfft)
    y, info, _ = MN.matched(a, a, phase="linear", delay=D)
    assert y.shape == (F + D, 2) and y[D:].tobytes() == a.tobytes() and np.abs(y[:D]).max() <= 1e-12 * np.abs(a).max()
    assert info["frames_out"] == F + D


def _distance(x, t, rate=RATE):
    """(hz, the linked smoothed level of x less that of t in dB, less its mean) on the default grid."""
    N = MN.nfft_of(max(len(x), len(t)))
    hz, sx = MN.smoothed_db(x, rate, N)
    _, st = MN.smoothed_db(t, rate, N)
    d = sx - st
    return hz, d - d.mean()


@pytest.mark.parametrize("F,G", [(3000, 2000), (40000, 30000)])
def test_the_step_matches(F, G):
    """A source coloured by 0.3 0.7^n, a white target, defaults at 48 kHz: the rms distance of the linked smoothed levels over the
    unclamped grid points above 100 Hz falls below a quarter of what it was (4.7 dB to 0.31 dB and 4.8 dB to 0.33 dB with these
    inputs).  What stays is the ripple that the interpolation between grid points and the smoothing of the result leave."""
    a, t = MN.coloured_noise(F, 1), MN.decaying_noise(G, 2)
    y, info, crv = MN.matched(a, t)
    hz, before = _distance(a, t)
    _, after = _distance(y, t)
    keep = (crv["gain_db"][:, 0] == crv["before_db"][:, 0]) & (hz > 100.0)
    r0, r1 = math.sqrt((before[keep] ** 2).mean()), math.sqrt((after[keep] ** 2).mean())
    print(f"F {F}, G {G}: {info['clamped']} clamped points, rms distance {r0:.2f} dB -> {r1:.2f} dB over {keep.sum()} points")
    assert keep.sum() >= 80 and r0 > 3.0
    assert r1 < 0.25 * r0
    # the step changes tone, not level: the curve's mean over the unclamped points is what the clamped ones took
    assert abs(crv["before_db"][:, 0].mean()) <= 1e-12


@pytest.mark.parametrize("lg", [4, 11, 12, 16, 18, 22])
def test_no_window_edge_of_the_default_grid_lies_near_an_integer(lg):
    """k_lo = ceil(..) and k_hi = floor(..) are made in C++ and here from the same doubles, with exp2 and pow that may differ in
    the last place; an edge within a rounding error of an integer (or the centre of an empty window within one of a half) could
    fall on different bins.  None is nearer than 1e-2; 1e-6 is a million times what the arithmetic can lose."""
    hz = MN.grid(20.0, 20000.0, 12)
    k_lo, k_hi, margin = MN.windows(hz, 1 << lg, RATE)
    print(f"Nfft 2^{lg}: margin {margin:.3e}, widest window {int((k_hi - k_lo).max()) + 1} bins")
    assert len(hz) == 120 and margin >= 1e-6
    assert (k_lo >= 1).all() and (k_hi <= (1 << lg) // 2).all() and (k_lo <= k_hi).all()


def test_the_windows_at_the_edges():
    # lo 1 Hz at Nfft 16: every point below the first bin's reach falls on bin 1 through the empty-window rule
    hz = MN.grid(1.0, 24000.0, 12)
    k_lo, k_hi, _ = MN.windows(hz, 16, RATE)
    assert (k_lo[:100] == 1).all() and (k_hi[:100] == 1).all() and k_hi[-1] == 8
    # two octaves at rate / 2: clipped at Nfft / 2
    hz = MN.grid(20.0, 24000.0, 12)
    k_lo, k_hi, _ = MN.windows(hz, 4096, RATE, 2.0)
    assert k_hi[-1] == 2048 and k_lo[-1] == math.ceil(hz[-1] * 0.5 * 4096 / RATE) and (k_hi[-12:] == 2048).all()


def test_a_silent_channel_and_a_silent_target():
    a, t = MN.coloured_noise(500, 1).copy(), MN.decaying_noise(300, 2).copy()
    a[:, 1] = 0.0
    for link in (True, False):
        y, info, crv = MN.matched(a, t, link=link)
        assert not y[:, 1].any() and y[:, 0].any()
        assert crv["gain_db"][:, 0].any() and (link or not crv["gain_db"][:, 1].any())
    t[:, 0] = 0.0
    y, info, crv = MN.matched(MN.coloured_noise(500, 1), t, link=False)
    assert not crv["gain_db"][:, 0].any() and crv["gain_db"][:, 1].any()
    y, info, crv = MN.matched(MN.coloured_noise(500, 1), np.zeros((300, 2), np.float32))
    assert not crv["gain_db"].any() and info["energy_target"] == 0.0


def test_flat_and_tilted_targets():
    """A flat target whitens: the matched source's smoothed level is level within the ripple; a tilt of -3 dB per octave leaves that slope."""
    a = MN.coloured_noise(3000, 1)
    for tilt in (0.0, -3.0):
        y, info, crv = MN.matched(a, None, tilt_db=tilt, boost_db=30.0, cut_db=30.0)
        assert info["target_frames"] == 0 and info["clamped"] == 0
        hz, s = MN.smoothed_db(y)
        keep = hz > 200.0
        slope = np.polyfit(np.log2(hz[keep]), s[keep], 1)[0]
        print(f"tilt {tilt}: slope {slope:.2f} dB per octave")
        assert abs(slope - tilt) <= 0.25


# -- Python and the plan ----------------------------------------------------------------------------------------------
def test_the_python_dataclass():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrMatch

    ir = np.zeros((5, 2), np.float32)
    m = IrMatch().to_c()
    assert (m.struct_size, m.mode, m.phase, m.link, m.rate, m.per_octave, m.lo_hz, m.hi_hz, m.octaves) == (80, _lib.MC_MATCH_FLAT, 0, 1, 0, 12, 20.0, 0.0, 1.0 / 3.0)
    assert (m.amount, m.boost_db, m.cut_db, m.floor_db, m.tilt_db, m.delay, list(m.reserved)) == (1.0, 12.0, 24.0, 120.0, 0.0, 0, [0, 0])
    m = IrMatch(ir=ir, rate=44100, lo=30, hi=16000, per_octave=24, octaves=0.5, amount=0.5, boost_db=6, cut_db=9, link=False, phase="linear", delay=64,
                tilt_db=-3).to_c()
    assert (m.mode, m.phase, m.link, m.rate, m.per_octave, m.lo_hz, m.hi_hz, m.octaves) == (_lib.MC_MATCH_TARGET, 1, 0, 44100, 24, 30.0, 16000.0, 0.5)
    assert (m.amount, m.boost_db, m.cut_db, m.tilt_db, m.delay) == (0.5, 6.0, 9.0, -3.0, 64)
    assert IrMatch(ir=ir, mode="off").to_c().mode == _lib.MC_MATCH_OFF and not IrMatch(mode="off").on() and IrMatch().on()

    class Wav:
        buffer, sampleRate = ir, 96000

    assert IrMatch(ir=Wav()).to_c().rate == 96000 and IrMatch(ir=Wav(), rate=48000).to_c().rate == 48000
    assert IrMatch(ir=Wav()).frames().shape == (5, 2) and IrMatch().frames() is None
    for bad in (dict(phase="maximum"), dict(mode="on")):
        with pytest.raises(ValueError):
            IrMatch(ir=ir, **bad).to_c()


def test_the_plan():
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrMatch, match_plan

    for F, G in ((5, 3), (8, 8), (9, 1), (1000, 1024), (1025, 9), (3000, 2000), (40000, 30000), (1 << 21, 1 << 21), (7, 1 << 21)):
        for kw in (dict(), dict(phase="linear", delay=3), dict(per_octave=96, hi=24000, octaves=2.0)):
            N = MN.nfft_of(F, G)
            hz = MN.grid(20.0, float(kw.get("hi", 20000)), kw.get("per_octave", 12))
            k_lo, k_hi, _ = MN.windows(hz, N, RATE, kw.get("octaves", 1.0 / 3.0))
            got = match_plan(IrMatch(ir=np.zeros((1, 2), np.float32), **kw), F, G, RATE)
            passes, J, rows = (1 if N <= 2048 else 2), len(hz), (N // 2 + 1 + 255) // 256
            assert got == dict(nfft=N, passes=passes, frames_out=F + kw.get("delay", 0), points=J, window_bins=int((k_hi - k_lo + 1).sum()),
                               device_bytes=8 * G + (passes + 1) * 16 * N + 2 * 16 * 256 * rows + 16 * ((N + 255) // 256) + 56 * J), (F, G, kw, got)
    # a flat target has no frames; a target at another rate is planned over its frames at the session's: ceil(441 * 160 / 147) = 480
    assert match_plan(IrMatch(), 100, 1 << 30)["nfft"] == 256
    assert match_plan(IrMatch(ir=np.zeros((441, 2), np.float32), rate=44100), 100, rate=48000)["nfft"] == 1024
    assert match_plan(IrMatch(ir=np.zeros((441, 2), np.float32), rate=44100), 100, rate=44100)["nfft"] == 1024
    assert match_plan(IrMatch(), 100, rate=32000)["points"] == len(MN.grid(20.0, 16000.0, 12))  # (hi defaults to half the rate)
    assert match_plan(IrMatch(per_octave=96, hi=24000), 100)["points"] == len(MN.grid(20.0, 24000.0, 96)) == 982
    assert match_plan(IrMatch(per_octave=96, lo=17, hi=24000), 100)["points"] == len(MN.grid(17.0, 24000.0, 96)) <= 1024
    for kw, F, G, name in ((dict(), (1 << 21) + 1, 1, "transform"), (dict(), 1, (1 << 21) + 1, "transform"), (dict(hi=24001), 100, 100, "hi_hz"),
                           (dict(lo=19000), 100, 100, "grid"), (dict(lo=1, per_octave=96, hi=24000), 100, 100, "grid"),
                           (dict(phase="linear", delay=157), 100, 100, "delay"), (dict(), 100, 0, "target_frames"), (dict(), 0, 100, "empty IR")):
        with pytest.raises(McError) as ex:
            match_plan(IrMatch(ir=np.zeros((1, 2), np.float32), **kw), F, G, RATE)
        assert ex.value.code == -1 and name in str(ex.value), (kw, str(ex.value))
    assert match_plan(IrMatch(ir=np.zeros((1, 2), np.float32), phase="linear", delay=156), 100, 100)["frames_out"] == 256
