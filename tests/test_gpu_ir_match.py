"""The match step of an IR load on the device (mc_load_ir_match, mc_load_ir_sweep_match; csrc/irmatch.hip.h over
csrc/fft64.hip.h): the stored taps, mc_ir_match_info and mc_ir_match_curve against the float64 restatement (tests/ir_match_np.py,
numpy's FFT, one channel at a time), the windows the smoothing kernel can get wrong, the parts of the definition that are exact
(a self match, a pure delay, a silent channel, a step that is off, repeated loads), a sweep capture, and the chain with the phase
and filter steps, shape, EQ and damping into the engine's output.

The bound per tap is |got - want| <= 2^-23 |want| + 1e-12 peak, the project's bound for double pipelines (tests/test_gpu_ir_phase.py
has the reasoning): both pipelines are double and differ by parts in 1e-15 of the peak, and the rounding to float then differs by
at most one ulp, at a tie.  On the CPU the restatement itself moves by 1.8e-16 and 3.5e-16 of the peak when its window sums are
made with math.fsum instead of numpy's order, so the order in which the device adds a window's bins is three orders of magnitude
inside the bound.  `peak` is the larger channel's.  The target's right channel is different noise at a third of the left's
level, so a wrong sign at a mirrored bin shows as crosstalk.  The curve agrees to 1e-9 dB, the energies to 1e-12.
profiles/irmatch.md has what an MI355X showed: over 46 loads no stored value differed from the restatement's, so no excess over one ulp."""
import ctypes as C
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_filter_np
import ir_match_np as MN
import ir_phase_np
from helpers import BASE, RMS_TOL, apply_params, rms
from test_gpu_ir_shape import _check_taps

pytestmark = pytest.mark.gpu

RATE = 48000


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irmatch", n_ref, sample_rate=rate, **kw)


def _match(ir=None, **kw):
    from cuda_audio_amd.engine import IrMatch

    return IrMatch(ir=ir, **kw)


def _n_ref(F):
    n = 16384
    while n < F + 1024 + 1:
        n *= 2
    return n


@functools.lru_cache(maxsize=None)
def _inputs(F, G, db=60.0):
    """(coloured source frames, white target frames), made once per size and never written to."""
    a, t = MN.coloured_noise(F, 3, db=db), MN.decaying_noise(G, 12, right=1.0 / 3.0, db=db)
    a.setflags(write=False)
    t.setflags(write=False)
    return a, t


@functools.lru_cache(maxsize=None)
def _restated(F, G, flat=False, db=60.0, **kw):
    a, t = _inputs(F, G, db)
    return MN.matched(a, None if flat else t, **kw)


def _check_bound(got, want32, peak=None):
    w = want32.astype(np.float64)
    err = np.abs(got.astype(np.float64) - w)
    peak = np.abs(w).max() if peak is None else peak
    slack = err - 2.0 ** -23 * np.abs(w)
    print(f"taps: largest deviation {err.max():.3e} (peak {peak:.3e}), largest excess over one ulp {slack.max() / peak:.3e} of the peak, "
          f"{np.count_nonzero(got != want32)} of {got.size} values differ")
    assert got.shape == want32.shape
    assert (slack <= 1e-12 * peak).all(), f"excess {slack.max() / peak:.3e} of the peak at {np.unravel_index(slack.argmax(), slack.shape)}"


def _check_info(got, want):
    print("match info:", got, "restated:", want)
    for k in ("frames", "target_frames", "frames_out", "nfft", "points", "clamped"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("energy_in", "energy_target", "energy_out"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert abs(got["energy_rest"] - want["energy_rest"]) <= 1e-12 * (want["energy_out"] + want["energy_rest"])
    for c in range(2):
        assert abs(got["mean_db"][c] - want["mean_db"][c]) <= 1e-9


def _check_curve(got, want):
    # (the library's exp2 and numpy's pow may differ in the last place of f_j)
    assert got["hz"].shape == want["hz"].shape and (np.abs(got["hz"] - want["hz"]) <= 4e-16 * want["hz"]).all()
    for k in ("before_db", "gain_db"):
        dev = np.abs(got[k] - want[k]).max()
        print(f"{k}: largest deviation {dev:.3e} dB over {want[k].shape[0]} points")
        assert got[k].shape == want[k].shape and dev <= 1e-9, k


def _load_and_check(F, G, flat=False, **kw):
    """One load of the source with the target on a fresh engine: taps, info and curve against the restatement; the taps come back."""
    a, t = _inputs(F, G)
    want, winfo, wcurve = _restated(F, G, flat, **kw)
    c = _conv(_n_ref(want.shape[0]))
    c.prepare(0, a, match=_match(None if flat else t, **kw))
    got, info, curve, sinfo = c.ir_taps(0), c.ir_match_info(0), c.ir_match_curve(0), c.ir_shape_info(0)
    c.close()
    assert sinfo["frames"] == sinfo["taps"] == want.shape[0] and sinfo["gain"] == 1.0
    _check_curve(curve, wcurve)
    _check_info(info, winfo)
    _check_bound(got, want)
    return got, winfo, wcurve


# Nfft = 16 (the smallest), 2048 (the last with one pass), 4096 (the first with two), 8192 and 2^17
@pytest.mark.parametrize("F,G,nfft", [(5, 3, 16), (1000, 1024, 2048), (1025, 9, 4096), (3000, 2000, 8192), (40000, 30000, 1 << 17)])
def test_matched_taps_match_the_restatement(gpu_lib, F, G, nfft):
    assert MN.nfft_of(F, G) == nfft
    _load_and_check(F, G)


VARIANTS = [dict(link=False), dict(flat=True, tilt_db=-3.0), dict(flat=True, tilt_db=2.0, link=False), dict(phase="linear", delay=5),
            dict(phase="linear", delay=3, link=False), dict(amount=0.5, octaves=1.0, per_octave=3)]


@pytest.mark.parametrize("F,G", [(5, 3), (1000, 1024), (1025, 9), (3000, 2000)])
@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_the_variants_at_the_small_shapes(gpu_lib, F, G, kw):
    """Linked and unlinked, a target and a flat line with a tilt, minimum and linear phase with a delay."""
    _load_and_check(F, G, **kw)


def test_the_largest_transform(gpu_lib):
    """F = G = 2^21: Nfft = 2^22 = 2048 x 2048.  The shape keeps a window of 4096 of the 2^21 frames so that n_ref stays 16384;
    noise that decays by 20 dB keeps the window near the peak's level.  The widest window of the default grid is 0.23 f Nfft /
    rate = 404 thousand bins here."""
    from cuda_audio_amd.engine import IrShape

    F = G = 1 << 21
    a, t = _inputs(F, G, 20.0)
    start, length = F // 2 - 2048, 4096
    assert MN.nfft_of(F, G) == MN.MAX_NFFT
    want, winfo, wcurve = _restated(F, G, db=20.0)
    c = _conv(16384)
    c.prepare(0, a, shape=IrShape(start=start, length=length), match=_match(t))
    got, info, curve, sinfo = c.ir_taps(0), c.ir_match_info(0), c.ir_match_curve(0), c.ir_shape_info(0)
    c.close()
    assert sinfo["frames"] == F and sinfo["taps"] == length and sinfo["gain"] == 1.0
    _check_curve(curve, wcurve)
    _check_info(info, winfo)
    _check_bound(got, want[start:start + length])


# -- the curve ----------------------------------------------------------------------------------------------------------
def test_the_clamped_points(gpu_lib):
    """boost_db = cut_db = 6 on the coloured source: 24 points of the linked curve are clamped, and the nearest raw value to a
    clamp is 0.19 dB away; the channels' own curves have 33 and 39, at least 0.066 dB away: the counts are stable."""
    for link, counts, margin in ((True, (24, 24), 0.18), (False, (33, 39), 0.065)):
        _, winfo, wcurve = _load_and_check(3000, 2000, boost_db=6.0, cut_db=6.0, link=link)
        b = wcurve["before_db"]
        assert tuple(int((np.abs(b[:, ch]) > 6.0).sum()) for ch in range(2)) == counts
        assert winfo["clamped"] == (counts[0] if link else sum(counts))
        assert np.abs(np.abs(b) - 6.0).min() >= margin
        assert np.abs(wcurve["gain_db"]).max() == 6.0


def _grid_with_window(width, nfft, rate=RATE, octaves=1.0 / 3.0):
    """lo_hz (whole Hz) of a two-point grid lo, 2 lo whose first window is `width` bins wide, no edge within 1e-3 of an integer."""
    for lo in range(100, 12000):
        k_lo, k_hi, margin = MN.windows(np.array([float(lo), 2.0 * lo]), nfft, rate, octaves)
        if k_hi[0] - k_lo[0] + 1 == width and margin >= 1e-3:
            return float(lo)
    raise AssertionError(width)


WINDOWS = [("lo 1 Hz at Nfft 16", 5, 3, dict(lo=1.0, hi=24000.0)),
           ("two octaves up to rate / 2", 3000, 2000, dict(octaves=2.0, hi=24000.0)),
           ("257 bins, J = 2", 3000, 2000, (257, 1.0 / 3.0)),
           ("513 bins, J = 2", 3000, 2000, (513, 2.0 / 3.0)),
           ("J = 1024", 1000, 1024, dict(per_octave=96, lo=14.8, hi=24000.0)),
           ("a twenty-fourth of an octave", 1025, 9, dict(octaves=1.0 / 24.0, per_octave=48))]


@pytest.mark.parametrize("name,F,G,kw", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_the_windows_the_smoothing_can_get_wrong(gpu_lib, name, F, G, kw):
    """Each read through the curve against the restatement: windows that the empty-window rule puts on bin 1, windows clipped at
    Nfft / 2 (up to three quarters of the spectrum wide), a window one bin past a row of 256 lanes and one past two, two grid points
    and 1024 (96 per octave from 14.8 Hz to 24 kHz; from 20 Hz there are 982)."""
    N = MN.nfft_of(F, G)
    if isinstance(kw, tuple):
        lo = _grid_with_window(kw[0], N, octaves=kw[1])
        kw = dict(lo=lo, hi=2.0 * lo + 1.0, per_octave=1, octaves=kw[1])
    hz = MN.grid(kw.get("lo", 20.0), kw.get("hi", 20000.0), kw.get("per_octave", 12))
    k_lo, k_hi, margin = MN.windows(hz, N, RATE, kw.get("octaves", 1.0 / 3.0))
    widths = k_hi - k_lo + 1
    print(f"{name}: J {len(hz)}, windows of {widths.min()} .. {widths.max()} bins, margin {margin:.2e}")
    assert margin >= 1e-6
    if name.startswith("lo 1"):
        assert (k_hi[:100] == 1).all() and len(hz) > 170
    elif name.startswith("two"):
        assert (k_hi[-12:] == N // 2).all() and widths.max() > 0.7 * (N // 2)
    elif "bins" in name:
        assert len(hz) == 2 and widths[0] in (257, 513)
    elif name.startswith("J ="):
        assert len(hz) == 1024
    _load_and_check(F, G, link=False, boost_db=40.0, cut_db=40.0, **kw)


# -- the exact parts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [5, 2000, 40000])
def test_a_self_match_stores_the_ir_bit_for_bit(gpu_lib, F):
    """raw = 0 at every point (both spectra go through the same kernels), so C = 1 exactly; also a target four times as loud, amount 0
    with another target, and the channels' own curves."""
    a = _inputs(F, F // 2 + 1)[0]
    other = _inputs(F, F // 2 + 1)[1]
    c = _conv(_n_ref(F + 100))
    for idx, (t, kw) in enumerate(((a, {}), (a * np.float32(4.0), {}), (other, dict(amount=0.0)), (a, dict(link=False)), (a * np.float32(4.0), dict(link=False)))):
        c.prepare(idx, a, match=_match(t, **kw))
        got, curve, info = c.ir_taps(idx), c.ir_match_curve(idx), c.ir_match_info(idx)
        print(f"F {F}, {kw}: {np.count_nonzero(got != a)} of {a.size} values differ, largest gain {np.abs(curve['gain_db']).max():.3e} dB")
        assert got.tobytes() == a.tobytes(), (F, idx)
        assert not curve["gain_db"].any() and info["clamped"] == 0 and info["frames_out"] == F
        if not kw.get("amount", 1.0) == 0.0:
            assert np.abs(curve["before_db"]).max() <= 1e-12
    c.close()


def test_a_linear_phase_unit_gain_is_a_pure_delay(gpu_lib):
    """g = 1 and D = 100: the IR from frame 100 on, bit for bit, and nothing above 1e-12 of the peak before it."""
    for F in (2000, 40000):
        a = _inputs(F, F // 2 + 1)[0]
        c = _conv(_n_ref(F + 100))
        for idx, link in enumerate((True, False)):
            c.prepare(idx, a, match=_match(a, phase="linear", delay=100, link=link))
            got, info = c.ir_taps(idx), c.ir_match_info(idx)
            print(f"F {F}, link {link}: before the delay {np.abs(got[:100]).max() / np.abs(a).max():.3e} of the peak")
            assert got.shape == (F + 100, 2) and got[100:].tobytes() == a.tobytes()
            assert np.abs(got[:100]).max() <= 1e-12 * np.abs(a).max() and info["frames_out"] == F + 100
        c.close()


def test_a_silent_source_channel_stores_zeros(gpu_lib):
    a, t = (v.copy() for v in _inputs(3000, 2000))
    for channel in (0, 1):
        z = a.copy()
        z[:, channel] = 0.0
        for link in (True, False):
            want, winfo, wcurve = MN.matched(z, t, link=link)
            c = _conv(16384)
            c.prepare(0, z, match=_match(t, link=link))
            got, info, curve = c.ir_taps(0), c.ir_match_info(0), c.ir_match_curve(0)
            c.close()
            assert not got[:, channel].any() and got[:, 1 - channel].any()
            assert link or not curve["gain_db"][:, channel].any()
            _check_curve(curve, wcurve)
            _check_info(info, winfo)
            _check_bound(got, want)
    # a silent target channel: that channel's own curve is 0 dB; a silent target: the linked curve is
    z = t.copy()
    z[:, 0] = 0.0
    c = _conv(16384)
    c.prepare(0, a, match=_match(z, link=False))
    c.prepare(1, a, match=_match(np.zeros_like(t)))
    curve = c.ir_match_curve(0)
    assert not curve["gain_db"][:, 0].any() and curve["gain_db"][:, 1].any() and c.ir_taps(0)[:, 0].tobytes() == a[:, 0].tobytes()
    assert not c.ir_match_curve(1)["gain_db"].any() and c.ir_taps(1).tobytes() == a.tobytes() and c.ir_match_info(1)["energy_target"] == 0.0
    c.close()


def _off_match():
    """MC_MATCH_OFF with nonsense in every other field."""
    from cuda_audio_amd import _lib

    m = _lib.McIrMatch()
    nan = float("nan")
    m.struct_size, m.mode, m.phase, m.link, m.rate, m.per_octave, m.lo_hz, m.hi_hz, m.octaves = 7, _lib.MC_MATCH_OFF, 9, 9, 1, 0, nan, -1.0, nan
    m.amount, m.boost_db, m.cut_db, m.floor_db, m.tilt_db, m.delay = nan, nan, nan, nan, nan, 1 << 31
    m.reserved[0] = 5
    return m


def test_a_match_that_is_off_is_the_wrapped_load_bit_for_bit(gpu_lib):
    """match = None (Python and C) and MC_MATCH_OFF against prepare(filter=...) and prepare_sweep(filter=...) without one; no match
    information is left (MC_ERR_STATE)."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrFilter, IrPhase, IrShape, _fp
    from test_gpu_ir_sweep import _recorded, _sw

    ir = np.ascontiguousarray(ir_phase_np.delayed_noise(5000))
    other = np.ascontiguousarray(_inputs(3000, 300)[1])
    fields, rec = _recorded("A")
    rec = np.ascontiguousarray(rec)
    shape = IrShape(fade_out=100, normalize="peak", target=0.05)
    phase, filt = IrPhase(), IrFilter(ir=other)
    outs = []
    for how in ("without", "none", "off", "c_null", "c_off"):
        c = _conv(16384)
        L, off = c._L, _off_match()
        if how in ("without", "none", "off"):
            kw = {} if how == "without" else dict(match=None if how == "none" else _match(other, mode="off"))
            c.prepare(0, ir, ir_rate=44100, shape=shape, phase=phase, filter=filt, **kw)
            c.prepare(1, ir, **kw)
            c.prepare_sweep(2, rec, _sw(fields), offset=-64, ir_frames=1024, shape=shape, filter=filt, **kw)
        else:
            m = None if how == "c_null" else C.byref(off)
            s, p, f, sw = shape.to_c(), phase.to_c(), filt.to_c(), _sw(fields).to_c()
            sw.rate = RATE
            assert L.mc_load_ir_match(c._h, 0, _fp(ir), len(ir), 1024, 44100, RATE, C.byref(s), None, None, None, C.byref(p), C.byref(f), _fp(other), len(other),
                                      m, None, 0) == 0
            assert L.mc_load_ir_match(c._h, 1, _fp(ir), len(ir), 1024, 0, 0, None, None, None, None, None, None, None, 0, m, None, 0) == 0
            assert L.mc_load_ir_sweep_match(c._h, 2, _fp(rec), len(rec), 1024, C.byref(sw), -64, 1024, C.byref(s), None, None, None, None, C.byref(f), _fp(other),
                                            len(other), m, None, 0) == 0
        for idx in range(3):
            with pytest.raises(McError) as ex:
                c.ir_match_info(idx)
            assert ex.value.code == -3
            with pytest.raises(McError) as ex:
                c.ir_match_curve(idx)
            assert ex.value.code == -3
        assert c.ir_filter_info(0)["frames_out"] > 0 and c.ir_filter_info(2)["frames"] == 1024
        outs.append([c.ir_taps(i) for i in range(3)] + [c.ir_spectra(i) for i in range(3)] + [c.ir_info(i) for i in range(3)])
        c.close()
    for other_out in outs[1:]:
        for x, y in zip(outs[0], other_out):
            if isinstance(x, dict):
                assert x == y
            else:
                assert x.tobytes() == y.tobytes()


def test_the_same_load_stores_the_same_bits(gpu_lib):
    """Twice on one engine and once on another: one pass (F = 200) and two (F = 3000), every kernel of the step."""
    for F, G, kw in ((200, 30, dict()), (200, 30, dict(link=False)), (3000, 2000, dict()), (3000, 2000, dict(link=False)),
                     (3000, 2000, dict(phase="linear", delay=7)), (3000, 2000, dict(phase="linear", delay=7, link=False)), (3000, 2000, dict(flat=True))):
        a, t = _inputs(F, G)
        kw = dict(kw)
        target = None if kw.pop("flat", False) else t
        taps = []
        for engine in range(2):
            c = _conv(16384)
            for idx in range(2 - engine):
                c.prepare(idx, a, match=_match(target, **kw))
                taps.append((c.ir_taps(idx), c.ir_spectra(idx), c.ir_match_info(idx), c.ir_match_curve(idx)))
            c.close()
        for t_, s, i, cv in taps[1:]:
            assert t_.tobytes() == taps[0][0].tobytes() and s.tobytes() == taps[0][1].tobytes() and i == taps[0][2], (F, G, kw)
            assert all(cv[k].tobytes() == taps[0][3][k].tobytes() for k in cv)


def test_refused_loads_leave_the_engine_as_it_was(gpu_lib):
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrShape

    a, t = (np.ascontiguousarray(v) for v in _inputs(3000, 2000))
    c = _conv(16384)
    c.prepare(0, a, shape=IrShape(fade_out=100), match=_match(t))

    def state():
        cv = c.ir_match_curve(0)
        return (c.ir_taps(0).tobytes(), c.ir_spectra(0).tobytes(), c.ir_info(0), c.ir_shape_info(0), c.ir_match_info(0), cv["gain_db"].tobytes(), c.num_irs())

    before = state()
    for kw in (dict(amount=2.0), dict(hi=24001.0), dict(lo=19000.0), dict(phase="linear", delay=1 << 19), dict(octaves=3.0), dict(per_octave=0)):
        for idx in (0, 1):
            with pytest.raises(McError) as ex:
                c.prepare(idx, a, match=_match(t, **kw))
            assert ex.value.code == -1, kw
    for idx in (0, 1):
        with pytest.raises(McError) as ex:
            c.prepare(idx, a, shape=IrShape(start=6000), match=_match(t))
        assert ex.value.code == -1
    with pytest.raises(McError) as ex:
        c.ir_match_info(1)
    assert ex.value.code == -1
    assert state() == before
    # a plain load over a matched one leaves no match information behind
    c.prepare(0, a)
    for get in (c.ir_match_info, c.ir_match_curve):
        with pytest.raises(McError) as ex:
            get(0)
        assert ex.value.code == -3
    c.close()
    # an engine without a sample rate has no grid
    c = _conv(16384, rate=None)
    with pytest.raises(McError) as ex:
        c.prepare(0, a, match=_match(t))
    assert ex.value.code == -1 and "session_rate" in str(ex.value)
    c.close()


# -- with the other sources and steps ---------------------------------------------------------------------------------
def test_a_sweep_capture_with_a_match(gpu_lib):
    """prepare_sweep(match=): the step acts on the deconvolved frames, which the plain capture stores."""
    from test_gpu_ir_sweep import _recorded, _sw

    fields, rec = _recorded("A")
    F = 1024
    t = _inputs(3000, 2000)[1]
    c = _conv(16384)
    c.prepare_sweep(0, rec, _sw(fields), offset=-64, ir_frames=F)
    frames = c.ir_taps(0)
    for idx, (target, kw) in ((1, (t, dict())), (2, (None, dict(tilt_db=-3.0, link=False)))):
        want, winfo, wcurve = MN.matched(frames, target, **kw)
        c.prepare_sweep(idx, rec, _sw(fields), offset=-64, ir_frames=F, match=_match(target, **kw))
        got, info = c.ir_taps(idx), c.ir_match_info(idx)
        assert c.ir_sweep_info(idx)["frames"] == F and c.ir_shape_info(idx)["frames"] == want.shape[0]
        _check_curve(c.ir_match_curve(idx), wcurve)
        _check_info(info, winfo)
        _check_bound(got, want)
    c.close()


def test_a_target_at_another_rate(gpu_lib):
    """A target at 44.1 kHz in a 48 kHz session: the step against the restatement fed the frames that a plain resampled load of
    that target stores."""
    a, t = _inputs(3000, 2000)
    c = _conv(16384)
    c.prepare(0, t, ir_rate=44100)
    t48 = c.ir_taps(0)
    G = -(-2000 * 160 // 147)
    assert t48.shape == (G, 2)

    class Wav:
        buffer, sampleRate = t, 44100

    for idx, m in ((1, _match(t, rate=44100)), (2, _match(Wav(), link=False))):
        want, winfo, wcurve = MN.matched(a, t48, link=m.link)
        c.prepare(idx, a, match=m)
        assert c.ir_match_info(idx)["target_frames"] == G
        _check_curve(c.ir_match_curve(idx), wcurve)
        _check_info(c.ir_match_info(idx), winfo)
        _check_bound(c.ir_taps(idx), want)
    c.close()


def test_the_chain_into_the_output(oracle_mod, gpu_lib):
    """Minimum phase, the filter, the match, then a shape that normalises, damping and an EQ band: the stored taps against the
    float64 restatements chained in the documented order (1b, 1c, 1d, then 2 .. 8), and 8 periods and one batch against the oracle
    fed the restated taps."""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrFilter, IrPhase, IrShape
    from cuda_audio_amd.synth import make_input

    n_ref, F, G = 16384, 1500, 4500
    cab = ir_phase_np.delayed_noise(F)
    room = ir_filter_np.decaying_noise(G, 3, right=0.7)
    target = _inputs(3000, 2000)[1]
    xovers, decay, origin = (400, 1600), (0, 4800, 1600), 10
    bands = [("peak", 1000.0, 4.0, 1.0)]
    fields = dict(fade_out=200, normalize="peak", target=0.05)
    y32 = ir_phase_np.min_phase(cab)[0]
    z32, finfo = ir_filter_np.filtered(y32, room)
    m32, minfo, mcurve = MN.matched(z32, target)
    want, winfo, wdinfo = ir_damp_np.damp64(m32, n_ref - 1024, RATE, RATE, xovers, decay, origin, bands, **fields)
    c = _conv(n_ref, max_batch=32)
    c.prepare(0, cab, shape=IrShape(**fields), eq=IrEq(bands=bands), damp=IrDamp(xovers=xovers, decay=decay, origin=origin), phase=IrPhase(),
              filter=IrFilter(ir=room), match=_match(target))
    c.prepare(1, cab)
    got = c.ir_taps(0)
    _check_taps(got, want)
    sinfo = c.ir_shape_info(0)
    assert sinfo["frames"] == F + G - 1 and sinfo["taps"] == winfo["taps"] and abs(sinfo["gain"] - winfo["gain"]) <= 1e-6 * winfo["gain"]
    assert c.ir_damp_info(0) == wdinfo and c.ir_phase_info(0)["frames"] == F and c.ir_filter_info(0)["frames_out"] == F + G - 1
    _check_info(c.ir_match_info(0), minfo)
    _check_curve(c.ir_match_curve(0), mcurve)
    assert abs(np.abs(got).max() - 0.05) <= 1e-6 * 0.05
    taps = [want.astype(np.float32), cab[:n_ref - 1024]]
    p1 = dict(BASE, select=1, level=0.8)
    xin = make_input(40 * 256)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, t in enumerate(taps):
        ref.prepare(i, t)
    apply_params(ref, BASE, p1, True)
    out = ref.process(xin[0], xin[1])
    assert rms(out) > 0.01
    apply_params(c, BASE, p1, False)
    mine = [np.stack(c.onProcess(xin[0, k * 256:(k + 1) * 256], xin[1, k * 256:(k + 1) * 256])) for k in range(8)]
    mine.append(c.process(xin[0, 8 * 256:], xin[1, 8 * 256:]))
    c.close()
    assert rms(np.concatenate(mine, axis=1) - out) <= RMS_TOL


def test_the_single_transform_form_takes_a_match(gpu_lib):
    """It keeps no taps, but a load with the step works there: the same output as the partitioned engine's."""
    from cuda_audio_amd.synth import make_input

    a, t = _inputs(3000, 2000)
    a = a * np.float32(0.1)
    xin = make_input(16 * 256)
    outs = []
    for form in ("partitioned", "single"):
        c = _conv(16384, form=form)
        c.prepare(0, a, match=_match(t))
        assert c.ir_match_info(0)["frames_out"] == 3000 and c.ir_shape_info(0)["frames"] == 3000 and c.ir_match_curve(0)["hz"].shape == (120,)
        outs.append(np.concatenate([np.stack(c.onProcess(xin[0, k * 256:(k + 1) * 256], xin[1, k * 256:(k + 1) * 256])) for k in range(16)], axis=1))
        c.close()
    assert rms(outs[0]) > 0.005 and rms(outs[0] - outs[1]) <= RMS_TOL
