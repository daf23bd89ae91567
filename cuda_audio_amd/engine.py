"""Python host mirror of the reference's `Convolution` class (src/conv.h:30-86)
over the C ABI of include/mcconv.h.

Same names and argument meaning as the reference for the hot-path surface:
`Convolution(name, fftSize)`, `cc[i].value.*`, `prepare(idx, wav, nframes=1024)`,
`onProcess`, `onMidiMessage`, `avgRuntime()`.  JACK port plumbing is replaced
by explicit buffers: `onProcess(in1, in2)` takes the two capture buffers and
returns the two playback buffers.  All arithmetic runs in libmcconv.so (HIP);
there is no CPU path here.
"""
import ctypes as C
import dataclasses
import math
import weakref

import numpy as np

from . import _lib
from ._lib import (MC_BLOCK, McCcValue, McConfig, McDecayQuery, McDensityQuery, McFloorQuery, McIaccQuery, McStiQuery, McResponseQuery, McResponseWindow, McIrDamp, McIrEq, McIrPlate, McIrSpring, McIrRoom, McIrRoomBands, McIrRoomHead, McIrRoomMics, McIrFilter, McIrMatch, McIrPhase, McIrShape, McIrSynth, McIrTail, McKernelStats, McSweep,
                   check)

CONV_DEFAULT_FFTSIZE = 512 * 256  # conv.h:10-12
CONV_MAX_SPEED = 1024             # conv.h:22-24
CONV_MAX_PREDELAY = 8192          # conv.h:26-28


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@dataclasses.dataclass
class IrShape:
    """What prepare(shape=...) does to an IR before it is truncated and transformed (mc_ir_shape, include/mcconv.h).
    Lengths and positions are frames at the session's rate; the defaults switch everything off."""

    start: int = 0          # frames skipped unconditionally at the front
    trim_db: float = 0.0    # [-120, 0]; < 0: the onset is the first frame within trim_db of the peak
    pre_roll: int = 0       # frames kept before the onset
    length: int = 0         # frames kept from there; 0 = all
    reverse: bool = False
    decay_t60: int = 0      # 0 = off; else a further 60 dB of exponential decay at tap decay_t60
    fade_out: int = 0       # raised-cosine fade over the last fade_out stored taps
    normalize: str = None   # "peak", "energy" or None
    target: float = 1.0     # peak: max |tap|; energy: sqrt(sum (hL^2 + hR^2) / 2)

    def to_c(self):
        norm = {None: _lib.MC_NORM_NONE, "peak": _lib.MC_NORM_PEAK, "energy": _lib.MC_NORM_ENERGY}
        if self.normalize not in norm:
            raise ValueError(f"normalize must be 'peak', 'energy' or None, not {self.normalize!r}")
        s = McIrShape()
        _lib.load().mc_default_ir_shape(C.byref(s))
        s.flags = _lib.MC_SHAPE_REVERSE if self.reverse else 0
        s.start, s.trim_db, s.pre_roll, s.length = int(self.start), float(self.trim_db), int(self.pre_roll), int(self.length)
        s.decay_t60, s.fade_out, s.normalize, s.target = int(self.decay_t60), int(self.fade_out), norm[self.normalize], float(self.target)
        return s


@dataclasses.dataclass
class IrEq:
    """What prepare(eq=...) filters an IR with after shaping and before the normalisation (mc_ir_eq, include/mcconv.h): up to
    8 bands in order, each `(kind, hz[, gain_db[, q]])` with kind one of "off", "lowcut", "highcut", "lowshelf", "highshelf",
    "peak"; gain_db defaults to 0 (the cuts ignore it), q to 0.70710678."""

    bands: list = dataclasses.field(default_factory=list)

    KINDS = {"off": _lib.MC_EQ_OFF, "lowcut": _lib.MC_EQ_LOWCUT, "highcut": _lib.MC_EQ_HIGHCUT, "lowshelf": _lib.MC_EQ_LOWSHELF,
             "highshelf": _lib.MC_EQ_HIGHSHELF, "peak": _lib.MC_EQ_PEAK}

    def to_c(self):
        if len(self.bands) > _lib.MC_EQ_MAX_BANDS:
            raise ValueError(f"{len(self.bands)} bands; at most {_lib.MC_EQ_MAX_BANDS}")
        eq = McIrEq()
        _lib.load().mc_default_ir_eq(C.byref(eq))
        for b, band in zip(eq.band, self.bands):
            kind, hz, *rest = band
            if kind not in self.KINDS or len(rest) > 2:
                raise ValueError(f"a band is (kind, hz[, gain_db[, q]]) with kind in {sorted(self.KINDS)}, not {band!r}")
            b.kind, b.freq_hz = self.KINDS[kind], float(hz)
            if len(rest) > 0:
                b.gain_db = float(rest[0])
            if len(rest) > 1:
                b.q = float(rest[1])
        return eq


def eq_response(eq, rate, hz):
    """|H| in dB of the bands of `eq` (an IrEq) at the frequencies hz (Hz) in a session at `rate` Hz: mc_ir_eq_response, host
    arithmetic only."""
    hz = np.ascontiguousarray(hz, dtype=np.float64).reshape(-1)
    db = np.empty_like(hz)
    dp = C.POINTER(C.c_double)
    check(_lib.load().mc_ir_eq_response(C.byref(eq.to_c()), int(rate), hz.ctypes.data_as(dp), hz.size, db.ctypes.data_as(dp)))
    return db


@dataclasses.dataclass
class IrDamp:
    """What prepare(damp=...) damps an IR with after the fade and before the EQ (mc_ir_damp, include/mcconv.h): 1 to 3 crossover
    frequencies (Hz, ascending) and one decay per band, low to high, len(xovers) + 1 of them: a further 60 dB at `decay`
    taps past `origin` (frames at the session's rate; 0 = that band is left alone).  No crossover switches damping off."""

    xovers: tuple = (400, 1600)
    decay: tuple = (0, 4800, 1600)
    origin: int = 0

    def to_c(self):
        if len(self.xovers) > _lib.MC_DAMP_MAX_XOVERS:
            raise ValueError(f"{len(self.xovers)} crossovers; at most {_lib.MC_DAMP_MAX_XOVERS}")
        if self.xovers and len(self.decay) != len(self.xovers) + 1:
            raise ValueError(f"{len(self.xovers)} crossovers make {len(self.xovers) + 1} bands, not {len(self.decay)} decays")
        d = McIrDamp()
        _lib.load().mc_default_ir_damp(C.byref(d))
        d.n_xovers = len(self.xovers)
        for k, hz in enumerate(self.xovers):
            d.xover_hz[k] = float(hz)
        if self.xovers:
            for j, t60 in enumerate(self.decay):
                d.decay_t60[j] = int(t60)
        d.origin = int(self.origin)
        return d


def damp_response(damp, rate, tap, hz):
    """The quasi-static response in dB of `damp` (an IrDamp) at stored tap `tap` and the frequencies hz (Hz) in a session at
    `rate` Hz: mc_ir_damp_response, host arithmetic only."""
    hz = np.ascontiguousarray(hz, dtype=np.float64).reshape(-1)
    db = np.empty_like(hz)
    dp = C.POINTER(C.c_double)
    check(_lib.load().mc_ir_damp_response(C.byref(damp.to_c()), int(rate), int(tap), hz.ctypes.data_as(dp), hz.size, db.ctypes.data_as(dp)))
    return db


@dataclasses.dataclass
class DecayQuery:
    """What ir_decay measures (mc_decay_query, include/mcconv.h): the broadband row and one row per centre frequency of `bands`
    (two band-pass sections of quality q each), time zero at the first tap within onset_db of the peak (0: tap 0), over taps
    [0, end) (0: all), with curve_points points of every row's decay curve."""

    rate: int = 44100
    bands: tuple = ()
    q: float = None          # None: the library's default, sqrt 2 (one octave)
    onset_db: float = -20.0
    end: int = 0
    curve_points: int = 0

    def to_c(self):
        if len(self.bands) > _lib.MC_DECAY_MAX_BANDS:
            raise ValueError(f"{len(self.bands)} bands; at most {_lib.MC_DECAY_MAX_BANDS}")
        d = McDecayQuery()
        _lib.load().mc_default_decay_query(C.byref(d))
        d.rate, d.n_bands, d.curve_points = int(self.rate), len(self.bands), int(self.curve_points)
        for k, hz in enumerate(self.bands):
            d.centre_hz[k] = float(hz)
        if self.q is not None:
            d.q = float(self.q)
        d.onset_db, d.end = float(self.onset_db), int(self.end)
        return d


@dataclasses.dataclass
class FloorQuery:
    """How ir_floor searches a loaded IR for its noise floor (mc_floor_query, include/mcconv.h has Lundeby's method as it is
    implemented): the broadband rows and, with 1 to 3 crossover frequencies (Hz, ascending), one row group per band of
    IrDamp's split; time zero and `end` as in DecayQuery; `window` the first averaging interval in taps (0: 30 ms);
    tail_fraction the last share of the taps that always counts as noise; margin_db how far above the noise the decay is cut;
    span_db the range above that which the late slope is fitted over; per_decade the intervals per 10 dB of decay; rounds the
    iterations, which always all run."""

    rate: int = 44100
    xovers: tuple = ()
    onset_db: float = -20.0
    end: int = 0
    window: int = 0
    tail_fraction: float = 0.1
    margin_db: float = 10.0
    span_db: float = 20.0
    per_decade: int = 5
    rounds: int = 5

    def to_c(self):
        if len(self.xovers) > _lib.MC_FLOOR_MAX_XOVERS:
            raise ValueError(f"{len(self.xovers)} crossovers; at most {_lib.MC_FLOOR_MAX_XOVERS}")
        q = McFloorQuery()
        _lib.load().mc_default_floor_query(C.byref(q))
        q.rate, q.n_xovers, q.window, q.end = int(self.rate), len(self.xovers), int(self.window), int(self.end)
        for k, hz in enumerate(self.xovers):
            q.xover_hz[k] = float(hz)
        q.onset_db, q.tail_fraction, q.margin_db, q.span_db = float(self.onset_db), float(self.tail_fraction), float(self.margin_db), float(self.span_db)
        q.per_decade, q.rounds = int(self.per_decade), int(self.rounds)
        return q


@dataclasses.dataclass
class DensityQuery:
    """How ir_density measures a loaded IR's echo density (mc_density_query, include/mcconv.h has the definition): a raised-cosine
    window of 2 half + 1 taps (0: 20 ms in all) every hop taps (0: a quarter of half); time zero and `end` as in DecayQuery;
    the mixing time is where the density first reaches `threshold`; decay_t60 (taps per 60 dB, 0: off) is the decay undone
    inside each window, ir_decay's t30 times the rate."""

    rate: int = 44100
    half: int = 0
    hop: int = 0
    onset_db: float = -20.0
    threshold: float = 1.0
    end: int = 0
    decay_t60: int = 0

    def to_c(self):
        q = McDensityQuery()
        _lib.load().mc_default_density_query(C.byref(q))
        q.rate, q.half, q.hop, q.end, q.decay_t60 = int(self.rate), int(self.half), int(self.hop), int(self.end), int(self.decay_t60)
        q.onset_db, q.threshold = float(self.onset_db), float(self.threshold)
        return q


def density_of_occupancy(p):
    """The normalised echo density of IrSynth's late field where its occupancy is p, 0 < p <= 1:
    p erfc(sqrt(p / 2)) / erfc(1 / sqrt 2).

    A frame of the late field sounds with probability p and is then a Gaussian g scaled by 1 / sqrt p, so the field's
    variance is p (1 / p) = 1 whatever p is and sigma = 1.  A sounding frame exceeds sigma exactly when |g| / sqrt p > 1, that is
    |g| > sqrt p, which a Gaussian does with probability erfc(sqrt(p / 2)); a silent frame never does.  The share of frames
    beyond sigma is therefore p erfc(sqrt(p / 2)), and the density divides it by the Gaussian share erfc(1 / sqrt 2): 1 at p = 1,
    0.158 at the floor p = 1 / 16 where a build-up starts."""
    p = float(p)
    return p * math.erfc(math.sqrt(p / 2.0)) / math.erfc(math.sqrt(1.0 / 2.0))  # (the same expression at p = 1: exactly 1)


@dataclasses.dataclass
class IrTail:
    """What prepare(tail=...) and prepare_sweep(tail=...) do to the tail of an IR before anything else sees it (mc_ir_tail,
    include/mcconv.h): mode "cut" fades every band to nothing at its knee, "extend" cross-fades it there into decaying noise,
    "off" does nothing.  0 to 3 crossover frequencies (Hz, ascending) make len(xovers) + 1 bands, low to high, each with a
    `knee` (a frame at the session's rate; None leaves the band alone) and, to extend, a `t60` (frames in which the noise
    falls 60 dB) and a `level_db` pair (10 log10 of the band's power per frame at the knee, left and right).  `fade` frames
    of cross-fade end at the knee; `length` is the number of frames the step hands on (0: as many as came in); seed and width
    are IrSynth's.  tail_from_floor fills the bands from ir_floor's result."""

    mode: str = "extend"
    xovers: tuple = ()
    knee: tuple = (None,)
    t60: tuple = (1,)
    level_db: tuple = ((0.0, 0.0),)
    fade: int = 0
    length: int = 0
    seed: int = 0
    width: float = 1.0

    MODES = {"off": _lib.MC_TAIL_OFF, "cut": _lib.MC_TAIL_CUT, "extend": _lib.MC_TAIL_EXTEND}

    def to_c(self):
        if self.mode not in self.MODES:
            raise ValueError(f"mode must be one of {sorted(self.MODES)}, not {self.mode!r}")
        if len(self.xovers) > _lib.MC_DAMP_MAX_XOVERS:
            raise ValueError(f"{len(self.xovers)} crossovers; at most {_lib.MC_DAMP_MAX_XOVERS}")
        bands = len(self.xovers) + 1
        if len(self.knee) != bands:
            raise ValueError(f"{len(self.xovers)} crossovers make {bands} bands, not {len(self.knee)} knees")
        t = McIrTail()
        _lib.load().mc_default_ir_tail(C.byref(t))
        t.mode, t.n_xovers, t.fade, t.width, t.seed, t.length = self.MODES[self.mode], len(self.xovers), int(self.fade), float(self.width), int(self.seed), int(self.length)
        for k, hz in enumerate(self.xovers):
            t.xover_hz[k] = float(hz)
        for j, k in enumerate(self.knee):
            t.knee[j] = _lib.MC_TAIL_LEFT_ALONE if k is None else int(k)
        for j, v in enumerate(self.t60[:bands]):
            t.t60[j] = int(v)
        for j, pair in enumerate(self.level_db[:bands]):
            t.level_db[j][0], t.level_db[j][1] = float(pair[0]), float(pair[1])
        return t


@dataclasses.dataclass
class IrPhase:
    """What prepare(phase=...) and prepare_sweep(phase=...) do to the phase of an IR after the conversion and the tail step and
    before everything else (mc_ir_phase, include/mcconv.h): mode "minimum" replaces the frames by the minimum-phase IR of the
    same magnitude response, which takes out the delay an IR carries inside it (for short IRs: cabinets, equaliser captures);
    "off" does nothing.  floor_db (40 .. 300) bounds how far below its largest bin the spectrum is followed; oversample (a
    power of two, 2 .. 64) is the transform's length over the IR's, rounded up to a power of two."""

    mode: str = "minimum"
    floor_db: float = 120.0
    oversample: int = 8

    MODES = {"off": _lib.MC_PHASE_OFF, "minimum": _lib.MC_PHASE_MINIMUM}

    def to_c(self):
        if self.mode not in self.MODES:
            raise ValueError(f"mode must be one of {sorted(self.MODES)}, not {self.mode!r}")
        over = int(self.oversample)
        if over < 2 or over > 64 or over & (over - 1):
            raise ValueError(f"oversample must be a power of two from 2 to 64, not {self.oversample!r}")
        p = McIrPhase()
        _lib.load().mc_default_ir_phase(C.byref(p))
        p.mode, p.floor_db, p.over_log2 = self.MODES[self.mode], float(self.floor_db), over.bit_length() - 1
        return p


def phase_plan(phase, frames):
    """What the phase step `phase` (an IrPhase) would do to `frames` frames at the session's rate (mc_ir_phase_plan, host
    arithmetic only): the transform's length, its passes and the device memory the step needs while it runs.  McError for
    frames or an oversampling beyond the step's limits (2^21 frames, a transform of 2^22 points)."""
    out = (C.c_double * 4)()
    check(_lib.load().mc_ir_phase_plan(C.byref(phase.to_c()), int(frames), out))
    return dict(nfft=int(out[0]), passes=int(out[1]), device_bytes=int(out[2]))


@dataclasses.dataclass
class IrFilter:
    """A second impulse response that prepare(filter=...) and prepare_sweep(filter=...) combine with the IR after the phase step
    and before everything else (mc_ir_filter, include/mcconv.h).  ir: float32 [frames, 2], or an object with such a `.buffer`
    (and a `.sampleRate`, which rate then defaults to).  op "convolve" cascades the two, so that the engine runs one IR; op
    "deconvolve" divides the filter out of the IR (a loop-back capture out of a measurement), regularised reg_db (20 .. 200)
    below the filter's strongest bin; "off" does nothing.  channels: "stereo" (left with left, right with right), "left" or
    "mid" ((L + R) / 2): one filter signal for both channels.  rate (Hz; None or 0 = the session's): the filter is converted
    to the session's rate on the device first.  frames_out: the frames the step hands on; 0 = all of a convolution, as many
    as went in of a deconvolution."""

    ir: object = None
    op: str = "convolve"
    channels: str = "stereo"
    rate: object = None
    reg_db: float = 60.0
    frames_out: int = 0

    OPS = {"off": _lib.MC_FILTER_OFF, "convolve": _lib.MC_FILTER_CONVOLVE, "deconvolve": _lib.MC_FILTER_DECONVOLVE}
    CHANNELS = {"stereo": _lib.MC_FILTER_STEREO, "left": _lib.MC_FILTER_LEFT, "mid": _lib.MC_FILTER_MID}

    def to_c(self):
        if self.op not in self.OPS:
            raise ValueError(f"op must be one of {sorted(self.OPS)}, not {self.op!r}")
        if self.channels not in self.CHANNELS:
            raise ValueError(f"channels must be one of {sorted(self.CHANNELS)}, not {self.channels!r}")
        rate = self.rate if self.rate is not None else getattr(self.ir, "sampleRate", None)
        f = McIrFilter()
        _lib.load().mc_default_ir_filter(C.byref(f))
        f.op, f.channels, f.rate, f.reg_db, f.frames_out = self.OPS[self.op], self.CHANNELS[self.channels], int(rate or 0), float(self.reg_db), int(self.frames_out)
        return f

    def frames(self):
        """The filter's frames as the library takes them: contiguous float32 [G, 2]."""
        if self.ir is None:
            raise ValueError("an IrFilter needs its ir")
        return _f32(getattr(self.ir, "buffer", self.ir)).reshape(-1, 2)


def filter_plan(filter, frames, session_rate=None):
    """What the filter step `filter` (an IrFilter with its ir) would do to `frames` frames at the session's rate
    (mc_ir_filter_plan, host arithmetic only): the transform's length, its passes, the device memory the step needs while it
    runs and the frames it hands on.  session_rate: needed when the filter has a rate of its own, for its length after the
    conversion.  McError for lengths beyond the step's limits (a transform of 2^22 points)."""
    f = filter.to_c()
    G = filter.frames().shape[0]
    if f.rate and session_rate and int(session_rate) != f.rate:
        g = math.gcd(int(session_rate), f.rate)
        G = -(-G * (int(session_rate) // g) // (f.rate // g))
    out = (C.c_double * 4)()
    check(_lib.load().mc_ir_filter_plan(C.byref(f), int(frames), G, out))
    return dict(nfft=int(out[0]), passes=int(out[1]), device_bytes=int(out[2]), frames_out=int(out[3]))


@dataclasses.dataclass
class IrMatch:
    """A match EQ that prepare(match=...) and prepare_sweep(match=...) apply to the IR after the filter step and before
    everything else (mc_ir_match, include/mcconv.h): the IR gets the smoothed spectrum of the target `ir` (float32 [frames, 2],
    or an object with such a `.buffer` and a `.sampleRate`, which rate then defaults to), or with ir=None of a flat line that
    tilts by tilt_db per octave (0 whitens, -3 aims at pink).  rate (Hz; None or 0 = the session's): the target is converted
    to the session's rate on the device first.  The spectra are compared at per_octave points per octave from lo to hi Hz
    (hi None: min(20000, half the session's rate)), each the mean power over `octaves` octaves; the difference, less its
    mean, times amount, is bounded to [-cut_db, boost_db] and applied as a minimum-phase correction, or with phase="linear"
    as a linear-phase one that delays the IR by `delay` frames.  link: one curve from the sum of both channels, which keeps
    the stereo balance; False gives each channel a curve of its own.  floor_db: how far below its largest level a smoothed
    spectrum is floored.  mode "off" does nothing."""

    ir: object = None
    rate: object = None
    lo: float = 20.0
    hi: object = None
    per_octave: int = 12
    octaves: float = 1.0 / 3.0
    amount: float = 1.0
    boost_db: float = 12.0
    cut_db: float = 24.0
    link: bool = True
    phase: str = "minimum"
    delay: int = 0
    tilt_db: float = 0.0
    floor_db: float = 120.0
    mode: object = None

    PHASES = {"minimum": _lib.MC_MATCH_MINIMUM, "linear": _lib.MC_MATCH_LINEAR}
    MODES = {"off": _lib.MC_MATCH_OFF, "target": _lib.MC_MATCH_TARGET, "flat": _lib.MC_MATCH_FLAT}

    def on(self):
        return self.mode != "off"

    def to_c(self):
        if self.phase not in self.PHASES:
            raise ValueError(f"phase must be one of {sorted(self.PHASES)}, not {self.phase!r}")
        mode = self.mode if self.mode is not None else ("flat" if self.ir is None else "target")
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {sorted(self.MODES)}, not {mode!r}")
        rate = self.rate if self.rate is not None else getattr(self.ir, "sampleRate", None)
        m = McIrMatch()
        _lib.load().mc_default_ir_match(C.byref(m))
        m.mode, m.phase, m.link, m.rate, m.per_octave = self.MODES[mode], self.PHASES[self.phase], int(bool(self.link)), int(rate or 0), int(self.per_octave)
        m.lo_hz, m.hi_hz, m.octaves = float(self.lo), float(self.hi or 0.0), float(self.octaves)
        m.amount, m.boost_db, m.cut_db, m.floor_db, m.tilt_db, m.delay = (float(self.amount), float(self.boost_db), float(self.cut_db), float(self.floor_db),
                                                                       float(self.tilt_db), int(self.delay))
        return m

    def frames(self):
        """The target's frames as the library takes them: contiguous float32 [G, 2]; None for a flat target."""
        if self.ir is None:
            return None
        return _f32(getattr(self.ir, "buffer", self.ir)).reshape(-1, 2)


def match_plan(match, frames, target_frames=None, rate=48000):
    """What the match step `match` (an IrMatch) would do to `frames` frames at the session's rate `rate` (mc_ir_match_plan,
    host arithmetic only): the transform's length, its passes, the device memory the step needs while it runs, the frames it
    hands on, the grid's points and the bins all windows hold together.  target_frames: the target's length at the session's
    rate (default: that of match.ir, converted when it has a rate of its own).  McError beyond the step's limits."""
    m = match.to_c()
    if target_frames is None:
        t = match.frames()
        target_frames = 0 if t is None else t.shape[0]
        if m.rate and int(rate) != m.rate:
            g = math.gcd(int(rate), m.rate)
            target_frames = -(-target_frames * (int(rate) // g) // (m.rate // g))
    out = (C.c_double * 6)()
    check(_lib.load().mc_ir_match_plan(C.byref(m), int(frames), int(target_frames), int(rate), out))
    return dict(nfft=int(out[0]), passes=int(out[1]), device_bytes=int(out[2]), frames_out=int(out[3]), points=int(out[4]), window_bins=int(out[5]))


PARTS = ("direct", "early", "late")


def _triple(v, cast):
    """A per-part field of IrParts: a scalar for all three parts, or (direct, early, late)."""
    if isinstance(v, (tuple, list, np.ndarray)):
        if len(v) != 3:
            raise ValueError(f"a per-part value is a scalar or (direct, early, late), not {v!r}")
        return tuple(cast(x) for x in v)
    return (cast(v),) * 3


@dataclasses.dataclass
class IrParts:
    """The direct sound, the early reflections and the late tail of an IR as three parts with controls of their own, which
    prepare(parts=...) and prepare_sweep(parts=...) apply after the match step and before everything else (mc_ir_parts,
    include/mcconv.h).  direct_end and early_end (frames at the session's rate, of the frames that reach the step) are where
    the direct part and the early part end; xfade: the lengths of the raised-cosine cross-fades around them.  delay (whole
    frames), gain_db, width (0 mono, 1 as it is, 2 the side signal doubled) and balance (-1 left .. +1 right) take a scalar,
    which applies to all three parts, or a triple (direct, early, late).  mute, swap (the part's input channels change
    places) and invert name parts: mute=("direct",).  frames_out: the frames the step hands on, 0 = all that the parts
    reach.  mode "off" does nothing."""

    direct_end: int = 0
    early_end: int = 0
    xfade: object = (0, 0)
    delay: object = 0
    gain_db: object = 0.0
    width: object = 1.0
    balance: object = 0.0
    mute: tuple = ()
    swap: tuple = ()
    invert: tuple = ()
    frames_out: int = 0
    mode: str = "on"

    MODES = {"off": _lib.MC_PARTS_OFF, "on": _lib.MC_PARTS_ON}

    def on(self):
        return self.mode != "off"

    def to_c(self):
        if self.mode not in self.MODES:
            raise ValueError(f"mode must be one of {sorted(self.MODES)}, not {self.mode!r}")
        p = _lib.McIrParts()
        _lib.load().mc_default_ir_parts(C.byref(p))
        p.mode, p.direct_end, p.early_end, p.frames_out = self.MODES[self.mode], int(self.direct_end), int(self.early_end), int(self.frames_out)
        flags = 0
        for shift, names in ((0, self.mute), (4, self.swap), (8, self.invert)):
            for name in (names,) if isinstance(names, str) else names:
                if name not in PARTS:
                    raise ValueError(f"a part is one of {PARTS}, not {name!r}")
                flags |= 1 << (shift + PARTS.index(name))
        p.flags = flags
        xf = self.xfade if isinstance(self.xfade, (tuple, list)) else (self.xfade, self.xfade)
        p.xfade[0], p.xfade[1] = int(xf[0]), int(xf[1])
        for k in range(3):
            p.delay[k], p.gain_db[k] = _triple(self.delay, int)[k], _triple(self.gain_db, float)[k]
            p.width[k], p.balance[k] = _triple(self.width, float)[k], _triple(self.balance, float)[k]
        return p


def parts_plan(parts, frames):
    """What the parts step `parts` (an IrParts) would do to `frames` frames at the session's rate (mc_ir_parts_plan, host
    arithmetic only): the frames it hands on, where the two cross-fades begin, the device memory the step needs while it runs,
    and the coefficients float64 [3, 4]: c_LL, c_LR, c_RL, c_RR of the direct, the early and the late part.  McError beyond the
    step's limits."""
    out, coef = (C.c_double * 4)(), (C.c_double * 12)()
    check(_lib.load().mc_ir_parts_plan(C.byref(parts.to_c()), int(frames), out, coef))
    return dict(frames_out=int(out[0]), fade_start=(int(out[1]), int(out[2])), device_bytes=int(out[3]), coef=np.array(coef[:12]).reshape(3, 4))


def parts_at(parts, onset, rate, direct_s=0.0025, early_s=0.08):
    """`parts` (an IrParts) with its boundaries put direct_s and early_s seconds after frame `onset` at `rate` Hz, rounded to
    frames (mc_ir_parts_at, host arithmetic only): onset is ir_shape_info(idx)["onset"] of a load that searched for it, or the
    origin a measurement reports.  Everything else of `parts` stays."""
    p = parts.to_c()
    check(_lib.load().mc_ir_parts_at(C.byref(p), int(onset), int(math.floor(direct_s * rate + 0.5)), int(math.floor(early_s * rate + 0.5))))
    return dataclasses.replace(parts, direct_end=int(p.direct_end), early_end=int(p.early_end))


def parts_from_density(parts, density, first=0, direct_s=0.0025, rate=None):
    """`parts` (an IrParts) with early_end at the mixing tap that `density` (ir_density's result) measured for the "LR" row and
    direct_end direct_s seconds after the measurement's origin.  `first` is ir_shape_info(idx)["first"] when the measured load
    trimmed the IR, else 0: the taps it skipped are added to both.  rate (Hz) defaults to the one the measurement's mix and
    mix_s imply.  ValueError when the row's status is 1: the density never reached the threshold, and there is no mixing
    tap."""
    row = density["rows"]["LR"]
    if row["status"] == 1 or not math.isfinite(row["mix"]):
        raise ValueError("the density never reached the threshold: there is no mixing tap to put early_end at")
    mix, origin = int(row["mix"]), int(density["origin"])
    if rate is None:
        rate = (mix - origin) / row["mix_s"] if mix > origin and row["mix_s"] > 0 else 0.0
    direct = min(int(math.floor(direct_s * rate + 0.5)), max(mix - origin, 0))
    p = parts.to_c()
    check(_lib.load().mc_ir_parts_at(C.byref(p), int(first) + origin, direct, max(mix - origin, 0)))
    return dataclasses.replace(parts, direct_end=int(p.direct_end), early_end=int(p.early_end))


def tail_from_floor(floor, first=0, mode="extend", fade=0, length=0, seed=0, width=1.0):
    """The IrTail that repairs the tail `floor` (ir_floor's result) found: per band the knee, the decay and the two channels'
    levels of the measured lines (mc_ir_tail_from_floor, host arithmetic only).  A band without a knee inside the analysed
    taps is left alone.  `first` is ir_shape_info(idx)["first"] when the measured load trimmed the IR, else 0; mode, fade,
    length, seed and width are passed on."""
    q, groups = floor["query"].to_c(), floor["groups"]
    rows = np.array([[[floor["rows"][(g, name)][f] for f in FLOOR_FIELDS] for name in DECAY_SETS] for g in range(groups)], np.float64)
    info = (C.c_uint64 * 2)(int(floor["origin"]), int(floor["taps"]))
    t = McIrTail()
    _lib.load().mc_default_ir_tail(C.byref(t))
    check(_lib.load().mc_ir_tail_from_floor(C.byref(q), rows.ctypes.data_as(C.POINTER(C.c_double)), info, int(first), C.byref(t)))
    bands = t.n_xovers + 1
    return IrTail(mode=mode, xovers=tuple(float(t.xover_hz[k]) for k in range(t.n_xovers)),
                  knee=tuple(None if t.knee[j] == _lib.MC_TAIL_LEFT_ALONE else int(t.knee[j]) for j in range(bands)),
                  t60=tuple(int(t.t60[j]) for j in range(bands)), level_db=tuple((float(t.level_db[j][0]), float(t.level_db[j][1])) for j in range(bands)),
                  fade=fade, length=length, seed=seed, width=width)


def tail_move_knee(tail, band, frame):
    """`tail` (an IrTail in mode "extend") with band `band`'s knee moved to `frame` and its two levels slid along the band's own
    line, 60 dB per t60 (mc_ir_tail_move_knee, host arithmetic only): how a rendered or synthesised IR, which has no noise
    floor, gets its knee at the mixing tap ir_density measured.  McError for a band the tail does not have or leaves alone."""
    t = tail.to_c()
    check(_lib.load().mc_ir_tail_move_knee(C.byref(t), int(band), int(frame)))
    bands = t.n_xovers + 1
    return dataclasses.replace(tail, knee=tuple(None if t.knee[j] == _lib.MC_TAIL_LEFT_ALONE else int(t.knee[j]) for j in range(bands)),
                               t60=tuple(int(t.t60[j]) for j in range(bands)),
                               level_db=tuple((float(t.level_db[j][0]), float(t.level_db[j][1])) for j in range(bands)))


def tail_width_from_iacc(tail, iacc_or_rho):
    """`tail` (an IrTail) with its width set to continue an IR whose late broadband IACF(0) is rho: width = min(max(1 - rho, 0), 1)
    (mc_ir_tail_width_from_iacc, host arithmetic only).  The tail's noise is R = rho gA + sqrt(1 - rho^2) gB, whose lag-0
    coefficient is rho exactly; a negative rho clamps to width 1, because the tail cannot be anti-correlated.  iacc_or_rho is rho
    or what ir_iacc returned, whose row (0, "late") is then read.  McError for a rho that is not finite, which a late window
    of status 1 gives."""
    rho = iacc_or_rho["rows"][(0, "late")]["iacf0"] if isinstance(iacc_or_rho, dict) else iacc_or_rho
    t = tail.to_c()
    check(_lib.load().mc_ir_tail_width_from_iacc(C.byref(t), float(rho)))
    return dataclasses.replace(tail, width=float(t.width))


@dataclasses.dataclass
class IrSynth:
    """The IR prepare_synth generates on the device (mc_ir_synth, include/mcconv.h): `frames` stereo frames at the session's
    rate, a pure function of the seed and these numbers.  A late field of Gaussian noise from frame late_start on, of standard
    deviation late_gain there and 60 dB down t60 frames later (0: no decay), its echo density building up over build_up
    frames (0: dense at once); `direct` on frame 0; n_early reflections placed in [early_first, early_last], the first of
    gain early_gain and the later ones falling as 1 / distance, panned within `width`, which also sets how far the channels of
    the late field differ (0: equal, 1: independent).  rate: set by prepare_synth from the engine's sample_rate."""

    frames: int = 48000
    seed: int = 0
    late_start: int = 0
    t60: int = 0
    build_up: int = 0
    late_gain: float = 1.0
    direct: float = 0.0
    n_early: int = 0
    early_first: int = 0
    early_last: int = 0
    early_gain: float = 1.0
    width: float = 1.0
    rate: int = 0

    def to_c(self):
        s = McIrSynth()
        _lib.load().mc_default_ir_synth(C.byref(s))
        s.frames, s.seed, s.late_start, s.t60, s.build_up = int(self.frames), int(self.seed), int(self.late_start), int(self.t60), int(self.build_up)
        s.late_gain, s.direct, s.early_gain, s.width = float(self.late_gain), float(self.direct), float(self.early_gain), float(self.width)
        s.n_early, s.early_first, s.early_last, s.rate = int(self.n_early), int(self.early_first), int(self.early_last), int(self.rate)
        return s


@dataclasses.dataclass
class IrRoom:
    """The rectangular room whose reflections prepare_synth(room=...) adds to a synthesised IR (mc_ir_room, include/mcconv.h;
    Allen and Berkley's image-source method): `size` (Lx, Ly, Lz) in metres, the `source` and the centre of the `receiver`
    pair inside it, and `beta`, the pressure reflection coefficient of the walls: one number for all six, or six for
    x=0, x=Lx, y=0, y=Ly, z=0, z=Lz.  The two omnidirectional receivers (left, right) sit `spacing` metres apart along `axis`
    (0, 1, 2 or "x", "y", "z").  `speed` is that of sound in m/s, `gain` the amplitude of an image 1 m away.  Images on the
    lattice -order .. order per axis are rendered (0: as many as arrive before the end); those arriving at or after frame
    `last` (0: the IR's length) are left out."""

    size: tuple = (5.0, 4.0, 3.0)
    source: tuple = (1.0, 1.5, 1.2)
    receiver: tuple = (3.5, 2.0, 1.5)
    beta: object = 0.9
    spacing: float = 0.2
    axis: object = 0
    speed: float = 343.0
    gain: float = 1.0
    order: int = 0
    last: int = 0

    AXES = {"x": 0, "y": 1, "z": 2}

    def to_c(self):
        beta = tuple(self.beta) if isinstance(self.beta, (tuple, list)) else (self.beta,) * 6
        if len(beta) != 6 or len(self.size) != 3 or len(self.source) != 3 or len(self.receiver) != 3:
            raise ValueError("size, source and receiver take three numbers, beta one or six")
        r = McIrRoom()
        _lib.load().mc_default_ir_room(C.byref(r))
        for k in range(3):
            r.size_m[k], r.source_m[k], r.receiver_m[k] = float(self.size[k]), float(self.source[k]), float(self.receiver[k])
        for k in range(6):
            r.beta[k] = float(beta[k])
        r.spacing_m, r.axis, r.speed, r.gain = float(self.spacing), int(self.AXES.get(self.axis, self.axis)), float(self.speed), float(self.gain)
        r.order, r.last = int(self.order), int(self.last)
        return r


def room_plan(room, rate, frames):
    """What a load of `frames` frames at `rate` would do with `room` (an IrRoom; mc_ir_room_plan, host arithmetic only): the
    order used, the images in its lattice, the frames up to which the lattice is complete, the direct sound's delay per
    channel (frames), the volume, and Sabine's and Eyring's reverberation times in seconds (0 when nothing absorbs), which
    the method's own decay outlasts: measure the tail (ir_floor), do not compute it."""
    out = (C.c_double * 8)()
    check(_lib.load().mc_ir_room_plan(C.byref(room.to_c()), int(rate), int(frames), out))
    return dict(order=int(out[0]), images=int(out[1]), complete=int(out[2]), direct=(out[3], out[4]), volume=out[5], sabine=out[6], eyring=out[7])


@dataclasses.dataclass
class IrSpring:
    """The spring tank whose response prepare_synth(spring=...) adds to a synthesised IR (mc_ir_spring, include/mcconv.h): up
    to three springs of round-trip times `delay_ms`, each a loop of `sections` all-pass sections of coefficient `dispersion`
    stretched so that the chirps end at `transition_hz`, a one-pole `damping` and the gain that `t60` seconds make; a
    Butterworth low-pass of `lowpass_order` at the transition; a second, weaker family of chirps above it (`high_gain`, 0:
    off, `high_sections`, `high_dispersion`, `high_delay` as a part of the period, `high_t60`); channel R's periods are
    (1 + stereo) times channel L's.  `log2_points` (0: by the length) fixes the transform's size; frames at and after `last`
    (0: the IR's length) get nothing from the spring."""

    sections: int = 100
    transition_hz: float = 4300.0
    dispersion: float = 0.62
    delay_ms: tuple = (66.0, 82.0)
    t60: float = 2.5
    damping: float = 0.2
    lowpass_order: int = 8
    high_gain: float = 0.1
    high_sections: int = 200
    high_dispersion: float = -0.6
    high_delay: float = 0.5
    high_t60: float = 1.0
    stereo: float = 0.03
    gain: float = 1.0
    log2_points: int = 0
    last: int = 0

    def to_c(self):
        delays = tuple(self.delay_ms) if isinstance(self.delay_ms, (tuple, list)) else (self.delay_ms,)
        if not 1 <= len(delays) <= 3:
            raise ValueError("delay_ms takes one to three numbers")
        p = McIrSpring()
        _lib.load().mc_default_ir_spring(C.byref(p))
        for k in range(3):
            p.delay_ms[k] = float(delays[k]) if k < len(delays) else 0.0
        p.sections, p.lowpass_order, p.high_sections, p.log2_points, p.last = (int(self.sections), int(self.lowpass_order), int(self.high_sections),
                                                                               int(self.log2_points), int(self.last))
        p.transition_hz, p.dispersion, p.t60_s, p.damping = float(self.transition_hz), float(self.dispersion), float(self.t60), float(self.damping)
        p.high_gain, p.high_dispersion, p.high_delay, p.high_t60_s = float(self.high_gain), float(self.high_dispersion), float(self.high_delay), float(self.high_t60)
        p.stereo, p.gain = float(self.stereo), float(self.gain)
        return p


def _spring_numbers(out):
    springs = int(out[3])
    return dict(points=int(out[0]), stretch=int(out[1]), transition=out[2], springs=springs, sections=int(out[4]), lowpass=bool(out[5]), last=int(out[6]),
                alias_db=out[7], delay=[(int(out[8 + 2 * s]), int(out[9 + 2 * s])) for s in range(springs)],
                loop_gain=[(out[14 + 2 * s], out[15 + 2 * s]) for s in range(springs)])


def spring_plan(spring, rate, frames):
    """What a load of `frames` frames at `rate` would do with `spring` (an IrSpring; mc_ir_spring_plan, host arithmetic only):
    the transform's points N, the stretch K, the effective transition rate / (2 K) in Hz, the springs, the sections, whether
    the low-pass is in, the frame E from which the spring adds nothing, the bound in dB on what wraps around relative to the
    first echo, and per spring (L, R) the loop's delay in frames and its gain."""
    out = (C.c_double * 24)()
    check(_lib.load().mc_ir_spring_plan(C.byref(spring.to_c()), int(rate), int(frames), out))
    return _spring_numbers(out)


def spring_response(spring, rate, hz):
    """H_L and H_R of `spring` at `rate` on the unit circle at the frequencies hz (mc_ir_spring_response, host arithmetic
    through the functions that make the kernel's constants) as complex128 [len(hz), 2]."""
    hz = np.ascontiguousarray(hz, np.float64).reshape(-1)
    out = np.zeros((hz.shape[0], 4), np.float64)
    dp = C.POINTER(C.c_double)
    check(_lib.load().mc_ir_spring_response(C.byref(spring.to_c()), int(rate), hz.ctypes.data_as(dp), hz.shape[0], out.ctypes.data_as(dp)))
    return np.stack([out[:, 0] + 1j * out[:, 1], out[:, 2] + 1j * out[:, 3]], axis=1)


@dataclasses.dataclass
class IrPlate:
    """The plate reverberator whose modes prepare_synth(plate=...) adds to a synthesised IR (mc_ir_plate, include/mcconv.h): a
    thin simply supported rectangular sheet of `size` (Lx, Ly) metres and `thickness_mm`, of `material` "steel" or (Young's
    modulus in GPa, density in kg/m^3, Poisson's ratio), driven at `driver` (x, y) and picked up at `pickups` ((x, y) left,
    (x, y) right).  The modes between low_hz and high_hz (0: min(20000, 0.45 rate)) sound; `t60` = (seconds towards 0 Hz,
    seconds at damp_hz), 0 for no loss at that end; `gain` is the RMS of the first milliseconds; frames at and after `last`
    (0: the IR's length) get nothing from the plate."""

    size: tuple = (2.04, 0.97)
    thickness_mm: float = 0.5
    material: object = "steel"
    driver: tuple = (0.83, 0.41)
    pickups: tuple = ((0.31, 0.67), (1.57, 0.29))
    low_hz: float = 20.0
    high_hz: float = 0.0
    t60: tuple = (4.0, 1.0)
    damp_hz: float = 10000.0
    gain: float = 1.0
    last: int = 0

    MATERIALS = {"steel": (200.0, 7850.0, 0.3)}

    def to_c(self):
        if isinstance(self.material, str):
            if self.material not in self.MATERIALS:
                raise ValueError(f"material {self.material!r}: one of {sorted(self.MATERIALS)} or (E in GPa, density, Poisson's ratio)")
            material = self.MATERIALS[self.material]
        else:
            material = tuple(self.material)
        if len(self.size) != 2 or len(self.driver) != 2 or len(self.pickups) != 2 or any(len(q) != 2 for q in self.pickups) or len(self.t60) != 2 \
                or len(material) != 3:
            raise ValueError("size, driver and t60 take two numbers, pickups two pairs, material a name or three numbers")
        p = McIrPlate()
        _lib.load().mc_default_ir_plate(C.byref(p))
        for k in range(2):
            p.size_m[k], p.driver_m[k], p.t60_s[k] = float(self.size[k]), float(self.driver[k]), float(self.t60[k])
            for a in range(2):
                p.pickup_m[k][a] = float(self.pickups[k][a])
        p.thickness_mm = float(self.thickness_mm)
        p.young_gpa, p.density, p.poisson = (float(v) for v in material)
        p.low_hz, p.high_hz, p.damp_hz, p.gain, p.last = float(self.low_hz), float(self.high_hz), float(self.damp_hz), float(self.gain), int(self.last)
        return p


def plate_plan(plate, rate, frames):
    """What a load of `frames` frames at `rate` would do with `plate` (an IrPlate; mc_ir_plate_plan, host arithmetic only): the
    modes kept, the lowest and the highest of them in Hz, the stiffness kappa, Weyl's modal density in modes per Hz, the decay
    times at low_hz and at the highest mode in seconds (0: no loss), and the (mode, frame) pairs the device would sum."""
    out = (C.c_double * 8)()
    check(_lib.load().mc_ir_plate_plan(C.byref(plate.to_c()), int(rate), int(frames), out))
    return dict(modes=int(out[0]), lowest=out[1], highest=out[2], kappa=out[3], density=out[4], t60=(out[5], out[6]), pairs=int(out[7]))


def plate_modes(plate, rate, first=0, count=None):
    """Rows first .. first + count of the mode table of `plate` at `rate` (mc_ir_plate_modes, host arithmetic only; count None:
    to the end) as float64 [count, 6]: m, n, f (Hz), sigma (1/s), a_L, a_R: the table a load uploads."""
    L = _lib.load()
    p = plate.to_c()
    if count is None:
        out = (C.c_double * 8)()
        check(L.mc_ir_plate_plan(C.byref(p), int(rate), 1, out))
        count = int(out[0]) - int(first)
    rows = np.zeros((max(int(count), 0), 6), np.float64)
    check(L.mc_ir_plate_modes(C.byref(p), int(rate), int(first), int(count), rows.ctypes.data_as(C.POINTER(C.c_double))))
    return rows


@dataclasses.dataclass
class IrRoomMics:
    """Directional microphones and a directional source in an IrRoom (mc_ir_room_mics, include/mcconv.h): prepare_synth(room=,
    mics=).  `pattern` is the receivers' first-order pattern, a name of PATTERNS or the number alpha of
    g = alpha + (1 - alpha) cos (1 omni, 0.5 cardioid, 0 figure-of-eight); `az` and `el` are their aims in degrees, azimuth from
    +x towards +y and elevation towards +z.  Each takes one value for both receivers or a pair (left, right).
    source_pattern, source_az and source_el are the source's.  The defaults are omni everywhere: the room as it is without
    microphones, bit for bit."""

    pattern: object = "omni"
    az: object = 0.0
    el: object = 0.0
    source_pattern: object = "omni"
    source_az: float = 0.0
    source_el: float = 0.0

    PATTERNS = {"omni": 1.0, "subcardioid": 0.75, "cardioid": 0.5, "supercardioid": 0.366, "hypercardioid": 0.25, "fig8": 0.0}

    @classmethod
    def alpha(cls, pattern):
        """The number of a pattern given by name or as a number."""
        if isinstance(pattern, str):
            if pattern not in cls.PATTERNS:
                raise ValueError(f"'{pattern}' is no pattern: {', '.join(cls.PATTERNS)} or a number")
            return cls.PATTERNS[pattern]
        return float(pattern)

    @classmethod
    def pair(cls, facing=0.0, angle=90.0, pattern="cardioid", **kw):
        """A pair of equal microphones that faces azimuth `facing` and opens by `angle` degrees: L aims at
        facing + angle / 2 and R at facing - angle / 2.  Azimuth runs counter-clockwise seen from above, so the microphone
        with the larger azimuth points to the left of someone who looks along `facing`: XY is pair(angle=90) with
        IrRoom.spacing 0, Blumlein pair(angle=90, pattern="fig8"), ORTF pair(angle=110) with spacing 0.17.
        IrRoom.spacing puts L at the smaller coordinate of `axis`, whatever the aims.  Someone looking along +x has their left
        at larger y, so with the spacing along y a pair facing +x would have its left microphone on the right: a spaced
        pair such as ORTF along y faces -x (facing=180), or swaps its aims (a negative angle).  Further keywords are
        IrRoomMics' own (el, source_pattern, ...)."""
        return cls(pattern=pattern, az=(float(facing) + float(angle) / 2.0, float(facing) - float(angle) / 2.0), **kw)

    @staticmethod
    def _two(v):
        v = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        if len(v) != 2:
            raise ValueError("pattern, az and el take one value or two (left, right)")
        return v

    def to_c(self):
        m = McIrRoomMics()
        _lib.load().mc_default_ir_room_mics(C.byref(m))
        pattern, az, el = self._two(self.pattern), self._two(self.az), self._two(self.el)
        for k in range(2):
            m.mic_pattern[k], m.mic_az_deg[k], m.mic_el_deg[k] = self.alpha(pattern[k]), float(az[k]), float(el[k])
        m.src_pattern, m.src_az_deg, m.src_el_deg = self.alpha(self.source_pattern), float(self.source_az), float(self.source_el)
        return m


def _mics_factors(out):
    return dict(source=(out[0], out[1]), receiver=(out[2], out[3]), factor=(out[4], out[5]))


def room_mics_plan(room, mics, rate, frames):
    """What `mics` (an IrRoomMics) do to the direct sound of `room` in a load of `frames` frames at `rate`
    (mc_ir_room_mics_plan, host arithmetic only): the source's factor towards each receiver, each receiver's factor towards the
    source, and their product, which multiplies the direct sound's gain / d; each as (left, right)."""
    out = (C.c_double * 8)()
    check(_lib.load().mc_ir_room_mics_plan(C.byref(room.to_c()), C.byref(mics.to_c()), int(rate), int(frames), out))
    return _mics_factors(out)


@dataclasses.dataclass
class IrRoomBands:
    """Walls and air that differ per frequency band in an IrRoom (mc_ir_room_bands, include/mcconv.h): prepare_synth(room=,
    bands=).  `xovers` are up to three crossover frequencies in Hz, ascending; they cut len(xovers) + 1 bands, low to high.
    `beta` is the walls' pressure reflection coefficient: one number for every band and wall, one per band, or six per band
    (IrRoom's order).  `air` is the air's loss in dB per metre: one number or one per band.  The room is rendered once per
    band and the renderings are joined by IrDamp's band split; with bands, IrRoom.beta is not used for rendering.  Equal bands
    without air store the unbanded room, bit for bit."""

    xovers: tuple = ()
    beta: object = 0.9
    air: object = 0.0

    @classmethod
    def from_absorption(cls, xovers, alpha, air=0.0):
        """Bands from energy absorption coefficients alpha in [0, 1], in the shapes `beta` takes: beta = sqrt(1 - alpha)."""
        def root(a):
            if isinstance(a, (tuple, list)):
                return tuple(root(v) for v in a)
            if not 0.0 <= float(a) <= 1.0:
                raise ValueError(f"alpha {a} outside [0, 1]")
            return math.sqrt(1.0 - float(a))

        return cls(xovers=tuple(xovers), beta=root(alpha), air=air)

    def _per_band(self, v, name, walls):
        B = len(tuple(self.xovers)) + 1
        v = tuple(v) if isinstance(v, (tuple, list)) else (v,) * B
        if len(v) != B:
            raise ValueError(f"{name} takes one value or one per band ({B})")
        if not walls:
            return tuple(float(x) for x in v)
        rows = tuple(tuple(x) if isinstance(x, (tuple, list)) else (x,) * 6 for x in v)
        if any(len(r) != 6 for r in rows):
            raise ValueError("beta takes one value, one per band, or six per band")
        return tuple(tuple(float(x) for x in r) for r in rows)

    def to_c(self):
        xovers = tuple(self.xovers)
        if len(xovers) > 3:
            raise ValueError("at most three crossovers")
        b = McIrRoomBands()
        _lib.load().mc_default_ir_room_bands(C.byref(b))
        b.n_xovers = len(xovers)
        for k, hz in enumerate(xovers):
            b.xover_hz[k] = float(hz)
        for j, row in enumerate(self._per_band(self.beta, "beta", True)):
            for w in range(6):
                b.beta[j][w] = row[w]
        for j, a in enumerate(self._per_band(self.air, "air", False)):
            b.air_db_per_m[j] = a
        return b


def _bands_report(out):
    B = int(out[0])
    return dict(bands=B, xovers=tuple(out[1 + k] for k in range(B - 1)), sabine=tuple(out[4 + j] for j in range(B)),
                eyring=tuple(out[8 + j] for j in range(B)))


def room_bands_plan(room, bands, rate, frames):
    """What a load of `frames` frames at `rate` would do with `bands` (an IrRoomBands) in `room` (mc_ir_room_bands_plan, host
    arithmetic only): the number of bands, the crossovers, and Sabine's and Eyring's reverberation times per band in seconds,
    the air's loss included (0 when nothing absorbs)."""
    out = (C.c_double * 16)()
    check(_lib.load().mc_ir_room_bands_plan(C.byref(room.to_c()), C.byref(bands.to_c()), int(rate), int(frames), out))
    return _bands_report(out)


@dataclasses.dataclass
class IrRoomHead:
    """A binaural listener in an IrRoom (mc_ir_room_head, include/mcconv.h): prepare_synth(room=, head=).  A rigid sphere of
    `radius` metres (Brown and Duda's structural model) takes the place of the receiver pair at IrRoom.receiver: each ear
    hears an arrival with a delay that depends on its direction and through a head-shadow shelf, up to +6 dB towards the ear
    and down to about -20 dB behind the head at high frequencies.  `facing` is the azimuth the listener looks along, in
    degrees from +x towards +y; `ear` is the ears' angle from it (90: on the axis through the head; Brown and Duda place them
    at 100, a little behind it); the left ear is channel 0.  `shadow` in [0, 1] scales the shelf: 0 leaves the delays alone.
    IrRoom.spacing and axis are not used with a head.  A far-field model of an upright head: no pinna, no torso, no
    elevation cue."""

    radius: float = 0.0875
    facing: float = 0.0
    ear: float = 90.0
    shadow: float = 1.0

    def to_c(self):
        h = McIrRoomHead()
        _lib.load().mc_default_ir_room_head(C.byref(h))
        h.radius_m, h.facing_az_deg, h.ear_deg, h.shadow = float(self.radius), float(self.facing), float(self.ear), float(self.shadow)
        return h


def _head_report(out):
    return dict(order=int(out[0]), complete=int(out[1]), direct=(out[2], out[3]), itd=out[4], angle=(out[5], out[6]), shadow=(out[7], out[8]),
                corner=out[9], k=out[10])


def room_head_plan(room, head, rate, frames):
    """What a load of `frames` frames at `rate` would do with `head` (an IrRoomHead) in `room` (mc_ir_room_head_plan, host
    arithmetic only): the lattice order and the frames up to which it is complete, the direct sound's delay at each ear
    (frames) and their difference right minus left in seconds (`itd`), its angle from each ear's axis (degrees), each ear's
    shadow factor h = alpha - 1, the shelf's corner in Hz and its prewarped constant K; pairs are (left, right)."""
    out = (C.c_double * 12)()
    check(_lib.load().mc_ir_room_head_plan(C.byref(room.to_c()), C.byref(head.to_c()), int(rate), int(frames), out))
    return _head_report(out)


@dataclasses.dataclass
class Sweep:
    """The exponential sine sweep whose recording prepare_sweep deconvolves (mc_sweep, include/mcconv.h): `frames` frames
    from f1_hz at frame 0 to f2_hz at the last, of peak `amplitude` (0.5 is WavFile's full scale), faded in and out over
    fade_in and fade_out frames.  rate 0: the engine's sample_rate in prepare_sweep, the library's default (44100) in
    sweep_frames."""

    frames: int = 0
    f1_hz: float = 20.0
    f2_hz: float = 20000.0
    amplitude: float = 0.5
    fade_in: int = 0
    fade_out: int = 0
    rate: int = 0

    def to_c(self):
        s = McSweep()
        _lib.load().mc_default_sweep(C.byref(s))
        s.frames, s.fade_in, s.fade_out = int(self.frames), int(self.fade_in), int(self.fade_out)
        s.f1_hz, s.f2_hz, s.amplitude = float(self.f1_hz), float(self.f2_hz), float(self.amplitude)
        if self.rate:
            s.rate = int(self.rate)
        return s


def sweep_frames(sweep):
    """The sweep as float32 mono frames (mc_sweep_generate): what to play through the room."""
    s = sweep.to_c()
    out = np.empty(max(int(s.frames), 0), np.float32)
    check(_lib.load().mc_sweep_generate(C.byref(s), _fp(out), 0, int(s.frames)))
    return out


SWEEP_MAX_FRAMES = 1 << 24  # M, F and |offset| of mc_load_ir_sweep
SWEEP_MAX_WORK = 1 << 40    # F * N

DECAY_SETS = ("L", "R", "LR")
DECAY_FIELDS = ("energy", "edt", "t20", "t30", "c50", "c80", "d50", "ts")
FLOOR_FIELDS = ("energy", "noise", "knee", "t", "peak_to_noise_db", "interval", "last_change", "status")
IACC_WINDOWS = ("early", "late", "all")
IACC_FIELDS = ("energy_l", "energy_r", "iacc", "lag", "iacf", "iacf0", "level_db", "status")
DENSITY_FIELDS = ("mix", "mix_s", "first", "max", "max_tap", "mean_after", "silent", "status")
STI_RATINGS = ((0.30, "bad"), (0.45, "poor"), (0.60, "fair"), (0.75, "good"))


def sti_rating(sti):
    """The word IEC 60268-16 puts on a speech transmission index: "bad" below 0.30, "poor" below 0.45, "fair" below 0.60,
    "good" below 0.75, "excellent" from there on (an edge belongs to the better word).  ValueError for a NaN."""
    sti = float(sti)
    if math.isnan(sti):
        raise ValueError("sti is NaN: it has no rating")
    for edge, word in STI_RATINGS:
        if sti < edge:
            return word
    return "excellent"


RESPONSE_CHANNELS = ("L", "R")
RESPONSE_FLOOR_DB = -400.0  # db where |H| = 0 (the floor of the decay curve)


def response_grid(lo=20, hi=20000, per_octave=24):
    """The frequencies lo 2^(i / per_octave) <= hi as float32 (mc_response_grid, host arithmetic only): per_octave points to the
    octave, the grid ir_response uses when it is given none."""
    hz = np.empty(_lib.MC_RSP_MAX_FREQ * 16, np.float32)
    n = _lib.load().mc_response_grid(float(lo), float(hi), int(per_octave), _fp(hz), hz.size)
    if n < 0:
        check(n)
    return hz[:n].copy()


def smooth_response(hz, power, octaves):
    """Fractional-octave smoothing of a power response (|H|^2) on an ascending grid hz: each point becomes the mean of the points
    within octaves / 2 on either side (mc_response_smooth, host arithmetic only).  octaves = 0 returns power as it is."""
    hz = _f32(hz).reshape(-1)
    power = np.ascontiguousarray(power, dtype=np.float64).reshape(-1)
    if power.size != hz.size:
        raise ValueError(f"{hz.size} frequencies and {power.size} powers")
    out = np.empty_like(power)
    dp = C.POINTER(C.c_double)
    check(_lib.load().mc_response_smooth(_fp(hz), power.ctypes.data_as(dp), hz.size, float(octaves), out.ctypes.data_as(dp)))
    return out


def waterfall_windows(slices, hop, length, rise=0, fall=0):
    """The windows of a waterfall for ir_response: `slices` windows of `length` taps, each `hop` taps after the one before, the
    first at the origin, all with the same raised-cosine edges."""
    if slices < 1 or hop < 0 or length < 1 or rise < 0 or fall < 0:
        raise ValueError("slices and length are at least 1; hop, rise and fall are not negative")
    return [(k * int(hop), int(length), int(rise), int(fall)) for k in range(int(slices))]


def decay_for_rt60(measured_s, target_s, rate):
    """The IrShape.decay_t60 (frames) that takes an IR whose decay time is measured_s seconds to target_s seconds at `rate`
    Hz.  The envelope 10^(-3 m / d) adds 60 rate / d dB/s to the slope, so 1 / target = 1 / measured + rate / d.  An envelope
    can only shorten: ValueError unless 0 < target_s < measured_s, both finite."""
    measured_s, target_s = float(measured_s), float(target_s)
    if not (math.isfinite(measured_s) and math.isfinite(target_s) and 0.0 < target_s < measured_s):
        raise ValueError(f"need 0 < target ({target_s}) < measured ({measured_s}), both finite")
    return int(round(float(rate) / (1.0 / target_s - 1.0 / measured_s)))


def damp_for_rt60(measured_s, target_s, rate):
    """IrDamp.decay for bands whose decay times were measured as measured_s (seconds, one per band, low to high) and are
    wanted as target_s: decay_for_rt60 per band, and 0 (the band is left alone) where the target is None, NaN or not below
    the measured time.  The bands overlap, so the result is a first aim to be iterated against ir_decay."""
    if len(measured_s) != len(target_s):
        raise ValueError(f"{len(measured_s)} measured times, {len(target_s)} targets")
    out = []
    for m, t in zip(measured_s, target_s):
        if t is None or math.isnan(float(t)) or not float(t) < float(m):
            out.append(0)
        else:
            out.append(decay_for_rt60(m, t, rate))
    return tuple(out)


class _CCValueView:
    """cc[i].value — attribute access backed by mc_get_params/mc_set_params."""

    _names = ("select", "predelay", "speed", "vsteps", "dry", "wet", "panDry", "panWet", "level")

    def __init__(self, eng, half):
        object.__setattr__(self, "_eng", eng)
        object.__setattr__(self, "_half", half)

    def _get(self):
        v = McCcValue()
        check(self._eng._L.mc_get_params(self._eng._h, self._half, C.byref(v)))
        return v

    def __getattr__(self, k):
        if k not in self._names:
            raise AttributeError(k)
        return getattr(self._get(), k)

    def __setattr__(self, k, val):
        if k not in self._names:
            raise AttributeError(k)
        v = self._get()
        setattr(v, k, val)
        check(self._eng._L.mc_set_params(self._eng._h, self._half, C.byref(v)))

    def update(self, **kw):
        v = self._get()
        for k, val in kw.items():
            if k not in self._names:
                raise AttributeError(k)
            setattr(v, k, val)
        check(self._eng._L.mc_set_params(self._eng._h, self._half, C.byref(v)))


class CC:
    """Convolution::CC (conv.h:33-50): controller numbers + current values."""

    def __init__(self, eng, half):
        self.device = None
        self.message = 176
        self.select = self.predelay = self.dry = self.wet = self.speed = 0
        self.panDry = self.panWet = self.level = 0
        self.value = _CCValueView(eng, half)

    def ccmap(self):
        return (self.select, self.predelay, self.dry, self.wet, self.speed, self.panDry, self.panWet, self.level)


def _on(step):
    """Whether a step of a load (an IrTail, IrPhase, IrFilter, IrMatch or IrParts, or None) is asked for and switched on."""
    return step is not None and getattr(step, "op", getattr(step, "mode", None)) != "off"


def _file_rates(ir_rate, session, eq, damp, tail, filter, match):
    """(ir_rate, session_rate) of a file load.  What is laid out in Hz or converts a second IR needs the session's rate in the
    call, and frames without a rate of their own then count as being at it; otherwise the rates are passed only to convert."""
    if _on(match) or _on(tail) or eq is not None or (damp is not None and damp.xovers) or (_on(filter) and filter.to_c().rate and session):
        return (int(session or 0) if ir_rate is None else int(ir_rate), int(session or 0))
    if ir_rate is not None and session is not None and int(ir_rate) != int(session):
        return (int(ir_rate), int(session))
    return (0, 0)


def _c_steps(shape, eq, damp, tail, phase, filter, match, parts):
    """The step objects as the widest entry points take them, after the source's own arguments: shape, eq, damp, tail, phase,
    filter, filter_lr, filter_frames, match, target_lr, target_frames, parts.  None or a step that is switched off is a null
    pointer (and no frames).  The second value holds the second IRs' arrays, which must outlive the call (the structs live in
    their byref objects)."""
    ref = lambda x: C.byref(x.to_c()) if x is not None else None  # noqa: E731
    head = (ref(shape), ref(eq), ref(damp), ref(tail if _on(tail) else None), ref(phase if _on(phase) else None))
    flr = filter.frames() if _on(filter) else None
    tlr = match.frames() if _on(match) else None
    m = ref(match if _on(match) else None)
    second = lambda a: (_fp(a), a.shape[0]) if a is not None else (None, 0)  # noqa: E731
    return (*head, ref(filter if _on(filter) else None), *second(flr), m, *second(tlr), ref(parts if _on(parts) else None)), (flr, tlr)


class Convolution:
    def __init__(self, name="Conv", fftSize=CONV_DEFAULT_FFTSIZE, *, max_batch=256, device=-1, compat=True,
                 part_begin=0, part_end=0, max_partitions=0, stream_threshold=0, precision="fp32", period=256, pipeline=False,
                 form="partitioned", sample_rate=None):
        self.name = name
        self.sample_rate = sample_rate  # session rate (Hz): prepare() converts IRs whose own rate differs; None = the reference's behaviour
        self._L = _lib.load()
        cfg = McConfig()
        self._L.mc_default_config(C.byref(cfg))
        cfg.device = device
        cfg.n_ref = fftSize
        cfg.max_batch = max_batch
        cfg.compat = 1 if compat else 0
        cfg.part_begin, cfg.part_end = part_begin, part_end
        cfg.max_partitions = max_partitions
        cfg.stream_threshold = stream_threshold
        cfg.precision = {"fp32": 0, "fp16": 1}[precision]
        cfg.period = period
        cfg.pipeline = 1 if pipeline else 0
        cfg.form = {"partitioned": 0, "single": 1}[form]
        h = C.c_void_p()
        check(self._L.mc_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.fftSize = fftSize
        self.max_batch = max_batch
        self.cc = [CC(self, 0), CC(self, 1)]

    # -- lifetime -----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.mc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self._L.mc_reset(self._h))

    def set_period(self, nframes):
        """JACK period the host calls onProcess with: 256, 512 or 1024 frames (resets the signal state)."""
        check(self._L.mc_set_period(self._h, nframes))

    # -- reference surface ----------------------------------------------------
    def prepare(self, idx, wav, nframes=1024, ir_rate=None, shape=None, eq=None, damp=None, tail=None, phase=None, filter=None, match=None, parts=None):
        """Convolution::prepare (conv.cu:207-253).  `wav` is float32 [frames, 2]
        (what WavFile.buffer holds) or an object with a `.buffer` of that shape.
        ir_rate (Hz; default: `wav.sampleRate` when it has one): when both it and the engine's sample_rate are known and
        differ, the IR is converted to the session's rate on the device (mc_load_ir_resampled).
        shape (an IrShape): trim, reverse, decay, fade and normalise the IR on the device, after the conversion and before
        the truncation; ir_shape_info(idx) then tells what was done.
        eq (an IrEq): filter the shaped taps with its bands before the normalisation; the engine needs a sample_rate, and
        ir_rate defaults to it.
        damp (an IrDamp): a further decay per frequency band, after the fade and before the EQ; the rates as for eq;
        ir_damp_info(idx) then tells what was done.
        tail (an IrTail whose mode is not "off"): cut or extend the tail of the frames band by band, after the conversion and
        before everything else; the rates as for eq; ir_tail_info(idx) then tells what was done.
        phase (an IrPhase whose mode is not "off"): convert the frames to minimum phase, after the tail step and before
        the shape; it needs no rate; ir_phase_info(idx) then tells what was done.
        filter (an IrFilter whose op is not "off"): convolve the frames with a second IR, or divide it out of them, after the
        phase step and before the shape; a filter with a rate of its own needs the engine's sample_rate;
        ir_filter_info(idx) then tells what was done.
        match (an IrMatch whose mode is not "off"): give the frames the smoothed spectrum of a target IR, or a flat one, after
        the filter step and before the shape; the engine needs a sample_rate; ir_match_info(idx) and
        ir_match_curve(idx) then tell what was done.
        parts (an IrParts whose mode is not "off"): the direct sound, the early reflections and the late tail get a gain, a
        delay, a width and a balance each, after the match step and before the shape; it needs no rate;
        ir_parts_info(idx) then tells what was done."""
        lr = _f32(getattr(wav, "buffer", wav)).reshape(-1, 2)
        if ir_rate is None:
            ir_rate = getattr(wav, "sampleRate", None)
        if shape is None and eq is None and not (damp is not None and damp.xovers) and not any(_on(s) for s in (tail, phase, filter, match, parts)):
            # (the reference's plain call)
            if ir_rate is not None and self.sample_rate is not None and int(ir_rate) != int(self.sample_rate):
                check(self._L.mc_load_ir_resampled(self._h, idx, _fp(lr), lr.shape[0], nframes, int(ir_rate), int(self.sample_rate)))
            else:
                check(self._L.mc_load_ir(self._h, idx, _fp(lr), lr.shape[0], nframes))
            return
        rates = _file_rates(ir_rate, self.sample_rate, eq, damp, tail, filter, match)
        steps, keep = _c_steps(shape, eq, damp, tail, phase, filter, match, parts)
        check(self._L.mc_load_ir_parts(self._h, idx, _fp(lr), lr.shape[0], nframes, *rates, *steps))

    def prepare_synth(self, idx, synth, nframes=1024, shape=None, eq=None, damp=None, room=None, tail=None, mics=None, bands=None, plate=None, head=None, spring=None):
        """Generate the IR `synth` (an IrSynth) describes on the device and store it at idx (mc_synth_ir): the frames take the
        place of a WAV's at the session's rate, and shape, eq and damp apply to them as in prepare().  A synthesised IR counts
        as shaped: ir_shape_info(idx)["frames"] is synth.frames.  The engine's sample_rate (which eq, damp, room and tail
        need) is passed unless synth.rate is set.
        room (an IrRoom): the reflections of a rectangular room are added to the frames; ir_room_info(idx) then tells what
        was rendered.  tail (an IrTail whose mode is not "off"): the tail step on the generated frames, as in prepare().
        mics (an IrRoomMics, with room): the receivers and the source of the room are directional; ir_room_mics_info(idx)
        then tells the direct sound's factors.  bands (an IrRoomBands, with room): the walls and the air differ per
        frequency band; ir_room_bands_info(idx) then tells the bands' reverberation times.  head (an IrRoomHead, with
        room): a rigid-sphere listener takes the receiver pair's place and the IR is binaural; ir_room_head_info(idx) then
        tells the ears' delays and shadow factors.
        plate (an IrPlate, without room, mics and bands): the modes of a plate reverberator are added to the frames
        (mc_synth_ir_plate); ir_plate_info(idx) then tells what was summed.
        spring (an IrSpring, without room, mics, bands, head and plate): the response of a spring tank is added to the
        frames (mc_synth_ir_spring); ir_spring_info(idx) then tells the plan it was rendered by."""
        if spring is not None and any(v is not None for v in (room, mics, bands, head, plate)):
            raise ValueError("a spring together with a room (room, mics, bands, head) or a plate in one load is not offered")
        s = synth.to_c()
        if not s.rate:
            s.rate = int(self.sample_rate or 0)
        if spring is not None:
            steps, keep = _c_steps(shape, eq, damp, tail, None, None, None, None)
            check(self._L.mc_synth_ir_spring(self._h, idx, nframes, C.byref(s), C.byref(spring.to_c()), *steps[:4]))
            return
        if plate is not None:
            if room is not None or mics is not None or bands is not None or head is not None:
                raise ValueError("a plate and a room (room, mics, bands, head) in one load are not offered")
            steps, keep = _c_steps(shape, eq, damp, tail, None, None, None, None)
            check(self._L.mc_synth_ir_plate(self._h, idx, nframes, C.byref(s), C.byref(plate.to_c()), *steps[:4]))
            return
        if bands is not None and room is None:
            raise ValueError("the bands need a room")
        if mics is not None and room is None:
            raise ValueError("the microphones need a room")
        if head is not None and room is None:
            raise ValueError("the head needs a room")
        ref = lambda x: C.byref(x.to_c()) if x is not None else None  # noqa: E731
        source = (ref(room), ref(mics), ref(bands))
        steps, keep = _c_steps(shape, eq, damp, tail, None, None, None, None)
        if head is not None:
            check(self._L.mc_synth_ir_room_head(self._h, idx, nframes, C.byref(s), *source, ref(head), *steps[:4]))
            return
        check(self._L.mc_synth_ir_room_bands(self._h, idx, nframes, C.byref(s), *source, *steps[:4]))

    def prepare_sweep(self, idx, recording, sweep, offset=0, ir_frames=None, nframes=1024, shape=None, eq=None, damp=None, tail=None, phase=None, filter=None, match=None, parts=None):
        """Deconvolve `recording` (float32 [frames, 2] or an object with such a `.buffer`: what was recorded while `sweep`, a
        Sweep, played) into an IR on the device and store it at idx (mc_load_ir_sweep): the frames take the place of a WAV's at
        the session's rate, and shape, eq and damp apply to them as in prepare().  IR frame m is the correlation at lag
        m + offset: a recording with no latency has its direct sound at frame -offset, and a negative offset keeps the
        pre-roll where the harmonic-distortion images land.  ir_frames defaults to max(1, M - N + 1 - offset), what the
        recording holds past the sweep, clamped to the library's caps.  The engine's sample_rate is passed unless sweep.rate
        is set (the library's default, 44100, when the engine has none either).  tail (an IrTail whose mode is not "off"): the
        tail step on the deconvolved frames.  phase (an IrPhase whose mode is not "off"): the phase step after it.  filter
        (an IrFilter whose op is not "off"): the filter step after that, the session's rate being the sweep's.  match (an
        IrMatch whose mode is not "off"): the match step after that.  parts (an IrParts whose mode is not "off"): the parts
        step after that.  The getters report each step as after prepare()."""
        lr = _f32(getattr(recording, "buffer", recording)).reshape(-1, 2)
        s = sweep.to_c()
        if not sweep.rate and self.sample_rate:
            s.rate = int(self.sample_rate)
        if ir_frames is None:
            ir_frames = max(1, lr.shape[0] - int(s.frames) + 1 - int(offset))
            ir_frames = max(1, min(ir_frames, SWEEP_MAX_FRAMES, SWEEP_MAX_WORK // max(int(s.frames), 1)))
        steps, keep = _c_steps(shape, eq, damp, tail, phase, filter, match, parts)
        check(self._L.mc_load_ir_sweep_parts(self._h, idx, _fp(lr), lr.shape[0], nframes, C.byref(s), int(offset), int(ir_frames), *steps))

    def onProcess(self, in1, in2):
        """One JACK period (conv.cu:287-466): returns (L, R) float32 arrays."""
        in1, in2 = _f32(in1), _f32(in2)
        n = in1.shape[0]
        outL, outR = np.empty(n, np.float32), np.empty(n, np.float32)
        check(self._L.mc_process(self._h, _fp(in1), _fp(in2), _fp(outL), _fp(outR), n))
        return outL, outR

    def onMidiMessage(self, sender, buffer):
        """conv.cu:278-285: a 3-byte controller message from `sender`."""
        if len(buffer) < 3:
            return
        for half, cc in enumerate(self.cc):
            if cc.device is sender and cc.message == buffer[0]:
                arr = (C.c_uint8 * 8)(*cc.ccmap())
                check(self._L.mc_handle_cc(self._h, half, arr, buffer[1], buffer[2]))

    def avgRuntime(self):
        return self._L.mc_avg_runtime_ms(self._h)

    # -- throughput surface -----------------------------------------------------
    def process(self, in1, in2, out=None):
        """Consecutive blocks from host arrays (length a multiple of 256) in ONE mc_process_batch call; returns
        float32 [2, n].  The engine cuts long runs into chunks itself (16384 blocks through its pinned staging
        buffer for pageable arrays; its preferred batch, three streams, for pinned ones - `pinned_array`)."""
        in1, in2 = _f32(in1), _f32(in2)
        n = in1.shape[0]
        if n % MC_BLOCK or in2.shape[0] != n:
            raise ValueError("inputs must have equal length, a multiple of 256")
        if out is None:
            out = np.empty((2, n), np.float32)
        elif (not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != (2, n)
              or not out[0].flags.c_contiguous or not out[1].flags.c_contiguous or not out.flags.writeable):
            # the library writes n float32 values through each row pointer: anything else would be written past or across
            raise ValueError("out must be a writeable float32 array of shape (2, n) with C-contiguous rows")
        check(self._L.mc_process_batch(self._h, _fp(in1), _fp(in2), _fp(out[0]), _fp(out[1]), n // MC_BLOCK))
        return out

    def pinned_array(self, shape):
        """float32 array in pinned host memory (mc_host_alloc): buffers of this kind let mc_process_batch overlap
        copy-in, kernels and copy-out.  Freed with the array (keeps a reference to its allocation)."""
        n = int(np.prod(shape))
        p = self._L.mc_host_alloc(n * 4)
        if not p:
            raise MemoryError("mc_host_alloc failed")
        buf = (C.c_float * n).from_address(p)
        weakref.finalize(buf, self._L.mc_host_free, p)  # every view of the array keeps `buf` alive
        return np.frombuffer(buf, dtype=np.float32).reshape(shape)

    def process_device(self, d_in1, d_in2, d_outL, d_outR, nblocks):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()); asynchronous."""
        check(self._L.mc_process_batch_device(self._h, d_in1, d_in2, d_outL, d_outR, nblocks))

    def process_slice_device(self, d_in1, d_in2, d_outL, d_outR, nblocks, first, count):
        """Block-sliced operation: the same batch on every GPU, this engine finishes output blocks
        [first, first + count) into d_outL / d_outR (count * 256 floats each); asynchronous."""
        check(self._L.mc_process_batch_slice_device(self._h, d_in1, d_in2, d_outL, d_outR, nblocks, first, count))

    def partial_device(self, d_in1, d_in2, d_partial, nblocks):
        check(self._L.mc_partial_batch_device(self._h, d_in1, d_in2, d_partial, nblocks))

    def finish_device(self, d_in1, d_in2, d_wet_sum, d_outL, d_outR, nblocks):
        check(self._L.mc_finish_batch_device(self._h, d_in1, d_in2, d_wet_sum, d_outL, d_outR, nblocks))

    def finish_slice_device(self, d_in1, d_in2, d_wet_sum_slice, d_outL, d_outR, nblocks, first, count):
        """The finish after a reduce-scatter: d_wet_sum_slice = [L | R] of blocks [first, first + count) only."""
        check(self._L.mc_finish_batch_slice_device(self._h, d_in1, d_in2, d_wet_sum_slice, d_outL, d_outR, nblocks, first, count))

    def sync(self):
        check(self._L.mc_sync(self._h))

    def fence(self):
        """Pipelined engines: the engine's stream waits for every batch issued so far (outputs complete in stream
        order after this)."""
        check(self._L.mc_fence(self._h))

    def fence_older(self):
        """... every batch except the most recently issued one."""
        check(self._L.mc_fence_older(self._h))

    def set_stream(self, stream_ptr):
        """hipStream_t as an int; None / 0 = the engine's own non-blocking stream (NOT ordered with the default
        stream: use `use_torch_stream` when the buffers are torch tensors)."""
        check(self._L.mc_set_stream(self._h, stream_ptr))

    def use_torch_stream(self, stream=None):
        """Launch on `stream` (default: torch's current stream) so that the engine is ordered with the torch ops
        and collectives that produce and consume its device buffers.  torch reports the default stream as handle 0,
        which mc_set_stream reads as "own stream": MC_STREAM_DEFAULT (hipStreamLegacy) names it explicitly."""
        import torch

        ptr = (stream or torch.cuda.current_stream()).cuda_stream
        check(self._L.mc_set_stream(self._h, ptr if ptr else 1))

    # -- introspection ----------------------------------------------------------
    def num_irs(self):
        return self._L.mc_num_irs(self._h)

    def ir_info(self, idx):
        out = (C.c_double * 6)()
        check(self._L.mc_ir_info(self._h, idx, out))
        return dict(sigma=(out[0], out[1]), alpha=(out[2], out[3]), taps=int(out[4]), partitions=int(out[5]))

    def ir_shape_info(self, idx):
        """What the shaped load of IR idx did (mc_ir_shape_info); McError -3 for an IR that was not loaded with a shape.  After a
        load with EQ bands gain, peak and energy are those of the equalised taps and eq_bands counts the bands."""
        out = (C.c_double * 8)()
        check(self._L.mc_ir_shape_info(self._h, idx, out))
        return dict(frames=int(out[0]), onset=int(out[1]), first=int(out[2]), taps=int(out[3]), gain=out[4], peak=out[5], energy=out[6],
                    eq_bands=int(out[7]))

    def ir_damp_info(self, idx):
        """What the damped load of IR idx did (mc_ir_damp_info): the crossovers, the tap the envelopes started at and the
        bands that were given a decay.  McError (MC_ERR_STATE) for an IR whose last load was not damped."""
        out = (C.c_double * 4)()
        check(self._L.mc_ir_damp_info(self._h, idx, out))
        return dict(xovers=int(out[0]), origin=int(out[1]), damped_bands=int(out[2]))

    def ir_synth_info(self, idx):
        """What prepare_synth generated for IR idx (mc_ir_synth_info): the frames, the reflections kept (those placed inside
        them) and the first frame of the late field.  McError (MC_ERR_STATE) for an IR whose last load was not synthesised."""
        out = (C.c_double * 4)()
        check(self._L.mc_ir_synth_info(self._h, idx, out))
        return dict(frames=int(out[0]), reflections=int(out[1]), late_start=int(out[2]))

    def ir_room_info(self, idx):
        """What the room of IR idx's load rendered (mc_ir_room_info): the lattice order used, the images kept per channel
        (counted on the device), the direct sound's delay per channel (frames), the frame E from which images were left out
        and the frames up to which the lattice is complete.  McError (MC_ERR_STATE) for an IR whose last load had no room."""
        out = (C.c_double * 8)()
        check(self._L.mc_ir_room_info(self._h, idx, out))
        return dict(order=int(out[0]), images=(int(out[1]), int(out[2])), direct=(out[3], out[4]), last=int(out[5]), complete=int(out[6]))

    def ir_spring_info(self, idx):
        """The plan the spring of IR idx's load was rendered by (mc_ir_spring_info), as spring_plan reports it.  McError
        (MC_ERR_STATE) for an IR whose last load had no spring."""
        out = (C.c_double * 24)()
        check(self._L.mc_ir_spring_info(self._h, idx, out))
        return _spring_numbers(out)

    def ir_plate_info(self, idx):
        """What the plate of IR idx's load summed (mc_ir_plate_info): the modes kept, those with a non-zero amplitude per
        channel, the frame E from which the plate adds nothing, the lowest and the highest kept mode in Hz and the stiffness
        kappa.  McError (MC_ERR_STATE) for an IR whose last load had no plate."""
        out = (C.c_double * 8)()
        check(self._L.mc_ir_plate_info(self._h, idx, out))
        return dict(modes=int(out[0]), sounding=(int(out[1]), int(out[2])), last=int(out[3]), lowest=out[4], highest=out[5], kappa=out[6])

    def ir_room_bands_info(self, idx):
        """The bands of IR idx's load (mc_ir_room_bands_info), as room_bands_plan reports them.  McError (MC_ERR_STATE) for an
        IR whose last load had no bands."""
        out = (C.c_double * 16)()
        check(self._L.mc_ir_room_bands_info(self._h, idx, out))
        return _bands_report(out)

    def ir_room_head_info(self, idx):
        """The head of IR idx's load (mc_ir_room_head_info), as room_head_plan reports it.  McError (MC_ERR_STATE) for an IR
        whose last load had no head."""
        out = (C.c_double * 12)()
        check(self._L.mc_ir_room_head_info(self._h, idx, out))
        return _head_report(out)

    def ir_room_mics_info(self, idx):
        """What the microphones of IR idx's load did to the direct sound (mc_ir_room_mics_info), as room_mics_plan reports it.
        McError (MC_ERR_STATE) for an IR whose last load had no microphones."""
        out = (C.c_double * 8)()
        check(self._L.mc_ir_room_mics_info(self._h, idx, out))
        return _mics_factors(out)

    def ir_sweep_info(self, idx):
        """What prepare_sweep deconvolved for IR idx (mc_ir_sweep_info): the sweep's frames N, the recording's M, the frames
        generated F and the offset.  McError (MC_ERR_STATE) for an IR whose last load was not from a sweep."""
        out = (C.c_double * 4)()
        check(self._L.mc_ir_sweep_info(self._h, idx, out))
        return dict(sweep_frames=int(out[0]), recording_frames=int(out[1]), frames=int(out[2]), offset=int(out[3]))

    def ir_decay(self, idx, bands=(), q=None, onset_db=-20.0, end=0, curve_points=0, rate=None):
        """The decay of the stored taps of IR idx, measured on the device (mc_ir_decay; include/mcconv.h has the definition).
        rate defaults to the engine's sample_rate, then to 44100.  Returns {"origin", "taps", "rows", "curve"}: rows maps
        (band, "L" | "R" | "LR") - band 0 is broadband, band b >= 1 is bands[b - 1] - to {energy, edt, t20, t30, c50, c80, d50, ts}
        (seconds and dB; NaN where the IR does not define one); curve is float64 [1 + len(bands), 3, curve_points] in dB, or
        None."""
        if rate is None:
            rate = self.sample_rate or 44100
        d = DecayQuery(rate=rate, bands=tuple(bands), q=q, onset_db=onset_db, end=end, curve_points=curve_points).to_c()
        groups = 1 + d.n_bands
        rows = np.empty((groups, 3, 8), np.float64)
        curve = np.empty((groups, 3, d.curve_points), np.float64) if d.curve_points else None
        info = (C.c_uint64 * 2)()
        dp = C.POINTER(C.c_double)
        check(self._L.mc_ir_decay(self._h, idx, C.byref(d), rows.ctypes.data_as(dp), curve.ctypes.data_as(dp) if curve is not None else None, info))
        return dict(origin=int(info[0]), taps=int(info[1]), curve=curve,
                    rows={(b, name): dict(zip(DECAY_FIELDS, (float(v) for v in rows[b, s]))) for b in range(groups) for s, name in enumerate(DECAY_SETS)})

    def ir_floor(self, idx, xovers=(), onset_db=-20.0, end=0, window=0, tail_fraction=0.1, margin_db=10.0, span_db=20.0, per_decade=5, rounds=5,
                 rate=None):
        """The noise floor of the stored taps of IR idx, searched for on the device (mc_ir_floor; include/mcconv.h has the
        method).  rate defaults to the engine's sample_rate, then to 44100.  Returns {"origin", "taps", "groups", "query",
        "rows"}: rows maps (group, "L" | "R" | "LR") - group 0 is broadband, with crossovers group j + 1 is band j of
        IrDamp's split, low to high - to {energy, noise (power per tap), knee (tap, fractional), t (the late decay time,
        seconds), peak_to_noise_db, interval (taps), last_change (taps), status}; status 1: too short or silent, 2: no decay
        above the floor, 3: a silent tail, no floor (knee = taps); NaN where a row has a status.  A clean IR has a knee near
        its end too: look at peak_to_noise_db before acting on one.  tail_from_floor turns the result into an IrTail."""
        if rate is None:
            rate = self.sample_rate or 44100
        query = FloorQuery(rate=rate, xovers=tuple(xovers), onset_db=onset_db, end=end, window=window, tail_fraction=tail_fraction,
                           margin_db=margin_db, span_db=span_db, per_decade=per_decade, rounds=rounds)
        q = query.to_c()
        groups = 1 + (q.n_xovers + 1 if q.n_xovers else 0)
        rows = np.empty((groups, 3, 8), np.float64)
        info = (C.c_uint64 * 2)()
        check(self._L.mc_ir_floor(self._h, idx, C.byref(q), rows.ctypes.data_as(C.POINTER(C.c_double)), info))
        return dict(origin=int(info[0]), taps=int(info[1]), groups=groups, query=query,
                    rows={(g, name): dict(zip(FLOOR_FIELDS, (float(v) for v in rows[g, s]))) for g in range(groups) for s, name in enumerate(DECAY_SETS)})

    def ir_density(self, idx, half=0, hop=0, onset_db=-20.0, end=0, threshold=1.0, decay_t60=0, profile=False, rate=None):
        """The echo density of the stored taps of IR idx, measured on the device (mc_ir_density; include/mcconv.h has the
        definition).  rate defaults to the engine's sample_rate, then to 44100.  Returns {"origin", "taps", "centres", "hop",
        "half", "rows", "profile"}: rows maps "L" | "R" | "LR" to {mix (the mixing tap), mix_s (seconds after the origin), first
        (the density of the first window), max, max_tap, mean_after (the mean density from the mixing tap on), silent (windows
        without a signal), status}; status 1: the density never reached the threshold, and mix, mix_s and mean_after are NaN.
        profile is float64 [centres, 3], window i centred on tap origin + i hop, or None."""
        if rate is None:
            rate = self.sample_rate or 44100
        q = DensityQuery(rate=rate, half=half, hop=hop, onset_db=onset_db, threshold=threshold, end=end, decay_t60=decay_t60).to_c()
        H = q.half or int(math.floor(0.01 * q.rate + 0.5))
        step = q.hop or max(1, H // 4)
        rows = np.empty((3, 8), np.float64)
        prof = None
        if profile:
            try:
                taps = int(self.ir_info(idx)["taps"])
            except _lib.McError:
                taps = 1  # (not loaded: the call below says so, after it has checked the query)
            n = min(q.end, taps) if q.end else taps
            prof = np.empty((max(n - 1, 0) // step + 1, 3), np.float64)
        info = (C.c_uint64 * 3)()
        dp = C.POINTER(C.c_double)
        check(self._L.mc_ir_density(self._h, idx, C.byref(q), rows.ctypes.data_as(dp), prof.ctypes.data_as(dp) if prof is not None else None, info))
        return dict(origin=int(info[0]), taps=int(info[1]), centres=int(info[2]), hop=step, half=H,
                    rows={name: dict(zip(DENSITY_FIELDS, (float(v) for v in rows[s]))) for s, name in enumerate(DECAY_SETS)},
                    profile=prof[:int(info[2])].copy() if prof is not None else None)

    def ir_iacc(self, idx, bands=(), q=None, max_lag=None, split=0, onset_db=-20.0, end=0, curve=False, rate=None):
        """The interaural cross-correlation of the stored taps of IR idx, measured on the device (mc_ir_iacc; include/mcconv.h
        has the definition).  rate defaults to the engine's sample_rate, then to 44100; max_lag=None is 1 ms at that rate,
        floor(0.001 rate + 0.5) taps; split is the early window's length in taps (0: 80 ms).  Returns {"origin", "taps", "split" (the
        first late tap), "max_lag", "rows", "curve"}: rows maps (g, "early" | "late" | "all") - group 0 is broadband, group g >= 1 is
        bands[g - 1] - to {energy_l, energy_r, iacc, lag (tau* in taps, positive: R is late), iacf (IACF(tau*), signed), iacf0,
        level_db (L over R), status}; status 1: an empty window or a silent channel, and all but the energies are NaN.  curve is
        float64 [1 + len(bands), 3, 2 max_lag + 1], IACF at lags -max_lag .. max_lag, or None."""
        if rate is None:
            rate = self.sample_rate or 44100
        if len(bands) > _lib.MC_DECAY_MAX_BANDS:
            raise ValueError(f"{len(bands)} bands; at most {_lib.MC_DECAY_MAX_BANDS}")
        c = McIaccQuery()
        self._L.mc_default_iacc_query(C.byref(c))
        c.rate, c.n_bands = int(rate), len(bands)
        c.max_lag = int(math.floor(0.001 * c.rate + 0.5)) if max_lag is None else int(max_lag)
        for k, hz in enumerate(bands):
            c.centre_hz[k] = float(hz)
        if q is not None:
            c.q = float(q)
        c.onset_db, c.end, c.split = float(onset_db), int(end), int(split)
        groups, lags = 1 + c.n_bands, 2 * min(c.max_lag, _lib.MC_IACC_MAX_LAG) + 1  # (a max_lag above the bound: the call says so)
        rows = np.empty((groups, 3, 8), np.float64)
        cv = np.empty((groups, 3, lags), np.float64) if curve else None
        info = (C.c_uint64 * 3)()
        dp = C.POINTER(C.c_double)
        check(self._L.mc_ir_iacc(self._h, idx, C.byref(c), rows.ctypes.data_as(dp), cv.ctypes.data_as(dp) if cv is not None else None, info))
        return dict(origin=int(info[0]), taps=int(info[1]), split=int(info[2]), max_lag=int(c.max_lag), curve=cv,
                    rows={(g, name): dict(zip(IACC_FIELDS, (float(v) for v in rows[g, w]))) for g in range(groups) for w, name in enumerate(IACC_WINDOWS)})

    def ir_sti(self, idx, bands=None, alpha=None, beta=None, mod_hz=None, snr_db=None, q=None, onset_db=-20.0, end=0, rate=None):
        """The speech transmission index of the stored taps of IR idx, measured on the device (mc_ir_sti; include/mcconv.h has
        the definition).  rate defaults to the engine's sample_rate, then to 44100.  bands=None means the seven octaves 125 Hz ..
        8 kHz with IEC 60268-16's weights for male speech; bands of one's own need alpha (one weight per band) and beta (one per
        pair of neighbours) too: ValueError without them.  mod_hz=None means the standard's 14 modulation frequencies.  snr_db, one
        value per band, adds stationary noise at that signal-to-noise ratio.  Returns {"origin", "taps", "sti", "rows", "mtf"}: sti
        maps "L" | "R" | "LR" to the index (NaN without bands or with a silent band: sti_rating gives the word for a number); rows
        maps (g, "L" | "R" | "LR") - group 0 is broadband, group g >= 1 is bands[g - 1] - to {energy, mti, status}; status 1: no
        energy, and mti is NaN.  mtf is float64 [1 + len(bands), 3, len(mod_hz)], the modulation transfer function."""
        if rate is None:
            rate = self.sample_rate or 44100
        c = McStiQuery()
        self._L.mc_default_sti_query(C.byref(c))
        if bands is None:
            bands = tuple(c.centre_hz)
            alpha = tuple(c.alpha) if alpha is None else alpha
            beta = tuple(c.beta) if beta is None else beta
        elif alpha is None or beta is None:
            raise ValueError("bands of one's own need alpha and beta: the default weights belong to the seven octaves")
        mod_hz = tuple(c.mod_hz)[:c.n_mod] if mod_hz is None else tuple(mod_hz)
        if len(bands) > _lib.MC_STI_MAX_BANDS:
            raise ValueError(f"{len(bands)} bands; at most {_lib.MC_STI_MAX_BANDS}")
        if len(alpha) != len(bands) or len(beta) != max(len(bands) - 1, 0):
            raise ValueError(f"{len(bands)} bands need {len(bands)} alpha and {max(len(bands) - 1, 0)} beta; got {len(alpha)} and {len(beta)}")
        if not 1 <= len(mod_hz) <= _lib.MC_STI_MAX_MOD:
            raise ValueError(f"{len(mod_hz)} modulation frequencies; 1 to {_lib.MC_STI_MAX_MOD}")
        if snr_db is not None and len(snr_db) != len(bands):
            raise ValueError(f"{len(bands)} bands need {len(bands)} snr_db; got {len(snr_db)}")
        c.rate, c.n_bands, c.n_mod = int(rate), len(bands), len(mod_hz)
        c.flags = _lib.MC_STI_SNR if snr_db is not None else 0
        for name, values in (("centre_hz", bands), ("alpha", alpha), ("beta", beta), ("snr_db", () if snr_db is None else snr_db), ("mod_hz", mod_hz)):
            field = getattr(c, name)
            for k in range(len(field)):
                field[k] = float(values[k]) if k < len(values) else 0.0
        if q is not None:
            c.q = float(q)
        c.onset_db, c.end = float(onset_db), int(end)
        groups = 1 + c.n_bands
        rows = np.empty((groups, 3, 4), np.float64)
        mtf = np.empty((groups, 3, c.n_mod), np.float64)
        sti = (C.c_double * 3)()
        info = (C.c_uint64 * 2)()
        dp = C.POINTER(C.c_double)
        check(self._L.mc_ir_sti(self._h, idx, C.byref(c), rows.ctypes.data_as(dp), mtf.ctypes.data_as(dp), sti, info))
        return dict(origin=int(info[0]), taps=int(info[1]), sti={name: float(sti[s]) for s, name in enumerate(DECAY_SETS)}, mtf=mtf,
                    rows={(g, name): dict(energy=float(rows[g, s, 0]), mti=float(rows[g, s, 1]), status=int(rows[g, s, 2]))
                          for g in range(groups) for s, name in enumerate(DECAY_SETS)})

    def ir_response(self, idx, hz=None, windows=None, onset_db=-20.0, end=0, rate=None):
        """The frequency response of the stored taps of IR idx, measured on the device (mc_ir_response; include/mcconv.h has the
        definition).  rate defaults to the engine's sample_rate, then to 44100.  hz=None means response_grid() clipped to 0.45 rate;
        at most 1024 frequencies, each in [0, rate / 2].  windows=None is the whole span from the origin; otherwise up to 64 windows,
        each a (first, count, rise, fall) tuple in taps from the origin or None for the whole span (waterfall_windows makes a row of
        them); a window clips to the span.  Returns {"origin", "taps", "hz", "spans", "rows", "h", "delay", "db", "phase"}: hz as
        float32; spans int [n_win, 2], the taps [a, b) of each window; h complex128 [n_win, 2, n_freq], phase counted from the
        origin; delay the group delay in taps from the origin (NaN where |H| = 0); db = 20 log10 |H| (-400 where |H| = 0); phase =
        atan2(Im, Re); rows maps (w, "L" | "R") to {energy, abs_sum, status}; status 1: a window without taps or a silent one,
        h is 0 and delay NaN."""
        if rate is None:
            rate = self.sample_rate or 44100
        if hz is None:
            hz = response_grid(20.0, min(20000.0, 0.45 * rate))
        hz = _f32(hz).reshape(-1)
        windows = [None] if windows is None else list(windows)
        if not 1 <= hz.size <= _lib.MC_RSP_MAX_FREQ:
            raise ValueError(f"{hz.size} frequencies; 1 to {_lib.MC_RSP_MAX_FREQ}")
        if not 1 <= len(windows) <= _lib.MC_RSP_MAX_WIN:
            raise ValueError(f"{len(windows)} windows; 1 to {_lib.MC_RSP_MAX_WIN}")
        c = McResponseQuery()
        self._L.mc_default_response_query(C.byref(c))
        c.rate, c.n_freq, c.n_win, c.onset_db, c.end = int(rate), hz.size, len(windows), float(onset_db), int(end)
        win = (McResponseWindow * len(windows))()
        for k, w in enumerate(windows):
            win[k].first, win[k].count, win[k].rise, win[k].fall = (0, 0, 0, 0) if w is None else (int(v) for v in w)
        resp = np.empty((len(windows), 2, hz.size, 3), np.float64)
        rows = np.empty((len(windows), 2, 4), np.float64)
        spans = np.empty((len(windows), 2), np.uint64)
        info = (C.c_uint64 * 2)()
        dp = C.POINTER(C.c_double)
        check(self._L.mc_ir_response(self._h, idx, C.byref(c), _fp(hz), win, resp.ctypes.data_as(dp), rows.ctypes.data_as(dp),
                                     spans.ctypes.data_as(C.POINTER(C.c_uint64)), info))
        h = resp[..., 0] + 1j * resp[..., 1]
        mag = np.abs(h)
        with np.errstate(divide="ignore"):
            db = np.where(mag > 0.0, np.maximum(20.0 * np.log10(mag), RESPONSE_FLOOR_DB), RESPONSE_FLOOR_DB)
        return dict(origin=int(info[0]), taps=int(info[1]), hz=hz.copy(), spans=spans.astype(np.int64), h=h, delay=resp[..., 2].copy(), db=db,
                    phase=np.arctan2(resp[..., 1], resp[..., 0]),
                    rows={(w, name): dict(energy=float(rows[w, s, 0]), abs_sum=float(rows[w, s, 1]), status=int(rows[w, s, 2]))
                          for w in range(len(windows)) for s, name in enumerate(RESPONSE_CHANNELS)})

    def ir_tail_info(self, idx):
        """What the tail step of IR idx's load did (mc_ir_tail_info): the bands it touched, the frames that came in, the frames
        it handed on and the first frame it changed.  McError (MC_ERR_STATE) for an IR whose last load had no tail step."""
        out = (C.c_double * 4)()
        check(self._L.mc_ir_tail_info(self._h, idx, out))
        return dict(bands=int(out[0]), frames=int(out[1]), length=int(out[2]), first=int(out[3]))

    def ir_phase_info(self, idx):
        """What the phase step of IR idx's load did (mc_ir_phase_info): the frames it took and handed on, the transform's length,
        the energy that went in and came out (energy_out / energy_in is what the truncation to `frames` kept), the centres of
        energy in frames (centre_in - centre_out is the delay removed) and the bins of either channel that the floor
        clamped.  McError (MC_ERR_STATE) for an IR whose last load had no phase step."""
        out = (C.c_double * 8)()
        check(self._L.mc_ir_phase_info(self._h, idx, out))
        return dict(frames=int(out[0]), nfft=int(out[1]), energy_in=float(out[2]), energy_out=float(out[3]), centre_in=float(out[4]),
                    centre_out=float(out[5]), clamped=(int(out[6]), int(out[7])))

    def ir_filter_info(self, idx):
        """What the filter step of IR idx's load did (mc_ir_filter_info): the frames it took, the filter's frames at the
        session's rate, the frames it handed on, the transform's length, the energy of the frames, of the filter and of what
        was stored, the energy left behind past frames_out, and the bins of either channel that a deconvolution
        regularised.  McError (MC_ERR_STATE) for an IR whose last load had no filter step."""
        out = (C.c_double * 10)()
        check(self._L.mc_ir_filter_info(self._h, idx, out))
        return dict(frames=int(out[0]), filter_frames=int(out[1]), frames_out=int(out[2]), nfft=int(out[3]), energy_in=float(out[4]),
                    energy_filter=float(out[5]), energy_out=float(out[6]), energy_rest=float(out[7]), regularised=(int(out[8]), int(out[9])))

    def ir_match_info(self, idx):
        """What the match step of IR idx's load did (mc_ir_match_info): the frames it took, the target's frames at the
        session's rate (0 for a flat target), the frames it handed on, the transform's length, the grid's points, the energy
        of the frames, of the target and of what was stored, the energy left behind past frames_out, the mean that was
        taken out of either channel's curve (dB) and the points that ran into boost_db or cut_db.  McError (MC_ERR_STATE)
        for an IR whose last load had no match step."""
        out = (C.c_double * 12)()
        check(self._L.mc_ir_match_info(self._h, idx, out))
        return dict(frames=int(out[0]), target_frames=int(out[1]), frames_out=int(out[2]), nfft=int(out[3]), points=int(out[4]), energy_in=float(out[5]),
                    energy_target=float(out[6]), energy_out=float(out[7]), energy_rest=float(out[8]), mean_db=(float(out[9]), float(out[10])),
                    clamped=int(out[11]))

    def ir_parts_info(self, idx):
        """What the parts step of IR idx's load did (mc_ir_parts_info): the frames it took and handed on, the two boundaries
        clamped to the frames, the weighted energy of the direct, the early and the late part as they came in (muted or not),
        drr_db = 10 log10(direct / (early + late)), the energy of what was stored, and the energy and the number of the
        contributions that landed outside the frames handed on.  McError (MC_ERR_STATE) for an IR whose last load had no parts
        step."""
        out = (C.c_double * 10)()
        check(self._L.mc_ir_parts_info(self._h, idx, out))
        rest = float(out[5]) + float(out[6])
        drr = 10.0 * math.log10(float(out[4]) / rest) if out[4] > 0 and rest > 0 else (math.inf if out[4] > 0 else -math.inf if rest > 0 else math.nan)
        return dict(frames=int(out[0]), frames_out=int(out[1]), direct_end=int(out[2]), early_end=int(out[3]), energy_direct=float(out[4]),
                    energy_early=float(out[5]), energy_late=float(out[6]), drr_db=drr, energy_out=float(out[7]), energy_lost=float(out[8]), lost=int(out[9]))

    def ir_match_curve(self, idx):
        """The curve of IR idx's match step (mc_ir_match_curve): hz [J], before_db [J, 2] (the smoothed difference to the target
        less its mean, per channel) and gain_db [J, 2] (what was applied at those frequencies), float64."""
        cap = _lib.MC_MATCH_MAX_POINTS
        hz, before, gain = (C.c_double * cap)(), (C.c_double * (2 * cap))(), (C.c_double * (2 * cap))()
        J = self._L.mc_ir_match_curve(self._h, idx, hz, before, gain, cap)
        if J < 0:
            check(J)
        return dict(hz=np.array(hz[:J]), before_db=np.array(before[:2 * J]).reshape(J, 2), gain_db=np.array(gain[:2 * J]).reshape(J, 2))

    def enable_kernel_timing(self, on=True):
        check(self._L.mc_enable_kernel_timing(self._h, 1 if on else 0))

    def kernel_stats(self, reset=False):
        """Timing of the launches that finish a call's own blocks (enable_kernel_timing) and the form the last of them took:
        `resident`, `partitions` swept and `fast_levels`, the form's code - 0 direct, 1..3 fast-FIR levels, 255 / 254 split / fused
        second-level transform, 253 overlap-save (the table in DESIGN.md §2.5c)."""
        ks = McKernelStats()
        check(self._L.mc_get_kernel_stats(self._h, C.byref(ks), 1 if reset else 0))
        return dict(launches=ks.launches, blocks=ks.blocks, total_ms=ks.total_ms, last_ms=ks.last_ms,
                    resident=bool(ks.resident), partitions=ks.partitions, fast_levels=ks.fast_levels)

    def algorithmic_bytes_per_block(self):
        return self._L.mc_algorithmic_bytes_per_block(self._h)

    def preferred_batch(self, at_most):
        """Batch length (blocks) <= at_most that wastes nothing of the second-level transform's chunks for the
        loaded IRs (mc_preferred_batch)."""
        return int(self._L.mc_preferred_batch(self._h, int(at_most)))

    def blocks_processed(self):
        return self._L.mc_blocks_processed(self._h)

    def park_stats(self):
        """JACK path: how many parked periods were used, gave up on their own (host away longer than the park time)
        and were told to give up (mc_debug_read item 6; host-side counters, no stream access)."""
        a = np.zeros(3, np.uint64)
        check(self._L.mc_debug_read(self._h, 6, 0, a.ctypes.data_as(C.c_void_p), 0, a.nbytes, None))
        return dict(used=int(a[0]), timed_out=int(a[1]), cancelled=int(a[2]))

    def tail_forms(self):
        """JACK path, 256-frame periods: tails by the form partition 0 took - frequency domain (the period was already there when
        the tail looked: calls back to back, periods launched on arrival) or time domain (a parked tail that had to wait).
        Counted by the kernel (mc_debug_read item 16; leaves the JACK path and waits for the stream)."""
        a = np.zeros(2, np.uint32)
        check(self._L.mc_debug_read(self._h, 16, 0, a.ctypes.data_as(C.c_void_p), 0, a.nbytes, None))
        return dict(frequency_domain=int(a[0]), time_domain=int(a[1]))

    def drop_stats(self):
        """Q8 regime: batches by the form their cut terms took (mc_debug_read item 9; host-side counters)."""
        a = np.zeros(4, np.uint64)
        check(self._L.mc_debug_read(self._h, 9, 0, a.ctypes.data_as(C.c_void_p), 0, a.nbytes, None))
        return dict(drop_fft=int(a[0]), forward_transforms=int(a[1]), tiles=int(a[2]), carried_periods=int(a[3]))

    def mac_stats(self):
        """Batch launches by the form their partition sums took (mc_debug_read item 10; host-side counters): `resident` counts the
        direct and the fast-FIR form, the streaming MAC has no counter, the overlap-save passes count in os_stats() (the table in
        DESIGN.md §2.5c)."""
        a = np.zeros(3, np.uint64)
        check(self._L.mc_debug_read(self._h, 10, 0, a.ctypes.data_as(C.c_void_p), 0, a.nbytes, None))
        return dict(fused=int(a[0]), split=int(a[1]), resident=int(a[2]))

    def os_stats(self):
        """Batches that took the overlap-save form of long settled batches and builds of its spectra (mc_debug_read
        item 11; host-side counters)."""
        a = np.zeros(2, np.uint64)
        check(self._L.mc_debug_read(self._h, 11, 0, a.ctypes.data_as(C.c_void_p), 0, a.nbytes, None))
        return dict(batches=int(a[0]), spectra_builds=int(a[1]))

    def param_generation(self, published=False):
        """Generation number of the parameter pair the last process call ran on (published=True: of the pair
        published last).  Every mc_set_params / mc_handle_cc publishes a new pair (csrc/params_handoff.h)."""
        a = np.zeros(1, np.uint64)
        check(self._L.mc_debug_read(self._h, 8 if published else 7, 0, a.ctypes.data_as(C.c_void_p), 0, a.nbytes, None))
        return int(a[0])

    def debug_dims(self):
        d = (C.c_uint64 * 4)()
        check(self._L.mc_debug_read(self._h, 1, 0, None, 0, 0, d))
        return dict(pstride=d[0], ring=d[1], max_batch=d[2], wet_ring=d[3])

    def debug_read(self, which, idx, dtype, offset_elems, count):
        a = np.empty(count, dtype=dtype)
        check(self._L.mc_debug_read(self._h, which, idx, a.ctypes.data_as(C.c_void_p), offset_elems * a.itemsize,
                                    a.nbytes, None))
        return a

    def ir_taps(self, idx):
        """The stored time-domain taps of IR idx, float32 [taps, 2] (mc_debug_read item 17)."""
        n = int(self.ir_info(idx)["taps"])
        return self.debug_read(17, idx, np.float32, 0, 2 * n).reshape(n, 2)

    def ir_spectra16(self, idx):
        """The fp16 copy of IR idx's spectra as stored, uint16 [256 bins][pstride][4] {L.re, L.im, R.re, R.im} (mc_debug_read
        item 18; fp16 engines only).  idx may name a merged-IR entry (256 ..)."""
        ps = self.debug_dims()["pstride"]
        return self.debug_read(18, idx, np.uint16, 0, 256 * ps * 4).reshape(256, ps, 4)

    def ir_spectra32(self, idx):
        """The fp32 spectra of IR idx as stored, float32 [256 bins][pstride][4] (mc_debug_read item 0), padding included."""
        ps = self.debug_dims()["pstride"]
        return self.debug_read(0, idx, np.float32, 0, 256 * ps * 4).reshape(256, ps, 4)

    def ir_scale16(self, idx):
        """The power-of-two scale of IR idx's fp16 copy (mc_debug_read item 20; fp16 engines only)."""
        return float(self.debug_read(20, idx, np.float32, 0, 1)[0])

    def delay_line(self):
        """The delay line as stored, float32 [256 bins][ring][4] {in1.re, in1.im, in2.re, in2.im} (mc_debug_read item 1)."""
        ring = self.debug_dims()["ring"]
        return self.debug_read(1, 0, np.float32, 0, 256 * ring * 4).reshape(256, ring, 4)

    def delay_line16(self):
        """The delay line's fp16 mirror as stored, uint16 [256 bins][ring][4] (mc_debug_read item 19; fp16 engines only)."""
        ring = self.debug_dims()["ring"]
        return self.debug_read(19, 0, np.uint16, 0, 256 * ring * 4).reshape(256, ring, 4)

    def slot_gains(self):
        """The gains of the delay line's slots, float32 [3 voice rows][ring][4] {L<-in1, L<-in2, R<-in1, R<-in2}
        (mc_debug_read item 21)."""
        ring = self.debug_dims()["ring"]
        return self.debug_read(21, 0, np.float32, 0, 3 * ring * 4).reshape(3, ring, 4)

    def ir_spectra(self, idx):
        """IR spectra as complex [2 ch][partitions][256 packed bins] (diagnostics)."""
        info, dims = self.ir_info(idx), self.debug_dims()
        ps = dims["pstride"]
        raw = self.debug_read(0, idx, np.float32, 0, 256 * ps * 4).reshape(256, ps, 4)
        P = info["partitions"]
        HL = raw[:, :P, 0] + 1j * raw[:, :P, 1]
        HR = raw[:, :P, 2] + 1j * raw[:, :P, 3]
        return np.stack([HL.T, HR.T])
