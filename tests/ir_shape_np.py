"""Float64 restatement of the IR shaping on load (mc_load_ir_shaped, cuda_audio_amd/csrc/irshape.hip.h).

Test infrastructure only: the product never imports it.  Order of operations (include/mcconv.h):
  1. the whole IR is converted to the session's rate when the rates differ (resample_np.resample) and rounded to float32,
     as the engine holds converted frames; F frames;
  2. s0 = min(start, F); trim_db < 0: a[m] = max(|L|, |R|) in float32 over frames s0 .. F - 1, peak = max a,
     t = peak * float32(10^(trim_db / 20)) as a float32 product, onset = the first m with a[m] >= t;
     first = s0 + max(0, onset - pre_roll);
  3. n = min(F - first, length or unlimited, cap) frames are kept (cap = n_ref - nframes); n = 0 raises ValueError;
  4. reversed if asked;
  5. tap m times exp2(-m 3 log2(10) / decay_t60);
  6. tap n - f + k (f = min(fade_out, n), k = 0 .. f - 1) times 0.5 (1 + cos(pi (k + 1) / (f + 1)));
  7. peak = max |tap|, energy = sqrt(sum (hL^2 + hR^2) / 2); gain = target / peak or target / energy (1 when that measure is 0
     or normalisation is off); stored tap = float32(value * gain).
"""
import numpy as np

from resample_np import resample

DECAY_K = 3.0 * np.log2(10.0)


def session_frames(x, src=None, dst=None):
    """Step 1: float32 [F, 2] frames at the session's rate."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 2)
    if src is None or dst is None or src == dst:
        return x
    return resample(x, src, dst).astype(np.float32)


def onset_of(xs, start=0, trim_db=0.0):
    """Step 2 on session-rate float32 frames: (s0, onset, threshold, a) with a = float32 max(|L|, |R|) of the frames after s0."""
    s0 = min(int(start), xs.shape[0])
    a = np.abs(xs[s0:]).max(axis=1) if xs.shape[0] > s0 else np.zeros(0, np.float32)
    if not trim_db < 0 or a.size == 0:
        return s0, 0, np.float32(0), a
    t = np.float32(a.max()) * np.float32(10.0 ** (float(np.float32(trim_db)) / 20.0))
    assert t.dtype == np.float32
    hit = np.nonzero(a >= t)[0]
    return s0, (int(hit[0]) if hit.size else 0), t, a


def onset_margin(xs, start=0, trim_db=0.0):
    """(largest frame before the onset / threshold, onset frame / threshold): a device that compares frames a rounding
    away from these must find the same onset when the first is well below 1 and the second well above."""
    _, onset, t, a = onset_of(xs, start, trim_db)
    below = float(a[:onset].max()) / float(t) if onset else 0.0
    return below, float(a[onset]) / float(t)


def assert_onset_margin(xs, start=0, trim_db=0.0):
    """What every test that trims asserts on the restatement first: the device's frames differ from these by at most 1e-5 of
    the peak (1e-4 of a -20 dB threshold), so a margin of 0.8 / 1.25 around the threshold pins the onset."""
    below, above = onset_margin(xs, start, trim_db)
    assert below <= 0.8 and above >= 1.25, (below, above)


def shape64(x, cap, src=None, dst=None, *, start=0, trim_db=0.0, pre_roll=0, length=0, reverse=False, decay_t60=0, fade_out=0,
            normalize=None, target=1.0):
    """x: [frames, 2] at src Hz (or at the session's rate); returns (float64 taps [n, 2] before the rounding of step 7, info)
    with info as Convolution.ir_shape_info gives it."""
    xs = session_frames(x, src, dst)
    F = xs.shape[0]
    s0, onset, _, _ = onset_of(xs, start, trim_db)
    first = s0 + max(0, onset - int(pre_roll))
    n = min(F - first, int(cap))
    if length:
        n = min(n, int(length))
    if n <= 0:
        raise ValueError("the shape leaves no frame")
    v = xs[first:first + n].astype(np.float64)
    if reverse:
        v = v[::-1].copy()
    m = np.arange(n, dtype=np.float64)
    if decay_t60:
        v = v * np.exp2(-(m * DECAY_K) / float(decay_t60))[:, None]
    f = min(int(fade_out), n)
    if f:
        k = np.arange(f, dtype=np.float64)
        v[n - f:] = v[n - f:] * (0.5 * (1.0 + np.cos(np.pi * (k + 1.0) / (f + 1.0))))[:, None]
    peak = float(np.abs(v).max())
    energy = float(np.sqrt((v * v).sum() / 2.0))
    measure = {None: 0.0, "peak": peak, "energy": energy}[normalize]
    gain = float(np.float32(target)) / measure if measure > 0.0 else 1.0
    return v * gain, dict(frames=F, onset=onset, first=first, taps=n, gain=gain, peak=peak, energy=energy)


def shape(x, cap, src=None, dst=None, **fields):
    """shape64 with the taps as the engine stores them: float32 [n, 2]."""
    v, info = shape64(x, cap, src, dst, **fields)
    return v.astype(np.float32), info


def quiet_lead_ir(frames=20000, lead=700, seed=31, norm=0.05):
    """The IR the trimming tests use: `lead` frames of Gaussian noise of RMS 1e-5 in front of synth.make_ir."""
    from cuda_audio_amd.synth import make_ir

    noise = (1e-5 * np.random.default_rng(3).standard_normal((lead, 2))).astype(np.float32)
    return np.concatenate([noise, make_ir(frames, seed=seed, norm=norm)], axis=0)
