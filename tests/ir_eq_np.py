"""Float64 restatement of the equalisation of an IR on load (mc_load_ir_eq, cuda_audio_amd/csrc/ireq.hip.h).

Test infrastructure only: the product never imports it.  Steps 1 to 6 are ir_shape_np.shape64's (with the normalisation
off, so that its taps are those before the gain); then
  6b. every band that is on filters the n taps, in order, from rest at tap 0: one biquad each, Audio-EQ-Cookbook
      coefficients in double from the float32 fields, a plain sequential loop (transposed direct form II);
  7.  peak = max |tap|, energy = sqrt(sum (hL^2 + hR^2) / 2) of the result; gain = float32(target) / that measure;
  8.  stored tap = float32(value * gain).
`response` is the analytic H(e^{jw}) of the same coefficients, which no recurrence enters.
"""
import functools

import numpy as np

from ir_shape_np import shape64

KINDS = ("off", "lowcut", "highcut", "lowshelf", "highshelf", "peak")
DEFAULT_Q = 0.70710678


def band_fields(band):
    """(kind, hz, gain_db, q) of a band given as (kind, hz[, gain_db[, q]]), the numbers as the float32 fields hold them."""
    kind, hz, *rest = band
    gain_db = rest[0] if len(rest) > 0 else 0.0
    q = rest[1] if len(rest) > 1 else DEFAULT_Q
    assert kind in KINDS
    return kind, float(np.float32(hz)), float(np.float32(gain_db)), float(np.float32(q))


def coefs(band, rate):
    """(b0, b1, b2, a1, a2) with a0 = 1: include/mcconv.h's table."""
    kind, hz, gain_db, q = band_fields(band)
    w0 = 2.0 * np.pi * hz / float(rate)
    c, al = np.cos(w0), np.sin(w0) / (2.0 * q)
    A = 10.0 ** (gain_db / 40.0)
    r = 2.0 * np.sqrt(A) * al
    if kind == "lowcut":
        b = ((1 + c) / 2, -(1 + c), (1 + c) / 2)
        a = (1 + al, -2 * c, 1 - al)
    elif kind == "highcut":
        b = ((1 - c) / 2, 1 - c, (1 - c) / 2)
        a = (1 + al, -2 * c, 1 - al)
    elif kind == "lowshelf":
        b = (A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r))
        a = ((A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r)
    elif kind == "highshelf":
        b = (A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r))
        a = ((A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r)
    else:
        b = (1 + al * A, -2 * c, 1 - al * A)
        a = (1 + al / A, -2 * c, 1 - al / A)
    return tuple(float(v / a[0]) for v in (b[0], b[1], b[2], a[1], a[2]))


def on_bands(bands):
    return [b for b in bands if b[0] != "off"]


def response(bands, rate, hz):
    """The cascade's complex H(e^{j 2 pi hz / rate}) at the frequencies hz."""
    z1 = np.exp(-2j * np.pi * np.asarray(hz, dtype=np.float64) / float(rate))
    H = np.ones(z1.shape, dtype=np.complex128)
    for band in on_bands(bands):
        b0, b1, b2, a1, a2 = coefs(band, rate)
        H = H * (b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1)
    return H


def response_db(bands, rate, hz):
    return 20.0 * np.log10(np.abs(response(bands, rate, hz)))


def biquad(v, c):
    """One band over the float64 taps v [n, 2], from rest: the sequential recurrence, one tap after the other."""
    b0, b1, b2, a1, a2 = c
    out = np.empty_like(v)
    for ch in range(v.shape[1]):
        s1 = s2 = 0.0
        y = []
        for x in v[:, ch].tolist():
            o = b0 * x + s1
            s1 = b1 * x - a1 * o + s2
            s2 = b2 * x - a2 * o
            y.append(o)
        out[:, ch] = y
    return out


def cascade(v, bands, rate):
    v = np.asarray(v, dtype=np.float64)
    for band in on_bands(bands):
        v = biquad(v, coefs(band, rate))
    return v


def eq64(x, cap, src, dst, bands, *, normalize=None, target=1.0, **fields):
    """x: [frames, 2] at src Hz in a session at dst Hz; returns (float64 taps [n, 2] before the rounding of step 8, info) with
    info as Convolution.ir_shape_info gives it after a load with these bands."""
    v, info = shape64(x, cap, src, dst, normalize=None, **fields)
    v = cascade(v, bands, dst)
    peak = float(np.abs(v).max())
    energy = float(np.sqrt((v * v).sum() / 2.0))
    measure = {None: 0.0, "peak": peak, "energy": energy}[normalize]
    gain = float(np.float32(target)) / measure if measure > 0.0 else 1.0
    info = dict(info, gain=gain, peak=peak, energy=energy, eq_bands=len(on_bands(bands)))
    return v * gain, info


def eq(x, cap, src, dst, bands, **fields):
    """eq64 with the taps as the engine stores them: float32 [n, 2]."""
    v, info = eq64(x, cap, src, dst, bands, **fields)
    return v.astype(np.float32), info


@functools.lru_cache(maxsize=None)
def impulse_taps(bands, rate, n):
    """A unit impulse through the bands (a tuple of tuples), n taps, rounded to float32: [n]."""
    x = np.zeros((n, 1))
    x[0, 0] = 1.0
    return cascade(x, bands, rate)[:, 0].astype(np.float32)
