"""Float64 restatement of the sweep capture (mc_sweep, mc_sweep_generate, mc_load_ir_sweep; include/mcconv.h has the
definition): the exponential sine sweep, the deconvolution weights and the correlation, the last as one masked dot per
output.  Every float field enters as the float32 the C struct holds, widened to double, as the library takes it."""
import numpy as np


def _f(x):
    return float(np.float32(x))


def _plan(frames, f1_hz, f2_hz, rate, amplitude=0.5):
    N, f1, f2, A = int(frames), _f(f1_hz), _f(f2_hz), _f(amplitude)
    Ls = (N - 1) / np.log(f2 / f1)
    return N, f1, f2, A, Ls


def phase(frames, f1_hz, f2_hz, rate, **_):
    """phi(n), n = 0 .. N - 1."""
    N, f1, f2, _, Ls = _plan(frames, f1_hz, f2_hz, rate)
    return (2.0 * np.pi * f1 * Ls / float(rate)) * np.expm1(np.arange(N, dtype=np.float64) / Ls)


def window(frames, fade_in=0, fade_out=0, **_):
    N = int(frames)
    w = np.ones(N)
    n = np.arange(fade_in, dtype=np.float64)
    w[:fade_in] *= 0.5 * (1.0 - np.cos(np.pi * (n + 1.0) / (fade_in + 1.0)))
    k = np.arange(fade_out, dtype=np.float64)
    w[N - fade_out:] *= 0.5 * (1.0 + np.cos(np.pi * (k + 1.0) / (fade_out + 1.0)))
    return w


def sweep(frames, f1_hz=20.0, f2_hz=20000.0, rate=44100, amplitude=0.5, fade_in=0, fade_out=0):
    """s64: the unrounded sweep."""
    return _f(amplitude) * window(frames, fade_in, fade_out) * np.sin(phase(frames, f1_hz, f2_hz, rate))


def weights(frames, f1_hz=20.0, f2_hz=20000.0, rate=44100, amplitude=0.5, fade_in=0, fade_out=0):
    """u[j] = (4 f2 / (A^2 Ls rate)) s64[j] exp(-(N - 1 - j) / Ls)."""
    N, _, f2, A, Ls = _plan(frames, f1_hz, f2_hz, rate, amplitude)
    s = sweep(frames, f1_hz, f2_hz, rate, amplitude, fade_in, fade_out)
    return (4.0 * f2 / (A * A * Ls * float(rate))) * s * np.exp(-(N - 1 - np.arange(N, dtype=np.float64)) / Ls)


def deconvolve(recording, sw, offset, ir_frames):
    """h[m] = sum_j u[j] r[m + j + offset], r = 0 outside the recording; [ir_frames, 2] in float64 (the library rounds it to
    float32 once).  recording: [M, 2]; sw: the keyword arguments of sweep()."""
    r = np.asarray(recording, dtype=np.float32).astype(np.float64).reshape(-1, 2)
    u = weights(**sw)
    M, N = len(r), len(u)
    h = np.zeros((int(ir_frames), 2))
    for m in range(int(ir_frames)):
        lo = m + int(offset)  # the recording's frame under u[0]
        j0, j1 = max(0, -lo), min(N, M - lo)
        if j1 > j0:
            h[m] = u[j0:j1] @ r[lo + j0:lo + j1]
    return h


def band_db(h, sw, points=8192):
    """The magnitude of one channel of an IR in dB over a `points` transform, between 4 f1 and f2 / 2: (min, max)."""
    H = np.abs(np.fft.rfft(h, points))
    hz = np.arange(len(H)) * float(sw["rate"]) / points
    sel = (hz >= 4.0 * sw["f1_hz"]) & (hz <= 0.5 * sw["f2_hz"])
    db = 20.0 * np.log10(H[sel])
    return float(db.min()), float(db.max())
