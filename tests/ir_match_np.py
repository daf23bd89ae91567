"""The match step of an IR load (include/mcconv.h, mc_ir_match; csrc/irmatch.hip.h) restated in float64 with numpy's FFT, one
channel at a time, exactly as the header defines it:

    Nfft = max(16, smallest power of two >= 2 max(F, G)); Pa = |FFT(a_c)|^2, Pt = |FFT(t_c)|^2 for k = 0 .. Nfft / 2
    grid f_j = lo 2^(j / per_octave) <= hi; window k_lo = ceil(f_j 2^(-octaves / 2) Nfft / rate) .. k_hi = floor(f_j 2^(octaves / 2)
    Nfft / rate), clipped to [1, Nfft / 2], the nearest bin when empty; Sa, St = the means over the window (flat: St =
    10^(tilt log2(f_j / 1000) / 10)); linked: the channels' levels added; S = max(S, max S 10^(-floor_db / 10));
    raw = 10 log10(St / Sa); m = mean raw; d = clamp(amount (raw - m), -cut_db, boost_db)
    per bin: u = per_octave log2(k rate / Nfft / lo) clipped to [0, J - 1]; dB interpolated linearly; L = dB ln 10 / 20
    minimum: c = Re IFFT(L), folded; C = exp(FFT(c)); Fo = F.   linear: C = exp(L) e^(-2 pi i (k D mod Nfft) / Nfft); Fo = F + D
    y = Re IFFT(A C); y[0 .. Fo)

and the inputs that the CPU and GPU tests share."""
import math

import numpy as np

MAX_NFFT = 1 << 22
LN10_20 = math.log(10.0) / 20.0


def nfft_of(F, G=0):
    n = 16
    while n < 2 * max(F, G):
        n *= 2
    return n


def grid(lo=20.0, hi=20000.0, per_octave=12):
    """f_j as float64: lo 2^(j / per_octave) while that double is <= hi."""
    out, j = [], 0
    while True:
        v = lo * 2.0 ** (j / per_octave)
        if not v <= hi:
            return np.array(out)
        out.append(v)
        j += 1


def windows(hz, nfft, rate, octaves=1.0 / 3.0):
    """(k_lo [J], k_hi [J], margin): the windows' bins, and how far the nearest edge (or, of an empty window, the centre from a
    half) lies from where a rounding error could move it, in bins."""
    down, up, half = 2.0 ** (-0.5 * octaves), 2.0 ** (0.5 * octaves), nfft // 2
    lo, hi, margin = [], [], math.inf
    for f in hz:
        a, b = f * down * nfft / rate, f * up * nfft / rate
        ka, kb = min(max(math.ceil(a), 1), half), min(max(math.floor(b), 1), half)
        if a > 1.0 and a < half:
            margin = min(margin, abs(a - round(a)))
        if b > 1.0 and b < half:
            margin = min(margin, abs(b - round(b)))
        if ka > kb:
            c = f * nfft / rate
            margin = min(margin, abs(c - math.floor(c) - 0.5))
            ka = kb = min(max(int(np.rint(c)), 1), half)
        lo.append(ka)
        hi.append(kb)
    return np.array(lo), np.array(hi), margin


def levels(p, k_lo, k_hi, add=np.sum):
    """The mean of the powers p over each window."""
    return np.array([float(add(p[a:b + 1])) / (b - a + 1) for a, b in zip(k_lo, k_hi)])


def curve(sa, st, amount=1.0, boost_db=12.0, cut_db=24.0, floor_db=120.0, dead=False):
    """(raw - m [J], d [J], m, clamped points) of one curve from the source's and the target's levels; dead: 0 dB throughout."""
    J = len(sa)
    if dead or sa.max() == 0.0 or st.max() == 0.0:
        return np.zeros(J), np.zeros(J), 0.0, 0
    rel = 10.0 ** (-floor_db / 10.0)
    raw = np.array([10.0 * math.log10(max(t, st.max() * rel) / max(s, sa.max() * rel)) for s, t in zip(sa, st)])
    m = 0.0
    for v in raw:
        m += v
    m /= J
    want = amount * (raw - m)
    return raw - m, np.clip(want, -cut_db, boost_db), m, int(np.count_nonzero((want < -cut_db) | (want > boost_db)))


def log_gain(d, nfft, rate, lo, per_octave):
    """L[k] for k = 0 .. Nfft / 2 from the curve d on the grid."""
    J = len(d)
    k = np.arange(nfft // 2 + 1, dtype=np.float64)
    u = np.zeros(nfft // 2 + 1)
    u[1:] = per_octave * np.log2(k[1:] * rate / nfft / lo)
    u = np.clip(u, 0.0, J - 1.0)
    i = np.minimum(np.floor(u).astype(np.int64), J - 2)
    return (d[i] + (u - i) * (d[i + 1] - d[i])) * LN10_20


def correction(L, nfft, phase="minimum", delay=0):
    """C[k] for k = 0 .. Nfft - 1 from L[k], k = 0 .. Nfft / 2."""
    full = np.concatenate([L, L[-2:0:-1]])
    if phase == "linear":
        k = np.arange(nfft, dtype=np.int64)
        ang = -2.0 * np.pi * ((k * int(delay)) % nfft).astype(np.float64) / nfft
        return np.exp(full) * (np.cos(ang) + 1j * np.sin(ang))
    c = np.fft.ifft(full).real
    c[1:nfft // 2] *= 2.0
    c[nfft // 2 + 1:] = 0.0
    return np.exp(np.fft.fft(c))


def match64(a, t=None, rate=48000, lo=20.0, hi=None, per_octave=12, octaves=1.0 / 3.0, amount=1.0, boost_db=12.0, cut_db=24.0, link=True,
            phase="minimum", delay=0, tilt_db=0.0, floor_db=120.0, add=np.sum):
    """a: [F, 2] frames, t: [G, 2] target frames at the session's rate, or None for a flat target.  Returns (float64 [Fo, 2] before
    the rounding, info as Convolution.ir_match_info gives it after such a load, curve as ir_match_curve gives it; energy_out is
    that of the taps rounded to float32, as the device stores them).  The float fields are taken as the struct holds them."""
    a = np.asarray(a).reshape(-1, 2).astype(np.float64)
    flat = t is None
    t = None if flat else np.asarray(t).reshape(-1, 2).astype(np.float64)
    amount, boost_db, cut_db, tilt_db, floor_db = (float(np.float32(v)) for v in (amount, boost_db, cut_db, tilt_db, floor_db))
    F, G = a.shape[0], 0 if flat else t.shape[0]
    N = nfft_of(F, G)
    D = int(delay) if phase == "linear" else 0
    Fo = F + D
    hi = min(20000.0, rate / 2.0) if not hi else float(hi)
    hz = grid(lo, hi, per_octave)
    J = len(hz)
    k_lo, k_hi, _ = windows(hz, N, rate, octaves)
    A = [np.fft.fft(a[:, c], N) for c in range(2)]
    sa = [levels((A[c].real ** 2 + A[c].imag ** 2)[:N // 2 + 1], k_lo, k_hi, add) for c in range(2)]
    if flat:
        st = [np.array([10.0 ** (tilt_db * math.log2(f / 1000.0) / 10.0) for f in hz])] * 2
    else:
        T = [np.fft.fft(t[:, c], N) for c in range(2)]
        st = [levels((T[c].real ** 2 + T[c].imag ** 2)[:N // 2 + 1], k_lo, k_hi, add) for c in range(2)]
    zero_a = [not a[:, c].any() for c in range(2)]
    zero_t = [False, False] if flat else [not t[:, c].any() for c in range(2)]
    kw = dict(amount=amount, boost_db=boost_db, cut_db=cut_db, floor_db=floor_db)
    if link:
        one = curve(sa[0] + sa[1], st[0] + st[1], dead=all(zero_a) or all(zero_t), **kw)
        curves, clamped = [one, one], one[3]
    else:
        curves = [curve(sa[c], st[c], dead=zero_a[c] or zero_t[c], **kw) for c in range(2)]
        clamped = curves[0][3] + curves[1][3]
    y = np.zeros((N, 2))
    for c in range(2):
        if zero_a[c]:
            continue
        C = correction(log_gain(curves[c][1], N, rate, lo, per_octave), N, phase, D)
        y[:, c] = np.fft.ifft(A[c] * C).real
    out = y[:Fo]
    info = dict(frames=F, target_frames=G, frames_out=Fo, nfft=N, points=J, energy_in=float((a * a).sum()), energy_target=0.0 if flat else float((t * t).sum()),
                energy_out=float((out.astype(np.float32).astype(np.float64) ** 2).sum()), energy_rest=float((y[Fo:] ** 2).sum()),
                mean_db=(curves[0][2], curves[1][2]), clamped=clamped)
    crv = dict(hz=hz, before_db=np.stack([curves[0][0], curves[1][0]], axis=1), gain_db=np.stack([curves[0][1], curves[1][1]], axis=1))
    return out, info, crv


def matched(a, t=None, **kw):
    """match64 with the taps as the engine stores them: float32 [Fo, 2]."""
    y, info, crv = match64(a, t, **kw)
    return y.astype(np.float32), info, crv


def smoothed_db(x, rate=48000, nfft=None, **kw):
    """10 log10 of the linked smoothed level of the frames x on the default grid (for the tests' own measurements)."""
    x = np.asarray(x).reshape(-1, 2).astype(np.float64)
    N = nfft or nfft_of(x.shape[0])
    hz = grid(kw.get("lo", 20.0), kw.get("hi", min(20000.0, rate / 2.0)), kw.get("per_octave", 12))
    k_lo, k_hi, _ = windows(hz, N, rate, kw.get("octaves", 1.0 / 3.0))
    s = sum(levels((np.abs(np.fft.fft(x[:, c], N)) ** 2)[:N // 2 + 1], k_lo, k_hi) for c in range(2))
    return hz, 10.0 * np.log10(s)


def decaying_noise(n, seed=0, level=0.25, right=0.7, db=60.0):
    """n frames [n, 2] float32 of noise that decays by `db` dB over its length; the right channel is different noise at `right`
    of the left's level."""
    rng = np.random.default_rng(1000 * seed + n)
    env = 10.0 ** (-(db / 20.0) * np.arange(n) / max(n, 1))
    x = np.stack([rng.standard_normal(n) * env, right * rng.standard_normal(n) * env], axis=1)
    return (level * x).astype(np.float32)


def coloured_noise(n, seed=0, **kw):
    """decaying_noise filtered by 0.3 0.7^m over 64 taps: a source with a tilt to match away."""
    x = decaying_noise(n, seed, **kw).astype(np.float64)
    h = 0.3 * 0.7 ** np.arange(64)
    return np.stack([np.convolve(x[:, c], h)[:n] for c in range(2)], axis=1).astype(np.float32)
