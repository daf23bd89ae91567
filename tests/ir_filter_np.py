"""The filter step of an IR load (include/mcconv.h, mc_ir_filter; csrc/irfilter.hip.h) restated in float64 with numpy's FFT, one
channel at a time, exactly as the header defines it:

    f_c = b_c (stereo), b_L (left) or (b_L + b_R) / 2 (mid); Nfft = max(16, smallest power of two >= F + G - 1)
    A = FFT(a_c padded to Nfft), B = FFT(f_c padded)
    convolve:    Y = A B
    deconvolve:  p = |B|^2, pm = max p, eps = 10^(-reg_db / 10), Y = A conj(B) / (p + eps pm); pm = 0: zeros;
                 the bins with p < eps pm are the regularised bins
    y = Re IFFT(Y); y[0 .. Fo), Fo = frames_out or F + G - 1 (convolve) or F (deconvolve)

and the inputs that the CPU and GPU tests share."""
import numpy as np

MAX_NFFT = 1 << 22


def nfft_of(F, G):
    n = 16
    while n < F + G - 1:
        n *= 2
    return n


def frames_out_of(F, G, op, frames_out=0):
    return int(frames_out) if frames_out else (F if op == "deconvolve" else F + G - 1)


def map_filter(b, channels="stereo"):
    """The filter's two channels f_L, f_R [G, 2] in float64 from its stereo frames b."""
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    if channels == "stereo":
        return b.copy()
    one = b[:, 0] if channels == "left" else 0.5 * (b[:, 0] + b[:, 1])
    return np.stack([one, one], axis=1)


def filter_channel(a, f, op="convolve", reg_db=60.0, frames_out=0):
    """One channel: (y [Fo] float64 before the rounding to float, the rest y[Fo .. Nfft), regularised bins, min p / pm)."""
    a, f = np.asarray(a, dtype=np.float64), np.asarray(f, dtype=np.float64)
    F, G = a.shape[0], f.shape[0]
    N, Fo = nfft_of(F, G), frames_out_of(F, G, op, frames_out)
    A, B = np.fft.fft(a, N), np.fft.fft(f, N)
    if op == "convolve":
        y, reg, cond = np.fft.ifft(A * B).real, 0, 1.0
    else:
        p = B.real * B.real + B.imag * B.imag
        pm = p.max()
        if pm == 0.0:
            return np.zeros(Fo), np.zeros(N - Fo), 0, 0.0
        thr = 10.0 ** (-float(np.float32(reg_db)) / 10.0) * pm
        reg, cond = int(np.count_nonzero(p < thr)), float(p.min() / pm)
        y = np.fft.ifft(A * np.conj(B) / (p + thr)).real
    return y[:Fo], y[Fo:], reg, cond


def filter64(a, b, op="convolve", channels="stereo", reg_db=60.0, frames_out=0):
    """a: [F, 2] frames, b: [G, 2] filter frames, both at the session's rate.  Returns (float64 [Fo, 2] before the rounding, info
    as Convolution.ir_filter_info gives it after such a load, with `condition` = (min p / pm per channel) beside it; its
    energy_out is that of the taps rounded to float32, as the device stores them)."""
    a = np.asarray(a).reshape(-1, 2)
    f = map_filter(b, channels)
    F, G = a.shape[0], f.shape[0]
    cols = [filter_channel(a[:, ch], f[:, ch], op, reg_db, frames_out) for ch in range(2)]
    y = np.stack([c[0] for c in cols], axis=1)
    a64 = a.astype(np.float64)
    info = dict(frames=F, filter_frames=G, frames_out=y.shape[0], nfft=nfft_of(F, G), energy_in=float((a64 * a64).sum()), energy_filter=float((f * f).sum()),
                energy_out=float((y.astype(np.float32).astype(np.float64) ** 2).sum()), energy_rest=float(sum((c[1] * c[1]).sum() for c in cols)),
                regularised=(cols[0][2], cols[1][2]), condition=(cols[0][3], cols[1][3]))
    return y, info


def filtered(a, b, **kw):
    """filter64 with the taps as the engine stores them: float32 [Fo, 2]."""
    y, info = filter64(a, b, **kw)
    return y.astype(np.float32), info


def decaying_noise(n, seed=0, level=0.25, right=0.7, db=60.0):
    """n frames [n, 2] float32 of noise that decays by `db` dB over its length; the right channel is different noise at `right`
    of the left's level."""
    rng = np.random.default_rng(1000 * seed + n)
    env = 10.0 ** (-(db / 20.0) * np.arange(n) / max(n, 1))
    x = np.stack([rng.standard_normal(n) * env, right * rng.standard_normal(n) * env], axis=1)
    return (level * x).astype(np.float32)


def integer_round_trip(n, G, seed=0):
    """(a, b, h): h [n, 2] of nonzero integers in +-[1, 512]; b [G, 2] = 8 followed by three values of -1 / 0 / 1, at frames 1 .. 3
    when G = 4 and spread over the G - 1 frames after the 8 otherwise, the last frame among them; a = h * b per channel, n + G - 1
    frames: all exact in float32 (|a| <= 512 * 11), and |B| >= 5 at every frequency."""
    rng = np.random.default_rng(77 * seed + n + G)
    h = rng.integers(1, 513, size=(n, 2)) * rng.choice([-1, 1], size=(n, 2))
    b = np.zeros((G, 2), np.int64)
    b[0] = 8
    for ch in range(2):
        at = np.concatenate([rng.choice(np.arange(1, G - 1), size=min(2, G - 2), replace=False), [G - 1]]) if G > 2 else np.arange(1, G)
        b[at, ch] = rng.integers(-1, 2, size=at.size)
        if G > 1 and b[G - 1, ch] == 0:
            b[G - 1, ch] = 1  # (the filter keeps its G frames)
    a = np.stack([np.convolve(h[:, ch], b[:, ch]) for ch in range(2)], axis=1)
    return a.astype(np.float32), b.astype(np.float32), h.astype(np.float32)


def comb(N):
    """delta[0] - delta[N / 4] on both channels, N / 4 + 1 frames: |B|^2 takes only the values 0, 2 and 4 on an N-point grid."""
    b = np.zeros((N // 4 + 1, 2), np.float32)
    b[0], b[N // 4] = 1.0, -1.0
    return b
