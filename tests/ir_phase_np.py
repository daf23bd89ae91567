"""The phase step of an IR load (include/mcconv.h, mc_ir_phase; csrc/irphase.hip.h) restated in float64 with numpy's FFT, one
channel at a time, exactly as the header defines it:

    Nfft = max(16, (smallest power of two >= F) * oversample)
    X = FFT(x padded to Nfft), p = |X|^2, pm = max p; pm = 0: zeros
    p = max(p, pm 10^(-floor_db / 10)); L = ln(p) / 2; c = Re IFFT(L)
    fold: c[0], c[Nfft / 2] kept, c[1 .. Nfft / 2) doubled, the rest zero
    C = FFT(c); Y = exp(Re C) (cos Im C + i sin Im C); y = Re IFFT(Y); y[0 .. F)

and the inputs with known answers that the CPU and GPU tests share."""
import numpy as np

MAX_FRAMES = 1 << 21
MAX_NFFT = 1 << 22


def nfft_of(F, oversample=8):
    n = 1
    while n < F:
        n *= 2
    return max(16, n * int(oversample))


def min_phase_channel(x, oversample=8, floor_db=120.0):
    """One channel: (y [F] float64 before the rounding to float, clamped bins)."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[0]
    N = nfft_of(F, oversample)
    X = np.fft.fft(x, N)
    p = X.real * X.real + X.imag * X.imag
    pm = p.max()
    if pm == 0.0:
        return np.zeros(F), 0
    thr = pm * 10.0 ** (-float(floor_db) / 10.0)
    clamped = int(np.count_nonzero(p < thr))
    L = 0.5 * np.log(np.maximum(p, thr))
    c = np.fft.ifft(L).real
    c[1:N // 2] *= 2.0
    c[N // 2 + 1:] = 0.0
    C = np.fft.fft(c)
    Y = np.exp(C.real) * (np.cos(C.imag) + 1j * np.sin(C.imag))
    return np.fft.ifft(Y).real[:F], clamped


def sums(v):
    """E and Ts of frames v [F, 2]: sum e and sum m e / sum e with e[m] = L[m]^2 + R[m]^2, in float64 (0 when E = 0)."""
    v = np.asarray(v, dtype=np.float64)
    e = (v * v).sum(axis=1)
    E = float(e.sum())
    return E, (float((np.arange(e.size, dtype=np.float64) * e).sum()) / E if E > 0.0 else 0.0)


def min_phase64(x, oversample=8, floor_db=120.0):
    """x: [F, 2] frames at the session's rate.  Returns (float64 [F, 2] before the rounding, info as Convolution.ir_phase_info
    gives it after such a load; its output sums are those of the taps rounded to float32, as the device stores them)."""
    x = np.asarray(x)
    F = x.shape[0]
    cols = [min_phase_channel(x[:, ch], oversample, floor_db) for ch in range(2)]
    y = np.stack([c[0] for c in cols], axis=1)
    Ein, Tin = sums(x)
    Eout, Tout = sums(y.astype(np.float32))
    return y, dict(frames=F, nfft=nfft_of(F, oversample), energy_in=Ein, energy_out=Eout, centre_in=Tin, centre_out=Tout,
                   clamped=(cols[0][1], cols[1][1]))


def min_phase(x, oversample=8, floor_db=120.0):
    """min_phase64 with the taps as the engine stores them: float32 [F, 2]."""
    y, info = min_phase64(x, oversample, floor_db)
    return y.astype(np.float32), info


def quadratic_product(K, r_max, seed=0, reflect=True):
    """(x, want): products of K / 2 real quadratic factors 1 - 2 r cos(t) z^-1 + r^2 z^-2 with zeros at radius 0.3 .. r_max and
    random angles.  In x every second factor is reflected outside the unit circle (r^2 - 2 r cos(t) z^-1 + z^-2, the same
    magnitude response); want is the all-inside product, the minimum-phase sequence of that magnitude.  K + 1 frames each."""
    rng = np.random.default_rng(seed)
    x, want = np.ones(1), np.ones(1)
    for i in range(K // 2):
        r = 0.3 + (r_max - 0.3) * (i + 0.5) / (K // 2)
        t = rng.uniform(0.1, np.pi - 0.1)
        inside = np.array([1.0, -2.0 * r * np.cos(t), r * r])
        want = np.convolve(want, inside)
        x = np.convolve(x, inside[::-1] if reflect and i % 2 else inside)
    return x, want


def delayed_noise(F, delay=None, seed=1, t60=None):
    """F frames [F, 2] float32: `delay` frames of silence (default F / 8), then noise that decays by 60 dB per t60 frames (default
    half the rest: 120 dB in all, so that the zeros the envelope moves inside the unit circle leave the cepstrum room in Nfft); the right channel has its own noise at 0.7 of the left's level."""
    rng = np.random.default_rng(seed + F)
    delay = F // 8 if delay is None else delay
    n = F - delay
    t60 = max(n // 2, 1) if t60 is None else t60
    env = 10.0 ** (-3.0 * np.arange(n) / t60)
    x = np.zeros((F, 2))
    x[delay:, 0] = rng.standard_normal(n) * env
    x[delay:, 1] = 0.7 * rng.standard_normal(n) * env
    return (0.25 * x).astype(np.float32)


def cumulative_energy(v):
    v = np.asarray(v, dtype=np.float64)
    return np.cumsum((v * v).reshape(v.shape[0], -1).sum(axis=1))
