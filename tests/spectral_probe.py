"""Narrow-band probes for the long-batch transforms (plain numpy, no GPU): a stream that puts ONE spectral line per probe into
z = in1 + j in2, and a measure that reads the engine's error at those lines and at their mirrors.

A two-in / two-out linear system acts on z as W[k] = A[k] Z[k] + B[k] conj(Z[N - k]).  White noise excites every bin alike, so a
fault at one bin (or one pair of bins) of an N-point transform is diluted by sqrt(N) in a whole-signal RMS.  A rotating pair
in1 = amp cos(2 pi q n / N + phi), in2 = amp sin(...) excites bin q alone: W[q] = A[q] Z[q] and W[N-q] = B[N-q] conj(Z[q]) read
the two coefficients separately; the mirrored pair (in2 negated: bin N - q) reads A[N-q] and B[q].  On a window of exactly N
frames every probe is exactly periodic, so a float64 FFT of the window is the exact projection onto the lines."""
import functools
import math

import numpy as np

from cuda_audio_amd.synth import make_input
from helpers import rms

PIECE = 1 << 20  # frames generated at a time
ROWS = 512       # q = k1 + 512 k2: (row, column) of the 512 x 8192 decomposition of the overlap-save transform
COLS = 8192


def q(k1, k2):
    return k1 + ROWS * k2


def check_bins(bins, N):
    """Refuses a probe list whose read-out bins (q and N - q of every probe) are not all distinct."""
    bins = [int(b) for b in bins]
    for b in bins:
        if not 0 < b < N:
            raise ValueError(f"probe bin {b} outside (0, {N})")
    if len(set(bins)) != len(bins):
        raise ValueError("a probe bin is listed twice")
    have = set(bins)
    for b in bins:
        if 2 * b != N and N - b in have:  # (q = N/2 is its own mirror: one real alternating line)
            raise ValueError(f"probe bins {b} and {N - b} are each other's mirror: the lines of one would be read as the other's")
    return bins


def phases(bins, N, seed):
    """The seeded phase of every probe (0 for q = N/2, whose line is real: a random phase would only scale it)."""
    ph = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, len(bins))
    return [0.0 if 2 * b == N else float(p) for b, p in zip(bins, ph)]


def tone(qbin, N, n0, n, coef=1.0):
    """coef * exp(2 pi j qbin (n0 + i) / N) for i < n (complex128); the product qbin * n reduced modulo N in int64 first: exact,
    where an unreduced argument (2^26 rad and more for the streams used here) costs the cosine its low bits."""
    i = np.arange(n0, n0 + n, dtype=np.int64)
    arg = ((int(qbin) * i) % N).astype(np.float64) * (2.0 * np.pi / N)
    return coef * (np.cos(arg) + 1j * np.sin(arg))


@functools.lru_cache(maxsize=2)
def _probe_period(bins, N, amp, seed):
    """One period of the summed probes: (cos part, sin part, alternating part), float64 [period] each.  A piece starting at
    frame o is the first piece turned by exp(2 pi j ((q o) mod N) / N): both arguments as tone() reduces them."""
    period = N // math.gcd(N, *bins) if bins else 2
    c, s, alt = np.zeros(period), np.zeros(period), np.zeros(period)
    for b, ph in zip(bins, phases(bins, N, seed)):
        first = tone(b, N, 0, min(PIECE, period), amp * np.exp(1j * ph))
        for o in range(0, period, PIECE):
            n = min(PIECE, period - o)
            t = first[:n] * tone(b, N, o, 1)[0]
            if 2 * b == N:
                alt[o:o + n] += t.real
            else:
                c[o:o + n] += t.real
                s[o:o + n] += t.imag
    return c, s, alt


def probe_stream(n_frames, bins, N, amp, noise_amp, dc, seed, mirror=False):
    """float32 [2, n_frames]: make_input's noise (amplitude noise_amp, offset dc: seams, Q1/Q2 sums and every block stay busy)
    plus one rotating pair per signed bin q of `bins`, 0 < q < N, with a phase drawn from default_rng(seed):
    in1 += amp cos(2 pi q n / N + phi), in2 += amp sin(...); mirror=True: in2 -= ..., i.e. the bin N - q.
    q = N/2 is the real alternating component amp (-1)^n: on in1 only, with mirror=True on in2 only."""
    bins = tuple(check_bins(bins, N))
    out = make_input(n_frames, amp=noise_amp, dc=dc)
    c, s, alt = _probe_period(bins, N, float(amp), seed)
    period = len(c)
    for o in range(0, n_frames, period):  # (period is even and the pieces start at its multiples: alt keeps its sign)
        n = min(period, n_frames - o)
        in1 = c[:n] + (0.0 if mirror else alt[:n])
        in2 = (-s[:n] + alt[:n]) if mirror else s[:n]
        out[0, o:o + n] = (out[0, o:o + n] + in1).astype(np.float32)
        out[1, o:o + n] = (out[1, o:o + n] + in2).astype(np.float32)
    return out


def name_bin(qbin):
    """A bin of the N = 512 x 8192-point transform as a row / column pair and as a bin of the 512-point transforms."""
    return dict(bin=int(qbin), k1=int(qbin % ROWS), k2=int(qbin // ROWS), bin512=qbin / COLS)


def spectrum(a, M):
    """fft(a[0] + j a[1]) / M of a [2, M] window, float64."""
    a = np.asarray(a, dtype=np.float64)
    assert a.shape == (2, M), (a.shape, M)
    return np.fft.fft(a[0] + 1j * a[1]) / M


def readout_bins(bins, N):
    """q and N - q of every probe; bin 0 for a stream without probes (the DC / alternating inputs).  Never N/2: the reference
    leaves the Nyquist bin of its transforms unwritten, so the oracle's wet line there is null whatever the
    input - the bin is excited and compared (it is always among the bins of `worst`), but it is no unit of measure."""
    return [b for p in bins if 2 * int(p) != N for b in (int(p), N - int(p))] if len(bins) else [0]


def probe_errors(got, want, dry, bins, N, d=1, Ww=None):
    """got, want, dry: [2, N / d] - a window of exactly N / d frames of the engine's output, the oracle's and the dry mix.  Every
    probe bin must be a multiple of d (it is then exactly periodic on the window and lands on bin q / d of its transform).
    Returns S (the rms of the wet lines |Ww| over the read-out bins q and N - q), floor (min |Ww| / S), worst (max |E| / S over
    the read-out bins and bins 0 and N/2, E the transform of got - want) with the bin where it happened - named as a bin of the
    N-point transform: (k1, k2) = (q % 512, q // 512) and 512-point bin q / 8192 -, the whole-window RMS of got - want and the
    worst 256-frame block's."""
    assert N % d == 0 and all(int(b) % d == 0 for b in bins), "probe bins must be multiples of d"
    M = N // d
    err = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    E = spectrum(err, M)
    if Ww is None:  # (a caller measuring several outputs against one oracle window passes the first result's Ww on)
        Ww = spectrum(np.asarray(want, dtype=np.float64) - np.asarray(dry, dtype=np.float64), M)
    read = np.array(readout_bins(bins, N), dtype=np.int64) // d
    lines = np.abs(Ww[read])
    S = float(np.sqrt(np.mean(lines ** 2)))
    chk = np.unique(np.concatenate([read, [0, M // 2]]))
    e = np.abs(E[chk])
    k = int(np.argmax(e))
    blocks = err.reshape(2, M // 256, 256)
    res = dict(S=S, floor=float(lines.min() / S), worst=float(e[k] / S), rms=rms(err),
               worst_block=float(np.sqrt(np.mean(blocks ** 2, axis=(0, 2)).max())), Ww=Ww, E=E)
    res.update(name_bin(int(chk[k]) * d))
    return res


def describe(r):
    return (f"worst {r['worst']:.3e} of S = {r['S']:.3e} at bin {r['bin']} = (k1 {r['k1']}, k2 {r['k2']}), 512-point bin {r['bin512']:.4f}; "
            f"floor {r['floor']:.3f}, rms {r['rms']:.3e}, worst block {r['worst_block']:.3e}")


# -- the probe lists of the tests -----------------------------------------------------------------------------------------
N_OS = ROWS * COLS  # 2^22: the overlap-save segment
AMP, NOISE_AMP, DC, SEED = 0.01, 0.05, 0.01, 7
# row 0 (pairs with itself through the mirrored column), row 256 (pairs with itself through 8191 - k2), the first and last rows
# and columns, rows either side of 256, 512-point bins 1 and 255, interior points; then, for the transforms along the block
# axis, block-axis bins 0, 1, 4096 and 8191 next to 512-point bins 0, 1 and 255 (8191 next to 255 at 512-point bin 254.9998:
# one bin higher lies inside the notch that the reference's unwritten Nyquist bin leaves, and the wet line there is 0.006 of
# the others); last the packed Nyquist bin
SMALL_BINS = check_bins(
    [q(0, 1), q(0, 4095), q(0, 16), q(0, 4080), q(0, 8175), q(256, 0), q(256, 4095), q(256, 8190),
     q(1, 0), q(2, 8191), q(511, 0), q(255, 1), q(257, 4000), q(3, 1000), q(64, 77), q(448, 8100),
     2, 16382, 16384, 8192 * 2 + 8192, 8192 * 253 + 16382, 8192 * 100 + 8192, N_OS // 2], N_OS)
# the same on a window of N / 4 frames: every bin moved to a multiple of 4 (rows 1, 2, 3 -> 4, 8, 4; 255 / 257 -> 252 / 260;
# 511 -> 504, since 508 is the mirror of (4, 8191); 16382 -> 16380)
LARGE_D = 4
LARGE_BINS = check_bins(
    [q(0, 1), q(0, 4095), q(0, 16), q(0, 4080), q(0, 8175), q(256, 0), q(256, 4095), q(256, 8190),
     q(4, 0), q(4, 8191), q(504, 0), q(252, 1), q(260, 4000), q(4, 1000), q(64, 77), q(448, 8100),
     8, 16380, 16384, 8192 * 2 + 8192, 8192 * 253 + 16380, 8192 * 100 + 8192, N_OS // 2], N_OS)
assert all(b % LARGE_D == 0 for b in LARGE_BINS)


def dc_heavy_stream(n_frames, level=0.2, noise_amp=0.02):
    """The inputs of the committed goldens (dc_heavy_input, alternating_input) at once: in1 = level + noise,
    in2 = level (-1)^n + noise; the Q1/Q2 block sums are then about 256 level."""
    out = make_input(n_frames, amp=noise_amp, dc=0.0)
    sign = np.where(np.arange(PIECE) % 2, -1.0, 1.0)
    for o in range(0, n_frames, PIECE):
        n = min(PIECE, n_frames - o)
        out[0, o:o + n] = (out[0, o:o + n] + level).astype(np.float32)
        out[1, o:o + n] = (out[1, o:o + n] + level * sign[:n]).astype(np.float32)
    return out
