"""Float64 restatement of the frequency response of a loaded IR (mc_ir_response, cuda_audio_amd/csrc/irresponse.hip.h).

Test infrastructure only: the product never imports it.  x = the n stored taps (float32 [n, 2]) as double, N = end ? min(end, n) : n
(include/mcconv.h):
  1. the origin o is ir_decay_np's step 1;
  2. window (first, count, rise, fall) covers the taps [a, b), a = min(o + first, N), b = count ? min(a + count, N) : N, L = b - a,
     with raised-cosine edges of r = min(rise, L) and f = min(fall, L - r) taps in the form of ir_shape_np's fade;
  3. per channel and frequency F (a float32 taken as double), theta = 2 pi F (m - o) / rate: F (m - o) is exact in double and is
     reduced modulo the rate exactly (np.fmod) before the division, so that theta carries two roundings however long the IR is.
     H = sum u x e^(-j theta), D = sum (m - o) u x e^(-j theta), E = sum (u x)^2, A = sum |u x|, every sum by math.fsum: the
     correctly rounded sum of its rounded terms;
  4. tau = Re(D conj H) / |H|^2, NaN when |H|^2 is 0 or not finite;
  5. status 1 when L = 0 or A is 0 or not finite: H = 0, tau = NaN.

check_against's tolerances are derived, not measured.  With u = 2^-53, n_w = the window's taps and STRETCH = the taps between
two seeds of the device's rotator (RSP_STRETCH):
  * |delta Re H|, |delta Im H| <= tol_H = (n_w + 3.3 STRETCH + 16) u A: n_w u covers any order of summing terms bounded by A, 3.3
    STRETCH u is the rotator's drift (Brent, Percival and Zimmermann's sqrt 5 u per complex product, plus the step's own u), 16 u the
    roundings of the weight, the products, the seed's argument and this file's own cos and sin;
  * the same for D with A_D = sum (m - o) |u x| in place of A;
  * tau = Re(D / H), so to first order delta tau is (|delta D| + |tau| |delta H|) / |H|: held to 2 (tol_D + |tau| tol_H) / |H| where
    |H| >= 1000 tol_H, so that first order is enough.  Points with a smaller |H| are counted as skipped, and the count must be
    `skips` (0 unless a case says otherwise);
  * E and A to n_w u relative;
  * o, N, the spans and the status are equal integers; NaN where and only where the restatement has it; H = 0 exactly under status 1.
"""
import ctypes
import ctypes.util
import math

import numpy as np

from ir_decay_np import origin

U = 2.0 ** -53
RUN, STRETCH, FT = 1024, 64, 256   # csrc/irresponse.hip.h's RSP_RUN, RSP_STRETCH, RSP_FT
MAX_FREQ, MAX_WIN = 1024, 64
CHANNELS = ("L", "R")
FLOOR_DB = -400.0

# 2^x as the C library has it: the engine's host arithmetic (mc_response_grid, mc_response_smooth) calls the same function, and
# the two are compared bit for bit; numpy's own exp2 may be a vectorised one that differs in the last place
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.exp2.restype = ctypes.c_double
_libm.exp2.argtypes = [ctypes.c_double]


def exp2(x):
    return float(_libm.exp2(float(x)))


def f32(v):
    return float(np.float32(v))


def span(window, o, N):
    """Step 2: (a, b, r, f) of a (first, count, rise, fall) window, or of None, the whole span."""
    first, count, rise, fall = (0, 0, 0, 0) if window is None else (int(v) for v in window)
    a = min(o + first, N)
    b = min(a + count, N) if count else N
    L = b - a
    r = min(rise, L)
    return a, b, r, min(fall, L - r)


def weights(L, r, f):
    """The window's weights u [L]: ir_shape_np's fade at the end, its mirror form at the start."""
    u = np.ones(L, np.float64)
    if r:
        k = np.arange(r, dtype=np.float64)
        u[:r] = 0.5 * (1.0 - np.cos(np.pi * (k + 1.0) / (r + 1.0)))
    if f:
        k = np.arange(f, dtype=np.float64)
        u[L - f:] = 0.5 * (1.0 + np.cos(np.pi * (k + 1.0) / (f + 1.0)))
    return u


def rotation(k, F, rate):
    """(cos theta, sin theta) [len(k)] of theta = 2 pi F k / rate with F k reduced modulo the rate exactly."""
    theta = 2.0 * np.pi * (np.fmod(F * k, float(rate)) / float(rate))
    return np.cos(theta), np.sin(theta)


def response(taps, rate, hz, windows=None, onset_db=-20.0, end=0):
    """taps: float32 [n, 2] as Convolution.ir_taps gives them.  Returns what Convolution.ir_response returns, and with it "d"
    (complex D [n_win, 2, n_freq]) and "abs_d" (A_D [n_win, 2]), which the tolerances need."""
    taps = np.asarray(taps, np.float32).reshape(-1, 2)
    n = taps.shape[0]
    N = min(int(end), n) if end else n
    hz = np.asarray(hz, np.float32).reshape(-1)
    windows = [None] if windows is None else list(windows)
    o = origin(taps, N, f32(onset_db))
    nw, nf = len(windows), hz.size
    h, d = np.zeros((nw, 2, nf), np.complex128), np.zeros((nw, 2, nf), np.complex128)
    delay = np.full((nw, 2, nf), np.nan)
    abs_d, spans, rows = np.zeros((nw, 2)), np.zeros((nw, 2), np.int64), {}
    for w, window in enumerate(windows):
        a, b, r, f = span(window, o, N)
        spans[w] = a, b
        k = np.arange(a - o, b - o, dtype=np.float64)
        v = taps[a:b].astype(np.float64) * weights(b - a, r, f)[:, None]
        dv = k[:, None] * v
        bad = []
        for c, name in enumerate(CHANNELS):
            E, A = math.fsum(v[:, c] * v[:, c]), math.fsum(np.abs(v[:, c]))
            bad.append(b == a or A == 0.0 or not math.isfinite(A))
            rows[(w, name)] = dict(energy=E, abs_sum=A, status=int(bad[c]))
            abs_d[w, c] = math.fsum(np.abs(dv[:, c]))
        for j, F in enumerate(hz.astype(np.float64)):
            if all(bad):
                break
            cs, sn = rotation(k, float(F), rate)
            for c in range(2):
                if bad[c]:
                    continue
                H = complex(math.fsum(v[:, c] * cs), -math.fsum(v[:, c] * sn))
                D = complex(math.fsum(dv[:, c] * cs), -math.fsum(dv[:, c] * sn))
                h[w, c, j], d[w, c, j] = H, D
                p = H.real * H.real + H.imag * H.imag
                if p != 0.0 and math.isfinite(p):
                    delay[w, c, j] = (D.real * H.real + D.imag * H.imag) / p
    mag = np.abs(h)
    with np.errstate(divide="ignore"):
        db = np.where(mag > 0.0, np.maximum(20.0 * np.log10(mag), FLOOR_DB), FLOOR_DB)
    return dict(origin=o, taps=N, hz=hz, spans=spans, rows=rows, h=h, delay=delay, db=db, phase=np.arctan2(h.imag, h.real), d=d, abs_d=abs_d)


def grid(lo=20.0, hi=20000.0, per_octave=24):
    """mc_response_grid: float32(lo 2^(i / per_octave)) while that double is <= hi."""
    out, i = [], 0
    while True:
        v = float(lo) * exp2(float(i) / float(per_octave))
        if not v <= float(hi):
            return np.array(out, np.float32)
        out.append(np.float32(v))
        i += 1


def neighbours(hz, octaves):
    """Per point f of the ascending grid hz, the points g with hz[g] in [hz[f] 2^(-octaves / 2), hz[f] 2^(octaves / 2)]: boolean [n, n]."""
    hz = np.asarray(hz, np.float32).astype(np.float64)
    down, up = exp2(-0.5 * octaves), exp2(0.5 * octaves)
    return (hz[None, :] >= (hz * down)[:, None]) & (hz[None, :] <= (hz * up)[:, None])


def smooth(hz, power, octaves):
    """mc_response_smooth: the mean of power[g], ascending g, over hz[g] in [hz[f] 2^(-octaves / 2), hz[f] 2^(octaves / 2)]."""
    power = np.asarray(power, np.float64)
    if octaves == 0.0:
        return power.copy()
    out = np.empty_like(power)
    for f, near in enumerate(neighbours(hz, octaves)):
        total = 0.0
        for v in power[near].tolist():
            total += v
        out[f] = total / int(np.count_nonzero(near))
    return out


def tolerances(want, w, c):
    """(tol_H, tol_D, n_w u) of window w, channel c of a restatement."""
    n_w = int(want["spans"][w, 1] - want["spans"][w, 0])
    k = (n_w + 3.3 * STRETCH + 16.0) * U
    return k * want["rows"][(w, CHANNELS[c])]["abs_sum"], k * float(want["abs_d"][w, c]), n_w * U


def check_against(got, want, skips=0):
    """got: Convolution.ir_response's result; want: response()'s.  The module's docstring has the bounds.  Prints the largest
    differences as fractions of their bounds and returns them."""
    for f in ("origin", "taps"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert np.array_equal(got["hz"], want["hz"]) and got["hz"].dtype == np.float32
    assert np.array_equal(got["spans"], want["spans"]), (got["spans"], want["spans"])
    assert set(got["rows"]) == set(want["rows"])
    assert got["h"].shape == want["h"].shape and got["delay"].shape == want["delay"].shape
    worst = dict(h=0.0, delay=0.0, energy=0.0, abs_sum=0.0)
    skipped = 0
    for w in range(want["h"].shape[0]):
        for c, name in enumerate(CHANNELS):
            g, r = got["rows"][(w, name)], want["rows"][(w, name)]
            assert g["status"] == r["status"], (w, name, g, r)
            tol_h, tol_d, rel = tolerances(want, w, c)
            for f in ("energy", "abs_sum"):
                if r[f]:
                    worst[f] = max(worst[f], abs(g[f] - r[f]) / r[f] / rel)
                else:
                    assert g[f] == 0.0, (w, name, f, g[f])
            gh, wh, gt, wt = got["h"][w, c], want["h"][w, c], got["delay"][w, c], want["delay"][w, c]
            if r["status"]:
                assert not gh.any() and np.isnan(gt).all(), (w, name, gh, gt)
                continue
            worst["h"] = max(worst["h"], float(max(np.max(np.abs(gh.real - wh.real)), np.max(np.abs(gh.imag - wh.imag)))) / tol_h)
            mag = np.abs(wh)
            held = mag >= 1000.0 * tol_h
            skipped += int(np.count_nonzero(~held))
            assert not np.isnan(gt[held]).any() and not np.isnan(wt[held]).any(), (w, name, gt, wt)
            if held.any():
                bound = 2.0 * (tol_d + np.abs(wt[held]) * tol_h) / mag[held]
                worst["delay"] = max(worst["delay"], float(np.max(np.abs(gt[held] - wt[held]) / np.maximum(bound, 5e-324))))
    print("largest differences as fractions of their bounds:", ", ".join(f"{f} {v:.1e}" for f, v in worst.items()), f"; {skipped} points skipped")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert skipped == skips, (skipped, skips)
    mag = np.abs(got["h"])
    with np.errstate(divide="ignore"):
        db = np.where(mag > 0.0, np.maximum(20.0 * np.log10(mag), FLOOR_DB), FLOOR_DB)
    assert np.array_equal(got["db"], db) and np.array_equal(got["phase"], np.arctan2(got["h"].imag, got["h"].real))
    return worst
