"""Float64 restatement of the decay measurement of a loaded IR (mc_ir_decay, cuda_audio_amd/csrc/irdecay.hip.h).

Test infrastructure only: the product never imports it.  x = the n stored taps (float32 [n, 2]) as double, N = end ? min(end, n) : n;
only taps [0, N) are searched and measured (include/mcconv.h):
  1. origin o: onset_db < 0: a[m] = max(|L|, |R|) in float32, peak = max a, t = peak * float32(10^(onset_db / 20)) as a float32
     product, o = the first m with a[m] >= t (ir_shape_np.onset_of); onset_db = 0: o = 0;
  2. row group 0: y = x.  Row group b >= 1: x[0 .. N) from rest at tap 0 through two identical band-pass sections
     (Audio-EQ-Cookbook, 0 dB peak gain: b = {al, 0, -al}, a = {1 + al, -2 c, 1 - al}, divided by a0; w0, c, al in double from the
     float32 fields), each one plain sequential loop (ir_eq_np.biquad: transposed direct form II);
  3. sets s = 0, 1, 2: e[m] = yL^2, yR^2, yL^2 + yR^2 for m in [o, N);
  4. EDC[m] = sum of e[k], k in [m, N), added up from the last tap backwards; E = EDC[o]; L[m] = 10 log10(EDC[m] / E);
  5. a decay time over (hi, lo): S = {m : lo <= L[m] <= hi}; NaN when L[N - 1] > lo or |S| < 2; else the least-squares slope a
     of L over x = m - min S, T = -60 / (a rate);
  6. C50, C80, D50 from EDC at k50 = o + floor(0.05 rate + 0.5) and k80 = o + floor(0.08 rate + 0.5); Ts = sum (m - o) e[m] / E / rate;
  7. the curve: max(L[o + floor(j (N - 1 - o) / (K - 1))], -400).
"""
import numpy as np

from ir_eq_np import biquad
from ir_shape_np import onset_of

SETS = ("L", "R", "LR")
FIELDS = ("energy", "edt", "t20", "t30", "c50", "c80", "d50", "ts")
RANGES = {"edt": (0.0, -10.0), "t20": (-5.0, -25.0), "t30": (-5.0, -35.0)}
DEFAULT_Q = float(np.float32(1.41421356))
EDGES = (-5.0, -10.0, -25.0, -35.0)
CURVE_FLOOR = -400.0


def band_coefs(hz, q, rate):
    """(b0, b1, b2, a1, a2) with a0 = 1 of one section."""
    hz, q = float(np.float32(hz)), float(np.float32(q))
    w0 = 2.0 * np.pi * hz / float(rate)
    c, al = np.cos(w0), np.sin(w0) / (2.0 * q)
    a0 = 1.0 + al
    return (float(al / a0), 0.0, float(-al / a0), float(-2.0 * c / a0), float((1.0 - al) / a0))


def origin(taps, N, onset_db):
    if not onset_db < 0:
        return 0
    return onset_of(np.asarray(taps, np.float32)[:N], 0, onset_db)[1]


def levels(y, o):
    """y: float64 [N, 2], the row group's taps.  Returns (EDC [3, N - o], L [3, N - o]) over taps o .. N - 1."""
    e2 = y[o:] * y[o:]
    e = np.stack([e2[:, 0], e2[:, 1], e2[:, 0] + e2[:, 1]])
    edc = np.cumsum(e[:, ::-1], axis=1)[:, ::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = 10.0 * np.log10(edc / edc[:, :1])
    return e, edc, L


def decay_time(L, hi, lo, rate):
    """L: the levels of taps o .. N - 1 of one row."""
    nan = float("nan")
    if not L[-1] <= lo:  # (the curve never gets to lo, or is not a number)
        return nan
    S = np.nonzero((L >= lo) & (L <= hi))[0]
    if S.size < 2:
        return nan
    x = (S - S[0]).astype(np.float64)
    y = L[S]
    n = float(S.size)
    a = (n * (x * y).sum() - x.sum() * y.sum()) / (n * (x * x).sum() - x.sum() ** 2)
    with np.errstate(divide="ignore"):
        return float(np.float64(-60.0) / (a * float(rate)))


def row_of(e, edc, L, o, N, rate):
    nan = float("nan")
    E = float(edc[0])
    row = dict.fromkeys(FIELDS, nan)
    row["energy"] = E
    if not E > 0.0:
        return row
    for name, (hi, lo) in RANGES.items():
        row[name] = decay_time(L, hi, lo, rate)
    for name, ms in (("c50", 0.05), ("c80", 0.08)):
        k = o + int(np.floor(ms * float(rate) + 0.5))
        if k >= N or edc[k - o] == 0.0:
            continue
        late = float(edc[k - o])
        with np.errstate(divide="ignore"):
            row[name] = float(10.0 * np.log10(np.float64(E - late) / late))
        if name == "c50":
            row["d50"] = (E - late) / E
    row["ts"] = float((np.arange(N - o, dtype=np.float64) * e).sum() / E / float(rate))
    return row


def decay(taps, rate, bands=(), q=None, onset_db=-20.0, end=0, curve_points=0, band_filter=None):
    """taps: float32 [n, 2] as Convolution.ir_taps gives them.  Returns what Convolution.ir_decay returns, plus "levels":
    {(band, set): L over taps origin .. N - 1} for assert_range_margin.  band_filter(x, c) -> float64 [N, 2] stands in for step 2's
    two sequential loops (test_ir_chunk_cpu.py runs them in extended precision to check this restatement itself)."""
    taps = np.asarray(taps, np.float32).reshape(-1, 2)
    n = taps.shape[0]
    N = min(int(end), n) if end else n
    q = DEFAULT_Q if q is None else q
    o = origin(taps, N, float(np.float32(onset_db)))
    x = taps[:N].astype(np.float64)
    K = int(curve_points)
    rows, lev = {}, {}
    curve = np.full((1 + len(bands), 3, K), np.nan) if K else None
    for b in range(1 + len(bands)):
        y = x
        if b:
            c = band_coefs(bands[b - 1], q, rate)
            y = band_filter(x, c) if band_filter else biquad(biquad(x, c), c)
        e, edc, L = levels(y, o)
        for s, name in enumerate(SETS):
            rows[(b, name)] = row_of(e[s], edc[s], L[s], o, N, rate)
            lev[(b, name)] = L[s]
            if K and edc[s, 0] > 0.0:
                at = (np.arange(K, dtype=np.int64) * (N - 1 - o)) // (K - 1)
                curve[b, s] = np.maximum(L[s][at], CURVE_FLOOR)
    return dict(origin=o, taps=N, rows=rows, curve=curve, levels=lev)


def range_margin(L, edges=EDGES):
    """The smallest distance (dB) of any level to any of the fit ranges' edges."""
    L = np.asarray(L, np.float64)
    L = L[np.isfinite(L)]
    return min((float(np.abs(L - edge).min()) for edge in edges), default=float("inf")) if L.size else float("inf")


def assert_range_margin(L, edges=EDGES):
    """What every comparison with the device asserts on the restatement first: no level within 1e-9 dB of -5, -10, -25 or -35 dB
    (the device's levels differ from these by far less), so that a tap moving in or out of a fit range cannot pass for an
    arithmetic difference.  The 0 dB edge is exempt: L[o] = 0 exactly by construction, on the device too."""
    m = range_margin(L, edges)
    assert m > 1e-9, m


def assert_margins(res):
    for L in res["levels"].values():
        assert_range_margin(L)


def sign_ir(n=6000, rate=8000, t60=0.25, seed=1):
    """h[m] = +-1 * 10^(-3 m / (t60 rate)), random signs per channel, float32: e[m] = r^m exactly up to the taps' rounding."""
    rng = np.random.default_rng(seed)
    sg = rng.integers(0, 2, size=(n, 2)) * 2.0 - 1.0
    m = np.arange(n, dtype=np.float64)
    return (sg * (10.0 ** (-3.0 * m / (t60 * rate)))[:, None]).astype(np.float32)


def noise_ir(n=6000, lead=37, rate=8000, t60=0.25, seed=7, amp=0.3):
    """`lead` zero frames, then n frames of amp * N(0, 1) * 10^(-3 m / (t60 rate)), float32."""
    rng = np.random.default_rng(seed)
    m = np.arange(n, dtype=np.float64)
    body = amp * rng.standard_normal((n, 2)) * (10.0 ** (-3.0 * m / (t60 * rate)))[:, None]
    return np.concatenate([np.zeros((lead, 2)), body]).astype(np.float32)


def check_against(got, want, rel=1e-6, db=1e-6):
    """got: Convolution.ir_decay's result; want: decay()'s.  1e-6 relative for energy, times, D50 and Ts, 1e-6 dB for C50, C80 and
    the curve, NaN where and only where the restatement has NaN.  Prints the largest differences."""
    assert got["origin"] == want["origin"] and got["taps"] == want["taps"], (got["origin"], got["taps"], want["origin"], want["taps"])
    assert set(got["rows"]) == set(want["rows"])
    worst = dict.fromkeys(FIELDS, 0.0)
    for key, w in want["rows"].items():
        g = got["rows"][key]
        for f in FIELDS:
            assert np.isnan(g[f]) == np.isnan(w[f]), (key, f, g[f], w[f])
            if np.isnan(w[f]):
                continue
            if np.isinf(w[f]):
                assert g[f] == w[f], (key, f, g[f], w[f])
                continue
            err = abs(g[f] - w[f]) if f in ("c50", "c80") else (abs(g[f] - w[f]) / abs(w[f]) if w[f] else abs(g[f]))
            worst[f] = max(worst[f], err)
    cerr = 0.0
    if want["curve"] is None:
        assert got["curve"] is None
    else:
        assert got["curve"].shape == want["curve"].shape
        assert np.array_equal(np.isnan(got["curve"]), np.isnan(want["curve"]))
        if not np.isnan(want["curve"]).all():
            cerr = float(np.nanmax(np.abs(got["curve"] - want["curve"])))
    print("largest differences:", ", ".join(f"{f} {v:.1e}" for f, v in worst.items()), f", curve {cerr:.1e} dB")
    for f, v in worst.items():
        assert v <= (db if f in ("c50", "c80") else rel), (f, v)
    assert cerr <= db, cerr
