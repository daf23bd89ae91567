"""Float64 restatement of the interaural cross-correlation of a loaded IR (mc_ir_iacc, cuda_audio_amd/csrc/iriacc.hip.h).

Test infrastructure only: the product never imports it.  x = the n stored taps (float32 [n, 2]) as double, N = end ? min(end, n) : n
(include/mcconv.h):
  1. the origin o and the row groups y (broadband, then one per band) are ir_decay_np's steps 1 and 2;
  2. k = min(o + (split ? split : floor(0.08 rate + 0.5)), N); windows early [o, k), late [k, N), all [o, N);
  3. lags tau = -T .. T;
  4. over a window [a, b): C(tau) = sum of y_L[m] y_R[m + tau] over the m with m and m + tau in [a, b), one np.dot of the two
     overlapping stretches per lag; E_L = y_L . y_L and E_R = y_R . y_R over [a, b);
  5. IACF(tau) = C(tau) / sqrt(E_L E_R); IACC = max |IACF|; tau* = the first lag from -T that attains it;
  6. row = {E_L, E_R, IACC, tau*, IACF(tau*), IACF(0), 10 log10(E_L / E_R), status}; status 1 (an empty window, or E_L E_R = 0)
     leaves all but the energies NaN, and the curve too.
"""
import numpy as np

from ir_decay_np import DEFAULT_Q, band_coefs, origin
from ir_eq_np import biquad

WINDOWS = ("early", "late", "all")
FIELDS = ("energy_l", "energy_r", "iacc", "lag", "iacf", "iacf0", "level_db", "status")
MAX_LAG = 1024


def default_lag(rate):
    return int(np.floor(0.001 * float(rate) + 0.5))


def window_row(yl, yr, T):
    """yl, yr: the window's doubles.  Returns (row, curve [2T + 1])."""
    nan = float("nan")
    n = yl.size
    EL, ER = (float(np.dot(yl, yl)), float(np.dot(yr, yr))) if n else (0.0, 0.0)
    row = dict.fromkeys(FIELDS, nan)
    row.update(energy_l=EL, energy_r=ER, status=1.0)
    curve = np.full(2 * T + 1, np.nan)
    if not EL * ER > 0.0:
        return row, curve
    den = float(np.sqrt(EL * ER))
    for tau in range(-T, T + 1):
        d = abs(tau)
        if d >= n:
            c = 0.0
        elif tau >= 0:  # m in [0, n - tau), R is read tau taps later
            c = float(np.dot(yl[:n - d], yr[d:]))
        else:
            c = float(np.dot(yl[d:], yr[:n - d]))
        curve[tau + T] = c / den
    at = int(np.argmax(np.abs(curve)))  # (the first of equal maxima)
    row.update(iacc=float(abs(curve[at])), lag=float(at - T), iacf=float(curve[at]), iacf0=float(curve[T]),
               level_db=float(10.0 * np.log10(EL / ER)), status=0.0)
    return row, curve


def iacc(taps, rate, bands=(), q=None, max_lag=None, split=0, onset_db=-20.0, end=0):
    """taps: float32 [n, 2] as Convolution.ir_taps gives them.  Returns what Convolution.ir_iacc(..., curve=True) returns."""
    taps = np.asarray(taps, np.float32).reshape(-1, 2)
    n = taps.shape[0]
    N = min(int(end), n) if end else n
    q = DEFAULT_Q if q is None else q
    T = default_lag(rate) if max_lag is None else int(max_lag)
    o = origin(taps, N, float(np.float32(onset_db)))
    k = min(o + (int(split) if split else int(np.floor(0.08 * float(rate) + 0.5))), N)
    x = taps[:N].astype(np.float64)
    rows = {}
    curve = np.full((1 + len(bands), 3, 2 * T + 1), np.nan)
    for g in range(1 + len(bands)):
        y = x
        if g:
            c = band_coefs(bands[g - 1], q, rate)
            y = biquad(biquad(x, c), c)
        for w, (name, (a, b)) in enumerate(zip(WINDOWS, ((o, k), (k, N), (o, N)))):
            rows[(g, name)], curve[g, w] = window_row(np.ascontiguousarray(y[a:b, 0]), np.ascontiguousarray(y[a:b, 1]), T)
    return dict(origin=o, taps=N, split=k, max_lag=T, rows=rows, curve=curve)


def margin(curve_row):
    """By how much |IACF(tau*)| exceeds |IACF| at every other lag (inf with a single lag)."""
    v = np.abs(np.asarray(curve_row, np.float64))
    at = int(np.argmax(v))
    rest = np.delete(v, at)
    return float(v[at] - rest.max()) if rest.size else float("inf")


def assert_margins(want, least=1e-6):
    """What every comparison with the device asserts on the restatement first: in every status-0 row |IACF(tau*)| exceeds |IACF| at
    every other lag by more than `least`, so that a flipped argmax cannot pass for rounding."""
    for (g, name), row in want["rows"].items():
        if row["status"] == 0.0:
            m = margin(want["curve"][g, WINDOWS.index(name)])
            assert m > least, (g, name, m)


def check_against(got, want, broad=1e-10, banded=1e-6, rel=1e-6, db=1e-6):
    """got: Convolution.ir_iacc's result; want: iacc()'s.  Equal integers (origin, taps, split, max_lag, tau*, status); IACC,
    IACF(tau*), IACF(0) and every curve entry to `broad` absolute in the broadband group and `banded` behind the band filters;
    the energies to `rel` relative, the level difference to `db` dB; NaN where and only where the restatement has NaN.  Prints
    the largest differences and returns them."""
    for f in ("origin", "taps", "split", "max_lag"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert set(got["rows"]) == set(want["rows"])
    worst = dict(broad=0.0, banded=0.0, energy=0.0, level_db=0.0)
    for key, w in want["rows"].items():
        g = got["rows"][key]
        kind = "banded" if key[0] else "broad"
        assert g["status"] == w["status"], (key, g["status"], w["status"])
        for f in FIELDS:
            assert np.isnan(g[f]) == np.isnan(w[f]), (key, f, g[f], w[f])
        for f in ("energy_l", "energy_r"):
            worst["energy"] = max(worst["energy"], abs(g[f] - w[f]) / w[f] if w[f] else abs(g[f]))
        if w["status"] != 0.0:
            continue
        assert g["lag"] == w["lag"], (key, g["lag"], w["lag"])
        for f in ("iacc", "iacf", "iacf0"):
            worst[kind] = max(worst[kind], abs(g[f] - w[f]))
        worst["level_db"] = max(worst["level_db"], abs(g["level_db"] - w["level_db"]))
    if got["curve"] is not None:
        assert got["curve"].shape == want["curve"].shape, (got["curve"].shape, want["curve"].shape)
        assert np.array_equal(np.isnan(got["curve"]), np.isnan(want["curve"]))
        diff = np.abs(got["curve"] - want["curve"])
        for g in range(diff.shape[0]):
            if not np.isnan(diff[g]).all():
                kind = "banded" if g else "broad"
                worst[kind] = max(worst[kind], float(np.nanmax(diff[g])))
    print("largest differences:", ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    assert worst["broad"] <= broad, worst
    assert worst["banded"] <= banded, worst
    assert worst["energy"] <= rel, worst
    assert worst["level_db"] <= db, worst
    return worst


def tail_width(rho):
    """mc_ir_tail_width_from_iacc's arithmetic: float32(min(max(1 - rho, 0), 1)); ValueError for a rho that is not finite."""
    rho = float(rho)
    if not np.isfinite(rho):
        raise ValueError("rho is not finite")
    return float(np.float32(min(max(1.0 - rho, 0.0), 1.0)))


def pair_ir(n=6000, lead=0, rate=8000, t60=0.25, seed=7, mix=0.6, amp=0.3):
    """ir_decay_np.noise_ir's L with R = mix L + sqrt(1 - mix^2) (an independent draw), so that IACC is neither 0 nor 1."""
    from ir_decay_np import noise_ir

    a = noise_ir(n=n, lead=lead, rate=rate, t60=t60, seed=seed, amp=amp).astype(np.float64)
    out = a.copy()
    out[:, 1] = mix * a[:, 0] + np.sqrt(1.0 - mix * mix) * a[:, 1]
    return out.astype(np.float32)
