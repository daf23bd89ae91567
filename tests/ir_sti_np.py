"""Float64 restatement of the speech transmission index of a loaded IR (mc_ir_sti, cuda_audio_amd/csrc/irsti.hip.h).

Test infrastructure only: the product never imports it.  x = the n stored taps (float32 [n, 2]) as double, N = end ? min(end, n) : n
(include/mcconv.h):
  1. the origin o and the row groups y (broadband, then one per band) are ir_decay_np's steps 1 and 2;
  2. over the taps m in [o, N), per channel and modulation frequency F (a float32 taken as double), theta = 2 pi F (m - o) / rate:
     C = sum of y^2 cos theta, S = sum of y^2 sin theta, E = sum of y^2, each one np.dot.  F (m - o) is exact in double and is
     reduced modulo the rate exactly (np.fmod) before the division, so that theta carries two roundings however long the IR is.
     The third channel set's C, S and E are the sums of L's and R's;
  3. m = hypot(C, S) / E, times 1 / (1 + 10^(-snr_db / 10)) in a band group when snr_db is given; a set with E = 0 or an E that is not
     finite has status 1 and NaN for m and all that follows from it;
  4. TI = 1 for m >= 1, 0 for m <= 0, else min(max((10 log10(m / (1 - m)) + 15) / 30, 0), 1); MTI = (sum of TI, ascending) / n_mod;
  5. STI = sum of alpha_b MTI_b (ascending) less beta_b sqrt(MTI_b MTI_(b+1)) one by one (ascending); NaN without bands.
"""
import numpy as np

from ir_decay_np import DEFAULT_Q, band_coefs, origin
from ir_eq_np import biquad

SETS = ("L", "R", "LR")
MAX_BANDS, MAX_MOD = 7, 16
OCTAVES = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0)
MOD_HZ = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
ALPHA = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
BETA = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)
RATINGS = ((0.30, "bad"), (0.45, "poor"), (0.60, "fair"), (0.75, "good"))


def f32(v):
    return float(np.float32(v))


def ti(m):
    """Step 4 for an m that is a number."""
    m = float(m)
    if m >= 1.0:
        return 1.0
    if m <= 0.0:
        return 0.0
    return float(min(max((10.0 * np.log10(m / (1.0 - m)) + 15.0) / 30.0, 0.0), 1.0))


def rating(sti):
    for edge, word in RATINGS:
        if sti < edge:
            return word
    return "excellent"


def sums(e, F, rate):
    """e: float64 [n], the squares of one channel from the origin on.  Returns (C, S) at modulation frequency F."""
    k = np.arange(e.size, dtype=np.float64)
    theta = 2.0 * np.pi * (np.fmod(F * k, float(rate)) / float(rate))
    return float(np.dot(e, np.cos(theta))), float(np.dot(e, np.sin(theta)))


def group_rows(y, o, rate, mod_hz, gain=1.0):
    """y: float64 [N, 2], a row group's taps.  Returns ({set: row}, mtf [3, n_mod])."""
    nan = float("nan")
    e = y[o:] * y[o:]
    E = [float(np.sum(e[:, 0])), float(np.sum(e[:, 1]))]
    CS = [[sums(np.ascontiguousarray(e[:, c]), f32(F), rate) for F in mod_hz] for c in range(2)]
    E.append(E[0] + E[1])
    CS.append([(CS[0][f][0] + CS[1][f][0], CS[0][f][1] + CS[1][f][1]) for f in range(len(mod_hz))])
    rows, mtf = {}, np.full((3, len(mod_hz)), np.nan)
    for s, name in enumerate(SETS):
        ok = bool(np.isfinite(E[s]) and E[s] != 0.0)
        if ok:
            for f in range(len(mod_hz)):
                mtf[s, f] = float(np.hypot(CS[s][f][0], CS[s][f][1])) / E[s] * gain
        total = 0.0
        for f in range(len(mod_hz)):
            total += ti(mtf[s, f]) if ok else 0.0
        rows[name] = dict(energy=E[s], mti=total / len(mod_hz) if ok else nan, status=0 if ok else 1)
    return rows, mtf


def sti(taps, rate, bands=None, alpha=None, beta=None, mod_hz=None, snr_db=None, q=None, onset_db=-20.0, end=0):
    """taps: float32 [n, 2] as Convolution.ir_taps gives them.  Returns what Convolution.ir_sti returns."""
    taps = np.asarray(taps, np.float32).reshape(-1, 2)
    n = taps.shape[0]
    N = min(int(end), n) if end else n
    if bands is None:
        bands, alpha, beta = OCTAVES, (ALPHA if alpha is None else alpha), (BETA if beta is None else beta)
    elif alpha is None or beta is None:
        raise ValueError("bands of one's own need alpha and beta")
    mod_hz = MOD_HZ if mod_hz is None else tuple(mod_hz)
    q = DEFAULT_Q if q is None else q
    o = origin(taps, N, f32(onset_db))
    x = taps[:N].astype(np.float64)
    rows, mtf = {}, np.full((1 + len(bands), 3, len(mod_hz)), np.nan)
    for g in range(1 + len(bands)):
        y, gain = x, 1.0
        if g:
            c = band_coefs(bands[g - 1], q, rate)
            y = biquad(biquad(x, c), c)
            if snr_db is not None:
                gain = 1.0 / (1.0 + 10.0 ** (-f32(snr_db[g - 1]) / 10.0))
        r, mtf[g] = group_rows(y, o, rate, mod_hz, gain)
        for name in SETS:
            rows[(g, name)] = r[name]
    out = {}
    for name in SETS:
        v = 0.0 if len(bands) else float("nan")
        mti = [rows[(b + 1, name)]["mti"] for b in range(len(bands))]
        for b in range(len(bands)):
            v += float(alpha[b]) * mti[b]
        for b in range(len(bands) - 1):
            v -= float(beta[b]) * float(np.sqrt(mti[b] * mti[b + 1]))
        out[name] = v
    return dict(origin=o, taps=N, sti=out, rows=rows, mtf=mtf)


def schroeder(r, n, F, rate):
    """m(F) of e[m] = r^m, m < n: |(1 - z^n) / (1 - z)| (1 - r) / (1 - r^n), z = r e^(-j 2 pi F / rate)."""
    z = r * np.exp(-2j * np.pi * np.asarray(F, np.float64) / float(rate))
    return np.abs((1.0 - z ** n) / (1.0 - z)) * (1.0 - r) / (1.0 - r ** n)


def check_against(got, want, broad=1e-10, broad_ti=1e-9, banded=1e-6, banded_ti=1e-5, rel=1e-6):
    """got: Convolution.ir_sti's result; want: sti()'s.  Equal integers (origin, taps, status); m to `broad` absolute in the
    broadband group and `banded` behind the band filters; MTI to `broad_ti` and `banded_ti`, STI to `banded_ti`; the energies to
    `rel` relative; NaN where and only where the restatement has NaN.  Prints the largest differences and returns them."""
    for f in ("origin", "taps"):
        assert got[f] == want[f], (f, got[f], want[f])
    assert set(got["rows"]) == set(want["rows"])
    assert got["mtf"].shape == want["mtf"].shape, (got["mtf"].shape, want["mtf"].shape)
    assert np.array_equal(np.isnan(got["mtf"]), np.isnan(want["mtf"]))
    worst = dict(broad=0.0, broad_mti=0.0, banded=0.0, banded_mti=0.0, sti=0.0, energy=0.0)
    for key, w in want["rows"].items():
        g = got["rows"][key]
        kind = "banded" if key[0] else "broad"
        assert g["status"] == w["status"], (key, g["status"], w["status"])
        assert np.isnan(g["mti"]) == np.isnan(w["mti"]), (key, g["mti"], w["mti"])
        assert not np.isnan(g["energy"]) or np.isnan(w["energy"]), (key, g["energy"], w["energy"])
        worst["energy"] = max(worst["energy"], abs(g["energy"] - w["energy"]) / w["energy"] if w["energy"] else abs(g["energy"]))
        if w["status"] == 0:
            worst[kind + "_mti"] = max(worst[kind + "_mti"], abs(g["mti"] - w["mti"]))
            s = SETS.index(key[1])
            worst[kind] = max(worst[kind], float(np.max(np.abs(got["mtf"][key[0], s] - want["mtf"][key[0], s]))))
    for name in SETS:
        assert np.isnan(got["sti"][name]) == np.isnan(want["sti"][name]), (name, got["sti"][name], want["sti"][name])
        if not np.isnan(want["sti"][name]):
            worst["sti"] = max(worst["sti"], abs(got["sti"][name] - want["sti"][name]))
    print("largest differences:", ", ".join(f"{f} {v:.1e}" for f, v in worst.items()))
    assert worst["broad"] <= broad, worst
    assert worst["broad_mti"] <= broad_ti, worst
    assert worst["banded"] <= banded, worst
    assert worst["banded_mti"] <= banded_ti and worst["sti"] <= banded_ti, worst
    assert worst["energy"] <= rel, worst
    return worst
