"""Float64 restatement of the echo density of a loaded IR (mc_ir_density, cuda_audio_amd/csrc/irdensity.hip.h), window by window.

Test infrastructure only: the product never imports it.  x = the n stored taps (float32 [n, 2]) as double, N = end ? min(end, n) : n,
the origin o is ir_decay_np.origin's (include/mcconv.h):
  H = half or floor(0.01 rate + 0.5); hop = hop or max(1, H // 4);
  h_k = (1 + cos(pi k / (H + 1))) / 2, k = -H .. H;
  centres t_i = o + i hop, i < I = (N - 1 - o) // hop + 1; window i = the taps tau in [max(t_i - H, 0), min(t_i + H, N - 1)];
  v_c[tau] = x_c[tau] * (exp2((tau - t_i) 3 log2(10) / decay_t60) if decay_t60 else 1);
  ws = sum h, S_c = sum h v_c^2, sigma_L = sqrt(S_L / ws), sigma_R likewise, sigma_LR = sqrt((S_L + S_R) / (2 ws));
  A_L = sum h [|v_L| > sigma_L], A_R likewise, A_LR = (sum h [|v_L| > sigma_LR] + sum h [|v_R| > sigma_LR]) / 2;
  eta_s[i] = A_s / (ws erfc(1 / sqrt 2)); a window with sigma_s = 0 is silent for set s;
  rows: i* = the first i with eta_s[i] >= threshold (a float32); {mix = t_(i*), mix_s = (t_(i*) - o) / rate, first = eta[0], max,
  max_tap = the tap of the first maximum, mean_after = the mean of eta over i >= i*, silent, status}; status 1 when the threshold
  is never reached: mix, mix_s and mean_after are NaN.
"""
import math

import numpy as np

from ir_decay_np import origin

SETS = ("L", "R", "LR")
FIELDS = ("mix", "mix_s", "first", "max", "max_tap", "mean_after", "silent", "status")
GAUSS_SHARE = 0.31731050786291415  # erfc(1 / sqrt 2)
DECAY_K = 9.965784284662087        # 3 log2(10)
EXACT = ("mix", "max_tap", "silent", "status")


def weights(H):
    k = np.arange(-H, H + 1, dtype=np.float64)
    return (1.0 + np.cos(np.pi * k / (H + 1.0))) / 2.0


def defaults(rate, half=0, hop=0):
    H = int(half) or int(math.floor(0.01 * float(rate) + 0.5))
    return H, int(hop) or max(1, H // 4)


def density(taps, rate, half=0, hop=0, onset_db=-20.0, end=0, threshold=1.0, decay_t60=0):
    """taps: float32 [n, 2] as Convolution.ir_taps gives them.  Returns what Convolution.ir_density(profile=True) returns, plus
    "sigma_margin": the smallest | |v| - sigma | / sigma over every window and channel set with sigma > 0, "threshold": the
    threshold as the library holds it, and "silent": bool [I, 3]."""
    taps = np.asarray(taps, np.float32).reshape(-1, 2)
    n = taps.shape[0]
    N = min(int(end), n) if end else n
    H, hop = defaults(rate, half, hop)
    threshold = float(np.float32(threshold))
    o = origin(taps, N, float(np.float32(onset_db)))
    x = taps[:N].astype(np.float64)
    h_all = weights(H)
    I = (N - 1 - o) // hop + 1
    eta = np.zeros((I, 3))
    silent = np.zeros((I, 3), bool)
    margin = float("inf")
    for i in range(I):
        t = o + i * hop
        lo, hi = max(t - H, 0), min(t + H, N - 1)
        k = np.arange(lo, hi + 1, dtype=np.int64) - t
        h = h_all[k + H]
        v = x[lo:hi + 1]
        if decay_t60:
            v = v * np.exp2(k.astype(np.float64) * DECAY_K / float(decay_t60))[:, None]
        ws = h.sum()
        S = (h[:, None] * (v * v)).sum(axis=0)
        a = np.abs(v)
        sigma = (math.sqrt(S[0] / ws), math.sqrt(S[1] / ws), math.sqrt((S[0] + S[1]) / (2.0 * ws)))
        A = [h[a[:, 0] > sigma[0]].sum(), h[a[:, 1] > sigma[1]].sum(), (h[a[:, 0] > sigma[2]].sum() + h[a[:, 1] > sigma[2]].sum()) / 2.0]
        for s in range(3):
            eta[i, s] = A[s] / (ws * GAUSS_SHARE)
            silent[i, s] = sigma[s] == 0.0
            if sigma[s] > 0.0:
                seen = a if s == 2 else a[:, s]
                margin = min(margin, float(np.abs(seen - sigma[s]).min() / sigma[s]))
    rows = {}
    nan = float("nan")
    for s, name in enumerate(SETS):
        e = eta[:, s]
        reached = np.nonzero(e >= threshold)[0]
        top = int(np.argmax(e))
        row = dict(mix=nan, mix_s=nan, first=float(e[0]), max=float(e[top]), max_tap=float(o + top * hop), mean_after=nan,
                   silent=float(silent[:, s].sum()), status=1.0)
        if reached.size:
            m = int(reached[0])
            row.update(mix=float(o + m * hop), mix_s=float(m * hop) / float(rate), mean_after=float(e[m:].sum() / (I - m)), status=0.0)
        rows[name] = row
    return dict(origin=o, taps=N, centres=I, hop=hop, half=H, rows=rows, profile=eta, sigma_margin=margin, threshold=threshold, silent=silent)


def assert_margins(res, least=1e-9):
    """What every comparison with the device asserts on the restatement first, so that the device can make no other decision
    than the restatement does: no |v| within `least` (relative) of its window's sigma; no eta within `least` (relative) of the
    threshold; and no other window within `least` (relative) of the largest eta, whose tap is compared exactly."""
    assert res["sigma_margin"] >= least, res["sigma_margin"]
    eta, th = res["profile"], res["threshold"]
    gap = float(np.abs(eta - th).min() / th)
    assert gap >= least, gap
    for s in range(3):
        e = eta[:, s]
        top = int(np.argmax(e))
        rest = np.delete(e, top)
        if rest.size and e[top] > 0.0:
            assert rest.max() <= e[top] * (1.0 - least), (s, top, float(rest.max()), float(e[top]))


def check_against(got, want, rel=1e-10):
    """got: Convolution.ir_density's result (profile=True); want: density()'s.  Equal integers for the origin, the taps, the
    centres, the mixing tap, the tap of the maximum, the silent count and the status; `rel` relative for every density; NaN where
    and only where the restatement has NaN.  Prints the largest difference."""
    for key in ("origin", "taps", "centres", "hop", "half"):
        assert got[key] == want[key], (key, got[key], want[key])
    worst = 0.0
    for name in SETS:
        g, w = got["rows"][name], want["rows"][name]
        for f in FIELDS:
            assert math.isnan(g[f]) == math.isnan(w[f]), (name, f, g[f], w[f])
            if math.isnan(w[f]):
                continue
            if f in EXACT:
                assert g[f] == w[f], (name, f, g[f], w[f])
            else:
                err = abs(g[f] - w[f])
                assert err <= rel * abs(w[f]), (name, f, g[f], w[f])
                worst = max(worst, err / abs(w[f]) if w[f] else 0.0)
    assert got["profile"].shape == want["profile"].shape == (want["centres"], 3)
    err = np.abs(got["profile"] - want["profile"])
    assert np.all(err <= rel * np.abs(want["profile"])), float(err.max())
    nz = want["profile"] != 0.0
    if nz.any():
        worst = max(worst, float((err[nz] / np.abs(want["profile"][nz])).max()))
    print(f"largest relative difference {worst:.1e} over {want['centres']} windows")


def impulse_profile(d, o, I, hop, H):
    """eta[i] of a single impulse at tap d for windows wholly inside the taps: h_(d - t_i) / (ws erfc(1 / sqrt 2)) where
    |d - t_i| <= H, 0 elsewhere."""
    h = weights(H)
    ws = h.sum()
    t = o + np.arange(I, dtype=np.int64) * hop
    k = d - t
    inside = np.abs(k) <= H
    out = np.zeros(I)
    out[inside] = h[k[inside] + H] / (ws * GAUSS_SHARE)
    return out
