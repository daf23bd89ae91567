"""Float64 restatement of the IR sample-rate conversion (mc_load_ir_resampled, cuda_audio_amd/csrc/resample.hip.h).

Test infrastructure only: the product never imports it.  For an IR at `src` Hz in a session at `dst` Hz:
g = gcd(src, dst), p = dst / g, q = src / g, s = min(1, dst / src); output frame m sits at input time m q / p,
kept exact as n0 = (m q) // p and frac = ((m q) % p) / p;
    y[m] = (src / dst) * sum_n x[n] k(x_m - n),   x[n] = 0 outside [0, frames),
    k(d) = rho s sinc(rho s d) I0(beta sqrt(1 - (d / W)^2)) / I0(beta) for |d| < W = Z / s, else 0,
with Z = 64, beta = 9, rho = 0.955; ceil(frames p / q) output frames, pre-ringing before m = 0 dropped.
"""
import math

import numpy as np

Z = 64
BETA = 9.0
RHO = 0.955
MIN_RATE, MAX_RATE = 8000, 384000


def geometry(src, dst):
    g = math.gcd(src, dst)
    p, q = dst // g, src // g
    s = min(1.0, dst / src)
    W = Z / s
    Wi = math.ceil(W)
    return dict(p=p, q=q, s=s, W=W, Wi=Wi, L=2 * Wi, a=RHO * s, gain=src / dst)


def out_frames(frames, src, dst):
    g = geometry(src, dst)
    return -(-frames * g["p"] // g["q"])


def coef(d, src, dst):
    """k(d) * src / dst, float64, for an array of distances d (input frames)."""
    g = geometry(src, dst)
    d = np.asarray(d, dtype=np.float64)
    u = d / g["W"]
    inside = np.abs(d) < g["W"]
    w = np.i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / np.i0(BETA)
    return np.where(inside, g["gain"] * g["a"] * np.sinc(g["a"] * d) * w, 0.0)


def resample(x, src, dst, n=None):
    """x: [frames] or [frames, channels]; returns float64 of the first n (default: all) converted frames."""
    x = np.asarray(x, dtype=np.float64)
    frames = x.shape[0]
    nout = out_frames(frames, src, dst)
    n = nout if n is None else min(n, nout)
    if src == dst:
        return x[:n].copy()
    g = geometry(src, dst)
    p, q, Wi, L = g["p"], g["q"], g["Wi"], g["L"]
    m = np.arange(n, dtype=np.int64)
    mq = m * q
    n0, ph = mq // p, mq % p
    frac = ph / p
    table = p <= n
    if table:  # coefficients per phase (the same values the direct form gives; just fewer Bessel evaluations)
        tab = coef((Wi - 1 - np.arange(L))[None, :] + (np.arange(p) / p)[:, None], src, dst)
    acc = np.zeros((n,) + x.shape[1:])
    for j in range(L):
        idx = n0 - Wi + 1 + j
        ok = (idx >= 0) & (idx < frames)
        k = tab[ph, j] if table else coef((Wi - 1 - j) + frac, src, dst)
        v = x[np.clip(idx, 0, frames - 1)]
        v = v * ok.reshape((-1,) + (1,) * (x.ndim - 1))
        acc += k.reshape((-1,) + (1,) * (x.ndim - 1)) * v
    return acc
