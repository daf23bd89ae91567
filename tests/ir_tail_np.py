"""Float64 restatement of the tail step of an IR load (mc_load_ir_tail, cuda_audio_amd/csrc/irtail.hip.h): step 1a, which cuts
every band of the F frames at its knee or cross-fades it there into decaying noise.

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is with sequential loops:
  x        the F frames at the session's rate as double, cut or zero-padded to F' = length or F;
  P_k(.)   ir_damp_np.lowpasses: crossover k's two identical high-cut sections from rest at frame 0 over [0, F');
  fades    band j with K_j < F' is touched: W_j = min(fade, K_j), fo = 1, fi = 0 before K_j - W_j,
           theta = (pi / 2) (m - (K_j - W_j) + 1) / (W_j + 1), fo = cos theta, fi = sin theta inside the fade, fo = 0, fi = 1 from K_j on;
           a band with K_j >= F' (or None) has fo = 1, fi = 0 throughout;
  noise    v_L = gA, v_R = rho gA + sqrt(1 - rho^2) gB from the Philox words W(m, 3) as ir_synth_np's late field makes them from W(m, 0);
  q_j      fi_j A_(j,c) g_j where fi_j > 0 and 0 elsewhere, g_j = exp2(-((m - K_j) 3 log2(10)) / t60[j]),
           A_(j,c) = sqrt(10^(level_db[j][c] / 10) / beta_j), beta_j the share of white noise that band j passes;
  y        fo_X x + sum_k (fo_(k-1) - fo_k) P_k(x) [+ q_X v + sum_k (q_(k-1) - q_k) P_k(v) when extending], added in that order;
           frames before the first touched one are the input's.
"""
import numpy as np

import ir_damp_np
from ir_shape_np import DECAY_K
from ir_synth_np import u, words

BETA_POINTS = 8192


def noise64(seed, width, n):
    """v [n, 2]."""
    w = words(seed, np.arange(n), 3)
    gA = np.sqrt(-2.0 * np.log(u(w[0]))) * np.cos(2.0 * np.pi * u(w[1]))
    gB = np.sqrt(-2.0 * np.log(u(w[2]))) * np.cos(2.0 * np.pi * u(w[3]))
    rho = 1.0 - float(np.float32(width))
    return np.stack([gA, rho * gA + np.sqrt(1.0 - rho * rho) * gB], axis=1)


def beta(xovers, rate):
    """[beta_0 .. beta_X]; [1] without a crossover."""
    if not xovers:
        return [1.0]
    hz = (np.arange(BETA_POINTS) + 0.5) / BETA_POINTS * (rate / 2.0)
    H2 = [ir_damp_np.section_response(f, rate, hz) ** 2 for f in xovers]
    B = [H2[0]] + [H2[k + 1] - H2[k] for k in range(len(H2) - 1)] + [1.0 - H2[-1]]
    return [float(np.mean(np.abs(b) ** 2)) for b in B]


def touched(knee, n):
    return knee is not None and int(knee) < n


def fades(n, knee, fade):
    """(fo [n], fi [n]) of one band."""
    fo, fi = np.ones(n), np.zeros(n)
    if not touched(knee, n):
        return fo, fi
    K = int(knee)
    W = min(int(fade), K)
    m = np.arange(K - W, K, dtype=np.float64)
    theta = (np.pi / 2.0) * (m - (K - W) + 1.0) / (W + 1.0)
    fo[K - W:K], fi[K - W:K] = np.cos(theta), np.sin(theta)
    fo[K:], fi[K:] = 0.0, 1.0
    return fo, fi


def first_changed(n, knee, fade):
    return min([int(k) - min(int(fade), int(k)) for k in knee if touched(k, n)], default=n)


def tail_info(F, n, knee, fade):
    return dict(bands=sum(1 for k in knee if touched(k, n)), frames=F, length=n, first=first_changed(n, knee, fade))


def tail64(x, rate, mode, knee, xovers=(), fade=0, width=1.0, seed=0, length=0, t60=None, level_db=None):
    """x: [F, 2] at the session's rate.  mode "cut" or "extend"; knee, t60, level_db per band, low to high.  Returns the
    float64 [F', 2] before the rounding to float32 and the info Convolution.ir_tail_info gives."""
    assert mode in ("cut", "extend") and len(knee) == len(xovers) + 1
    src = np.asarray(x, np.float32).reshape(-1, 2)
    F = src.shape[0]
    n = int(length) or F
    xs = np.zeros((n, 2))
    xs[:min(F, n)] = src[:min(F, n)]
    X = len(xovers)
    f = [fades(n, knee[j], fade) for j in range(X + 1)]
    Px = ir_damp_np.lowpasses(xs, xovers, rate) if X else []
    y = f[X][0][:, None] * xs
    for k in range(1, X + 1):
        y = y + (f[k - 1][0] - f[k][0])[:, None] * Px[k - 1]
    if mode == "extend":
        v = noise64(seed, width, n)
        Pv = ir_damp_np.lowpasses(v, xovers, rate) if X else []
        b = beta(xovers, rate)
        m = np.arange(n, dtype=np.float64)
        q = []
        for j in range(X + 1):
            qj = np.zeros((n, 2))
            on = f[j][1] > 0.0
            if on.any():
                g = np.exp2(-((m[on] - float(int(knee[j]))) * DECAY_K) / float(int(t60[j])))
                A = np.sqrt(10.0 ** (np.array([float(np.float32(l)) for l in level_db[j]]) / 10.0) / b[j])
                qj[on] = (f[j][1][on] * g)[:, None] * A[None, :]
            q.append(qj)
        y = y + q[X] * v
        for k in range(1, X + 1):
            y = y + (q[k - 1] - q[k]) * Pv[k - 1]
    first = first_changed(n, knee, fade)
    y[:first] = xs[:first]
    return y, tail_info(F, n, knee, fade)


def tailed(x, rate, mode, knee, **kw):
    """tail64 with the frames as the device hands them on: float32 [F', 2]."""
    y, info = tail64(x, rate, mode, knee, **kw)
    return y.astype(np.float32), info
