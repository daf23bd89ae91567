"""The parts step of an IR load (include/mcconv.h, mc_ir_parts; csrc/irparts.hip.h) restated in float64 with numpy, one channel
pair at a time, exactly as the header defines it:

    s_k = b_k - floor(x_k / 2); u_k(m) = 0 for m < s_k, 1 for m >= s_k + x_k, else (1 - cos(pi (m - s_k + 1) / (x_k + 1))) / 2
    w_0 = 1 - u_0, w_1 = u_0 - u_1, w_2 = u_1
    g = 10^(gain_db / 20) (negated: invert), a = (1 + width) / 2, b = (1 - width) / 2, gl = 1 - balance (balance > 0), gr = 1 + balance
    (balance < 0); c_LL = g gl a, c_LR = g gl b, c_RL = g gr b, c_RR = g gr a; swap exchanges the columns
    output frame n, parts 0, 1, 2 that are not muted: m = n - delay_p, 0 <= m < F and w_p(m) > 0: t = w_p(m) x[m];
    acc_L += fma(c_LR, t_R, c_LL t_L); acc_R += fma(c_RL, t_L, c_RR t_R)

The fma is made exactly where it matters (a product with 0, 1 or .5 is exact, and so the fma is the rounded sum) and as a
product and a sum otherwise, which differs from it by half an ulp of a double.  Test infrastructure only."""
import numpy as np

PARTS = ("direct", "early", "late")
MAX_DELAY = 1 << 24


def _three(v):
    return tuple(v) if isinstance(v, (tuple, list, np.ndarray)) else (v, v, v)


def starts(direct_end, early_end, xfade):
    return direct_end - xfade[0] // 2, early_end - xfade[1] // 2


def fade(m, s, x):
    """u_k at the frames m (int64 array)."""
    m = np.asarray(m, dtype=np.int64)
    u = 0.5 * (1.0 - np.cos(np.pi * (m - s + 1).astype(np.float64) / (float(x) + 1.0)))
    return np.where(m < s, 0.0, np.where(m >= s + x, 1.0, u))


def weights(F, direct_end=0, early_end=0, xfade=(0, 0)):
    """w [3, F] float64."""
    s0, s1 = starts(direct_end, early_end, xfade)
    m = np.arange(F, dtype=np.int64)
    u0, u1 = fade(m, s0, xfade[0]), fade(m, s1, xfade[1])
    return np.stack([1.0 - u0, u0 - u1, u1])


def coefficients(gain_db=0.0, width=1.0, balance=0.0, swap=(), invert=()):
    """c [3, 4] float64: c_LL, c_LR, c_RL, c_RR per part, from the struct's floats."""
    c = np.empty((3, 4))
    for p, name in enumerate(PARTS):
        g = 10.0 ** (float(np.float32(_three(gain_db)[p])) / 20.0) * (-1.0 if name in swap_names(invert) else 1.0)
        w, bal = float(np.float32(_three(width)[p])), float(np.float32(_three(balance)[p]))
        a, b = (1.0 + w) / 2.0, (1.0 - w) / 2.0
        gl, gr = (1.0 - bal if bal > 0 else 1.0), (1.0 + bal if bal < 0 else 1.0)
        row = [g * gl * a, g * gl * b, g * gr * b, g * gr * a]
        if name in swap_names(swap):
            row = [row[1], row[0], row[3], row[2]]
        c[p] = row
    return c


def swap_names(names):
    return (names,) if isinstance(names, str) else tuple(names)


def supports(F, direct_end=0, early_end=0, xfade=(0, 0)):
    """[(lo, hi)] of the three parts inside [0, F); empty when lo >= hi."""
    s0, s1 = starts(direct_end, early_end, xfade)
    return [(0, min(F, s0 + xfade[0])), (s0, min(F, s1 + xfade[1])), (s1, F)]


def frames_out_of(F, direct_end=0, early_end=0, xfade=(0, 0), delay=0, mute=(), frames_out=0):
    """Fo by the header's rule; 0 when the load is refused."""
    if frames_out:
        return int(frames_out)
    most = 0
    for p, (lo, hi) in enumerate(supports(F, direct_end, early_end, xfade)):
        if PARTS[p] not in swap_names(mute) and lo < hi:
            most = max(most, hi + int(_three(delay)[p]))
    return most


def parts64(x, direct_end=0, early_end=0, xfade=(0, 0), delay=0, gain_db=0.0, width=1.0, balance=0.0, mute=(), swap=(), invert=(), frames_out=0):
    """x: [F, 2] frames.  Returns (float64 [Fo, 2] before the rounding, info as Convolution.ir_parts_info gives it after such a
    load; its energy_out is that of the taps rounded to float32, as the device stores them)."""
    x = np.asarray(x).reshape(-1, 2).astype(np.float64)
    F = x.shape[0]
    w, c = weights(F, direct_end, early_end, xfade), coefficients(gain_db, width, balance, swap, invert)
    Fo = frames_out_of(F, direct_end, early_end, xfade, delay, mute, frames_out)
    assert Fo >= 1, "the load is refused"
    acc = np.zeros((Fo, 2))
    e = (x * x).sum(axis=1)
    energy = [float((w[p] * w[p] * e).sum()) for p in range(3)]
    lost_e, lost = 0.0, 0
    for p, name in enumerate(PARTS):
        if name in swap_names(mute):
            continue
        d = int(_three(delay)[p])
        m = np.flatnonzero(w[p] > 0.0)
        n = m + d
        out = (n < 0) | (n >= Fo)
        lost += int(out.sum())
        lost_e += float((w[p][m[out]] ** 2 * e[m[out]]).sum())
        m, n = m[~out], n[~out]
        tl, tr = w[p][m] * x[m, 0], w[p][m] * x[m, 1]
        acc[n, 0] += c[p][1] * tr + c[p][0] * tl
        acc[n, 1] += c[p][2] * tl + c[p][3] * tr
    y32 = acc.astype(np.float32).astype(np.float64)
    rest = energy[1] + energy[2]
    info = dict(frames=F, frames_out=Fo, direct_end=min(int(direct_end), F), early_end=min(int(early_end), F), energy_direct=energy[0],
                energy_early=energy[1], energy_late=energy[2], energy_out=float((y32 * y32).sum()), energy_lost=lost_e, lost=lost,
                drr_db=10.0 * np.log10(energy[0] / rest) if energy[0] > 0 and rest > 0 else None)
    return acc, info


def parted(x, **kw):
    """parts64 with the taps as the engine stores them: float32 [Fo, 2]."""
    y, info = parts64(x, **kw)
    return y.astype(np.float32), info


def noise(n, seed=0, level=0.25, db=60.0):
    """n frames [n, 2] float32 of noise that decays by `db` dB over its length; the right channel is different noise at a third of
    the left's level, so that a crossed coefficient shows."""
    rng = np.random.default_rng(4000 * seed + n)
    env = 10.0 ** (-(db / 20.0) * np.arange(n) / max(n, 1))
    x = np.stack([rng.standard_normal(n) * env, rng.standard_normal(n) * env / 3.0], axis=1)
    return (level * x).astype(np.float32)


def random_layout(rng, F):
    """(direct_end, early_end, xfade) within the struct's rules, boundaries anywhere from 0 to past F."""
    while True:
        b0, b1 = sorted(int(v) for v in rng.integers(0, F + F // 4 + 2, size=2))
        x = tuple(int(v) for v in rng.integers(0, max(F // 2, 2), size=2))
        s0, s1 = starts(b0, b1, x)
        if s0 >= 0 and s0 + x[0] <= s1:
            return b0, b1, x
