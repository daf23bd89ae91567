"""float64 restatements of mc_ir_spring (include/mcconv.h), for the spring tests.

(a) spring_plan64, spring_response64, spring64: the contract itself: the constants in spring_check's order of operations, the
    transfer function bin by bin on the circle of radius rho with the same square-and-multiply steps, np.fft.ifft, the radius
    undone.
(b) recursion64: the model run in time, sample by sample: delay lines, all-pass sections, the one-pole, the loop's feedback,
    the biquads (designed from the analogue poles, not by (a)'s formulas).  It shares no code with (a) beyond the rounding of
    the fields to float32.
"""
import math

import numpy as np

RADIUS = 1e8
Q = 2.0 ** 40
DEFAULTS = dict(sections=100, transition_hz=4300.0, dispersion=0.62, delay_ms=(66.0, 82.0), t60=2.5, damping=0.2, lowpass_order=8, high_gain=0.1,
                high_sections=200, high_dispersion=-0.6, high_delay=0.5, high_t60=1.0, stereo=0.03, gain=1.0, log2_points=0, last=0)


def f32(v):
    return float(np.float32(v))


def fields(**kw):
    """The struct's fields as the library sees them: floats rounded to float32, then taken as double."""
    p = dict(DEFAULTS)
    p.update(kw)
    d = tuple(p["delay_ms"]) if isinstance(p["delay_ms"], (tuple, list)) else (p["delay_ms"],)
    p["delay_ms"] = tuple(f32(v) for v in d if v != 0)
    for k in ("transition_hz", "dispersion", "t60", "damping", "high_gain", "high_dispersion", "high_delay", "high_t60", "stereo", "gain"):
        p[k] = f32(p[k])
    return p


def loop_fields(rate, K, M, a, L, g, **kw):
    """Fields of one spring whose loop has the stretch K, M sections of coefficient a, the delay L frames and a gain near g
    (t60 is a float32): transition_hz, sections, dispersion, delay_ms and t60 from them, the rest from kw."""
    own = float(np.rint((M * K * (1.0 - f32(a))) / (1.0 + f32(a))))
    ms = 1000.0 * (L + own) / rate
    t60 = 0.0 if g == 0 else -3.0 * (f32(ms) / 1000.0) / math.log10(abs(g))
    out = dict(transition_hz=rate / (2.0 * K), sections=M, dispersion=a, delay_ms=(ms,), t60=t60, stereo=0.0, high_gain=0.0, lowpass_order=0, damping=0.0)
    out.update(kw)
    return out


def _gain(t60, T):
    return -math.pow(10.0, (-3.0 * T) / t60) if t60 != 0 else 0.0


# -- (a) ----------------------------------------------------------------------------------------------------------------
def spring_plan64(rate, frames, **kw):
    """spring_check's numbers: a dict with the constants (K, M, L[s][c], g[s][c], Lh, gh, bq ...) and, with frames, N, E, lnrho and
    the alias bound."""
    p = fields(**kw)
    S = len(p["delay_ms"])
    K = max(1.0, float(np.rint(rate / (2.0 * p["transition_hz"]))))
    a, c, ah = p["dispersion"], p["damping"], p["high_dispersion"]
    M, Mh = int(p["sections"]), int(p["high_sections"])
    MK = M * K
    own = float(np.rint((MK * (1.0 - a)) / (1.0 + a)))
    L, g, Lh, gh = [], [], [], []
    gmax = trip = ghmax = htrip = 0.0
    for s in range(S):
        L.append([]), g.append([]), Lh.append([]), gh.append([])
        for ch in range(2):
            T0 = p["delay_ms"][s] / 1000.0
            T = T0 * (1.0 + p["stereo"]) if ch else T0
            l = float(np.rint(T * rate)) - own
            assert l >= 1
            L[s].append(int(l)), g[s].append(_gain(p["t60"], T))
            Lh[s].append(int(max(1.0, float(np.rint((p["high_delay"] * T) * rate))))), gh[s].append(_gain(p["high_t60"], T))
            gmax, trip = max(gmax, abs(g[s][ch])), max(trip, l + (MK * (1.0 + a)) / (1.0 - a))
            ghmax, htrip = max(ghmax, abs(gh[s][ch])), max(htrip, Lh[s][ch] + (Mh * (1.0 - ah)) / (1.0 + ah))
    nb = p["lowpass_order"] // 2 if K > 1 else 0
    bq = []
    if nb:
        W, n = math.tan(math.pi / (2.0 * K)), float(p["lowpass_order"])
        for i in range(nb):
            q = (2.0 * math.sin((math.pi * (2.0 * i + 1.0)) / (2.0 * n))) * W
            a0 = (1.0 + q) + W * W
            bq.append(((W * W) / a0, (2.0 * (W * W - 1.0)) / a0, ((1.0 - q) + W * W) / a0))
    pl = dict(S=S, K=int(K), M=M, Mh=Mh, a=a, c=c, ah=ah, hg=p["high_gain"], high=p["high_gain"] != 0, scale=p["gain"] / math.sqrt(S), L=L, g=g, Lh=Lh,
              gh=gh, bq=bq, ft=rate / (2.0 * K), lnrho=0.0)
    if frames:
        E = min(p["last"], frames) if p["last"] else frames
        lg = int(p["log2_points"])
        if not lg:
            lg = 10
            while (1 << lg) < 2 * E:
                lg += 1
        N = 1 << lg
        assert E <= N // 2 and lg <= 22
        bound = math.pow(gmax, math.floor((N - E) / trip))
        if pl["high"]:
            bound = max(bound, math.pow(ghmax, math.floor((N - E) / htrip)))
        bound /= RADIUS
        pl.update(N=N, E=E, F=frames, lnrho=math.log(RADIUS) / N, alias=bound, alias_db=max(-400.0, 20.0 * math.log10(bound)) if bound > 0 else -400.0)
    return pl


def plan_numbers(pl):
    """The twenty-four numbers of mc_ir_spring_plan from spring_plan64's dict."""
    out = [0.0] * 24
    out[:8] = [pl["N"], pl["K"], pl["ft"], pl["S"], pl["M"], 1.0 if pl["bq"] else 0.0, pl["E"], pl["alias_db"]]
    for s in range(pl["S"]):
        for ch in range(2):
            out[8 + 2 * s + ch], out[14 + 2 * s + ch] = float(pl["L"][s][ch]), pl["g"][s][ch]
    return out


def _pow(A, m):
    """A^m by square-and-multiply from m's highest bit down."""
    if not m:
        return np.ones_like(A)
    r = A.copy()
    for b in range(m.bit_length() - 2, -1, -1):
        r = r * r
        if (m >> b) & 1:
            r = r * A
    return r


def _eval(pl, zp):
    """H_L and H_R where zp(q) = z^-q, in spring_eval's order."""
    z1 = zp(1)
    zK = z1 if pl["K"] == 1 else zp(pl["K"])
    A = (pl["a"] + zK) / (1.0 + pl["a"] * zK)
    P = (1.0 - pl["c"]) / (1.0 - pl["c"] * z1)
    CP = _pow(A, pl["M"]) * P
    B = None
    if pl["bq"]:
        z2 = z1 * z1
        B = np.ones_like(z1)
        for b0, a1, a2 in pl["bq"]:
            B = B * ((b0 * ((1.0 + 2.0 * z1) + z2)) / ((1.0 + a1 * z1) + a2 * z2))
    Ch = _pow((pl["ah"] + z1) / (1.0 + pl["ah"] * z1), pl["Mh"]) if pl["high"] else None
    H = [np.zeros_like(z1), np.zeros_like(z1)]
    for s in range(pl["S"]):
        for ch in range(2):
            u = CP * zp(pl["L"][s][ch])
            h = u / (1.0 - pl["g"][s][ch] * u)
            if B is not None:
                h = B * h
            if pl["high"]:
                uh = Ch * zp(pl["Lh"][s][ch])
                h = h + pl["hg"] * (uh / (1.0 - pl["gh"][s][ch] * uh))
            H[ch] = H[ch] + h
    return pl["scale"] * H[0], pl["scale"] * H[1]


def spring_response64(rate, hz, **kw):
    """H_L, H_R on the unit circle at hz: complex128 [len(hz), 2]."""
    pl = spring_plan64(rate, 0, **kw)
    nu = np.asarray(hz, np.float64) / rate

    def zp(q):
        turn = nu * q
        frac = turn - np.floor(turn)
        return np.cos(2.0 * np.pi * frac) - 1j * np.sin(2.0 * np.pi * frac)

    return np.stack(_eval(pl, zp), axis=1)


def spring64(rate, frames, **kw):
    """The spring's term of a load of `frames` frames, in whole quanta of 2^-40: float64 [frames, 2] (zero from E on), and the plan."""
    pl = spring_plan64(rate, frames, **kw)
    N, E = pl["N"], pl["E"]
    k = np.arange(N, dtype=np.int64)

    def zp(q):
        ang = ((k * q) % N).astype(np.float64) * (2.0 / N)
        return np.exp(-(q * pl["lnrho"])) * (np.cos(np.pi * ang) - 1j * np.sin(np.pi * ang))

    HL, HR = _eval(pl, zp)
    x = np.fft.ifft(HL + 1j * HR)
    up = np.exp(np.arange(E) * pl["lnrho"])
    out = np.zeros((frames, 2))
    out[:E, 0], out[:E, 1] = x.real[:E] * up, x.imag[:E] * up
    return np.rint(out * Q) / Q, pl  # (the accumulator's quantum: to nearest, ties to even)


# -- (b) ----------------------------------------------------------------------------------------------------------------
class _Delay:
    def __init__(self, n):
        self.buf, self.at = [0.0] * n, 0

    def step(self, x):
        y = self.buf[self.at]
        self.buf[self.at] = x
        self.at = (self.at + 1) % len(self.buf)
        return y


class _AllPass:  # y[n] = a x[n] + x[n - K] - a y[n - K]
    def __init__(self, a, K):
        self.a, self.x, self.y = a, _Delay(K), _Delay(K)

    def step(self, x):
        y = self.a * x + self.x.step(x)
        y -= self.a * self.y.buf[self.y.at]
        self.y.step(y)
        return y


def _loop(n, a, K, M, c, L, g):
    """n frames of the impulse response of U / (1 - g U), U = A^M P z^-L, run sample by sample."""
    cells, line = [_AllPass(a, K) for _ in range(M)], _Delay(L)
    pole, out = 0.0, []
    w = 0.0
    for t in range(n):
        w = line.buf[line.at]  # U's output now: what went into the line L frames ago
        v = (1.0 if t == 0 else 0.0) + g * w
        for cell in cells:
            v = cell.step(v)
        pole = (1.0 - c) * v + c * pole
        line.step(pole)
        out.append(w)
    return np.array(out)


def _butter(x, order, K):
    """Butterworth low-pass at rate / (2 K) from its analogue poles by the bilinear transform with pre-warping, as biquads
    run sample by sample."""
    W = math.tan(math.pi / (2 * K))
    y = list(x)
    for i in range(order // 2):
        pole = W * complex(-math.sin(math.pi * (2 * i + 1) / (2 * order)), math.cos(math.pi * (2 * i + 1) / (2 * order)))
        zpole = (1 + pole) / (1 - pole)
        a1, a2 = -2 * zpole.real, abs(zpole) ** 2
        b0 = (1 + a1 + a2) / 4  # unity at 0 Hz
        x1 = x2 = y1 = y2 = 0.0
        for t, v in enumerate(y):
            o = b0 * (v + 2 * x1 + x2) - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, v, y1, o
            y[t] = o
    return np.array(y)


def recursion64(rate, n, **kw):
    """n frames of the tank's own impulse response h (no radius, no wrap, `last` not applied): float64 [n, 2]."""
    p = fields(**kw)
    S = len(p["delay_ms"])
    K = max(1, int(np.rint(rate / (2.0 * p["transition_hz"]))))
    a, M = p["dispersion"], int(p["sections"])
    own = int(np.rint(M * K * (1 - a) / (1 + a)))
    out = np.zeros((n, 2))
    for s in range(S):
        for ch in range(2):
            T = p["delay_ms"][s] / 1000.0 * ((1 + p["stereo"]) if ch else 1.0)
            g = -10.0 ** (-3 * T / p["t60"]) if p["t60"] else 0.0
            h = _loop(n, a, K, M, p["damping"], int(np.rint(T * rate)) - own, g)
            if p["lowpass_order"] and K > 1:
                h = _butter(h, p["lowpass_order"], K)
            if p["high_gain"]:
                gh = -10.0 ** (-3 * T / p["high_t60"]) if p["high_t60"] else 0.0
                h = h + p["high_gain"] * _loop(n, p["high_dispersion"], 1, int(p["high_sections"]), 0.0, max(1, int(np.rint(p["high_delay"] * T * rate))), gh)
            out[:, ch] += h
    return out * (p["gain"] / math.sqrt(S))


def group_delay_closed(w, L, M, K, a):
    """The first echo's group delay in frames at w radians per frame: L + M K (1 - a^2) / (1 + 2 a cos(w K) + a^2)."""
    return L + M * K * (1 - a * a) / (1 + 2 * a * np.cos(w * K) + a * a)
