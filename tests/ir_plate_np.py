"""Float64 restatement of a plate reverberator's IR (mc_synth_ir_plate, cuda_audio_amd/csrc/irplate.hip.h).

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is once more over numpy
arrays, everything in float64 from the float32 fields:
  plate     kappa = sqrt(E h^2 / (12 rho (1 - nu^2))), E = young_gpa 1e9, h = thickness_mm 1e-3;
  modes     m, n >= 1: f = (pi kappa / 2) ((m / Lx)^2 + (n / Ly)^2), kept when low <= f <= high (0: min(20000, 0.45 rate)), m
            ascending and n ascending within m; the operations in the library's order, so f is the library's double;
  loss      s_i = t60_i ? 3 ln 10 / t60_i : 0, sigma = s0 + (s1 - s0) f / damp_hz;
  amplitude a_c = gain 4 sqrt(2 / M) Phi(driver) Phi(pickup c), Phi(x, y) = sin(m pi x / Lx) sin(n pi y / Ly);
  term      for t < E = last ? min(last, F) : F: a_c exp(-sigma t / rate) cos(2 pi frac(nu t)), nu = f / rate, the phase nu t
            formed and reduced in np.longdouble (the library reduces it in turns with a fused multiply-add);
  sum       q = rint(a_c exp cos 2^40) as int64, summed per frame and channel;
  a frame   ir_synth_np.frames64 + acc 2^-40; frames() rounds it to float32 once.
"""
import math

import numpy as np

import ir_synth_np

MAX_MODES = 1 << 18
GROUP = 32
SLAB = 256
MAX_PAIRS = 1 << 36
Q = float(2 ** 40)
STEEL = (200.0, 7850.0, 0.3)
DEFAULTS = dict(size=(2.04, 0.97), thickness_mm=0.5, material="steel", driver=(0.83, 0.41), pickups=((0.31, 0.67), (1.57, 0.29)), low_hz=20.0,
                high_hz=0.0, t60=(4.0, 1.0), damp_hz=10000.0, gain=1.0, last=0)


def spec(**kw):
    """The fields of an IrPlate with the library's defaults; the material as three numbers."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    p = dict(DEFAULTS, **kw)
    p["material"] = STEEL if p["material"] == "steel" else tuple(p["material"])
    return p


def _f(v):
    return float(np.float32(v))


def kappa(p):
    p = spec(**p)
    E, rho, nu = (_f(v) for v in p["material"])
    E, h = E * 1e9, _f(p["thickness_mm"]) * 1e-3
    return math.sqrt(E * (h * h) / (12.0 * rho * (1.0 - nu * nu)))


def high(p, rate):
    p = spec(**p)
    return _f(p["high_hz"]) if _f(p["high_hz"]) != 0.0 else min(20000.0, 0.45 * float(rate))


def last(p, F):
    p = spec(**p)
    return min(int(p["last"]), int(F)) if p["last"] else int(F)


def loss(t60):
    return 3.0 * math.log(10.0) / _f(t60) if _f(t60) != 0.0 else 0.0


def modes(p, rate):
    """The mode table: dict(m, n int64 [M]; f, sigma float64 [M]; a float64 [M, 2]; M)."""
    p = spec(**p)
    Lx, Ly = (_f(v) for v in p["size"])
    lo, hi = _f(p["low_hz"]), high(p, rate)
    c = math.pi * kappa(p) / 2.0
    # every (m, n) that could lie at or under hi, with room to spare; the comparison below decides
    m_max = int(Lx * math.sqrt(hi / c)) + 2
    n_max = int(Ly * math.sqrt(hi / c)) + 2
    m = np.arange(1, m_max + 1, dtype=np.float64)[:, None]
    n = np.arange(1, n_max + 1, dtype=np.float64)[None, :]
    f = c * ((m / Lx) * (m / Lx) + (n / Ly) * (n / Ly))
    keep = (f >= lo) & (f <= hi)
    mi, ni = np.nonzero(keep)  # (row-major: m ascending, n ascending within m)
    f = f[keep]
    mm, nn = (mi + 1).astype(np.float64), (ni + 1).astype(np.float64)
    M = len(f)
    s0, s1 = loss(p["t60"][0]), loss(p["t60"][1])
    sigma = s0 + ((s1 - s0) * f) / _f(p["damp_hz"])

    def phi(at):
        return np.sin((mm * math.pi * _f(at[0])) / Lx) * np.sin((nn * math.pi * _f(at[1])) / Ly)

    a = np.zeros((M, 2))
    if M:
        scale = _f(p["gain"]) * 4.0 * math.sqrt(2.0 / float(M))
        d = phi(p["driver"])
        for ch in range(2):
            a[:, ch] = (scale * d) * phi(p["pickups"][ch])
    return dict(m=mi + 1, n=ni + 1, f=f, sigma=sigma, a=a, M=M)


def bracket(p, rate, count, skip=0):
    """(low_hz, high_hz) as float32-exact numbers that keep exactly the `count` modes after the `skip` lowest of p's own bracket
    (by frequency), each bound in the middle of a gap of at least a thousand float32 steps."""
    f = np.sort(modes(p, rate)["f"])
    assert skip + count < len(f) and (skip == 0 or skip >= 1)
    lo_gap = (f[skip - 1], f[skip]) if skip else (f[0] - 1.0, f[0])
    hi_gap = (f[skip + count - 1], f[skip + count])
    out = []
    for a, b in (lo_gap, hi_gap):
        mid = float(np.float32(0.5 * (a + b)))
        assert a < mid < b and min(mid - a, b - mid) > 1000.0 * float(np.spacing(np.float32(mid))), (a, mid, b)
        out.append(mid)
    return tuple(out)


def sums(p, rate, t, chunk=4096):
    """The integer sums of the plate's term at the frames t (ascending; the caller keeps them under E): int64 [len(t), 2]."""
    tb = modes(p, rate)
    t = np.asarray(t, np.int64)
    acc = np.zeros((len(t), 2), np.int64)
    nu = (tb["f"] / float(rate)).astype(np.longdouble)
    dec = tb["sigma"] / float(rate)
    for i in range(0, len(t), chunk):
        tt = t[i:i + chunk]
        ph = nu[:, None] * tt[None, :].astype(np.longdouble)
        turn = (ph - np.rint(ph)).astype(np.float64)
        v = np.exp(-(dec[:, None] * tt[None, :].astype(np.float64))) * np.cos(2.0 * np.pi * turn)  # [M, T]
        for ch in range(2):
            acc[i:i + chunk, ch] = np.rint(tb["a"][:, ch][:, None] * v * Q).astype(np.int64).sum(axis=0)
    return acc


def render(p, rate, F):
    """(acc int64 [F, 2], info): the integer sums and what mc_ir_plate_info reports."""
    p = spec(**p)
    F = int(F)
    tb = modes(p, rate)
    E = last(p, F)
    acc = np.zeros((F, 2), np.int64)
    acc[:E] = sums(p, rate, np.arange(E))
    info = dict(modes=tb["M"], sounding=(int((tb["a"][:, 0] != 0).sum()), int((tb["a"][:, 1] != 0).sum())), last=E,
                lowest=float(tb["f"].min()), highest=float(tb["f"].max()), kappa=kappa(p))
    return acc, info


def frames64(p, rate, **synth):
    """The F frames before the rounding to float32: ir_synth_np's three terms, then the plate's.  (float64 [F, 2], info)"""
    base = ir_synth_np.frames64(**synth)
    acc, info = render(p, rate, len(base))
    return base + acc.astype(np.float64) * (1.0 / Q), info


def frames(p, rate, **synth):
    out, info = frames64(p, rate, **synth)
    return out.astype(np.float32), info


def plan(p, rate, F):
    """What mc_ir_plate_plan reports."""
    p = spec(**p)
    tb = modes(p, rate)
    Lx, Ly = (_f(v) for v in p["size"])
    s0, s1 = loss(p["t60"][0]), loss(p["t60"][1])
    k = kappa(p)

    def t60_at(f):
        s = s0 + ((s1 - s0) * f) / _f(p["damp_hz"])
        return 3.0 * math.log(10.0) / s if s > 0.0 else 0.0

    hi = float(tb["f"].max())
    return dict(modes=tb["M"], lowest=float(tb["f"].min()), highest=hi, kappa=k, density=Lx * Ly / (2.0 * k), t60=(t60_at(_f(p["low_hz"])), t60_at(hi)),
                pairs=last(p, F) * tb["M"])
