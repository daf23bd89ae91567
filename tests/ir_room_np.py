"""Float64 restatement of the reflections of a rectangular room (mc_synth_ir_room, cuda_audio_amd/csrc/irroom.hip.h).

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is once more over numpy
arrays, everything in float64 from the float32 fields:
  receivers r_L, r_R = receiver -/+ spacing / 2 along axis;
  images    n in [-N, N]^3, u in {0, 1}^3: p_a = ((1 - 2 u_a) s_a + 2 n_a L_a) - r_a, d = |p|,
            a = gain b_x b_y b_z / d, b_a = beta_(a,0)^|n_a - u_a| beta_(a,1)^|n_a| (0^0 = 1), tau = d rate / c;
  taps      k0 = floor(tau), f = tau - k0, s = sin(pi f); k = -15 .. 16, x = k - f:
            w_k = (k odd ? s : -s) / (pi x) * (1 + cos(pi x / 16)) / 2; f == 0: the one tap k = 0;
  sum       channel c of an image is kept iff k0 < E = last ? min(last, F) : F; q = rint(a w_k 2^40) as int64, added by
            np.add.at into acc[k0 + k] where 0 <= k0 + k < F;
  a frame   ir_synth_np.frames64 + acc 2^-40; frames() rounds it to float32 once.
"""
import math

import numpy as np

import ir_synth_np

MAX_ORDER = 32
Q = float(2 ** 40)
DEFAULTS = dict(size=(5.0, 4.0, 3.0), source=(1.0, 1.5, 1.2), receiver=(3.5, 2.0, 1.5), beta=0.9, spacing=0.2, axis=0, speed=343.0, gain=1.0, order=0,
                last=0)
K = np.arange(-15, 17)


def spec(**kw):
    """The fields of an IrRoom with the library's defaults; beta as six numbers."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    p = dict(DEFAULTS, **kw)
    p["beta"] = tuple(p["beta"]) if isinstance(p["beta"], (tuple, list)) else (p["beta"],) * 6
    return p


def _f(v):
    return float(np.float32(v))


def geometry(p):
    """(L [3], s [3], r [2, 3], beta [6], c, gain) in float64 from the float32 fields."""
    p = spec(**p)
    L, s, centre = (np.array([_f(v) for v in p[k]]) for k in ("size", "source", "receiver"))
    r = np.stack([centre, centre])
    r[0, p["axis"]] = centre[p["axis"]] - _f(p["spacing"]) / 2.0
    r[1, p["axis"]] = centre[p["axis"]] + _f(p["spacing"]) / 2.0
    return L, s, r, np.array([_f(b) for b in p["beta"]]), _f(p["speed"]), _f(p["gain"])


def last(p, F):
    p = spec(**p)
    return min(int(p["last"]), int(F)) if p["last"] else int(F)


def order(p, rate, F):
    """N: the order given, or with 0 the smallest whose lattice holds every image that arrives before frame E."""
    p = spec(**p)
    if p["order"]:
        return int(p["order"])
    L, _, _, _, c, _ = geometry(p)
    return int(math.ceil(float(last(p, F)) * c / (float(rate) * 2.0 * float(L.min()))))


def complete(p, rate, N):
    L, _, _, _, c, _ = geometry(p)
    return int(math.floor(float(2 * N) * float(L.min()) * float(rate) / c))


def images(p, rate, F, N=None):
    """Every image of the lattice: dict(n [M, 3], u [M, 3], d [M, 2], a [M, 2], tau [M, 2]), the last axis the channel."""
    p = spec(**p)
    L, s, r, beta, c, gain = geometry(p)
    if N is None:
        N = order(p, rate, F)
    rng = np.arange(-N, N + 1)
    grid = np.meshgrid(rng, rng, rng, (0, 1), (0, 1), (0, 1), indexing="ij")
    n, u = (np.stack(g, axis=-1).reshape(-1, 3) for g in (grid[:3], grid[3:]))
    q = (1 - 2 * u).astype(np.float64) * s + (2 * n).astype(np.float64) * L
    pos = q[:, None, :] - r[None, :, :]  # [M, 2, 3]
    d = np.sqrt(pos[..., 0] * pos[..., 0] + pos[..., 1] * pos[..., 1] + pos[..., 2] * pos[..., 2])
    b = np.full(len(n), gain)
    for ax in range(3):
        b = b * (np.power(beta[2 * ax], np.abs(n[:, ax] - u[:, ax]).astype(np.float64)) * np.power(beta[2 * ax + 1], np.abs(n[:, ax]).astype(np.float64)))
    return dict(n=n, u=u, d=d, a=b[:, None] / d, tau=d * float(rate) / c, order=N)


def assert_floor_margin(tau, E, exact=0):
    """No delay that decides anything - one of an image kept, or within a frame of E - lies within 1e-7 of a whole frame, where
    a rounding could move floor(tau) on the device: but for the `exact` delays that are whole frames by construction.  With E a
    whole number this covers the decision k0 < E too."""
    t = np.asarray(tau, np.float64).ravel()
    t = t[t < E + 1]
    dist = np.abs(t - np.rint(t))
    assert int((dist == 0).sum()) == exact, (int((dist == 0).sum()), exact)
    near = dist[dist > 0]
    assert near.size == 0 or near.min() > 1e-7, near.min()


def render(p, rate, F, N=None):
    """(acc int64 [F, 2], covered bool [F, 2], info): the integer sums, the frames some kept window of an image with a != 0
    reaches, and what mc_ir_room_info reports."""
    p = spec(**p)
    F = int(F)
    im = images(p, rate, F, N)
    E = last(p, F)
    acc = np.zeros((F, 2), np.int64)
    covered = np.zeros((F, 2), bool)
    k0 = np.floor(im["tau"])
    keep = k0 < E
    for ch in range(2):
        sel = keep[:, ch] & (im["a"][:, ch] != 0.0)
        a, tau, base = im["a"][sel, ch], im["tau"][sel, ch], k0[sel, ch].astype(np.int64)
        f = tau - np.floor(tau)
        s = np.sin(np.pi * f)
        x = K[None, :].astype(np.float64) - f[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(K[None, :] & 1, s[:, None], -s[:, None]) / (np.pi * x) * ((1.0 + np.cos(np.pi * x / 16.0)) / 2.0)
        whole = f == 0.0
        w[whole] = (K == 0).astype(np.float64)
        qv = np.rint(a[:, None] * w * Q).astype(np.int64)
        m = base[:, None] + K[None, :]
        ok = (m >= 0) & (m < F)
        np.add.at(acc[:, ch], m[ok], qv[ok])
        reach = ok & ~(whole[:, None] & (K[None, :] != 0))
        covered[np.unique(m[reach]), ch] = True
    direct = im["tau"][(np.abs(im["n"]).sum(axis=1) == 0) & (im["u"].sum(axis=1) == 0)][0]
    info = dict(order=im["order"], images=(int(keep[:, 0].sum()), int(keep[:, 1].sum())), direct=(float(direct[0]), float(direct[1])), last=E,
                complete=complete(p, rate, im["order"]))
    return acc, covered, info


def frames64(p, rate, N=None, **synth):
    """The F frames before the rounding to float32: ir_synth_np's three terms, then the room's.  (float64 [F, 2], covered, info)"""
    base = ir_synth_np.frames64(**synth)
    acc, covered, info = render(p, rate, len(base), N)
    return base + acc.astype(np.float64) * (1.0 / Q), covered, info


def frames(p, rate, N=None, **synth):
    out, covered, info = frames64(p, rate, N, **synth)
    return out.astype(np.float32), covered, info


def plan(p, rate, F):
    """What mc_ir_room_plan reports."""
    p = spec(**p)
    L, s, r, beta, c, _ = geometry(p)
    N = order(p, rate, F)
    V = float(L[0] * L[1] * L[2])
    area = np.array([L[1] * L[2], L[1] * L[2], L[0] * L[2], L[0] * L[2], L[0] * L[1], L[0] * L[1]])
    S, A = float(area.sum()), float((area * (1.0 - beta * beta)).sum())
    k = 24.0 * math.log(10.0) / c
    d = np.sqrt(((s[None, :] - r) ** 2).sum(axis=1))
    with np.errstate(divide="ignore"):
        eyring = k * V / (-S * float(np.log1p(-A / S))) if A > 0 else 0.0
    return dict(order=N, images=8 * (2 * N + 1) ** 3, complete=complete(p, rate, N), direct=(float(d[0] * rate / c), float(d[1] * rate / c)), volume=V,
                sabine=k * V / A if A > 0 else 0.0, eyring=eyring)
