"""Float64 restatement of the binaural listener in the room of mc_synth_ir_room_head (cuda_audio_amd/csrc/irroom.hip.h), on top
of tests/ir_room_np.py, tests/ir_room_mics_np.py and tests/ir_room_bands_np.py.

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is once more, sequential:
  head      a rigid sphere of radius a at the room's receiver (both ears from the centre; spacing and axis are not used); ear
            axes e_L = (cos(az + ear), sin(az + ear), 0), e_R = (cos(az - ear), sin(az - ear), 0), float64 from the float32 fields;
  per ear   cs = clip((e . p) / d, -1, 1), th = arccos(cs), g = cs >= 0 ? -cs : th - pi / 2, tau = (a g + d) rate / c,
            h = shadow (0.95 cos(1.2 th) + 0.05); k0, f, the taps and the keep rule are ir_room_np's;
  sums      accP takes rint(a_c w 2^40) and accS rint((a_c h_c) w 2^40), a_c the room's b / d, times the band's air factor, times
            the source's factor with microphones;
  shelf     K = tan(c / (a rate)), b0 = 1 / (1 + K), b1 = -b0, a1 = -(1 - K) / (1 + K); S = accS 2^-40 through y = b0 v + s,
            s' = b1 v - a1 y from rest over all F frames (ir_eq_np.biquad with b2 = a2 = 0: the plain sequential loop);
  term      r = S + accP 2^-40; with bands r = HP(join of the accS_j) + join of the accP_j (ir_room_bands_np.join);
  a frame   ir_synth_np.frames64 + r; frames() rounds it to float32 once.
A dot product and a + b c are written without the definition's fused roundings: numpy has no fma, and the difference is an ulp
or two of a double (the GPU tests' bar allows for it).
"""
import math

import numpy as np

import ir_eq_np
import ir_room_bands_np
import ir_room_mics_np
import ir_room_np
import ir_synth_np
from ir_room_np import K, Q

DEFAULTS = dict(radius=0.0875, facing=0.0, ear=90.0, shadow=1.0)


def _f(v):
    return float(np.float32(v))


def spec(**kw):
    """The fields of an IrRoomHead with the library's defaults."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def centred(room):
    """The room as the head sees it: both receivers at the centre."""
    return ir_room_np.spec(**dict(room, spacing=0.0))


def ear_axes(head):
    """[2, 3]: e_L, e_R."""
    h = spec(**head)
    az, ear = _f(h["facing"]) * np.pi / 180, _f(h["ear"]) * np.pi / 180
    return np.array([[np.cos(az + ear), np.sin(az + ear), 0.0], [np.cos(az - ear), np.sin(az - ear), 0.0]])


def complete(room, head, rate, N):
    L, _, _, _, c, _ = ir_room_np.geometry(room)
    return int(math.floor((2.0 * float(N) * float(L.min()) - _f(spec(**head)["radius"])) * float(rate) / c))


def order(room, head, rate, F):
    """N: the order given, or with 0 the smallest whose lattice is complete up to E for this head."""
    room = ir_room_np.spec(**room)
    if room["order"]:
        return int(room["order"])
    N, E = max(1, ir_room_np.order(room, rate, F)), ir_room_np.last(room, F)
    while complete(room, head, rate, N) < E:
        N += 1
    return N


def ears(pos, d, head):
    """(th [M, 2], g [M, 2], h [M, 2]) of arrivals from pos [M, 3] (from the centre), d = |pos|."""
    hd = spec(**head)
    e = ear_axes(hd)
    dot = pos[:, None, 2] * e[None, :, 2] + (pos[:, None, 1] * e[None, :, 1] + pos[:, None, 0] * e[None, :, 0])
    cs = np.minimum(1.0, np.maximum(-1.0, dot / d[:, None]))
    th = np.arccos(cs)
    g = np.where(cs >= 0.0, -cs, th - np.pi / 2)
    return th, g, _f(hd["shadow"]) * (0.95 * np.cos(1.2 * th) + 0.05)


def images(room, head, rate, F, N=None):
    """ir_room_np.images of the centred room with the head's delays: tau [M, 2] per ear, and th, h [M, 2]."""
    room = centred(room)
    if N is None:
        N = order(room, head, rate, F)
    im = ir_room_np.images(room, rate, F, N)
    L, s, r, _, c, _ = ir_room_np.geometry(room)
    q = (1 - 2 * im["u"]).astype(np.float64) * s + (2 * im["n"]).astype(np.float64) * L
    pos = q - r[0][None, :]
    d = im["d"][:, 0]
    th, g, h = ears(pos, d, head)
    a = _f(spec(**head)["radius"])
    return dict(im, tau=(a * g + d[:, None]) * float(rate) / c, th=th, h=h)


def render_band(room, mics, head, beta, air, rate, F, N=None):
    """One band's two accumulators: (accP int64 [F, 2], accS int64 [F, 2], covered, info); info is ir_room_np's with `tau`, `h`
    of every image and `negative`, the share of kept ears whose shadow factor is below 0."""
    room = centred(room)
    if beta is not None:
        room = ir_room_np.spec(**dict(room, beta=tuple(beta)))
    F = int(F)
    im = images(room, head, rate, F, N)
    amp = im["a"]
    if _f(air) != 0.0:
        amp = amp * np.exp2(-(im["d"] * ir_room_bands_np.air_constant(air)))
    if mics is not None:
        gs, gr = ir_room_mics_np.factors(room, mics, im)
        assert (gr == 1.0).all()  # (ears are not microphones)
        amp = amp * (gs * gr)
    E = ir_room_np.last(room, F)
    accP, accS = np.zeros((F, 2), np.int64), np.zeros((F, 2), np.int64)
    covered = np.zeros((F, 2), bool)
    k0 = np.floor(im["tau"])
    keep = k0 < E
    for ch in range(2):
        sel = keep[:, ch] & (amp[:, ch] != 0.0)
        a, tau, base = amp[sel, ch], im["tau"][sel, ch], k0[sel, ch].astype(np.int64)
        sh = a * im["h"][sel, ch]
        f = tau - np.floor(tau)
        s = np.sin(np.pi * f)
        x = K[None, :].astype(np.float64) - f[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(K[None, :] & 1, s[:, None], -s[:, None]) / (np.pi * x) * ((1.0 + np.cos(np.pi * x / 16.0)) / 2.0)
        whole = f == 0.0
        w[whole] = (K == 0).astype(np.float64)
        t = base[:, None] + K[None, :]
        ok = (t >= 0) & (t < F)
        np.add.at(accP[:, ch], t[ok], np.rint(a[:, None] * w * Q).astype(np.int64)[ok])
        np.add.at(accS[:, ch], t[ok], np.rint(sh[:, None] * w * Q).astype(np.int64)[ok])
        reach = ok & ~(whole[:, None] & (K[None, :] != 0))
        covered[np.unique(t[reach]), ch] = True
    first = (np.abs(im["n"]).sum(axis=1) == 0) & (im["u"].sum(axis=1) == 0)
    direct = im["tau"][first][0]
    info = dict(order=im["order"], images=(int(keep[:, 0].sum()), int(keep[:, 1].sum())), direct=(float(direct[0]), float(direct[1])), last=E,
                complete=complete(room, head, rate, im["order"]), tau=im["tau"], h=im["h"], negative=float((im["h"][keep] < 0).mean()) if keep.any() else 0.0)
    return accP, accS, covered, info


def shelf_coefs(room, head, rate):
    """(K, (b0, b1, 0, a1, 0)) of the shelf's fixed high-pass."""
    _, _, _, _, c, _ = ir_room_np.geometry(room)
    Kc = math.tan(c / (_f(spec(**head)["radius"]) * float(rate)))
    b0 = 1.0 / (1.0 + Kc)
    return Kc, (b0, -b0, 0.0, -(1.0 - Kc) / (1.0 + Kc), 0.0)


def highpass(v, room, head, rate):
    """HP over the float64 frames v [F, 2], from rest, one frame after the other."""
    return ir_eq_np.biquad(np.asarray(v, np.float64), shelf_coefs(room, head, rate)[1])


def hp_response(room, head, rate, hz):
    """HP(e^jw) at hz (complex)."""
    b0, b1, _, a1, _ = shelf_coefs(room, head, rate)[1]
    z = np.exp(-2j * np.pi * np.asarray(hz, np.float64) / float(rate))
    return (b0 + b1 * z) / (1.0 + a1 * z)


def term(room, mics, bands, head, rate, F, N=None):
    """(r float64 [F, 2], covered, info): the room's term of a headed room, `bands` None or ir_room_bands_np's fields."""
    if bands is None:
        accP, accS, covered, info = render_band(room, mics, head, None, 0.0, rate, F, N)
        return highpass(accS.astype(np.float64) * (1.0 / Q), room, head, rate) + accP.astype(np.float64) * (1.0 / Q), covered, info
    b = ir_room_bands_np.spec(**bands)
    out = [render_band(room, mics, head, b["beta"][j], b["air"][j], rate, F, N) for j in range(len(b["xovers"]) + 1)]
    covered = np.zeros_like(out[0][2])
    for o in out:
        covered |= o[2]
    rP = ir_room_bands_np.join([o[0] for o in out], b["xovers"], rate)
    rS = ir_room_bands_np.join([o[1] for o in out], b["xovers"], rate)
    return highpass(rS, room, head, rate) + rP, covered, out[0][3]


def frames64(room, mics, bands, head, rate, N=None, **synth):
    """The F frames before the rounding to float32: ir_synth_np's three terms, then r.  (float64 [F, 2], covered, info)"""
    base = ir_synth_np.frames64(**synth)
    r, covered, info = term(room, mics, bands, head, rate, len(base), N)
    return base + r, covered, info


def frames(room, mics, bands, head, rate, N=None, **synth):
    out, covered, info = frames64(room, mics, bands, head, rate, N, **synth)
    return out.astype(np.float32), covered, info


def plan(room, head, rate, F):
    """What mc_ir_room_head_plan reports."""
    room = centred(room)
    N = order(room, head, rate, F)
    L, s, r, _, c, _ = ir_room_np.geometry(room)
    pos = (s - r[0])[None, :]
    d = np.sqrt((pos * pos).sum(axis=1))
    th, g, h = ears(pos, d, head)
    a = _f(spec(**head)["radius"])
    tau = (a * g[0] + d[0]) * float(rate) / c
    return dict(order=N, complete=complete(room, head, rate, N), direct=(float(tau[0]), float(tau[1])), itd=float(tau[1] - tau[0]) / float(rate),
                angle=(float(np.degrees(th[0, 0])), float(np.degrees(th[0, 1]))), shadow=(float(h[0, 0]), float(h[0, 1])), corner=c / (math.pi * a),
                k=shelf_coefs(room, head, rate)[0])
