"""Float64 restatement of directional microphones and a directional source in the room of mc_synth_ir_room_mics
(cuda_audio_amd/csrc/irroom.hip.h), on top of tests/ir_room_np.py.

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is once more:
  aims      the unit vector of (az, el) in degrees is (cos el cos az, cos el sin az, sin el), float64 from the float32 fields;
  receiver  cr = (m_c . p) / d, gr = alpha_c + (1 - alpha_c) cr, p the image as its receiver sees it;
  source    the image (n, u) aims along v'_a = (1 - 2 u_a) v_a; cs = -(v' . p) / d, gs = alpha_s + (1 - alpha_s) cs;
  amplitude a_c = (b / d_c) (gs_c gr_c); everything else is ir_room_np's.
A dot product is written z z' + (y y' + x x'), the definition's order, without its fused roundings: numpy has no fma, and the
difference is an ulp or two of a double (the GPU tests' bar allows for it).  With alpha = 1 a factor is exactly 1 here as well:
(1 - alpha) cos is then exactly 0.
"""
import numpy as np

import ir_room_np
import ir_synth_np
from ir_room_np import K, Q

PATTERNS = {"omni": 1.0, "subcardioid": 0.75, "cardioid": 0.5, "supercardioid": 0.366, "hypercardioid": 0.25, "fig8": 0.0}
DEFAULTS = dict(pattern=1.0, az=0.0, el=0.0, source_pattern=1.0, source_az=0.0, source_el=0.0)


def _f(v):
    return float(np.float32(v))


def spec(**kw):
    """The fields of an IrRoomMics with the library's defaults: pattern, az and el as pairs (left, right), patterns as numbers."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    m = dict(DEFAULTS, **kw)
    for k in ("pattern", "az", "el"):
        m[k] = tuple(m[k]) if isinstance(m[k], (tuple, list)) else (m[k], m[k])
    m["pattern"] = tuple(PATTERNS.get(v, v) for v in m["pattern"])
    m["source_pattern"] = PATTERNS.get(m["source_pattern"], m["source_pattern"])
    return m


def aim(az, el):
    a, e = _f(az) * np.pi / 180, _f(el) * np.pi / 180
    return np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])


def _dot(a, p):
    return p[..., 2] * a[..., 2] + (p[..., 1] * a[..., 1] + p[..., 0] * a[..., 0])


def factors(room, mics, im):
    """(gs [M, 2], gr [M, 2]) of every image of ir_room_np.images(room, ...)."""
    m = spec(**mics)
    L, s, r, _, _, _ = ir_room_np.geometry(room)
    q = (1 - 2 * im["u"]).astype(np.float64) * s + (2 * im["n"]).astype(np.float64) * L
    pos = q[:, None, :] - r[None, :, :]  # [M, 2, 3]
    d = im["d"]
    v = (1 - 2 * im["u"]).astype(np.float64) * aim(m["source_az"], m["source_el"])  # [M, 3]
    alpha_s = _f(m["source_pattern"])
    gs = alpha_s + (1.0 - alpha_s) * (-_dot(v[:, None, :], pos) / d)
    gr = np.empty_like(gs)
    for c in range(2):
        alpha = _f(m["pattern"][c])
        gr[:, c] = alpha + (1.0 - alpha) * (_dot(aim(m["az"][c], m["el"][c])[None, :], pos[:, c, :]) / d[:, c])
    return gs, gr


def render(room, mics, rate, F, N=None):
    """ir_room_np.render with the microphones: (acc int64 [F, 2], covered, info); info is ir_room_np's with `mics`, what
    mc_ir_room_mics_plan reports of the direct sound, and `negative`, the share of kept images whose factor is below 0."""
    room = ir_room_np.spec(**room)
    F = int(F)
    im = ir_room_np.images(room, rate, F, N)
    gs, gr = factors(room, mics, im)
    amp = im["a"] * (gs * gr)
    E = ir_room_np.last(room, F)
    acc = np.zeros((F, 2), np.int64)
    covered = np.zeros((F, 2), bool)
    k0 = np.floor(im["tau"])
    keep = k0 < E
    for ch in range(2):
        sel = keep[:, ch] & (amp[:, ch] != 0.0)
        a, tau, base = amp[sel, ch], im["tau"][sel, ch], k0[sel, ch].astype(np.int64)
        f = tau - np.floor(tau)
        s = np.sin(np.pi * f)
        x = K[None, :].astype(np.float64) - f[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(K[None, :] & 1, s[:, None], -s[:, None]) / (np.pi * x) * ((1.0 + np.cos(np.pi * x / 16.0)) / 2.0)
        whole = f == 0.0
        w[whole] = (K == 0).astype(np.float64)
        qv = np.rint(a[:, None] * w * Q).astype(np.int64)
        t = base[:, None] + K[None, :]
        ok = (t >= 0) & (t < F)
        np.add.at(acc[:, ch], t[ok], qv[ok])
        reach = ok & ~(whole[:, None] & (K[None, :] != 0))
        covered[np.unique(t[reach]), ch] = True
    first = (np.abs(im["n"]).sum(axis=1) == 0) & (im["u"].sum(axis=1) == 0)
    direct = im["tau"][first][0]
    g0, r0 = gs[first][0], gr[first][0]
    info = dict(order=im["order"], images=(int(keep[:, 0].sum()), int(keep[:, 1].sum())), direct=(float(direct[0]), float(direct[1])), last=E,
                complete=ir_room_np.complete(room, rate, im["order"]),
                mics=dict(source=(float(g0[0]), float(g0[1])), receiver=(float(r0[0]), float(r0[1])), factor=(float(g0[0] * r0[0]), float(g0[1] * r0[1]))),
                negative=float(((gs * gr)[keep] < 0).mean()))
    return acc, covered, info


def frames64(room, mics, rate, N=None, **synth):
    """The F frames before the rounding to float32: ir_synth_np's three terms, then the room's.  (float64 [F, 2], covered, info)"""
    base = ir_synth_np.frames64(**synth)
    acc, covered, info = render(room, mics, rate, len(base), N)
    return base + acc.astype(np.float64) * (1.0 / Q), covered, info


def plan(room, mics, rate, F):
    """What mc_ir_room_mics_plan reports: the direct sound's factors."""
    room = ir_room_np.spec(**room)
    im = ir_room_np.images(room, rate, F, N=0)  # (the direct sound and its seven first mirrors in the walls at 0)
    gs, gr = factors(room, mics, im)
    first = im["u"].sum(axis=1) == 0
    g0, r0 = gs[first][0], gr[first][0]
    return dict(source=(float(g0[0]), float(g0[1])), receiver=(float(r0[0]), float(r0[1])), factor=(float(g0[0] * r0[0]), float(g0[1] * r0[1])))
