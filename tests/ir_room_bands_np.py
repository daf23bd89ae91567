"""Float64 restatement of walls and air per frequency band in the room of mc_synth_ir_room_bands
(cuda_audio_amd/csrc/irroom.hip.h), on top of tests/ir_room_np.py, tests/ir_room_mics_np.py and tests/ir_damp_np.py.

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is once more, sequential:
  bands     X crossovers cut B = X + 1 bands; crossover k is ir_damp_np's: two identical high-cut sections from rest at frame 0;
  rendering band j is the room with beta[j] for its walls and a_c = ((b / d_c) air_c) (gs_c gr_c), air_c = exp2(-(d_c k_j)),
            k_j = float32(air[j]) log2(10) / 20; where air[j] == 0 no factor is applied; everything else is ir_room_np's, each
            band into its own int64 accumulator acc_j;
  join      D_k = (acc_(k-1) - acc_k) 2^-40, the difference in int64; P_k = ir_damp_np.lowpasses(D_k) over all F frames;
            r = (P_1 + .. + P_X) + acc_X 2^-40, added low to high with the accumulator's term last;
  a frame   ir_synth_np.frames64 + r; frames() rounds it to float32 once.
`by_bands` is the algebraically equal other form, sum_j B_j(acc_j 2^-40) over ir_damp_np.bands, for the test that compares them.
"""
import math

import numpy as np

import ir_damp_np
import ir_room_mics_np
import ir_room_np
import ir_synth_np
from ir_room_np import K, Q

DEFAULTS = dict(xovers=(), beta=0.9, air=0.0)


def _f(v):
    return float(np.float32(v))


def spec(**kw):
    """The fields of an IrRoomBands with the library's defaults: beta as B rows of six numbers, air as B numbers."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    b = dict(DEFAULTS, **kw)
    b["xovers"] = tuple(b["xovers"])
    B = len(b["xovers"]) + 1
    beta = tuple(b["beta"]) if isinstance(b["beta"], (tuple, list)) else (b["beta"],) * B
    assert len(beta) == B, (beta, B)
    b["beta"] = tuple(tuple(r) if isinstance(r, (tuple, list)) else (r,) * 6 for r in beta)
    air = tuple(b["air"]) if isinstance(b["air"], (tuple, list)) else (b["air"],) * B
    assert len(air) == B and all(len(r) == 6 for r in b["beta"])
    b["air"] = air
    return b


def air_constant(db_per_m):
    """k_j of the definition."""
    return _f(db_per_m) * np.log2(10.0) / 20.0


def render_band(room, mics, beta, air, rate, F, N=None):
    """ir_room_np.render (mics None) or ir_room_mics_np.render with the band's walls and its air factor, applied to b / d before
    the microphones' factor: (acc int64 [F, 2], covered, info)."""
    room = ir_room_np.spec(**dict(room, beta=tuple(beta)))
    F = int(F)
    im = ir_room_np.images(room, rate, F, N)
    amp = im["a"]
    if _f(air) != 0.0:
        amp = amp * np.exp2(-(im["d"] * air_constant(air)))
    if mics is not None:
        gs, gr = ir_room_mics_np.factors(room, mics, im)
        amp = amp * (gs * gr)
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
    direct = im["tau"][(np.abs(im["n"]).sum(axis=1) == 0) & (im["u"].sum(axis=1) == 0)][0]
    info = dict(order=im["order"], images=(int(keep[:, 0].sum()), int(keep[:, 1].sum())), direct=(float(direct[0]), float(direct[1])), last=E,
                complete=ir_room_np.complete(room, rate, im["order"]), tau=im["tau"])
    return acc, covered, info


def accumulators(room, mics, bands, rate, F, N=None):
    """([acc_0 .. acc_X] int64 [F, 2], covered of any band, info of band 0: the counts are a matter of geometry)."""
    b = spec(**bands)
    out = [render_band(room, mics, b["beta"][j], b["air"][j], rate, F, N) for j in range(len(b["xovers"]) + 1)]
    covered = np.zeros_like(out[0][1])
    for _, c, _ in out:
        covered |= c
    return [a for a, _, _ in out], covered, out[0][2]


def join(accs, xovers, rate):
    """r [F, 2] of the definition from the band accumulators: the difference form."""
    X = len(xovers)
    assert len(accs) == X + 1
    top = accs[X].astype(np.float64) * (1.0 / Q)
    if not X:
        return top
    total = None
    for k in range(1, X + 1):
        D = (accs[k - 1] - accs[k]).astype(np.float64) * (1.0 / Q)  # (the difference in int64, converted once)
        P = ir_damp_np.lowpasses(D, (xovers[k - 1],), rate)[0]
        total = P if total is None else total + P
    return total + top


def by_bands(accs, xovers, rate):
    """sum_j B_j(acc_j 2^-40) over ir_damp_np.bands: what `join` equals algebraically."""
    total = np.zeros(accs[0].shape, np.float64)
    for j, acc in enumerate(accs):
        x = acc.astype(np.float64) * (1.0 / Q)
        if not xovers:
            return x
        total = total + ir_damp_np.bands(x, ir_damp_np.lowpasses(x, xovers, rate))[j]
    return total


def frames64(room, mics, bands, rate, N=None, **synth):
    """The F frames before the rounding to float32: ir_synth_np's three terms, then r.  (float64 [F, 2], covered, info)"""
    base = ir_synth_np.frames64(**synth)
    accs, covered, info = accumulators(room, mics, bands, rate, len(base), N)
    return base + join(accs, spec(**bands)["xovers"], rate), covered, info


def frames(room, mics, bands, rate, N=None, **synth):
    out, covered, info = frames64(room, mics, bands, rate, N, **synth)
    return out.astype(np.float32), covered, info


def plan(room, bands, rate, F):
    """What mc_ir_room_bands_plan reports."""
    b = spec(**bands)
    L, _, _, _, c, _ = ir_room_np.geometry(room)
    V = float(L[0] * L[1] * L[2])
    area = np.array([L[1] * L[2], L[1] * L[2], L[0] * L[2], L[0] * L[2], L[0] * L[1], L[0] * L[1]])
    S = float(area.sum())
    k = 24.0 * math.log(10.0) / c
    sabine, eyring = [], []
    for row, air in zip(b["beta"], b["air"]):
        beta = np.array([_f(v) for v in row])
        A = float((area * (1.0 - beta * beta)).sum())
        m = _f(air) * math.log(10.0) / 10.0
        with np.errstate(divide="ignore"):
            ey = -S * float(np.log1p(-A / S)) + 4.0 * m * V
        sa = A + 4.0 * m * V
        sabine.append(k * V / sa if sa > 0 else 0.0)
        eyring.append(k * V / ey if ey > 0 else 0.0)
    return dict(bands=len(b["beta"]), xovers=tuple(_f(x) for x in b["xovers"]), sabine=tuple(sabine), eyring=tuple(eyring))
