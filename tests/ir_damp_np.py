"""Float64 restatement of the damping of an IR on load (mc_load_ir_damped, cuda_audio_amd/csrc/irdamp.hip.h).

Test infrastructure only: the product never imports it.  Steps 1 to 6 are ir_shape_np.shape64's (with the normalisation off,
so that its taps are those before the gain); then, with x those n taps, X crossovers and rate the session's,
  6a. P_k = x through two identical sections in cascade (ir_eq_np.biquad twice, a plain sequential loop each), each the
      cookbook high cut at xover k with q = float32(0.70710678), from rest at tap 0;
      o = min(origin, n), t(m) = max(m, o) - o, g_j[m] = exp2(-(t(m) 3 log2(10)) / decay[j]) or 1 where decay[j] = 0;
      y = g_X x + (g_0 - g_1) P_1 + .. + (g_(X-1) - g_X) P_X, added in that order;
  6b. ir_eq_np.cascade over y;
  7.  peak, energy and gain of the result; 8. stored tap = float32(value * gain).
`bands` gives the B_j the output is the weighted sum of, `response_db` the quasi-static response, which no recurrence enters.
"""
import functools

import numpy as np

import ir_decay_np
import ir_eq_np
from ir_shape_np import DECAY_K, shape64

# the aiming case: three octave bands read before and after damping the upper two
AIM = dict(rate=8000, xovers=(400, 1600), decay=(0, 4800, 1600), origin=37, bands=(125, 800, 3200))


def xover_coefs(hz, rate):
    """One section of a crossover: the high cut at hz, q = float32(0.70710678)."""
    return ir_eq_np.coefs(("highcut", hz, 0.0, ir_eq_np.DEFAULT_Q), rate)


def lowpasses(x, xovers, rate):
    """[P_1 .. P_X] of the float64 taps x [n, 2]."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for hz in xovers:
        c = xover_coefs(hz, rate)
        out.append(ir_eq_np.biquad(ir_eq_np.biquad(x, c), c))
    return out


def bands(x, P):
    """[B_0 .. B_X]: B_0 = P_1, B_j = P_(j+1) - P_j, B_X = x - P_X."""
    return [P[0]] + [P[k + 1] - P[k] for k in range(len(P) - 1)] + [x - P[-1]]


def envelopes(n, decay, origin):
    """g [X + 1, n]."""
    o = min(int(origin), n)
    t = np.maximum(np.arange(n, dtype=np.float64), o) - o
    return np.stack([np.exp2(-(t * DECAY_K) / float(d)) if d else np.ones(n) for d in decay])


def combine(x, P, decay, origin):
    """y of step 6a from x and its low-passes."""
    assert len(decay) == len(P) + 1
    g = envelopes(x.shape[0], decay, origin)
    y = g[-1][:, None] * x
    for k in range(1, len(P) + 1):
        y = y + (g[k - 1] - g[k])[:, None] * P[k - 1]
    return y


def damp(x, xovers, decay, origin, rate):
    """Step 6a over the float64 taps x [n, 2]."""
    x = np.asarray(x, dtype=np.float64)
    if not xovers:
        return x
    return combine(x, lowpasses(x, xovers, rate), decay, origin)


def damp_info(n, xovers, decay, origin):
    return dict(xovers=len(xovers), origin=min(int(origin), n), damped_bands=sum(1 for d in decay if d))


def damp64(x, cap, src, dst, xovers, decay, origin=0, bands=(), *, normalize=None, target=1.0, eq_first=False, **fields):
    """x: [frames, 2] at src Hz in a session at dst Hz; returns (float64 taps [n, 2] before the rounding of step 8, shape info,
    damp info) as Convolution.ir_shape_info and ir_damp_info give them after such a load.  eq_first swaps 6a and 6b: the
    wrong order, for the test that tells them apart."""
    v, info = shape64(x, cap, src, dst, normalize=None, **fields)
    if eq_first:
        v = damp(ir_eq_np.cascade(v, bands, dst), xovers, decay, origin, dst)
    else:
        v = ir_eq_np.cascade(damp(v, xovers, decay, origin, dst), bands, dst)
    peak = float(np.abs(v).max())
    energy = float(np.sqrt((v * v).sum() / 2.0))
    measure = {None: 0.0, "peak": peak, "energy": energy}[normalize]
    gain = float(np.float32(target)) / measure if measure > 0.0 else 1.0
    info = dict(info, gain=gain, peak=peak, energy=energy, eq_bands=len(ir_eq_np.on_bands(bands)))
    return v * gain, info, damp_info(v.shape[0], xovers, decay, origin)


def damped(x, cap, src, dst, xovers, decay, origin=0, bands=(), **fields):
    """damp64 with the taps as the engine stores them: float32 [n, 2]."""
    v, info, dinfo = damp64(x, cap, src, dst, xovers, decay, origin, bands, **fields)
    return v.astype(np.float32), info, dinfo


def section_response(hz_x, rate, hz):
    """One section's complex H(e^{j 2 pi hz / rate})."""
    return ir_eq_np.response((("highcut", hz_x, 0.0, ir_eq_np.DEFAULT_Q),), rate, hz)


def response(xovers, decay, origin, rate, tap, hz):
    """g_X + sum_k (g_(k-1) - g_k) H_k^2 at stored tap `tap`, o taken as `origin`: complex."""
    t = max(int(tap), int(origin)) - int(origin)
    g = [float(np.exp2(-(t * DECAY_K) / float(d))) if d else 1.0 for d in decay]
    out = np.full(np.shape(hz), g[len(xovers)], dtype=np.complex128)
    for k, hz_x in enumerate(xovers, start=1):
        out = out + (g[k - 1] - g[k]) * section_response(hz_x, rate, hz) ** 2
    return out


def response_db(xovers, decay, origin, rate, tap, hz):
    return 20.0 * np.log10(np.abs(response(xovers, decay, origin, rate, tap, hz)))


@functools.lru_cache(maxsize=None)
def aim_case():
    """(the IR, its damped taps as float32, ir_decay_np.decay of the IR, of the damped taps) for AIM, computed once."""
    ir = ir_decay_np.noise_ir(n=12000, lead=37, rate=AIM["rate"], t60=0.6, seed=7)
    y = damp(ir.astype(np.float64), AIM["xovers"], AIM["decay"], AIM["origin"], AIM["rate"]).astype(np.float32)
    before = ir_decay_np.decay(ir, AIM["rate"], bands=AIM["bands"])
    after = ir_decay_np.decay(y, AIM["rate"], bands=AIM["bands"])
    for a in (ir, y):
        a.setflags(write=False)
    return ir, y, before, after
