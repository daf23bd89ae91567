"""Float64 restatement of the synthesis of an IR from a seed (mc_synth_ir, cuda_audio_amd/csrc/irsynth.hip.h).

Test infrastructure only: the product never imports it.  include/mcconv.h has the definition; here it is once more, frame by
frame over numpy arrays:
  W(i, s)   Philox4x32-10 in uint64 arithmetic masked to 32 bits, counter {i, 0, s, 0}, key {seed lo, seed hi};
  u(w)      (w + 0.5) / 2^32;
  late      m >= late_start, t = m - late_start: gA, gB by Box-Muller from W(m, 0), L = gA, R = rho gA + sqrt(1 - rho^2) gB with
            rho = 1 - float32(width); envelope float32(late_gain) * exp2(-(t 3 log2(10)) / t60); occupancy from W(m, 1) in
            integers, scale 1 / sqrt(p);
  direct    float32(direct) on frame 0;
  early     table() from W(j, 2), added in ascending j;
  a frame   late + direct + reflections in float64; frames() rounds it to float32 once.
"""
import numpy as np

from ir_shape_np import DECAY_K

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

DEFAULTS = dict(frames=0, seed=0, late_start=0, t60=0, build_up=0, late_gain=1.0, direct=0.0, n_early=0, early_first=0, early_last=0,
                early_gain=1.0, width=1.0)


def philox(counter, key):
    """Philox4x32-10: counter = four arrays (or ints) of 32-bit words, key = two; returns four uint64 arrays holding 32-bit words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 bits: inside 64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def words(seed, i, s):
    """W(i, s) for an array of i."""
    seed = int(seed)
    return philox((i, 0, s, 0), (seed & 0xFFFFFFFF, seed >> 32))


def u(w):
    return (w.astype(np.float64) + 0.5) / 4294967296.0


def spec(**kw):
    """The fields of an IrSynth with the library's defaults."""
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def table(p):
    """The reflections kept: [(pos, gL, gR)] in ascending j."""
    p = spec(**p)
    out = []
    if not p["n_early"]:
        return out
    first, span = int(p["early_first"]), int(p["early_last"]) - int(p["early_first"]) + 1
    w = words(p["seed"], np.arange(p["n_early"]), 2)
    eg, width = float(np.float32(p["early_gain"])), float(np.float32(p["width"]))
    for j in range(p["n_early"]):
        pos = first + ((int(w[0][j]) * span) >> 32)
        if pos >= p["frames"]:
            continue
        g = eg * (-1.0 if int(w[1][j]) & 1 else 1.0) * float(first + 1) / float(pos + 1)
        pan = width * (2.0 * float(u(w[2][j:j + 1])[0]) - 1.0)
        out.append((pos, g * (1.0 - pan if pan >= 0.0 else 1.0), g * (1.0 + pan if pan <= 0.0 else 1.0)))
    return out


def occupancy(p):
    """(occupied [n] bool, p [n] float64) of the late frames t = 0 .. F - late_start - 1."""
    p = spec(**p)
    F, ls, B = int(p["frames"]), int(p["late_start"]), int(p["build_up"])
    n = max(F - ls, 0)
    occ, prob = np.ones(n, dtype=bool), np.ones(n)
    k = min(n, max(B - 1, 0))  # frames with t + 1 < B
    if k:
        a = np.arange(1, k + 1, dtype=np.uint64)
        w = words(p["seed"], np.arange(ls, ls + k), 1)[0]
        occ[:k] = (w < np.uint64(1 << 28)) | (w * np.uint64(B * B) < ((a * a) << S32))
        r = a.astype(np.float64) / float(B)
        prob[:k] = np.maximum(1.0 / 16.0, r * r)
    return occ, prob


def late64(p):
    """The late field alone: float64 [F, 2], zero before late_start."""
    p = spec(**p)
    F, ls = int(p["frames"]), int(p["late_start"])
    out = np.zeros((F, 2))
    if ls >= F:
        return out
    m = np.arange(ls, F)
    t = (m - ls).astype(np.float64)
    w = words(p["seed"], m, 0)
    gA = np.sqrt(-2.0 * np.log(u(w[0]))) * np.cos(2.0 * np.pi * u(w[1]))
    gB = np.sqrt(-2.0 * np.log(u(w[2]))) * np.cos(2.0 * np.pi * u(w[3]))
    rho = 1.0 - float(np.float32(p["width"]))
    env = float(np.float32(p["late_gain"])) * (np.exp2(-(t * DECAY_K) / float(p["t60"])) if p["t60"] else np.ones(len(t)))
    occ, prob = occupancy(p)
    scale = np.where(occ, 1.0 / np.sqrt(prob), 0.0)
    out[ls:, 0] = np.where(occ, gA * env * scale, 0.0)
    out[ls:, 1] = np.where(occ, (rho * gA + np.sqrt(1.0 - rho * rho) * gB) * env * scale, 0.0)
    return out


def frames64(**p):
    """The F frames before the rounding to float32: float64 [F, 2]."""
    p = spec(**p)
    out = late64(p)
    out[0] += float(np.float32(p["direct"]))
    for pos, gL, gR in table(p):
        out[pos, 0] += gL
        out[pos, 1] += gR
    return out


def frames(**p):
    """The F frames as the device generates them: float32 [F, 2]."""
    return frames64(**p).astype(np.float32)
