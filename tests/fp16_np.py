"""fp16 storage (mc_config.precision = 1) restated in numpy: float64 arithmetic that rounds exactly where the engine rounds.

The engine keeps, next to the fp32 spectra of every IR (d_H, mc_debug_read item 0) and the fp32 delay line (d_fdl, item 1),
  - d_H16 (item 18): each fp32 entry times the IR's power-of-two scale16 (item 20), rounded to the nearest half, ties to even
    (pack_half4 = __floats2half2_rn, csrc/kernels.hip.h; written by k_to_half from load_ir and consolidate_voices, csrc/mcconv.hip);
  - d_fdl16 (item 19): each delay-line entry times FDL16_SCALE = 16, rounded the same way, by whoever writes the fp32 slot
    (k_fwd, and the three JACK tails of csrc/jack_tail.hip.h).
k_mac_stream<.., HALF = true> (mac_stream_body, csrc/kernels.hip.h) reads both, converts the halves to float (exact, subnormal
halves included), multiplies the slot's four gains by inv = {1 / (scale16 of IR 0 x 16), 1 / (scale16 of IR 1 x 16)} in float -
powers of two - and sums the products in fp32.  What this module restates is that sum with every product and sum in float64: fed the
engine's own fp32 buffers, what remains between it and the engine is fp32 arithmetic.

Layouts (as the engine stores them): an entry is four numbers {a.re, a.im, b.re, b.im}; for an IR a = left, b = right channel of
the partition's 512-point spectrum, [256 bins][pstride partitions][4]; for the delay line a = input 1, b = input 2 of the block's
spectrum, [256 bins][ring slots][4].  Bin 0 packs {DC, Nyquist} into {re, im}: both real, multiplied component by component.
Block t of the stream sits in slot t & (ring - 1).  Gains are {L <- in1, L <- in2, R <- in1, R <- in2} per slot (item 21).

Which partitions the engine reads from the fp16 copies: [lo16, hi), hi = the voice's partitions rounded up to 16.  Below lo16 it
reads the fp32 buffers.  lo16 by path, as read in the code:
  - batches (mc_process with several blocks; launch_mac_batch's streaming branch -> launch_mac_stream(e, a, pb, pe, ...), pb = 0
    without partition shards): lo16 = 0.  An fp16 engine's batches never take the resident kernel (mo->resident needs !e->half).
  - 256-frame periods (process_one, make_plan: `first = pb == 0 ? 2 : pb`): lo16 = 2.  k_tail1 sums partition 0 (the new block)
    and partition 1 (the block before it, `xprev = fdl[...]`, the fp32 delay line) against vset.H0 / H1 = d_H.  Partition 0 takes
    one of two forms, which mc_debug_read item 16 counts: in the frequency domain, the new block's spectrum times H[0] like any
    other partition; or, for a tail that was parked and had to wait for its period, in the time domain, the new frames against
    the IR's first 256 fp32 taps.  Neither reads a half, and in exact arithmetic both are the same 256-tap convolution: one
    restatement serves both.  (An fp16 engine never parks a period - process_one asks for !e->half - so it takes the second
    form only under MCCONV_TAIL_FORM=td, which is how the tests reach it.)
  - 512- and 1024-frame periods (process_period_fused, launch_mac: launch_mac_stream(e, av, pm, pl.hi[a], pm, ...), pm = 2 or
    4 blocks): lo16 = pm.
    k_tailp sums partitions 0 .. pm - 1 of each of the period's blocks itself, the period's own blocks from registers and the
    older ones from the fp32 delay line (`xold[q] = fdl[...]`).
"""
import numpy as np

FDL16_SCALE = 16.0
SCALE16_MAX_EXP = 122  # load_ir and consolidate_voices hold the exponent of scale16 to this: scale16 x 16 and its reciprocal stay normal floats
LO16 = {"batch": 0, 256: 2, 512: 2, 1024: 4}


def quantise(a32, scale):
    """What pack_half4 stores: (a32 * float32(scale)) in float32, rounded to the nearest half, ties to even, subnormal halves
    kept, overflow to infinity.  Returns the bits as uint16."""
    a = np.asarray(a32, dtype=np.float32) * np.float32(scale)
    with np.errstate(over="ignore"):
        return a.astype(np.float16).view(np.uint16)


def dequantise(bits):
    """What unpack_half4 returns: the halves as float32, exactly (still scaled)."""
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float32)


def scale_rule(H32):
    """scale16 as load_ir states it: 2^(13 - ex) with max |H| = m 2^ex, 0.5 <= m < 1 (frexp), ex = 0 for an all-zero IR; the
    exponent 13 - ex is held to SCALE16_MAX_EXP."""
    mx = float(np.max(np.abs(np.asarray(H32, dtype=np.float32)))) if np.size(H32) else 0.0
    ex = int(np.frexp(np.float32(mx))[1]) if mx > 0.0 else 0
    return float(np.ldexp(np.float32(1.0), min(13 - ex, SCALE16_MAX_EXP)))


def scale_rule_merged(coefs, scales):
    """scale16 of a merged entry M = sum_j c_j H_j (consolidate_voices): from the bound sum_j |c_j| 2^14 / scale16_j >= max |M|,
    summed in double, by the same rule and clamp."""
    bound = 0.0
    for c, s in zip(coefs, scales):
        bound += abs(float(np.float32(c))) * 16384.0 / float(s)
    ex = int(np.frexp(bound)[1]) if bound > 0.0 else 0
    return float(np.ldexp(np.float32(1.0), min(13 - ex, SCALE16_MAX_EXP)))


def _cplx(a):
    a = np.asarray(a, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1], a[..., 2] + 1j * a[..., 3]


def partition_sum(H0, H1, X, gains, slots, lo, hi, packed_bin0=True):
    """mac_stream_body in float64.  H0, H1 [256][pstride][4]: the IRs of input 1 and input 2; X [256][ring][4]: the delay
    line; gains [ring][4]: the slots' gains g; slots: slot0 + t of every block wanted; partitions [lo, hi).
    Per partition p, with x = X[slot], slot = (slot0 + t - p) & (ring - 1), and g = gains[slot]:
        a0 = H0.a x.a, a1 = H1.a x.b, a2 = H0.b x.a, a3 = H1.b x.b    (cmac; at bin 0, packed: re * re and im * im)
        Y.a += g.x a0 + g.y a1,   Y.b += g.z a2 + g.w a3
    Returns Y [len(slots)][256][4] float64."""
    ring = X.shape[1]
    assert ring & (ring - 1) == 0 and gains.shape == (ring, 4)
    slots = np.asarray(slots, dtype=np.int64)
    Y = np.zeros((len(slots), 256, 4))
    if hi <= lo:
        return Y
    h0a, h0b = _cplx(np.asarray(H0)[:, lo:hi])
    h1a, h1b = _cplx(np.asarray(H1)[:, lo:hi])
    p = np.arange(lo, hi, dtype=np.int64)
    g64 = np.asarray(gains, dtype=np.float64)
    for i, st in enumerate(slots):
        s = (st - p) & (ring - 1)
        xa, xb = _cplx(np.asarray(X)[:, s])
        g = g64[s]
        xa0, xa2 = xa * g[None, :, 0], xa * g[None, :, 2]
        xb1, xb3 = xb * g[None, :, 1], xb * g[None, :, 3]
        ya = np.einsum("kp,kp->k", h0a, xa0) + np.einsum("kp,kp->k", h1a, xb1)
        yb = np.einsum("kp,kp->k", h0b, xa2) + np.einsum("kp,kp->k", h1b, xb3)
        if packed_bin0:  # {DC, Nyquist}: two real products per path
            ya[0] = (np.sum(h0a[0].real * xa0[0].real + h1a[0].real * xb1[0].real)
                     + 1j * np.sum(h0a[0].imag * xa0[0].imag + h1a[0].imag * xb1[0].imag))
            yb[0] = (np.sum(h0b[0].real * xa2[0].real + h1b[0].real * xb3[0].real)
                     + 1j * np.sum(h0b[0].imag * xa2[0].imag + h1b[0].imag * xb3[0].imag))
        Y[i, :, 0], Y[i, :, 1], Y[i, :, 2], Y[i, :, 3] = ya.real, ya.imag, yb.real, yb.imag
    return Y


def inv_gains(gains, scale0, scale1, swap=False):
    """The gains as the HALF kernel uses them: g * {inv.x, inv.y, inv.x, inv.y} in float32, inv = 1 / (scale16 * 16) in float32
    (launch_mac_stream).  swap: inv.x and inv.y exchanged - a fault, for the sensitivity tests."""
    with np.errstate(divide="ignore", over="ignore"):
        ix = np.float32(1.0) / (np.float32(scale0) * np.float32(FDL16_SCALE))
        iy = np.float32(1.0) / (np.float32(scale1) * np.float32(FDL16_SCALE))
    if swap:
        ix, iy = iy, ix
    return np.asarray(gains, dtype=np.float32) * np.array([ix, iy, ix, iy], dtype=np.float32)


def partition_sum_q(H0, H1, X, H0q, H1q, Xq, scale0, scale1, gains, slots, lo16, hi, lo=0, swap_inv=False):
    """The sum as an fp16 engine forms it: partitions [lo, lo16) from the fp32 buffers H0, H1, X; partitions [lo16, hi) from the
    dequantised halves H0q, H1q (scaled by scale0, scale1) and Xq (scaled by 16) with the gains of inv_gains()."""
    Y = partition_sum(H0, H1, X, gains, slots, lo, min(lo16, hi))
    Y += partition_sum(H0q, H1q, Xq, inv_gains(gains, scale0, scale1, swap_inv), slots, max(lo16, lo), hi)
    return Y


def wet_blocks(Y):
    """Linear mode (compat = 0, no predelay): the packed 512-point inverse transform of every block's partition sums and the
    overlap-add of neighbouring segments.  Y [n + 1][256][4] for blocks t0 - 1 .. t0 + n - 1; returns the wet frames of blocks
    t0 .. t0 + n - 1, float64 [2][256 n]: block t = first half of segment t + second half of segment t - 1."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0] - 1
    out = np.zeros((2, n * 256))
    for c in range(2):
        S = np.zeros((n + 1, 257), dtype=np.complex128)
        S[:, 1:256] = Y[:, 1:, 2 * c] + 1j * Y[:, 1:, 2 * c + 1]
        S[:, 0] = Y[:, 0, 2 * c]
        S[:, 256] = Y[:, 0, 2 * c + 1]
        seg = np.fft.irfft(S, 512, axis=1)
        out[c] = (seg[1:, :256] + seg[:-1, 256:]).reshape(-1)
    return out


def spectra(frames2, nparts=None):
    """Entries {a.re, a.im, b.re, b.im} of the 512-point spectra of the zero-padded 256-frame pieces of frames2 [n][2] (the
    layout test_ir_spectra_match_numpy documents): float64 [256][pieces][4], bin 0 = {DC, Nyquist}."""
    f = np.asarray(frames2, dtype=np.float64)
    P = (len(f) + 255) // 256
    pad = np.zeros((max(P, nparts or 0) * 256, 2))
    pad[: len(f)] = f
    seg = np.zeros((pad.shape[0] // 256, 512, 2))
    seg[:, :256] = pad.reshape(-1, 256, 2)
    F = np.fft.rfft(seg, axis=1)  # [pieces][257][2]
    out = np.zeros((256, F.shape[0], 4))
    for c in range(2):
        out[1:, :, 2 * c] = F[:, 1:256, c].real.T
        out[1:, :, 2 * c + 1] = F[:, 1:256, c].imag.T
        out[0, :, 2 * c] = F[:, 0, c].real
        out[0, :, 2 * c + 1] = F[:, 256, c].real
    return out


def worst_block(got, want):
    """Largest RMS difference over the 256-frame blocks of [2][256 n], in units of want's RMS over the whole window."""
    d = (np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).reshape(2, -1, 256)
    per = np.sqrt(np.mean(d * d, axis=(0, 2)))
    return float(per.max() / np.sqrt(np.mean(np.asarray(want, dtype=np.float64) ** 2)))


# ---- the inputs of tests/test_gpu_fp16_storage.py, shared with the sensitivity cases of tests/test_fp16_np_cpu.py
TIERS = {  # n_ref, taps of IR 0 / IR 1
    "a": (8192, (7000, 6500)),
    "b": (131072, (88200, 80000)),
    "c": (262144, (256000, 256000)),
    "d": (1048576, (600000, 600000)),
    # the tiers above sweep a few partitions of zero padding at the end (the sweep ends at a multiple of 16); here the last
    # partition of the sweep holds taps, so one dropped there would show
    "e": (8192, (4096, 3900)),
}
LOUDER = 64.0  # IR 1 over IR 0: two different scale16
QUIET_AMP = 2.0 ** -27  # the quiet stream: 16 |X| of a few 2^-20, some tens of quanta of a subnormal half


def flat_ir(taps, seed, level=1.0):
    """Flat-envelope Gaussian noise, float32 [taps][2]: every partition weighs the same in the sum.  At level LOUDER the taps'
    energy is 0.01, so that the output stays a decade inside the engine's saturating clamp at +-1 on every stream here."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((taps, 2)) * (level * 0.1 / (LOUDER * np.sqrt(taps)))).astype(np.float32)


def tier_irs(tier):
    t0, t1 = TIERS[tier][1]
    return [flat_ir(t0, 100 + ord(tier)), flat_ir(t1, 200 + ord(tier), LOUDER)]


def wide_ir():
    """An IR spanning 140 dB and more: partition 0 at 1.0, partition 2 at 1e-7, partition 3 at 1e-9.  The scale rule puts the
    largest entry in [2^12, 2^13) and the smallest normal half is 2^-14, 160 dB below: at 1e-7 only the smallest entries of a
    partition are stored as subnormal halves, at 1e-9 all of them are."""
    rng = np.random.default_rng(77)
    h = np.zeros((1024, 2))
    h[:256] = rng.standard_normal((256, 2)) * 0.05
    h[512:768] = rng.standard_normal((256, 2)) * 0.05e-7
    h[768:] = rng.standard_normal((256, 2)) * 0.05e-9
    return h.astype(np.float32)


def stream(kind, nframes):
    """The input streams [2][nframes] float32: 'noise' = make_input; 'full' = in1 = 1, in2 = (-1)^n (|X| = 256 at the packed bin:
    4096 in the mirror, the largest legal value); 'quiet' = noise at QUIET_AMP, whose mirror is all subnormal halves."""
    from cuda_audio_amd.synth import make_input

    if kind == "noise":
        return make_input(nframes)
    if kind == "quiet":
        return make_input(nframes, seed=4321, dc=0.0, amp=QUIET_AMP)
    assert kind == "full"
    x = np.ones((2, nframes), np.float32)
    x[1, 1::2] = -1.0
    return x
