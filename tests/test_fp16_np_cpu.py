"""The fp16-storage restatement (tests/fp16_np.py) checked on the CPU: its rounding against hand-written bit patterns, its
unquantised sum against direct convolution, and its sensitivity - each fault the GPU tests (tests/test_gpu_fp16_storage.py) are
for must move the restated output by at least ten times their ceiling on their own inputs."""
import numpy as np
import pytest

import fp16_np as f16

CEILING = 1e-4  # the ceiling of the GPU tests' bar, in units of the window's wet RMS


# ---- quantise / dequantise: round to nearest even, subnormal halves kept

def _q(v, scale=1.0):
    return int(f16.quantise(np.array([v], np.float32), scale)[0])


def test_quantise_ties_go_to_even():
    assert _q(1.0) == 0x3C00
    assert _q(1.0 + 2.0 ** -11) == 0x3C00  # halfway between 0x3C00 and 0x3C01
    assert _q(1.0 + 3 * 2.0 ** -11) == 0x3C02  # halfway between 0x3C01 and 0x3C02
    assert _q(1.0 + 2.0 ** -11 + 2.0 ** -20) == 0x3C01  # just above the tie
    assert _q(1.0 + 3 * 2.0 ** -11 - 2.0 ** -20) == 0x3C01  # just below the next
    assert _q(-(1.0 + 2.0 ** -11)) == 0xBC00 and _q(-(1.0 + 3 * 2.0 ** -11)) == 0xBC02
    assert _q(2048.0 + 1.0) == 0x6800 and _q(2048.0 + 3.0) == 0x6802  # spacing 2 from 2048 on
    assert _q(0.5, 2.0) == 0x3C00 and _q(3.0, 2.0 ** -1) == 0x3E00  # the scale is applied first


def test_quantise_at_every_binade_edge():
    for e in range(-14, 16):
        top = (e + 15) << 10  # 2^e
        assert _q(2.0 ** e) == top
        assert _q(2.0 ** e * (1 + 2.0 ** -10)) == top + 1  # the next half above
        assert _q(2.0 ** e * (1 + 2.0 ** -11)) == top  # tie above the edge: to the even one, 2^e
        assert _q(-(2.0 ** e)) == 0x8000 | top
        if e == -14:  # below the smallest normal half the spacing stays 2^-24: the subnormals
            assert _q(2.0 ** e * (1 - 2.0 ** -10)) == 0x03FF  # the largest subnormal
            assert _q(2.0 ** e * (1 - 2.0 ** -11)) == 0x0400  # tie between 0x03FF and 0x0400: even
            assert _q(2.0 ** e * (1 - 2.0 ** -11 - 2.0 ** -20)) == 0x03FF
            continue
        assert _q(2.0 ** e * (1 - 2.0 ** -11)) == top - 1  # the last half below
        assert _q(2.0 ** e * (1 - 2.0 ** -12)) == top  # tie below the edge (the spacing halves there): to the even one, 2^e
        assert _q(2.0 ** e * (1 - 2.0 ** -12 - 2.0 ** -20)) == top - 1


def test_quantise_subnormal_halves_largest_finite_and_zeros():
    assert _q(2.0 ** -24) == 0x0001  # the smallest subnormal
    assert _q(2.0 ** -25) == 0x0000  # tie between 0 and 0x0001: even
    assert _q(2.0 ** -25 * (1 + 2.0 ** -20)) == 0x0001
    assert _q(3 * 2.0 ** -25) == 0x0002  # tie between 0x0001 and 0x0002
    assert _q(5 * 2.0 ** -25) == 0x0002  # tie between 0x0002 and 0x0003
    assert _q(1023 * 2.0 ** -24) == 0x03FF and _q(-1023 * 2.0 ** -24) == 0x83FF
    assert _q(1023.5 * 2.0 ** -24) == 0x0400  # tie between the largest subnormal and the smallest normal
    assert _q(65504.0) == 0x7BFF and _q(-65504.0) == 0xFBFF
    assert _q(65519.0) == 0x7BFF  # below the halfway point to 2^16
    assert _q(65520.0) == 0x7C00  # the halfway point rounds to even: infinity
    assert _q(4096.0) == 0x6C00  # the mirror's largest legal value (|X| = 256, times 16)
    assert _q(0.0) == 0x0000 and _q(-0.0) == 0x8000
    # the inverse is exact and keeps subnormal halves
    bits = np.array([0x0001, 0x03FF, 0x0400, 0x3C00, 0x7BFF, 0x8001, 0x0000, 0x8000], np.uint16)
    want = np.array([2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 1.0, 65504.0, -(2.0 ** -24), 0.0, -0.0], np.float32)
    got = f16.dequantise(bits)
    assert got.dtype == np.float32 and np.array_equal(got, want) and np.signbit(got[7]) and not np.signbit(got[6])
    every = np.arange(0x7C00, dtype=np.uint16)  # every finite non-negative half survives the round trip
    assert np.array_equal(f16.quantise(f16.dequantise(every), 1.0), every)


def test_scale_rule():
    one = np.zeros((256, 16, 4), np.float32)
    assert f16.scale_rule(one) == 2.0 ** 13  # all zero: ex = 0
    for mx, ex in ((1.0, 1), (0.99, 0), (0.5, 0), (40.0, 6), (2.0 ** -20, -19), (3e-36, -118), (2.0 ** -116, -115)):
        one[3, 2, 1] = -mx
        assert f16.scale_rule(one) == 2.0 ** min(13 - ex, f16.SCALE16_MAX_EXP), mx
    s = np.float32(f16.scale_rule(one)) * np.float32(16)  # the quietest: scale x 16 and its reciprocal are normal floats
    assert np.isfinite(s) and np.float32(1) / s >= np.finfo(np.float32).tiny
    # a merged entry: sum |c_j| 2^14 / scale_j = 0.5 * 2 + 0.25 * 8 = 3 -> ex = 2
    assert f16.scale_rule_merged([0.5, -0.25], [2.0 ** 13, 2.0 ** 11]) == 2.0 ** 11
    assert f16.scale_rule_merged([0.0], [2.0 ** 13]) == 2.0 ** 13
    assert f16.scale_rule_merged([1.0], [2.0 ** 122]) == 2.0 ** 120  # bound 2^-108: ex = -107
    assert f16.scale_rule_merged([2.0 ** -10], [2.0 ** 122]) == 2.0 ** 122  # bound 2^-118: 13 + 117 = 130, held to 122


# ---- the unquantised restatement is the convolution

def _ring(x, ring):
    """The delay line after all of x [2][256 nb] went in: float64 [256][ring][4], block t in slot t & (ring - 1)."""
    X = f16.spectra(np.asarray(x, np.float64).T)
    nb = X.shape[1]
    out = np.zeros((256, ring, 4))
    first = max(0, nb - ring)
    out[:, np.arange(first, nb) & (ring - 1)] = X[:, first:]
    return out


def test_unquantised_restatement_is_direct_convolution(oracle_mod):
    rng = np.random.default_rng(5)
    h0 = (rng.standard_normal((1900, 2)) * 0.1).astype(np.float32)  # 8 partitions
    h1 = (rng.standard_normal((1100, 2)) * 0.3).astype(np.float32)  # 5 partitions
    nb, ring, n = 40, 32, 12
    x = f16.stream("noise", nb * 256)
    H0, H1 = f16.spectra(h0, 16), f16.spectra(h1, 16)
    g = np.array([0.7, -0.4, 0.3, 0.9])
    gains = np.tile(g, (ring, 1))
    Y = f16.partition_sum(H0, H1, _ring(x, ring), gains, np.arange(nb - n - 1, nb), 0, 16)
    got = f16.wet_blocks(Y)
    N = nb * 256
    c = lambda xi, h: oracle_mod.direct_conv(xi, h)[:N]
    want = np.stack([g[0] * c(x[0], h0[:, 0]) + g[1] * c(x[1], h1[:, 0]), g[2] * c(x[0], h0[:, 1]) + g[3] * c(x[1], h1[:, 1])])
    want = want[:, (nb - n) * 256:]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"restatement against direct convolution: {err:.3e} of the peak")
    assert err <= 1e-12
    # split at any lo16, the two ranges add up to the whole
    Y2 = f16.partition_sum(H0, H1, _ring(x, ring), gains, np.arange(nb - n - 1, nb), 0, 3)
    Y2 += f16.partition_sum(H0, H1, _ring(x, ring), gains, np.arange(nb - n - 1, nb), 3, 16)
    assert np.abs(Y2 - Y).max() <= 1e-12 * np.abs(Y).max()


# ---- sensitivity, on the inputs of the GPU tests' smallest tier

RING, NB, WINDOW, HI = 128, 200, 16, 32  # blocks pushed (the ring wraps), blocks compared, partitions swept (28 rounded up to 16)


def _trunc(a32, scale):
    """A pack that truncates toward zero."""
    a = np.abs(np.asarray(a32, np.float32) * np.float32(scale)).astype(np.float64)
    h = a.astype(np.float16)
    over = h.astype(np.float64) > a
    bits = h.view(np.uint16).copy()
    bits[over] -= 1
    return bits | (np.signbit(np.asarray(a32, np.float32)).astype(np.uint16) << 15)


def _flush(bits):
    """An unpack that flushes subnormal halves."""
    v = f16.dequantise(bits).copy()
    v[(np.asarray(bits) & 0x7C00) == 0] = 0.0
    return v


def _tier(tier, hi):
    irs = f16.tier_irs(tier)
    H = [f16.spectra(ir, hi).astype(np.float32) for ir in irs]
    sc = [f16.scale_rule(h) for h in H]
    assert sc[0] >= 16 * sc[1]  # IR 1 is 64 times louder: the scales differ (by 32 or 64 or 128, as the largest entries fall)
    gains = np.tile(np.float32([0.2, 0.2, 0.2, 0.2]), (RING, 1))
    out = {}
    for kind in ("noise", "quiet", "full"):
        x = f16.stream(kind, NB * 256)
        X = _ring(x, RING).astype(np.float32)
        Xold = _ring(x[:, : (NB - RING) * 256], RING).astype(np.float32)  # what the slots held RING blocks earlier
        out[kind] = (X, Xold)
    return H, sc, gains, out, hi


@pytest.fixture(scope="module")
def tier_a():
    return _tier("a", HI)


def _run(tier_a, kind, lo16=0, pack=f16.quantise, unpack=f16.dequantise, swap=False, hi=None, stale=None):
    H, sc, gains, streams, hi_all = tier_a
    hi = hi_all if hi is None else hi
    X, Xold = streams[kind]
    Hq = [unpack(pack(H[i], sc[i])) for i in (0, 1)]
    X16 = pack(X, f16.FDL16_SCALE)
    if stale is not None:
        X16[:, stale] = pack(Xold, f16.FDL16_SCALE)[:, stale]
    slots = np.arange(NB - WINDOW - 1, NB)
    return f16.wet_blocks(f16.partition_sum_q(H[0], H[1], X, Hq[0], Hq[1], unpack(X16), sc[0], sc[1], gains, slots, lo16, hi, swap_inv=swap))


FAULTS = {
    "pack truncates": dict(pack=_trunc),
    "unpack flushes subnormal halves": dict(unpack=_flush),
    "inv.x and inv.y swapped": dict(swap=True),
    "last partition dropped": dict(hi=27),  # IR 0's partition 27, the last that holds taps
    "lo16 one too low": dict(lo16=1),
    "lo16 one too high": dict(lo16=3),
    "one delay-line slot stale": dict(stale=(NB - 10) & (RING - 1)),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_restatement_sees_the_fault(tier_a, fault):
    """Each fault moves the worst 256-frame block of the window by at least 10 x CEILING of the wet RMS on one of the GPU tests'
    streams at tier a (a fault that any of the streams shows fails the GPU test)."""
    kw = FAULTS[fault]
    base_lo16 = 2 if fault.startswith("lo16") else 0  # the period path's split for the faults that move it
    margins = {}
    for kind in ("noise", "quiet", "full"):
        want = _run(tier_a, kind, lo16=base_lo16)
        got = _run(tier_a, kind, **dict(dict(lo16=base_lo16), **kw))
        margins[kind] = f16.worst_block(got, want) / CEILING
    print(f"{fault}: moves the worst block by " + ", ".join(f"{m:.1f} ({k})" for k, m in margins.items()) + " x the ceiling")
    assert max(margins.values()) >= 10.0, margins


def test_restatement_sees_the_last_partition_of_the_sweep_dropped():
    """Tier e: 16 partitions, a multiple of the sweep's granule, so the last partition of the sweep itself holds taps (at tiers a
    to d the sweep ends in zero padding and a kernel that stopped one partition early would compute the same)."""
    t = _tier("e", 16)
    m = f16.worst_block(_run(t, "noise", hi=15), _run(t, "noise")) / CEILING
    print(f"tier e, partition 15 of 16 dropped: moves the worst block by {m:.1f} x the ceiling")
    assert m >= 10.0


def test_quantisation_itself_is_far_above_the_ceiling(tier_a):
    """What the old bar had to absorb: the quantised sum differs from the unquantised one by some 1e-4 .. 1e-2 of the wet RMS."""
    H, sc, gains, streams, _ = tier_a
    slots = np.arange(NB - WINDOW - 1, NB)
    for kind in ("noise", "quiet"):
        exact = f16.wet_blocks(f16.partition_sum(H[0], H[1], streams[kind][0], gains, slots, 0, HI))
        q = f16.worst_block(_run(tier_a, kind), exact)
        print(f"{kind}: quantisation moves the worst block by {q:.3e} of the wet RMS")
        assert q > 1e-4
