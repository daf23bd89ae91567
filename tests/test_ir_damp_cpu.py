"""Damping of an IR on load, the part that needs no GPU: the layout and defaults of mc_ir_damp, every refused field (checked
before the engine is looked at, so a null engine will do), mc_ir_damp_response against the float64 restatement
(tests/ir_damp_np.py), the restatement's own properties, and how well a decay aimed by 1 / T = 1 / T_before + rate / decay_t60
lands when it is measured as mc_ir_decay measures."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from cuda_audio_amd import _lib
import ir_damp_np

AIM = ir_damp_np.AIM


def _default():
    d = _lib.McIrDamp()
    _lib.load().mc_default_ir_damp(C.byref(d))
    return d


def test_symbols_layout_and_defaults():
    L = _lib.load()
    for name in ("mc_default_ir_damp", "mc_load_ir_damped", "mc_ir_damp_info", "mc_ir_damp_response"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert _lib.MC_DAMP_MAX_XOVERS == 3
    assert C.sizeof(_lib.McIrDamp) == 64
    assert (_lib.McIrDamp.xover_hz.offset, _lib.McIrDamp.decay_t60.offset, _lib.McIrDamp.origin.offset) == (8, 24, 56)
    d = _default()
    assert d.struct_size == 64 and d.n_xovers == 0 and d.reserved == 0 and d.origin == 0
    assert list(d.xover_hz) == [250.0, 2000.0, 8000.0]
    assert list(d.decay_t60) == [0, 0, 0, 0]


def _load(d, rates=(48000, 48000), shape=None, eq=None):
    """mc_load_ir_damped with a null engine."""
    L = _lib.load()
    rc = L.mc_load_ir_damped(None, 0, None, 100, 1024, rates[0], rates[1], C.byref(shape) if shape is not None else None,
                             C.byref(eq) if eq is not None else None, C.byref(d) if d is not None else None)
    return rc, L.mc_last_error().decode()


def _damp(xovers=(400.0, 1600.0), **fields):
    d = _default()
    d.n_xovers = len(xovers)
    for k, hz in enumerate(xovers):
        d.xover_hz[k] = hz
    for k, v in fields.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("d,rates,named", [
    (_damp(struct_size=60), (48000, 48000), "struct_size"),
    (_damp(n_xovers=4), (48000, 48000), "n_xovers"),
    (_damp((9.0, 1600.0)), (48000, 48000), "xover_hz[0]"),
    (_damp((400.0, 0.46 * 48000)), (48000, 48000), "xover_hz[1]"),
    (_damp((400.0, 1600.0, math.nan)), (48000, 48000), "xover_hz[2]"),
    (_damp((400.0, 400.0)), (48000, 48000), "xover_hz[1]"),
    (_damp((400.0, 1600.0, 800.0)), (48000, 48000), "xover_hz[2]"),
    (_damp(), (0, 0), "session_rate"),
    (_damp(), (44100, 7999), "session_rate"),
    (_damp(), (384001, 48000), "ir_rate"),
], ids=["struct_size", "four", "9hz", "above", "nan", "equal", "descending", "rates00", "session", "ir_rate"])
def test_bad_fields_are_refused_before_the_engine_is_looked_at(d, rates, named):
    rc, msg = _load(d, rates)
    assert rc == -1 and named in msg, msg


def test_the_checks_come_in_the_stated_order():
    """struct_size, n_xovers, the rates, the crossovers, then eq and shape as mc_load_ir_eq checks them."""
    eq = _lib.McIrEq()
    _lib.load().mc_default_ir_eq(C.byref(eq))
    eq.band[0].kind = 6
    sh = _lib.McIrShape()
    _lib.load().mc_default_ir_shape(C.byref(sh))
    sh.trim_db = 1.0
    for d, rates, named in ((_damp((9.0,), struct_size=60, n_xovers=4), (0, 0), "struct_size"), (_damp((9.0,), n_xovers=4), (0, 0), "n_xovers"),
                            (_damp((9.0,)), (0, 0), "session_rate"), (_damp((9.0,)), (48000, 48000), "xover_hz[0]"),
                            (_damp(), (48000, 48000), "kind")):
        rc, msg = _load(d, rates, shape=sh, eq=eq)
        assert rc == -1 and named in msg, msg
    rc, msg = _load(_damp(), shape=sh)
    assert rc == -1 and "trim_db" in msg, msg


def test_a_good_damping_reaches_the_pointer_checks():
    for d, rates in ((_damp(), (48000, 48000)), (_damp((10.0, 0.45 * 48000)), (44100, 48000)), (_damp((250.0, 2000.0, 8000.0)), (48000, 48000))):
        rc, msg = _load(d, rates)
        assert rc == -1 and "null" in msg, msg


def test_damping_off_looks_at_no_other_field():
    """n_xovers = 0, or no mc_ir_damp at all: the call is mc_load_ir_eq, whose own refusal of the null engine is what comes
    back - also with rates 0 / 0, which mean no conversion there."""
    junk = _damp((), struct_size=1, origin=2**63, reserved=7)
    junk.xover_hz[0], junk.xover_hz[1], junk.xover_hz[2] = math.nan, -1.0, 0.0
    junk.decay_t60[3] = 5
    for d in (junk, None):
        for rates in ((0, 0), (44100, 48000)):
            rc, msg = _load(d, rates)
            assert rc == -1 and "null" in msg, msg


def test_python_damp_maps_onto_the_struct():
    from cuda_audio_amd.engine import IrDamp

    d = IrDamp().to_c()
    assert (d.struct_size, d.n_xovers, d.origin) == (64, 2, 0)
    assert list(d.xover_hz)[:2] == [400.0, 1600.0] and list(d.decay_t60) == [0, 4800, 1600, 0]
    d = IrDamp(xovers=(250, 2000, 8000), decay=(1, 2, 3, 4), origin=9).to_c()
    assert (d.n_xovers, d.origin, list(d.decay_t60)) == (3, 9, [1, 2, 3, 4])
    assert bytes(IrDamp(xovers=(), decay=()).to_c()) == bytes(_default())
    with pytest.raises(ValueError):
        IrDamp(xovers=(1, 2, 3, 4), decay=(0,) * 5).to_c()
    with pytest.raises(ValueError):
        IrDamp(xovers=(400, 1600), decay=(0, 1)).to_c()


# -- mc_ir_damp_response ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,xovers,decay,origin,tap", [
    (8000, (400, 1600), (0, 4800, 1600), 37, 2000),
    (48000, (250, 2000, 8000), (96000, 0, 24000, 12000), 0, 30000),
    (384000, (500,), (0, 100000), 1000, 500000),
    (44100, (300, 3000), (20000, 9000, 4000), 5000, 100),
])
def test_response_matches_the_restatement(rate, xovers, decay, origin, tap):
    """1e-9 dB where the formula itself is determined that well.  Its denominator 1 + a1 z^-1 + a2 z^-2 is of the size of w0^2 near
    and below the crossover, so one ulp of a1 moves a section by 2.2e-16 / w0^2: 6e-11 dB for 500 Hz at 384 kHz, the lowest
    w0 here, but 3e-8 dB for 10 Hz at 384 kHz, where two libraries' cosines need not agree to the last bit: that corner
    is not in the list."""
    from cuda_audio_amd.engine import IrDamp, damp_response

    hz = np.geomspace(10.0, 0.45 * rate, 96)
    got = damp_response(IrDamp(xovers, decay, origin), rate, tap, hz)
    want = ir_damp_np.response_db(xovers, decay, origin, rate, tap, hz)
    print(f"{len(xovers)} crossovers at {rate} Hz, tap {tap}: {want.min():+.2f} .. {want.max():+.2f} dB, max difference {np.abs(got - want).max():.2e} dB")
    assert np.abs(got - want).max() <= 1e-9
    if tap <= origin:  # (no envelope has begun)
        assert np.abs(got).max() <= 1e-9


def test_response_is_0_db_at_the_origin_and_with_damping_off():
    from cuda_audio_amd.engine import IrDamp, damp_response

    hz = np.geomspace(10.0, 3600.0, 32)
    for tap in (0, 36, 37):
        assert np.abs(damp_response(IrDamp(origin=37), 8000, tap, hz)).max() <= 1e-12
    assert np.all(damp_response(IrDamp(xovers=(), decay=()), 8000, 5000, hz) == 0.0)


def test_equal_decays_have_the_broadband_envelopes_response():
    from cuda_audio_amd.engine import IrDamp, damp_response

    hz = np.geomspace(10.0, 0.45 * 48000, 32)
    got = damp_response(IrDamp((250, 2000, 8000), (9600,) * 4, 100), 48000, 4900, hz)
    want = 20.0 * np.log10(np.exp2(-(4800 * ir_damp_np.DECAY_K) / 9600.0))
    assert abs(want + 30.0) < 1e-9  # (half of decay_t60 past the origin: 30 dB)
    assert np.abs(got - want).max() <= 1e-9


def test_response_approaches_the_outer_bands_envelopes():
    """At 10 Hz every H_k^2 is nearly 1 and the response nearly g_0; at 0.45 rate every H_k^2 is nearly 0 and the response nearly
    g_X.  How nearly follows from |R - g_0| <= sum |g_(k-1) - g_k| |H_k^2 - 1| and |R - g_X| <= sum |g_(k-1) - g_k| |H_k|^2, with
    the H_k of the restatement at those two frequencies."""
    from cuda_audio_amd.engine import IrDamp, damp_response

    rate, xovers, decay, origin, tap = 48000, (250, 2000, 8000), (96000, 48000, 24000, 12000), 64, 12064
    g = ir_damp_np.envelopes(tap + 1, decay, origin)[:, tap]
    dg = np.abs(g[:-1] - g[1:])
    lo, hi = 10.0, 0.45 * rate
    H2 = {f: np.array([ir_damp_np.section_response(x, rate, np.array([f]))[0] ** 2 for x in xovers]) for f in (lo, hi)}
    got = damp_response(IrDamp(xovers, decay, origin), rate, tap, [lo, hi])
    for f, gj, dev, r in ((lo, g[0], float((dg * np.abs(H2[lo] - 1.0)).sum()), got[0]), (hi, g[-1], float((dg * np.abs(H2[hi])).sum()), got[1])):
        assert dev < gj
        bound = -20.0 * np.log10(1.0 - dev / gj)
        print(f"{f:.0f} Hz: {r:+.6f} dB against the band's {20 * np.log10(gj):+.6f} dB, bound {bound:.2e} dB")
        assert abs(r - 20.0 * np.log10(gj)) <= bound + 1e-9
        assert bound < 0.1 * 20.0 * np.log10(g[0] / g[-1])  # (small against the 52.5 dB between the two envelopes)
    assert got[0] - got[1] > 40.0  # -7.5 dB against -60 dB


def test_response_refuses_a_bad_damping():
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrDamp, damp_response

    for d, rate in ((IrDamp((5.0,), (0, 100)), 48000), (IrDamp((1000.0,), (0, 100)), 4000), (IrDamp((1000.0, 900.0), (0, 100, 100)), 48000)):
        with pytest.raises(McError) as ex:
            damp_response(d, rate, 10, [100.0])
        assert ex.value.code == -1


# -- the restatement's own properties --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _noise(n=3000, seed=4):
    x = np.random.default_rng(seed).standard_normal((n, 2)) * np.exp(-np.arange(n) / 600.0)[:, None]
    x.setflags(write=False)
    return x


def test_equal_decays_are_the_plain_envelope_exactly():
    x = _noise()
    y = ir_damp_np.damp(x, (400, 1600, 5000), (2400,) * 4, 100, 48000)
    t = np.maximum(np.arange(len(x)), 100) - 100.0
    assert np.array_equal(y, np.exp2(-(t * ir_damp_np.DECAY_K) / 2400.0)[:, None] * x)


def test_zero_decays_and_a_late_origin_change_nothing():
    x = _noise()
    assert np.array_equal(ir_damp_np.damp(x, (400, 1600), (0, 0, 0), 0, 48000), x)
    for origin in (len(x), len(x) + 5):
        assert np.array_equal(ir_damp_np.damp(x, (400, 1600), (0, 4800, 1600), origin, 48000), x)
    assert not np.array_equal(ir_damp_np.damp(x, (400, 1600), (0, 4800, 1600), len(x) - 2, 48000), x)


def test_the_bands_telescope_to_the_input():
    x = _noise()
    B = ir_damp_np.bands(x, ir_damp_np.lowpasses(x, (400, 1600, 5000), 48000))
    assert len(B) == 4
    total = B[0] + B[1] + B[2] + B[3]
    assert np.abs(total - x).max() <= 1e-12 * np.abs(x).max()
    # and the output is their weighted sum
    decay, origin = (0, 4800, 1600, 800), 50
    g = ir_damp_np.envelopes(len(x), decay, origin)
    want = sum(g[j][:, None] * B[j] for j in range(4))
    got = ir_damp_np.damp(x, (400, 1600, 5000), decay, origin, 48000)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max()


def test_restatement_order_and_info():
    """Damping sees the faded taps, the bands see the damped ones and the normalisation the bands' output; no crossover is
    ir_eq_np.eq64 itself."""
    import ir_eq_np
    from ir_shape_np import quiet_lead_ir, shape64

    ir = quiet_lead_ir(3000)
    fields = dict(fade_out=64, normalize="peak", target=0.02)
    bands = [("peak", 1000, 12.0)]
    v, info, dinfo = ir_damp_np.damp64(ir, 2000, None, 48000, (400, 1600), (0, 4800, 1600), 5000, bands, **fields)
    assert abs(np.abs(v).max() / float(np.float32(0.02)) - 1) <= 1e-12
    assert info["eq_bands"] == 1 and info["taps"] == 2000
    assert dinfo == dict(xovers=2, origin=2000, damped_bands=2)
    w, winfo = ir_eq_np.eq64(ir, 2000, None, 48000, bands, **fields)
    np.testing.assert_array_equal(v, w)  # (the origin lies past the last tap)
    assert info == winfo
    v, info, dinfo = ir_damp_np.damp64(ir, 2000, None, 48000, (400, 1600), (0, 4800, 1600), 700, bands, **fields)
    pre, _ = shape64(ir, 2000, fade_out=64)
    np.testing.assert_allclose(v / info["gain"], ir_eq_np.cascade(ir_damp_np.damp(pre, (400, 1600), (0, 4800, 1600), 700, 48000), bands, 48000),
                               rtol=1e-12, atol=0)
    swapped = ir_damp_np.damp64(ir, 2000, None, 48000, (400, 1600), (0, 4800, 1600), 700, bands, eq_first=True, **fields)[0]
    assert np.abs(swapped - v).max() > 1e-3 * np.abs(v).max()
    assert dinfo["origin"] == 700 and info["peak"] != winfo["peak"]


# -- aiming ----------------------------------------------------------------------------------------------------------------
def test_a_decay_aimed_by_the_slopes_lands_within_a_tenth():
    """1 / T = 1 / T_before + rate / decay_t60 per band, from that band's own T30 before damping.  2.2 %, 4.3 % and 6.2 % on this
    input: the bands overlap and a band's decay curve is bent, so the aim is a first step, not the answer."""
    _, _, before, after = ir_damp_np.aim_case()
    assert before["origin"] == after["origin"] == AIM["origin"]
    for b, d in enumerate(AIM["decay"], start=1):
        t0, t1 = before["rows"][(b, "LR")]["t30"], after["rows"][(b, "LR")]["t30"]
        want = 1.0 / (1.0 / t0 + AIM["rate"] / d) if d else t0
        print(f"{AIM['bands'][b - 1]} Hz: T30 {t0:.4f} s before, {t1:.4f} s after, aimed at {want:.4f} s: {abs(t1 / want - 1) * 100:.1f} %")
        assert abs(t1 / want - 1) <= 0.10


def test_damp_for_rt60():
    from cuda_audio_amd.engine import damp_for_rt60, decay_for_rt60

    got = damp_for_rt60((2.9, 2.6, 2.4), (None, 1.8, 1.2), 48000)
    assert got == (0, decay_for_rt60(2.6, 1.8, 48000), decay_for_rt60(2.4, 1.2, 48000))
    assert damp_for_rt60((2.9, 2.6, 2.4, 2.0), (math.nan, 2.6, 3.0, 1.0), 44100) == (0, 0, 0, decay_for_rt60(2.0, 1.0, 44100))
    assert damp_for_rt60((1.0,), (None,), 48000) == (0,)
    with pytest.raises(ValueError):
        damp_for_rt60((1.0, 2.0), (0.5,), 48000)
    with pytest.raises(ValueError):
        damp_for_rt60((1.0,), (0.0,), 48000)  # (decay_for_rt60's own refusal: a target must be positive)
