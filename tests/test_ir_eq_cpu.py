"""Equalisation of an IR on load, the part that needs no GPU: the layout and defaults of mc_ir_eq, every refused field (checked
before the engine is looked at, so a null engine will do), mc_ir_eq_response against the analytic response of the float64
restatement (tests/ir_eq_np.py), and the restatement's recurrence against that response."""
import ctypes as C
import math

import numpy as np
import pytest

from cuda_audio_amd import _lib
import ir_eq_np

BANDS3 = (("lowcut", 80), ("peak", 1000, 6.0, 2.0), ("highcut", 8000))
BANDS8 = (("lowcut", 30, 0, 1.2), ("lowshelf", 200, 6.0), ("peak", 400, -12.0, 4.0), ("peak", 1000, 6.0, 2.0), ("peak", 2500, 3.5, 0.3),
          ("peak", 5200, -36.0, 32.0), ("highshelf", 6000, -9.0, 0.5), ("highcut", 15000, 0, 0.9))


def _default():
    eq = _lib.McIrEq()
    _lib.load().mc_default_ir_eq(C.byref(eq))
    return eq


def test_symbols_layout_and_defaults():
    L = _lib.load()
    for name in ("mc_default_ir_eq", "mc_load_ir_eq", "mc_ir_eq_response"):
        assert name in _lib.SYMBOLS
        assert hasattr(L, name)
    assert C.sizeof(_lib.McEqBand) == 16
    assert C.sizeof(_lib.McIrEq) == 8 + 16 * 8
    assert _lib.MC_EQ_MAX_BANDS == 8
    assert (_lib.MC_EQ_OFF, _lib.MC_EQ_LOWCUT, _lib.MC_EQ_HIGHCUT, _lib.MC_EQ_LOWSHELF, _lib.MC_EQ_HIGHSHELF, _lib.MC_EQ_PEAK) == (0, 1, 2, 3, 4, 5)
    eq = _default()
    assert eq.struct_size == 136 and eq.reserved == 0
    for b in eq.band:
        assert b.kind == _lib.MC_EQ_OFF and b.gain_db == 0.0 and b.q == np.float32(0.70710678)


def _refused(rates=(48000, 48000), struct_size=None, **fields):
    """mc_load_ir_eq with a null engine, band 2 a peak at 1 kHz with `fields` over it."""
    L = _lib.load()
    eq = _default()
    eq.band[2].kind = _lib.MC_EQ_PEAK
    for k, v in fields.items():
        setattr(eq.band[2], k, v)
    if struct_size is not None:
        eq.struct_size = struct_size
    rc = L.mc_load_ir_eq(None, 0, None, 100, 1024, rates[0], rates[1], None, C.byref(eq))
    return rc, L.mc_last_error().decode()


@pytest.mark.parametrize("fields,named", [
    (dict(struct_size=132), "struct_size"),
    (dict(kind=6), "kind"),
    (dict(freq_hz=9.0), "freq_hz"),
    (dict(freq_hz=0.46 * 48000), "freq_hz"),
    (dict(freq_hz=math.nan), "freq_hz"),
    (dict(q=0.05), ": q "),
    (dict(q=33.0), ": q "),
    (dict(q=math.inf), ": q "),
    (dict(gain_db=25.0), "gain_db"),
    (dict(gain_db=-37.0), "gain_db"),
])
def test_bad_fields_are_refused_before_the_engine_is_looked_at(fields, named):
    rc, msg = _refused(**fields)
    assert rc == -1 and named in msg, msg
    if "struct_size" not in fields and fields.get("kind") != 6:
        assert "band 2" in msg, msg


@pytest.mark.parametrize("rates,named", [
    ((0, 0), "session_rate"), ((44100, 0), "session_rate"), ((44100, 7999), "session_rate"), ((44100, 384001), "session_rate"),
    ((0, 48000), "ir_rate"), ((7999, 48000), "ir_rate"), ((384001, 48000), "ir_rate"),
])
def test_a_band_that_is_on_needs_the_rates(rates, named):
    rc, msg = _refused(rates)
    assert rc == -1 and named in msg, msg


def test_a_good_eq_reaches_the_pointer_checks():
    """Everything valid: the null engine is what is refused, with a band on and with none (then through mc_load_ir_shaped,
    where 0 / 0 is no error), and a bad shape is refused by its own check."""
    L = _lib.load()
    for rates in ((48000, 48000), (44100, 48000)):
        rc, msg = _refused(rates)
        assert rc == -1 and "null" in msg, msg
    # the limits themselves are inside
    for fields in (dict(freq_hz=10.0), dict(freq_hz=0.45 * 48000), dict(q=0.1), dict(q=32.0), dict(gain_db=24.0), dict(gain_db=-36.0)):
        rc, msg = _refused(**fields)
        assert rc == -1 and "null" in msg, (fields, msg)
    # a cut does not look at its gain; a band that is off at none of its fields
    for fields in (dict(kind=_lib.MC_EQ_LOWCUT, gain_db=99.0), dict(kind=_lib.MC_EQ_OFF, freq_hz=1.0, q=0.0, gain_db=math.nan)):
        rc, msg = _refused(**fields)
        assert rc == -1 and "null" in msg, (fields, msg)
    off = _default()
    for rates in ((0, 0), (44100, 48000)):
        assert L.mc_load_ir_eq(None, 0, None, 100, 1024, rates[0], rates[1], None, C.byref(off)) == -1
        assert "null" in L.mc_last_error().decode()
    s = _lib.McIrShape()
    L.mc_default_ir_shape(C.byref(s))
    s.trim_db = 1.0
    on = _default()
    on.band[0].kind = _lib.MC_EQ_LOWCUT
    for eq in (off, on):
        assert L.mc_load_ir_eq(None, 0, None, 100, 1024, 48000, 48000, C.byref(s), C.byref(eq)) == -1
        assert "trim_db" in L.mc_last_error().decode()


def test_python_eq_maps_onto_the_struct():
    from cuda_audio_amd.engine import IrEq

    eq = IrEq(bands=[("lowcut", 120), ("peak", 2500, 6.0, 1.5), ("highshelf", 6000, -9)]).to_c()
    assert eq.struct_size == 136
    got = [(b.kind, b.freq_hz, b.gain_db, b.q) for b in eq.band]
    q = np.float32(0.70710678)
    assert got[:3] == [(_lib.MC_EQ_LOWCUT, 120.0, 0.0, q), (_lib.MC_EQ_PEAK, 2500.0, 6.0, 1.5), (_lib.MC_EQ_HIGHSHELF, 6000.0, -9.0, q)]
    assert all(g[0] == _lib.MC_EQ_OFF for g in got[3:])
    assert bytes(IrEq().to_c()) == bytes(_default())
    with pytest.raises(ValueError):
        IrEq(bands=[("bell", 100)]).to_c()
    with pytest.raises(ValueError):
        IrEq(bands=[("peak", 100)] * 9).to_c()


@pytest.mark.parametrize("rate", [44100, 384000])
@pytest.mark.parametrize("bands", [BANDS3, BANDS8], ids=["3", "8"])
def test_response_matches_the_analytic_one(bands, rate):
    from cuda_audio_amd.engine import IrEq, eq_response

    hz = np.geomspace(10.0, 0.45 * rate, 64)
    got = eq_response(IrEq(bands=list(bands)), rate, hz)
    want = ir_eq_np.response_db(bands, rate, hz)
    print(f"{len(bands)} bands at {rate} Hz: {want.min():+.2f} .. {want.max():+.2f} dB, max difference {np.abs(got - want).max():.2e} dB")
    assert np.abs(got - want).max() <= 1e-6
    assert np.abs(want).max() > 3.0
    # no band on: 0 dB, whatever the other fields hold
    assert np.all(eq_response(IrEq(bands=[("off", 1.0, 99.0, 0.0)]), rate, hz) == 0.0)


def test_response_refuses_a_bad_eq():
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import IrEq, eq_response

    for eq, rate in ((IrEq(bands=[("peak", 5.0, 3.0)]), 48000), (IrEq(bands=[("peak", 1000.0, 3.0)]), 4000)):
        with pytest.raises(McError) as ex:
            eq_response(eq, rate, [100.0])
        assert ex.value.code == -1


def test_the_restated_recurrence_has_the_analytic_response():
    """A unit impulse through three bands at 48 kHz, 32768 taps rounded to float32: their transform is H(e^{jw}) on the grid."""
    rate, n = 48000, 32768
    h = ir_eq_np.impulse_taps(BANDS3, rate, n)
    assert h.dtype == np.float32 and h.shape == (n,)
    got = np.fft.rfft(h.astype(np.float64))
    want = ir_eq_np.response(BANDS3, rate, np.arange(n // 2 + 1) * rate / n)
    err = np.abs(got - want).max()
    print(f"max |rfft - H| {err:.2e}, max |H| {np.abs(want).max():.3f}")
    assert err <= 1e-6
    assert 1.9 < np.abs(want).max() < 2.1


def test_restatement_order_and_info():
    """The bands see the faded taps and the normalisation sees the bands' output; no band on is ir_shape_np.shape64 itself."""
    from ir_shape_np import quiet_lead_ir, shape64

    ir = quiet_lead_ir(3000)
    fields = dict(fade_out=64, normalize="peak", target=0.02)
    v, info = ir_eq_np.eq64(ir, 2000, None, 48000, [("peak", 1000, 12.0)], **fields)
    assert abs(np.abs(v).max() / float(np.float32(0.02)) - 1) <= 1e-12
    assert info["eq_bands"] == 1 and info["taps"] == 2000
    pre, pinfo = shape64(ir, 2000, fade_out=64)
    np.testing.assert_allclose(v / info["gain"], ir_eq_np.cascade(pre, [("peak", 1000, 12.0)], 48000), rtol=1e-12, atol=0)
    assert info["peak"] != pinfo["peak"]
    w, winfo = ir_eq_np.eq64(ir, 2000, None, 48000, [("off", 1000)], **fields)
    s, sinfo = shape64(ir, 2000, **fields)
    np.testing.assert_array_equal(w, s)
    assert winfo == dict(sinfo, eq_bands=0)
