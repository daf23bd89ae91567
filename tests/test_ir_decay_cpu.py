"""The decay measurement without a GPU: the float64 restatement (tests/ir_decay_np.py) against closed forms, its edge rules, the
margin check the device comparisons rely on, mc_ir_decay's argument errors and decay_for_rt60."""
import ctypes as C
import math

import numpy as np
import pytest

import ir_decay_np
from ir_decay_np import assert_range_margin, decay, sign_ir


def test_restatement_against_closed_forms():
    """e[m] = r^m: every decay time is T, C50 and Ts are geometric sums.  What remains is the float32 rounding of the taps."""
    rate, T, n = 8000, 0.25, 6000
    res = decay(sign_ir(n, rate, T), rate, onset_db=0.0)
    assert res["origin"] == 0 and res["taps"] == n
    r = 10.0 ** (-6.0 / 2000.0)
    c50 = 10.0 * math.log10((1.0 - r ** 400) / (r ** 400 - r ** 6000))
    c80 = 10.0 * math.log10((1.0 - r ** 640) / (r ** 640 - r ** 6000))
    ts = r / (1.0 - r) / rate
    for name in ir_decay_np.SETS:
        row = res["rows"][(0, name)]
        print(name, {k: f"{v:.12g}" for k, v in row.items()})
        for f in ("edt", "t20", "t30"):
            assert abs(row[f] / T - 1.0) <= 1e-6, (name, f, row[f])
        assert abs(row["c50"] - c50) <= 1e-6 and abs(row["c80"] - c80) <= 1e-6
        assert abs(row["ts"] / ts - 1.0) <= 1e-6
        assert abs(row["d50"] / ((1.0 - r ** 400) / (1.0 - r ** 6000)) - 1.0) <= 1e-6
        want_e = (2.0 if name == "LR" else 1.0) * (1.0 - r ** 6000) / (1.0 - r)
        assert abs(row["energy"] / want_e - 1.0) <= 1e-6


def test_unit_impulse_and_two_taps():
    one = decay(np.array([[1.0, 1.0]], np.float32), 8000, onset_db=0.0, curve_points=4)
    for name, e in zip(ir_decay_np.SETS, (1.0, 1.0, 2.0)):
        row = one["rows"][(0, name)]
        assert row["energy"] == e and row["ts"] == 0.0
        assert all(math.isnan(row[f]) for f in ("edt", "t20", "t30", "c50", "c80", "d50"))
    np.testing.assert_array_equal(one["curve"], np.zeros((1, 3, 4)))
    # two taps, the second 20 dB below the first: L = {0, -20.04}.  EDT: one tap in [-10, 0]; T20: the curve ends above -25
    # (L[N - 1] > lo) ... and T30 likewise; k50 = 400 >= N
    two = decay(np.array([[1.0, 0.5], [0.1, 0.0]], np.float32), 8000, onset_db=0.0)
    row = two["rows"][(0, "L")]
    assert abs(row["energy"] - (1.0 + float(np.float32(0.1)) ** 2)) < 1e-15
    assert all(math.isnan(row[f]) for f in ("edt", "t20", "t30", "c50", "c80", "d50"))
    assert abs(row["ts"] - float(np.float32(0.1)) ** 2 / row["energy"] / 8000) < 1e-18
    # the right channel ends in a zero tap: L = {0, -inf}; the curve gets below every lo, but no range holds two taps
    rowr = two["rows"][(0, "R")]
    assert rowr["energy"] == 0.25 and rowr["ts"] == 0.0 and all(math.isnan(rowr[f]) for f in ("edt", "t20", "t30"))
    # three taps, L = {0, -4.77, -21.76}: two of them in EDT's range, a slope through two points; the curve ends above -25
    three = decay(np.array([[1.0, 0.0], [0.7, 0.0], [0.1, 0.0]], np.float32), 8000, onset_db=0.0)
    f = [float(np.float32(v)) ** 2 for v in (1.0, 0.7, 0.1)]
    want = -60.0 / (10.0 * math.log10((f[1] + f[2]) / sum(f)) * 8000)
    assert abs(three["rows"][(0, "L")]["edt"] / want - 1.0) < 1e-12 and math.isnan(three["rows"][(0, "L")]["t20"])
    assert three["rows"][(0, "R")]["energy"] == 0.0 and math.isnan(three["rows"][(0, "R")]["ts"])
    # all zero: energy 0, everything else NaN, the curve too
    zero = decay(np.zeros((5, 2), np.float32), 8000, curve_points=3)
    assert zero["origin"] == 0
    for row in zero["rows"].values():
        assert row["energy"] == 0.0 and all(math.isnan(row[f]) for f in ir_decay_np.FIELDS[1:])
    assert np.isnan(zero["curve"]).all()


def test_range_margin_catches_a_level_on_an_edge():
    L = np.array([0.0, -3.0, -7.0, -12.0, -30.0, -50.0, -np.inf])
    assert_range_margin(L)
    assert_range_margin(np.array([0.0, 0.0, -1.0]))  # (the 0 dB edge is exempt)
    for edge in (-5.0, -10.0, -25.0, -35.0):
        for off in (0.0, 5e-10, -5e-10):
            with pytest.raises(AssertionError):
                assert_range_margin(np.append(L, edge + off))
        assert_range_margin(np.append(L, edge + 1e-8))


def test_band_sections_peak_at_0_db():
    """The section's |H| at its centre is 1 (0 dB peak gain) and two of them in cascade are 3 dB down half an octave away for
    q = sqrt 2 ... loosely: between 4 and 8 dB for the pair."""
    rate, hz = 48000, 1000.0
    b0, b1, b2, a1, a2 = ir_decay_np.band_coefs(hz, ir_decay_np.DEFAULT_Q, rate)

    def mag(f):
        z = np.exp(-2j * np.pi * f / rate)
        return abs((b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z))

    assert abs(mag(hz) - 1.0) < 1e-12
    for f in (hz / 2 ** 0.5, hz * 2 ** 0.5):
        assert 4.0 < -40.0 * math.log10(mag(f)) < 8.0


def _query(L, **fields):
    from cuda_audio_amd import _lib

    q = _lib.McDecayQuery()
    L.mc_default_decay_query(C.byref(q))
    for k, v in fields.items():
        if k == "centre_hz":
            for i, hz in enumerate(v):
                q.centre_hz[i] = hz
        else:
            setattr(q, k, v)
    return q


def test_default_query_and_argument_errors_need_no_gpu():
    from cuda_audio_amd import _lib

    L = _lib.load()
    q = _query(L)
    assert C.sizeof(_lib.McDecayQuery) == 72 and q.struct_size == 72
    assert (q.rate, q.n_bands, q.curve_points, q.end) == (44100, 0, 0, 0)
    assert q.q == np.float32(1.41421356) and q.onset_db == -20.0 and all(v == 0.0 for v in q.centre_hz)
    rows, curve, info = (C.c_double * 264)(), (C.c_double * (33 * 1024))(), (C.c_uint64 * 2)()
    bad = [("struct_size", dict(struct_size=8)), ("rate", dict(rate=7999)), ("rate", dict(rate=384001)), ("n_bands", dict(n_bands=11)),
           ("curve_points", dict(curve_points=1)), ("curve_points", dict(curve_points=1025)),
           ("centre_hz[1]", dict(n_bands=2, centre_hz=[1000.0, 9.0])), ("centre_hz[0]", dict(n_bands=1, centre_hz=[0.46 * 44100])),
           ("centre_hz[0]", dict(n_bands=1, centre_hz=[float("nan")])), ("q ", dict(q=0.05)), ("q ", dict(q=33.0)), ("q ", dict(q=float("nan"))),
           ("onset_db", dict(onset_db=0.5)), ("onset_db", dict(onset_db=-121.0)), ("onset_db", dict(onset_db=float("nan")))]
    for field, kw in bad:
        # (a null engine behind a bad query: the query is looked at first)
        assert L.mc_ir_decay(None, 0, C.byref(_query(L, **kw)), rows, curve, info) == -1
        assert field.encode() in L.mc_last_error(), (field, L.mc_last_error())
    # centre frequencies past n_bands are not looked at; then the pointers, by name
    unused = _query(L, n_bands=1, centre_hz=[1000.0, 1.0])
    assert L.mc_ir_decay(None, 0, C.byref(unused), rows, curve, info) == -1 and b"null engine" in L.mc_last_error()
    assert L.mc_ir_decay(None, 0, None, rows, curve, info) == -1 and b"null query" in L.mc_last_error()
    L.mc_default_decay_query(None)


def test_decay_for_rt60():
    from cuda_audio_amd.engine import decay_for_rt60

    assert decay_for_rt60(0.25, 0.15, 8000) == 3000
    assert decay_for_rt60(2.0, 1.0, 48000) == 96000
    # the envelope's slope adds: an IR of decay time m shaped with the result decays in t
    m, t, rate = 1.7, 0.9, 44100
    d = decay_for_rt60(m, t, rate)
    assert abs(1.0 / (1.0 / m + rate / d) - t) < 1e-5
    for bad in ((0.25, 0.25), (0.25, 0.3), (0.25, 0.0), (0.25, -0.1), (0.0, 0.1), (float("inf"), 0.1), (0.25, float("nan")),
                (float("nan"), 0.1)):
        with pytest.raises(ValueError):
            decay_for_rt60(*bad, 8000)
