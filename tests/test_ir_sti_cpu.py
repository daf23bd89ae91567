"""The speech transmission index as tests/ir_sti_np.py states it (no GPU): Schroeder's closed form for an exponential decay, two
spikes, a single tap, noise, the transmission index at its clamps, and the words sti_rating puts on an index."""
import math

import numpy as np
import pytest

from ir_decay_np import sign_ir
from ir_sti_np import ALPHA, BETA, MOD_HZ, f32, rating, schroeder, sti, ti


@pytest.mark.parametrize("rate,n,t60", [(8000, 6000, 0.25), (48000, 24000, 0.5), (48000, 48000, 2.0)])
def test_an_exponential_decay_has_schroeders_closed_form(rate, n, t60):
    """sign_ir has e[m] = r^m (1 + d_m), r = 10^(-6 / (t60 rate)), |d_m| <= 2 2^-24 + 2^-48: a tap is one float32 rounding of its
    value (relative 2^-24) and is squared.  Numerator and denominator of m are sums of e with weights of modulus <= 1, so each
    moves by at most 2 2^-24 = 1.2e-7 relative to E, and m by at most twice that, 2.4e-7.  The roundings are not all of one
    sign, and the difference seen is below 1e-9."""
    res = sti(sign_ir(n=n, rate=rate, t60=t60), rate, bands=(), alpha=(), beta=(), onset_db=0.0)
    assert res["origin"] == 0 and res["taps"] == n
    r = 10.0 ** (-6.0 / (t60 * rate))
    want = schroeder(r, n, [f32(F) for F in MOD_HZ], rate)
    for s in range(3):
        diff = float(np.max(np.abs(res["mtf"][0, s] - want)))
        print(f"set {s}: largest difference from the closed form {diff:.2e}")
        assert diff <= 2.4e-7
    assert all(math.isnan(v) for v in res["sti"].values())  # (no bands: no index)


def test_two_spikes_are_a_comb():
    """Taps 1 at frames 0 and d: C + jS = 1 + e^(j theta_d), E = 2, m = |cos(pi F d / rate)|.  rate 48000 and d = 1920 put a
    zero on 12.5 Hz: theta_d = pi."""
    rate, d = 48000, 1920
    ir = np.zeros((4000, 2), np.float32)
    ir[0] = ir[d] = 1.0
    res = sti(ir, rate, bands=(), alpha=(), beta=(), onset_db=0.0)
    want = np.abs(np.cos(np.pi * np.array([f32(F) for F in MOD_HZ]) * d / rate))
    assert np.max(np.abs(res["mtf"][0] - want[None, :])) <= 1e-14
    assert f32(MOD_HZ[-1]) == 12.5 and res["mtf"][0, 0, -1] <= 1e-14 and ti(res["mtf"][0, 0, -1]) == 0.0
    assert res["rows"][(0, "L")]["energy"] == 2.0 and res["rows"][(0, "LR")]["energy"] == 4.0


def test_a_single_tap_transmits_everything():
    """One tap at the origin: every broadband sum is the tap's square and m = 1 at every F.  Behind a band filter the tap
    rings for a few periods of the centre, so the seven bands are put at 6 .. 18 kHz, where that is well under a millisecond:
    m(12.5 Hz) >= 1 - (2 pi 12.5 0.001)^2 / 2 = 0.997, above the upper clamp 0.969, every TI is 1 and the index with the default
    weights is sum alpha - sum beta = 1."""
    ir = np.zeros((4800, 2), np.float32)
    ir[0] = (0.5, -0.25)
    res = sti(ir, 48000, bands=tuple(6000.0 + 2000.0 * b for b in range(7)), alpha=ALPHA, beta=BETA, onset_db=0.0)
    assert np.array_equal(res["mtf"][0], np.ones((3, len(MOD_HZ))))
    assert np.min(res["mtf"]) >= 0.997
    assert all(row["mti"] == 1.0 and row["status"] == 0 for row in res["rows"].values())
    assert all(abs(v - 1.0) <= 1e-12 for v in res["sti"].values())
    assert abs(sum(ALPHA) - sum(BETA) - 1.0) <= 1e-12


def test_noise_halves_and_leaves_alone():
    ir = sign_ir(n=4000, rate=48000, t60=0.3)
    bands = (500.0, 1000.0, 2000.0)
    kw = dict(bands=bands, alpha=(0.3, 0.4, 0.5), beta=(0.1, 0.1), onset_db=0.0)
    clean = sti(ir, 48000, **kw)
    half = sti(ir, 48000, snr_db=(0.0,) * 3, **kw)
    quiet = sti(ir, 48000, snr_db=(120.0,) * 3, **kw)
    assert np.array_equal(half["mtf"][0], clean["mtf"][0]) and np.array_equal(quiet["mtf"][0], clean["mtf"][0])  # (broadband: no noise)
    assert np.max(np.abs(half["mtf"][1:] - 0.5 * clean["mtf"][1:])) <= 1e-15
    assert np.max(np.abs(quiet["mtf"][1:] - clean["mtf"][1:])) <= 1e-12
    assert all(half["sti"][s] < clean["sti"][s] for s in ("L", "R", "LR"))
    assert all(abs(quiet["sti"][s] - clean["sti"][s]) <= 1e-12 for s in ("L", "R", "LR"))


def test_the_transmission_index_is_continuous_at_its_clamps():
    lo, hi = 1.0 / (1.0 + 10.0 ** 1.5), 1.0 / (1.0 + 10.0 ** -1.5)  # m / (1 - m) = 10^-1.5 and 10^1.5: -15 and +15 dB
    # a step of at most 1e-9 in m moves TI by at most 5e-9 (dTI/dm <= 5 inside the clamps)
    assert ti(lo * (1 - 1e-9)) == 0.0 and 0.0 <= ti(lo * (1 + 1e-9)) <= 5e-9
    assert ti(hi * (1 + 1e-9)) == 1.0 and 0.0 <= 1.0 - ti(hi * (1 - 1e-9)) <= 5e-9
    assert abs(ti(0.5) - 0.5) <= 1e-15
    assert ti(1.0) == 1.0 and ti(1.0 + 1e-12) == 1.0 and ti(math.nextafter(1.0, 0.0)) == 1.0
    assert ti(0.0) == 0.0 and ti(-1e-12) == 0.0 and ti(5e-324) == 0.0
    grid = np.linspace(0.0, 1.0, 20001)
    v = np.array([ti(m) for m in grid])
    assert np.all(np.diff(v) >= 0.0) and np.max(np.diff(v)) <= 5.0 * (grid[1] - grid[0]) + 1e-12  # (dTI/dm <= 5 inside the clamps)


def test_a_silent_channel_has_a_status_and_no_index():
    ir = sign_ir(n=2000, rate=48000, t60=0.2)
    ir[:, 1] = 0.0
    res = sti(ir, 48000, bands=(1000.0,), alpha=(1.0,), beta=(), onset_db=0.0)
    for g in (0, 1):
        assert res["rows"][(g, "R")] == dict(energy=0.0, mti=res["rows"][(g, "R")]["mti"], status=1) and math.isnan(res["rows"][(g, "R")]["mti"])
        assert np.isnan(res["mtf"][g, 1]).all() and np.array_equal(res["mtf"][g, 0], res["mtf"][g, 2])
    assert math.isnan(res["sti"]["R"]) and res["sti"]["L"] == res["sti"]["LR"]


def test_custom_bands_need_weights():
    with pytest.raises(ValueError):
        sti(np.ones((8, 2), np.float32), 48000, bands=(1000.0,))


def test_the_rating_at_its_edges():
    from cuda_audio_amd.engine import sti_rating

    for v, word in ((0.0, "bad"), (0.2999, "bad"), (0.30, "poor"), (0.4499, "poor"), (0.45, "fair"), (0.5999, "fair"), (0.60, "good"), (0.7499, "good"),
                    (0.75, "excellent"), (1.0, "excellent"), (-0.1, "bad")):
        assert sti_rating(v) == word == rating(v), (v, word)
    with pytest.raises(ValueError):
        sti_rating(float("nan"))
