"""The spring's definition without a GPU: the library's plan and response (host arithmetic) against the float64 restatement (a)
of tests/ir_spring_np.py, (a) against the independent time recursion (b) within the plan's alias bound, the alias identity of
the radius, and the closed-form group delay of the first echo."""
import numpy as np
import pytest

import ir_response_np
import ir_spring_np as sp

RATE = 8000

# (frames, fields): the loops of the issue's small cases, then the low-pass, the high loop and two springs
CASES = {
    "short loop": (700, sp.loop_fields(RATE, 3, 7, 0.62, 40, -0.8, damping=0.3)),
    "slow decay": (700, sp.loop_fields(RATE, 5, 30, 0.62, 20, -0.95, damping=0.2)),
    "low-pass": (600, sp.loop_fields(RATE, 4, 9, 0.5, 33, -0.7, damping=0.1, lowpass_order=6)),
    "high loop": (600, sp.loop_fields(RATE, 2, 6, 0.55, 61, -0.6, damping=0.25, high_gain=0.3, high_sections=11, high_dispersion=-0.5, high_delay=0.4,
                                      high_t60=0.02)),
    "two springs": (800, dict(sp.loop_fields(RATE, 3, 5, 0.6, 50, -0.7, damping=0.2, lowpass_order=2, stereo=0.07, gain=0.5), delay_ms=(7.0, 9.5))),
}


def _spring(fields):
    from cuda_audio_amd.engine import IrSpring

    return IrSpring(**fields)


@pytest.mark.parametrize("name", list(CASES) + ["default"])
def test_the_plan_and_the_response_match_the_restatement(name):
    from cuda_audio_amd.engine import spring_plan, spring_response

    frames, fields = CASES.get(name, (96000, {}))
    rate = RATE if name in CASES else 48000
    want = sp.spring_plan64(rate, frames, **fields)
    got = spring_plan(_spring(fields), rate, frames)
    print(name, got)
    assert (got["points"], got["stretch"], got["springs"], got["sections"], got["lowpass"], got["last"]) == (want["N"], want["K"], want["S"], want["M"],
                                                                                                               bool(want["bq"]), want["E"])
    assert got["transition"] == want["ft"] and got["delay"] == [tuple(v) for v in want["L"]]
    np.testing.assert_allclose(np.array(got["loop_gain"]), np.array(want["g"]), rtol=1e-14)
    assert abs(got["alias_db"] - want["alias_db"]) <= 1e-9 * abs(want["alias_db"])
    hz = np.concatenate([[0.0, rate / 2.0, 1.0], np.linspace(20.0, rate / 2.0 - 20.0, 61)])
    H, W = spring_response(_spring(fields), rate, hz), sp.spring_response64(rate, hz, **fields)
    err = np.abs(H - W).max() / np.abs(W).max()
    print(f"response: max |H| {np.abs(W).max():.3f}, deviation {err:.2e}")
    # M + M_h complex products of about 3 ulp each, the loop's 1 / (1 - |g|) on top: far below this
    assert err <= 1e-10
    assert np.all(H[0].imag == 0)  # real at 0 Hz


def test_the_issues_loops_are_the_ones_asked_for():
    a = sp.spring_plan64(RATE, 700, **CASES["short loop"][1])
    assert (a["K"], a["M"], a["L"][0], a["c"]) == (3, 7, [40, 40], sp.f32(0.3)) and abs(a["g"][0][0] + 0.8) < 1e-6
    b = sp.spring_plan64(RATE, 700, **CASES["slow decay"][1])
    assert (b["K"], b["M"], b["L"][0]) == (5, 30, [20, 20]) and abs(b["g"][0][0] + 0.95) < 1e-6


@pytest.mark.parametrize("name", list(CASES))
def test_the_frequency_form_is_the_time_recursion_within_the_alias_bound(name):
    frames, fields = CASES[name]
    got, plan = sp.spring64(RATE, frames, **fields)
    want = sp.recursion64(RATE, frames, **fields)
    err = np.abs(got - want).max()
    print(f"{name}: N {plan['N']}, alias bound {plan['alias']:.2e}, max |a - b| {err:.2e}, peak {np.abs(want).max():.3f}")
    assert np.abs(want).max() > 0.05
    assert err <= plan["alias"] + 1e-9


def test_the_alias_identity_of_the_radius():
    """With N forced to 1024 and a loop that has hardly decayed by then, (a)[t] = sum_m (b)[t + 1024 m] 1e-8^m."""
    fields = dict(sp.loop_fields(RATE, 3, 7, 0.62, 40, -0.97, damping=0.1, stereo=0.1), log2_points=10)
    got, plan = sp.spring64(RATE, 500, **fields)
    assert plan["N"] == 1024
    h = sp.recursion64(RATE, 4096, **fields)
    folded = sum(h[1024 * m:1024 * m + 500] * 1e-8 ** m for m in range(4))
    wrap = np.abs(h[1024:1524]).max() * 1e-8
    err_plain, err = np.abs(got - h[:500]).max(), np.abs(got - folded).max()
    print(f"first wrap {wrap:.2e} (bound {plan['alias']:.2e}); |a - h| {err_plain:.2e}, |a - folded| {err:.2e}")
    assert wrap <= plan["alias"]
    assert err_plain > 0.2 * wrap  # the wrap is there ...
    assert err <= 1e-11            # ... and is what the identity says: what is left is rounding (the fifth term is below 1e-40)


def test_the_group_delay_of_the_first_echo_is_the_closed_form():
    """g = 0: one echo.  The measurement of tests/ir_response_np.py on (a)'s taps against L + M K (1 - a^2) / (1 + 2 a cos(w K) + a^2)."""
    M, K, a, L = 20, 2, 0.5, 400
    fields = sp.loop_fields(RATE, K, M, a, L, 0.0)
    taps, plan = sp.spring64(RATE, 1024, **fields)
    assert plan["L"][0] == [L, L]
    first, last = L + M * K * (1 - a) / (1 + a), L + M * K * (1 + a) / (1 - a)
    assert (round(first), round(last)) == (413, 520)
    energy = (taps[:, 0] ** 2).sum()
    print(f"energy {energy:.6f}, outside [413, 700): {(taps[:413, 0] ** 2).sum() + (taps[700:, 0] ** 2).sum():.2e}")
    assert abs(energy - 1.0) < 1e-6  # all-pass
    hz = np.array([100.0, 300.0, 600.0, 900.0, 1200.0, 1500.0, 1800.0], np.float32)  # below f_t = 2000
    r = ir_response_np.response(taps.astype(np.float32), RATE, hz, windows=[(300, 400, 0, 0)], onset_db=0.0)
    want = sp.group_delay_closed(2 * np.pi * hz.astype(np.float64) / RATE, L, M, K, sp.f32(a))
    got = r["delay"][0, 0] + 0.0  # (onset_db 0: the origin is tap 0, and delays count from it)
    print("closed form", np.round(want, 3), "measured", np.round(got, 3), "difference", np.round(got - want, 4))
    assert np.abs(got - want).max() <= GROUP_DELAY_MARGIN


# The echo starts at frame 400 (a^M of it; the lows follow at 413) and the window [300, 700) leaves 3e-26 of its energy out, so
# the measured delay is the closed form up to the taps' rounding to float32.  Measured by the test above on the restatement
# (CPU): at most 2.9e-6 frames over the seven frequencies.  1e-4 frames allows for the window's edges and for taps that round
# the other way; tests/test_gpu_ir_spring.py holds the device to the same margin.
GROUP_DELAY_MARGIN = 1e-4


# One spring without damping, t60 2 s, 4 s at 8 kHz, with a short cascade (20 sections, K = 2, a = 0.5)
DECAY_FIELDS = dict(sections=20, transition_hz=2000.0, dispersion=0.5, delay_ms=(66.0,), t60=2.0, damping=0.0, stereo=0.0, high_gain=0.0, lowpass_order=0)
DECAY_FRAMES = 4 * RATE
# Measured by the test below on the restatement (CPU): T30 = 2.1346 s, 0.1346 s from t60_s.  Two things move it: the Schroeder
# curve of an echo train is a staircase, and the loop gain is per round trip while the round trip grows with frequency (515 frames
# and the cascade's 13 at 0 Hz to 120 at f_t), so the highs decay more slowly per second.  0.15 s allows for the staircase's
# steps moving by a frame; tests/test_gpu_ir_spring.py holds the device to the same margin.
DECAY_MARGIN = 0.15


def test_the_decay_time_of_the_restatement():
    import ir_decay_np

    taps, plan = sp.spring64(RATE, DECAY_FRAMES, **DECAY_FIELDS)
    assert plan["L"][0] == [515, 515] and abs(plan["g"][0][0] + 10.0 ** (-3 * 0.066 / 2.0)) < 1e-7
    row = ir_decay_np.decay(taps.astype(np.float32), RATE)["rows"][(0, "L")]
    print(f"T30 {row['t30']:.4f} s, T20 {row['t20']:.4f} s, EDT {row['edt']:.4f} s")
    assert abs(row["t30"] - 2.0) <= DECAY_MARGIN
    # without the cascade the round trip is the same at every frequency and only the staircase is left
    taps, _ = sp.spring64(RATE, DECAY_FRAMES, **dict(DECAY_FIELDS, sections=0))
    t30 = ir_decay_np.decay(taps.astype(np.float32), RATE)["rows"][(0, "L")]["t30"]
    print(f"no cascade: T30 {t30:.4f} s")
    assert abs(t30 - 2.0) < 0.02
