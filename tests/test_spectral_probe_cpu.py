"""The probe measure of tests/spectral_probe.py proved on the oracle alone (no GPU): a healthy stand-in for the engine - the
oracle's window rounded to float32 - reads far below the bar the GPU tests use, faults planted at single bins read far above
it, and the first of them passes the whole-signal and per-block bars the suite had until now: the gap the probes close."""
import functools

import numpy as np
import pytest

from helpers import BASE, RMS_TOL, _dry, rms
from spectral_probe import AMP, DC, N_OS, NOISE_AMP, SEED, SMALL_BINS, check_bins, describe, probe_errors, probe_stream, q, tone

N_REF, P16, WIN = 8192, 32, 16384  # the small tier of test_gpu_spectral_probe.py
HOP = 16384 - P16
NB = P16 + 400 + 2 * HOP
P0, P1 = dict(BASE, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)
GPU_BAR = 1e-4  # test_gpu_spectral_probe.py asserts worst <= this


@functools.lru_cache(maxsize=1)
def _window():
    """The oracle's last 16384 blocks of the plain probe stream, the dry mix there, the healthy stand-in and its measure."""
    import oracle
    from cuda_audio_amd.synth import make_ir

    x = probe_stream(NB * 256, SMALL_BINS, N_OS, AMP, NOISE_AMP, DC, SEED)
    u = oracle.Upols(N_REF, True)
    u.prepare(0, make_ir(7000, seed=11, norm=0.02))
    u.prepare(1, make_ir(6500, seed=22, norm=0.02))
    u.set(0, **P0)
    u.set(1, **P1)
    want = u.range(x[0], x[1], NB - WIN, WIN)
    u.close()
    dry = _dry(x[:, (NB - WIN) * 256:], P0, P1)
    healthy = want.astype(np.float32)
    for a in (want, dry, healthy):
        a.setflags(write=False)
    return want, dry, healthy, probe_errors(healthy, want, dry, SMALL_BINS, N_OS)


def _planted(lines):
    """The healthy stand-in plus exact tones: {bin: complex amplitude added to the line of L + j R there}."""
    want, dry, healthy, r0 = _window()
    got = healthy.astype(np.float64)
    for b, a in lines.items():
        t = tone(b, N_OS, 0, N_OS, a)
        got[0] += t.real
        got[1] += t.imag
    return probe_errors(got, want, dry, SMALL_BINS, N_OS, Ww=r0["Ww"])


def test_collisions_are_refused():
    for pair in ([1, q(511, 8191)], [256, q(256, 8191)], [5, 5], [0], [N_OS]):
        with pytest.raises(ValueError):
            check_bins(pair, N_OS)
    check_bins([N_OS // 2, 1], N_OS)
    with pytest.raises(ValueError):
        probe_stream(1024, [1, N_OS - 1], N_OS, AMP, NOISE_AMP, DC, SEED)


def test_each_probe_is_one_line():
    """Without the carrier, bin q of z = in1 + j in2 holds the probe and bin N - q nothing; mirrored, the other way round;
    a tone far into a stream keeps its phase (the product q n is reduced in integers)."""
    N, bins = 4096, [3, 700, 2048]
    for mirror in (False, True):
        x = probe_stream(3 * N + 5, bins, N, 1.0, 0.0, 0.0, SEED, mirror=mirror).astype(np.float64)
        Z = np.fft.fft(x[0, 2 * N:3 * N] + 1j * x[1, 2 * N:3 * N]) / N
        hot = [N - b if mirror else b for b in bins]
        assert np.allclose(np.abs(Z[hot]), 1.0, atol=1e-6)
        Z[hot] = 0
        assert np.abs(Z).max() < 1e-6
    big = 4 * N_OS + 2  # a bin near N: q n reaches 2^46
    t = tone(N_OS - 1, N_OS, big, 4)
    assert np.allclose(t, np.exp(-2j * np.pi * (np.arange(4) + 2) / N_OS), atol=1e-12)


def test_the_oracle_meets_the_conditions_the_gpu_tests_rely_on():
    want, dry, healthy, r = _window()
    wet = want - dry
    print(describe(r), f"; wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert r["floor"] >= 0.1
    assert np.abs(wet).max() < 0.5
    assert rms(want) > 0.01
    assert r["worst"] <= 1e-6  # float32 rounding of the output alone


def test_a_three_percent_error_at_one_bin_passes_the_old_bars_and_fails_the_probe():
    """A line of typical height (0.53 S; the heights run from 0.13 S to 2.5 S): 3 % of it is 7e-6 RMS spread over the window."""
    b = q(255, 1)
    Ww = _window()[3]["Ww"]
    r = _planted({b: 0.03 * Ww[b]})
    print(describe(r), f"; the line is {abs(Ww[b]) / r['S']:.2f} S")
    assert r["rms"] <= RMS_TOL and r["worst_block"] <= 2 * RMS_TOL  # the gap: neither bar of the suite sees it
    assert r["worst"] > 10 * GPU_BAR and r["bin"] == b and (r["k1"], r["k2"]) == (255, 1)


def test_exchanged_partner_lines_fail_the_probe():
    b = q(64, 77)
    Ww = _window()[3]["Ww"]
    r = _planted({b: Ww[N_OS - b] - Ww[b], N_OS - b: Ww[b] - Ww[N_OS - b]})
    print(describe(r))
    assert r["worst"] > 10 * GPU_BAR and r["bin"] in (b, N_OS - b)


@pytest.mark.parametrize("b", [q(0, 4080), q(256, 4095)], ids=["row0", "row256"])
def test_a_conjugated_line_in_a_self_paired_row_fails_the_probe(b):
    Ww = _window()[3]["Ww"]
    r = _planted({b: np.conj(Ww[b]) - Ww[b]})
    print(describe(r))
    assert r["worst"] > 10 * GPU_BAR and r["bin"] == b
