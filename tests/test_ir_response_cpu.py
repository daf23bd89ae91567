"""The float64 restatement of the frequency response (tests/ir_response_np.py) against what is known without it: numpy's FFT at bin
frequencies, closed forms of one and two spikes, the shape restatement's fade, and the properties of the grid and of the smoothing
(no GPU, no library)."""
import numpy as np

from ir_iacc_np import pair_ir
from ir_response_np import check_against, grid, neighbours, response, smooth, span, weights
from ir_shape_np import shape64

RATE = 48000


def test_the_restatement_against_the_fft_at_bin_frequencies():
    """rate 48000, 4096 taps: bin k is k 11.71875 Hz, an exact float, and rfft's e^(-j 2 pi k m / 4096) is the definition's kernel
    with the origin at tap 0.  Held to 1e-12 A."""
    ir = pair_ir(4096, rate=RATE, seed=11)
    bins = np.array([0, 1, 2, 3, 17, 100, 512, 1000, 2047, 2048])
    hz = (bins * 11.71875).astype(np.float32)
    assert np.array_equal(hz.astype(np.float64), bins * 11.71875)
    got = response(ir, RATE, hz, onset_db=0.0)
    assert got["origin"] == 0 and got["taps"] == 4096 and got["spans"].tolist() == [[0, 4096]]
    for c, name in enumerate("LR"):
        want = np.fft.rfft(ir[:, c].astype(np.float64))[bins]
        A = got["rows"][(0, name)]["abs_sum"]
        assert A == float(np.sum(np.abs(ir[:, c].astype(np.float64))))
        assert np.max(np.abs(got["h"][0, c] - want)) <= 1e-12 * A
        assert abs(got["rows"][(0, name)]["energy"] - float(np.sum(ir[:, c].astype(np.float64) ** 2))) <= 1e-12
    assert np.array_equal(got["db"], 20.0 * np.log10(np.abs(got["h"]))) and np.array_equal(got["phase"], np.angle(got["h"]))


def test_one_spike_and_two():
    """A spike d taps after the origin: |H| = 1 and the group delay is d at every frequency.  Two unit spikes d apart:
    |H| = 2 |cos(pi F d / rate)|."""
    hz = np.array([0.0, 20.0, 63.5, 1000.0, 2500.5, 9999.9, 24000.0], np.float32)
    for d in (0, 1, 37, 1023, 1024, 1025):
        ir = np.zeros((d + 50, 2), np.float32)
        ir[0, 0], ir[d, 1] = 0.5, 0.25  # (L at the origin, R d taps later)
        got = response(ir, RATE, hz, onset_db=-6.0)
        assert got["origin"] == 0
        assert np.max(np.abs(np.abs(got["h"][0, 1]) - 0.25)) <= 1e-15 and np.max(np.abs(got["delay"][0, 1] - d)) <= 1e-9
        assert np.array_equal(got["h"][0, 0], np.full(hz.size, 0.5 + 0j)) and not got["delay"][0, 0].any()
    for d in (1, 37, 1023, 1025):
        ir = np.zeros((d + 50, 2), np.float32)
        ir[0] = ir[d] = 1.0
        got = response(ir, RATE, hz[:-1], onset_db=0.0)
        comb = 2.0 * np.abs(np.cos(np.pi * (np.fmod(hz[:-1].astype(np.float64) * d, RATE) / RATE)))
        assert np.max(np.abs(np.abs(got["h"][0, 0]) - comb)) <= 1e-14
        assert np.max(np.abs(got["delay"][0, 0] - d / 2.0)) <= 1e-9  # (two equal spikes: linear phase about their middle)
        assert got["rows"][(0, "L")] == dict(energy=2.0, abs_sum=2.0, status=0)


def test_windows_clip_and_their_edges_are_the_shaped_loads_fade():
    assert span(None, 5, 100) == (5, 100, 0, 0)
    assert span((10, 20, 3, 4), 5, 100) == (15, 35, 3, 4)
    assert span((10, 200, 3, 4), 5, 100) == (15, 100, 3, 4)
    assert span((95, 0, 0, 0), 5, 100) == (100, 100, 0, 0) and span((500, 7, 9, 9), 5, 100) == (100, 100, 0, 0)
    assert span((0, 10, 8, 8), 0, 100) == (0, 10, 8, 2) and span((0, 10, 10, 1), 0, 100) == (0, 10, 10, 0) and span((0, 10, 99, 0), 0, 100) == (0, 10, 10, 0)
    # the fall is ir_shape_np's fade, bit for bit, and the rise is its mirror image to the last place but one
    x = np.ones((300, 2), np.float32)
    for f in (1, 2, 17, 300):
        faded = shape64(x, 300, fade_out=f)[0][:, 0]
        assert np.array_equal(weights(300, 0, f), faded)
        assert np.max(np.abs(weights(300, f, 0) - faded[::-1])) <= 2.0 ** -52
    u = weights(100, 30, 50)
    assert np.all(u[30:50] == 1.0) and np.all(np.diff(u[:31]) > 0) and np.all(np.diff(u[49:]) < 0) and 0.0 < u[0] < u[29] < 1.0 and 0.0 < u[-1] < 1.0
    # a windowed response is the response of the weighted taps
    ir = pair_ir(900, lead=12, rate=RATE, seed=4)
    hz = np.array([100.0, 2500.5], np.float32)
    got = response(ir, RATE, hz, windows=[(7, 400, 30, 50), None, (900, 0, 0, 0)])
    o = got["origin"]
    assert o >= 12 and got["spans"].tolist() == [[o + 7, o + 407], [o, 912], [912, 912]]
    weighted = np.zeros_like(ir)
    weighted[o + 7:o + 407] = (ir[o + 7:o + 407].astype(np.float64) * weights(400, 30, 50)[:, None]).astype(np.float32)
    plain = response(weighted, RATE, hz, windows=[(o + 7, 400, 0, 0)], onset_db=0.0)
    k = o  # (plain's origin is 0: its phase and delay are counted o taps earlier)
    turn = np.exp(2j * np.pi * hz.astype(np.float64) * k / RATE)
    assert np.max(np.abs(plain["h"][0] * turn[None, :] - got["h"][0])) <= 1e-6 * got["rows"][(0, "L")]["abs_sum"]  # (float32 weights)
    assert got["rows"][(2, "L")] == dict(energy=0.0, abs_sum=0.0, status=1) and np.isnan(got["delay"][2]).all() and not got["h"][2].any()
    assert (got["db"][2] == -400.0).all()
    check_against(got, got)


def test_grid_and_smooth():
    hz = grid(20.0, 20000.0, 24)
    assert hz.dtype == np.float32 and hz[0] == 20.0 and hz[24] == 40.0 and hz[-1] <= 20000.0 and np.all(np.diff(hz) > 0)
    assert hz.size == 240 and grid(20.0, 20.0, 1).tolist() == [20.0] and grid(1000.0, 8000.0, 1).tolist() == [1000.0, 2000.0, 4000.0, 8000.0]
    assert np.max(np.abs(hz.astype(np.float64) / (20.0 * 2.0 ** (np.arange(240) / 24.0)) - 1.0)) <= 2.0 ** -24
    rng = np.random.default_rng(5)
    power = rng.random(240)
    assert smooth(hz, power, 0.0).tobytes() == power.tobytes()
    flat = smooth(hz, np.full(240, 0.3), 1.0)
    assert np.max(np.abs(flat - 0.3)) <= 1e-15
    # The neighbours of an interior point of a 24-per-octave grid over one octave: 12 below, itself, 12 above = 25.  The two
    # outermost of them sit on the interval's edges, hz[f] 2^(+-1/2), to the rounding of the float32 grid (2^-24 relative), which
    # puts each of them in or out: exactly one octave counts 23 to 25 (24 everywhere on this grid), and an octave wider by 2^-20 (under a thousandth of the
    # grid's step, sixteen times the rounding) counts 25 everywhere.
    def counts(octaves):
        return np.count_nonzero(neighbours(hz, octaves), axis=1).tolist()

    wide, exact = counts(1.0 + 2.0 ** -20), counts(1.0)
    print("interior counts at exactly one octave:", {c: exact[13:-13].count(c) for c in sorted(set(exact[13:-13]))})
    assert set(wide[13:-13]) == {25} and wide[0] == 13 and wide[-1] == 13
    assert set(exact[13:-13]) <= {23, 24, 25}
    spike = np.zeros(240)
    spike[100] = 25.0
    out = smooth(hz, spike, 1.0 + 2.0 ** -20)
    assert np.all(out[88:113] == 1.0) and not out[:88].any() and not out[113:].any()
