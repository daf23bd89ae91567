"""The decay measurement on the device (mc_ir_decay, csrc/irdecay.hip.h) against the float64 restatement (tests/ir_decay_np.py)
applied to the taps the engine stores (Convolution.ir_taps), and against closed forms.

Tolerances (ir_decay_np.check_against): 1e-6 relative for energy, times, D50 and Ts, 1e-6 dB for C50, C80 and the curve, NaN where
and only where the restatement has NaN.  The chunked recurrence of the bands is within 1.4e-9 relative RMS of the sequential one
at this module's lengths (test_gpu_ir_long_carry.py has a 10 Hz band over 523 264 taps) and non-negative double sums
over at most 4 M terms add 1e-9 at most; the margin over both is test_gpu_ir_eq.py's.  Every comparison asserts first that no level of the restatement lies within 1e-9 dB of an edge of a fit
range (assert_margins)."""
import functools
import math

import numpy as np
import pytest

import ir_decay_np
from ir_decay_np import assert_margins, check_against, decay, noise_ir, sign_ir

pytestmark = pytest.mark.gpu

RATE = 8000
T = 0.25


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irdecay", n_ref, sample_rate=rate, **kw)


def _compare(c, idx, rate, **query):
    """ir_decay of IR idx against the restatement of its stored taps."""
    want = decay(c.ir_taps(idx), rate, **query)
    assert_margins(want)
    got = c.ir_decay(idx, **query)
    check_against(got, want)
    return got, want


def _closed_forms(rows):
    r = 10.0 ** (-6.0 / 2000.0)
    c50 = 10.0 * math.log10((1.0 - r ** 400) / (r ** 400 - r ** 6000))
    ts = r / (1.0 - r) / RATE
    for name in ir_decay_np.SETS:
        row = rows[(0, name)]
        print(name, {k: f"{v:.12g}" for k, v in row.items()})
        for f in ("edt", "t20", "t30"):
            assert abs(row[f] / T - 1.0) <= 1e-6, (name, f, row[f])
        assert abs(row["c50"] - c50) <= 1e-6
        assert abs(row["ts"] / ts - 1.0) <= 1e-6


def test_sign_ir_against_closed_forms(gpu_lib):
    c = _conv(16384)
    c.prepare(0, sign_ir(6000, RATE, T))
    got = c.ir_decay(0, onset_db=0.0)
    assert got["origin"] == 0 and got["taps"] == 6000 and got["curve"] is None
    _closed_forms(got["rows"])
    _compare(c, 0, RATE, onset_db=0.0)
    c.close()


def test_noise_ir_bands_and_curve(gpu_lib):
    c = _conv(16384)
    c.prepare(0, noise_ir(6000, 37, RATE, T, seed=7))
    got, want = _compare(c, 0, RATE, bands=(250, 1000), onset_db=-20.0, curve_points=64)
    c.close()
    assert want["origin"] == 37 and got["origin"] == 37
    assert len(got["rows"]) == 9 and got["curve"].shape == (3, 3, 64)
    assert not np.isnan(got["curve"]).any() and (got["curve"][:, :, 0] == 0.0).all()
    t30 = [got["rows"][(b, "LR")]["t30"] for b in range(3)]
    print("T30 broadband, 250 Hz, 1 kHz:", t30)
    assert all(0.2 < t < 0.3 for t in t30)


@functools.lru_cache(maxsize=None)
def _edge_ir(n, lead):
    """n taps in all: `lead` zeros, then noise that has decayed by 90 dB at the last tap."""
    body = n - lead
    return noise_ir(body, lead, RATE, t60=max(body, 2) / 1.5 / RATE, seed=11 + n % 7)


# 1, 2: shorter than a fit; 255 .. 257: one chunk of the backward sum (and one workgroup of the map kernels) and a tap either
# side; 16385: one workgroup's span of the chunk passes and a tap; 40000: 157 chunks, more than the 128 runs of the bands' carry
# pass, so its runs are longer than one chunk.  end = 33001 and an origin of 300 fall in mid-chunk.
EDGE_CASES = [(16384, 1, 0, 0), (16384, 2, 0, 0), (16384, 255, 0, 0), (16384, 256, 0, 0), (16384, 257, 0, 0), (65536, 16385, 0, 0),
              (65536, 40000, 0, 0), (65536, 40000, 0, 33001), (16384, 4300, 300, 0)]


@pytest.mark.parametrize("n_ref,n,lead,end", EDGE_CASES)
def test_edges_of_the_chunking(gpu_lib, n_ref, n, lead, end):
    c = _conv(n_ref)
    c.prepare(0, _edge_ir(n, lead))
    assert c.ir_info(0)["taps"] == n
    got, want = _compare(c, 0, RATE, bands=(1000,), onset_db=-20.0, end=end, curve_points=17)
    c.close()
    assert got["taps"] == (end or n)
    if lead:
        assert got["origin"] == lead
    if n >= 255:
        assert not math.isnan(got["rows"][(0, "LR")]["t30"]) and not math.isnan(got["rows"][(1, "LR")]["t30"])


def test_a_carry_longer_than_one_tile(gpu_lib):
    """524 588 taps are 2050 chunks: the carry of the backward sum stages 2048 at a time, so its chain crosses a tile border.
    Broadband only: the restatement of these rows is vectorised, a band's is a Python loop over every tap."""
    n = 2048 * 256 + 300
    c = _conv(1048576)
    c.prepare(0, _edge_ir(n, 0))
    assert c.ir_info(0)["taps"] == n
    got, _ = _compare(c, 0, RATE, curve_points=33)
    c.close()
    assert got["taps"] == n and not math.isnan(got["rows"][(0, "LR")]["t30"])


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_the_analysed_taps_are_the_stored_ones(gpu_lib, precision):
    """After conversion, shaping and EQ: the measurement is that of what ir_taps reads."""
    from ir_shape_np import assert_onset_margin, quiet_lead_ir, session_frames
    from test_gpu_ir_eq import LENGTH_BANDS, _ieq, _ishape
    from test_gpu_ir_shape import COMBINED_A

    ir = quiet_lead_ir()
    assert_onset_margin(session_frames(ir, 44100, 48000), 0, COMBINED_A["trim_db"])
    c = _conv(65536, 48000, precision=precision)
    c.prepare(0, ir, ir_rate=44100, shape=_ishape(COMBINED_A), eq=_ieq(LENGTH_BANDS))
    sinfo = c.ir_shape_info(0)
    assert sinfo["eq_bands"] == 2 and sinfo["taps"] > 20000
    got, _ = _compare(c, 0, 48000, bands=(500,), curve_points=32)
    c.close()
    assert got["taps"] == sinfo["taps"]


def test_nothing_is_disturbed(gpu_lib):
    """64 periods, a batch, the stored taps and both infos with ir_decay calls in between, against a run without them."""
    from cuda_audio_amd.engine import IrShape
    from cuda_audio_amd.synth import make_input

    ir = noise_ir(6000, 37, RATE, T, seed=7)
    x = make_input(96 * 256)
    query = dict(bands=(250, 1000), curve_points=64)
    runs = []
    for ask in (False, True):
        c = _conv(16384, max_batch=32)
        c.prepare(0, ir, shape=IrShape(fade_out=100, normalize="peak", target=0.05))
        c.prepare(1, sign_ir(3000, RATE, T) * np.float32(0.01))
        c.cc[1].value.select = 1
        out, asked = [], []
        for k in range(64):
            if ask and k in (0, 32, 33):
                asked.append(c.ir_decay(k % 2, **query))
            out.append(np.stack(c.onProcess(x[0, k * 256:(k + 1) * 256], x[1, k * 256:(k + 1) * 256])))
        if ask:
            asked.append(c.ir_decay(0, **query))
        out.append(c.process(x[0, 64 * 256:], x[1, 64 * 256:]))
        runs.append((np.concatenate(out, axis=1), c.ir_taps(0), c.ir_taps(1), c.ir_info(0), c.ir_info(1), c.ir_shape_info(0)))
        c.close()
    for a, b in zip(*runs):
        if isinstance(a, dict):
            assert a == b
        else:
            np.testing.assert_array_equal(a, b)
    assert np.abs(runs[0][0]).max() > 0.01
    # two calls return identical bytes (calls 0 and 3 asked the same of IR 0, periods apart)
    first, again = asked[0], asked[3]
    assert first["origin"] == again["origin"] and first["taps"] == again["taps"]
    assert first["curve"].tobytes() == again["curve"].tobytes()
    for key, row in first["rows"].items():
        assert np.array(list(row.values())).tobytes() == np.array(list(again["rows"][key].values())).tobytes()


def test_refusals(gpu_lib):
    from cuda_audio_amd._lib import McError

    ir = sign_ir(3000, RATE, T)
    single = _conv(16384, form="single")
    single.prepare(0, ir)
    with pytest.raises(McError) as ex:
        single.ir_decay(0)
    assert ex.value.code == -3
    single.close()
    c = _conv(16384)
    c.prepare(0, ir)
    for idx in (1, 255, 256, 1 << 40):
        with pytest.raises(McError) as ex:
            c.ir_decay(idx)
        assert ex.value.code == -1 and "IR not loaded" in str(ex.value)
    with pytest.raises(McError) as ex:  # (the query comes before the index)
        c.ir_decay(1, curve_points=1)
    assert ex.value.code == -1 and "curve_points" in str(ex.value)
    c.prepare(1, np.zeros((700, 2), np.float32))
    got = c.ir_decay(1, bands=(1000,), curve_points=8)
    assert got["origin"] == 0 and got["taps"] == 700
    for row in got["rows"].values():
        assert row["energy"] == 0.0 and all(math.isnan(row[f]) for f in ir_decay_np.FIELDS[1:])
    assert np.isnan(got["curve"]).all()
    np.testing.assert_array_equal(c.ir_taps(0), ir)
    c.close()


def test_aiming_a_decay_time(gpu_lib):
    """decay_t60 = decay_for_rt60(measured, target) lands an exponential IR on the target; a noisy one on what the restatement
    of the reloaded taps measures (its slope over -5 .. -35 dB is not its mean slope)."""
    from cuda_audio_amd.engine import IrShape, decay_for_rt60

    target = 0.15
    c = _conv(16384)
    ir = sign_ir(6000, RATE, T)
    c.prepare(0, ir)
    t30 = c.ir_decay(0, onset_db=0.0)["rows"][(0, "LR")]["t30"]
    d = decay_for_rt60(t30, target, RATE)
    assert d == 3000
    c.prepare(0, ir, shape=IrShape(decay_t60=d))
    now = c.ir_decay(0, onset_db=0.0)["rows"][(0, "LR")]["t30"]
    print(f"sign IR: measured {t30:.9f} s, decay_t60 {d}, now {now:.9f} s")
    assert abs(now / target - 1.0) <= 1e-6
    noisy = noise_ir(6000, 37, RATE, T, seed=7)
    c.prepare(1, noisy)
    t30 = c.ir_decay(1)["rows"][(0, "LR")]["t30"]
    c.prepare(1, noisy, shape=IrShape(decay_t60=decay_for_rt60(t30, target, RATE)))
    got, want = _compare(c, 1, RATE)
    print(f"noise IR: measured {t30:.6f} s, aimed at {target} s, now {got['rows'][(0, 'LR')]['t30']:.6f} s")
    c.close()
