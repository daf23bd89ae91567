"""The chunked recurrences of the IR tools (csrc/chunkwalk.hip.h, carry_scan of csrc/ireq.hip.h: EQ, damping, the tail step, the
floor search, the decay measurement) at lengths where a run of the carry pass is three chunks and more, and with bands whose
carry matrices are ill-conditioned: where the other modules stop at 40 000 taps (157 chunks, K = 2).  Every case is one load or
one query against the module's own sequential float64 restatement (ir_eq_np, ir_damp_np, ir_tail_np, ir_floor_np, ir_decay_np)
with that module's own check and bar; nothing is new but the shapes.  The input is noise that falls 60 dB over its length, loaded
at the session's rate.  tests/ir_chunk_np.py states the scheme in numpy and tests/test_ir_chunk_cpu.py runs it without a device.

Geometry (48 kHz, n_ref 131072, well-conditioned filters: a failure is an indexing fault):
  65 793 taps   258 chunks and a tap into the last, K = 3, 86 runs and 42 idle lanes in the carry, 5 workgroups;
  130 048 taps  508 chunks, K = 4, exactly 127 runs: the 128th is empty.
Conditioning (384 kHz, n_ref 524288, 523 264 taps: 2044 chunks, K = 16, a last run of 12 chunks): 10 Hz bands, the
worst-conditioned the limits allow.  524288 is the smallest power-of-two n_ref at which the numpy model puts the low cut and
the peak, with carry matrices raised in double, over the bar of 1e-6 relative RMS over all taps (the low cut: 1.8e-7 at 131072,
5.6e-7 at 262144, 3.9e-6 here; over the last eighth alone it is over the bar at 131072 already, 8.4e-6, and the high cut is
over all taps at 262144, 1.7e-6).  Besides the module's check over all taps, the same bar is held over the last eighth of the
taps alone, where an error of the carry shows (the float rounding of a stored tap is relative, 2.5e-8, and does not eat the bar
there).  tests/test_ir_chunk_cpu.py checks every restatement used here against
the same loop in extended precision: all lie within a tenth of their bar, over all taps and over the last eighth, the 10 Hz
decay band's late curve points included (1.5e-9 dB), so the restatement is the reference throughout.

Relative RMS of the stored taps against the restatement, all taps / last eighth.  "model": tests/ir_chunk_np.py on the host
(emulated, no fused multiply-adds); "device": an MI355X (measured), before = carry matrices raised in double (ieq_matpow, up to
the commit that added this module), after = raised in long double and rounded once (carry_powers).

  case                          model, double      model, long double   device, before     device, after
  low cut 10 Hz q 32            3.9e-6 / 1.3e-4    6.3e-9 / 2.1e-7      3.9e-6 / 1.3e-4    2.6e-8 / 2.0e-7
  peak 10 Hz +24 dB q 32        1.3e-6 / 1.9e-4    6.0e-10 / 9.7e-8     1.3e-6 / 1.9e-4    2.5e-8 / 9.7e-8
  high cut 10 Hz                7.6e-7 / 1.1e-6    2.4e-9 / 3.4e-9      7.6e-7 / 1.1e-6    2.5e-8 / 2.6e-8
  the three in one load         1.3e-4 / 1.9e-4    5.3e-8 / 5.9e-8      1.3e-4 / 1.9e-4    5.5e-8 / 6.2e-8
  peak 172.8 kHz -36 dB q 0.1   6.0e-16 / 5.8e-16  5.8e-16 / 5.9e-16    2.5e-8 / 2.5e-8    2.5e-8 / 2.5e-8
  damping, 10 Hz crossover      1.2e-8 / 2.5e-6    3.4e-11 / 7.7e-9     2.4e-8 / 2.6e-8    2.4e-8 / 2.6e-8
The device's figures hold the float rounding of the stored taps (2.5e-8), the model's do not.  Before, the low cut, the peak and
the three in one load failed over all taps and over the last eighth, the high cut over the last eighth alone; after, every case
passes.  The band at the top edge is well-conditioned, and the damping's 4 x 4 matrices were raised in long double before as
well: their two device columns are the same arithmetic.  The model had predicted every device figure to its two digits.
The decay of a 10 Hz band (largest differences of check_against: relative, curve in dB):
  model, double       energy 1.6e-5, edt 7.9e-6, c50 7.5e-5 dB, curve 2.7e-4 dB
  model, long double  energy 1.4e-8, edt 5.5e-9, c50 5.9e-8 dB, curve 1.4e-7 dB
  device, before      energy 1.6e-5, edt 7.9e-6, c50 7.5e-5 dB, curve 2.7e-4 dB   (fails)
  device, after       energy 1.4e-8, edt 5.8e-9, c50 6.1e-8 dB, curve 1.2e-7 dB"""
import functools

import numpy as np
import pytest

import ir_damp_np
import ir_decay_np
import ir_eq_np
import ir_floor_np
import ir_tail_np
from helpers import rms
from ir_chunk_np import COND_BANDS, COND_DAMP, COND_DECAY, COND_N, COND_N_REF, COND_RATE, falling_noise
from test_gpu_ir_eq import LENGTH_BANDS, _check_eq_info
from test_gpu_ir_shape import _check_taps

pytestmark = pytest.mark.gpu

NFRAMES = 1024
GEO_RATE, GEO_N_REF = 48000, 131072
GEO_LENGTHS = (65793, 130048)
XOVERS3 = (250, 2000, 8000)


def _conv(n_ref, rate):
    from cuda_audio_amd.engine import Convolution

    return Convolution("longcarry", n_ref, sample_rate=rate, stream_threshold=8, max_batch=8)


@functools.lru_cache(maxsize=None)
def noisy_falling(n, rate):
    """The same over a floor 50 dB down, after 37 taps of silence: n taps in all."""
    ir = ir_floor_np.noisy_ir(n - 37, 37, rate, t60=(n - 37) / rate, floor_db=-50.0, seed=3 + n % 5, noise_seed=17 + n % 3)
    ir.setflags(write=False)
    return ir


def _check_taps_and_late(label, got, want64):
    """_check_taps over all taps, then its relative RMS bar over the last eighth alone."""
    n = len(want64)
    late = slice(n - n // 8, n)
    err = got.astype(np.float64) - want64

    def rel(part):  # (a cut tail is zero from its last knee on: then the stored taps must be zero too, and 0 / 0 prints as 0)
        e, w = rms(err[part]), rms(want64[part])
        return e / w if w else (np.inf if e else 0.0)

    print(f"{label}: relative rms {rel(slice(None)):.2e} over all taps, {rel(late):.2e} over the last eighth")
    _check_taps(got, want64)
    assert rms(err[late]) <= 1e-6 * rms(want64[late]), f"last eighth: rms {rms(err[late]):.3e} vs {rms(want64[late]):.3e}"


# -- geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", GEO_LENGTHS)
def test_eq_geometry(gpu_lib, n):
    from cuda_audio_amd.engine import IrEq

    ir = falling_noise(n, GEO_RATE)
    want, winfo = ir_eq_np.eq64(ir, GEO_N_REF - NFRAMES, None, GEO_RATE, LENGTH_BANDS)
    assert winfo["taps"] == n
    c = _conv(GEO_N_REF, GEO_RATE)
    c.prepare(0, ir, eq=IrEq(bands=list(LENGTH_BANDS)))
    got, sinfo = c.ir_taps(0), c.ir_shape_info(0)
    c.close()
    _check_taps_and_late(f"eq {n}", got, want)
    _check_eq_info(sinfo, winfo)


@pytest.mark.parametrize("n", GEO_LENGTHS)
def test_damping_geometry(gpu_lib, n):
    from cuda_audio_amd.engine import IrDamp

    decay, origin = (20000, 9000, 6000, 2500), 300  # (test_gpu_ir_damp.LENGTH_DAMP; the origin in mid-chunk)
    ir = falling_noise(n, GEO_RATE)
    want, winfo, wdinfo = ir_damp_np.damp64(ir, GEO_N_REF - NFRAMES, None, GEO_RATE, XOVERS3, decay, origin)
    assert winfo["taps"] == n and wdinfo == dict(xovers=3, origin=origin, damped_bands=4)
    c = _conv(GEO_N_REF, GEO_RATE)
    c.prepare(0, ir, damp=IrDamp(xovers=XOVERS3, decay=decay, origin=origin))
    got, sinfo, dinfo = c.ir_taps(0), c.ir_shape_info(0), c.ir_damp_info(0)
    c.close()
    _check_taps_and_late(f"damping {n}", got, want)
    _check_eq_info(sinfo, winfo)
    assert dinfo == wdinfo


# end = 100001: 391 chunks in mid-chunk, K = 4, 98 runs, the last of them three chunks long
@pytest.mark.parametrize("n,end", [(65793, 0), (130048, 100001)])
def test_decay_geometry(gpu_lib, n, end):
    query = dict(bands=(1000,), onset_db=-20.0, end=end, curve_points=17)
    c = _conv(GEO_N_REF, GEO_RATE)
    c.prepare(0, falling_noise(n, GEO_RATE))
    want = ir_decay_np.decay(c.ir_taps(0), GEO_RATE, **query)
    ir_decay_np.assert_margins(want)
    got = c.ir_decay(0, **query)
    c.close()
    assert got["taps"] == (end or n)
    ir_decay_np.check_against(got, want)
    assert not np.isnan(got["rows"][(1, "LR")]["t30"])


@pytest.mark.parametrize("n", GEO_LENGTHS)
def test_floor_geometry(gpu_lib, n):
    c = _conv(GEO_N_REF, GEO_RATE)
    c.prepare(0, noisy_falling(n, GEO_RATE))
    want = ir_floor_np.floor(c.ir_taps(0), GEO_RATE, xovers=XOVERS3)
    ir_floor_np.assert_margins(want)
    got = c.ir_floor(0, xovers=XOVERS3)
    c.close()
    assert got["taps"] == n and got["origin"] == 37 and got["groups"] == 5
    ir_floor_np.check_against(got, want)
    assert got["rows"][(0, "LR")]["status"] == 0


def _tail_spec(X, knee, length):
    bands = X + 1
    return dict(xovers=XOVERS3[:X], knee=tuple(knee + 7 * j for j in range(bands)), t60=tuple(knee - 11 * j for j in range(bands)),
                level_db=tuple((-42.0 - 3.0 * j, -44.5 + 2.0 * j) for j in range(bands)), fade=32, length=length, seed=12345, width=0.75)


# extend: 70 000 frames to 130 048 taps, the noise alone past the recording; cut: 130 048 frames
@pytest.mark.parametrize("mode,X,frames,length", [("extend", 0, 70000, 130048), ("extend", 3, 70000, 130048), ("cut", 3, 130048, 0)])
def test_tail_geometry(gpu_lib, mode, X, frames, length):
    from cuda_audio_amd.engine import IrTail

    ir = noisy_falling(frames, GEO_RATE)
    spec = _tail_spec(X, frames // 2, length)
    want, winfo = ir_tail_np.tail64(ir, GEO_RATE, mode, **spec)
    assert winfo == dict(bands=X + 1, frames=frames, length=length or frames, first=frames // 2 - 32)
    c = _conv(GEO_N_REF, GEO_RATE)
    c.prepare(0, ir, tail=IrTail(mode=mode, **spec))
    got, tinfo = c.ir_taps(0), c.ir_tail_info(0)
    c.close()
    assert tinfo == winfo, (tinfo, winfo)
    _check_taps_and_late(f"tail {mode} X = {X}", got, want)
    np.testing.assert_array_equal(got[:winfo["first"]], ir[:winfo["first"]])
    if length > frames:
        assert np.count_nonzero(got[frames:]) > 2 * (length - frames) - 10


# -- conditioning ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cond_eq_want(name):
    want, winfo = ir_eq_np.eq64(falling_noise(COND_N, COND_RATE), COND_N, None, COND_RATE, COND_BANDS[name])
    want.setflags(write=False)
    return want, winfo


@functools.lru_cache(maxsize=None)
def cond_damp_want():
    xovers, decay, origin = COND_DAMP
    want, winfo, wdinfo = ir_damp_np.damp64(falling_noise(COND_N, COND_RATE), COND_N, None, COND_RATE, xovers, decay, origin)
    want.setflags(write=False)
    return want, winfo, wdinfo


@pytest.mark.parametrize("name", list(COND_BANDS))
def test_eq_conditioning(gpu_lib, name):
    from cuda_audio_amd.engine import IrEq

    want, winfo = cond_eq_want(name)
    assert winfo["taps"] == COND_N and winfo["eq_bands"] == len(COND_BANDS[name])
    c = _conv(COND_N_REF, COND_RATE)
    c.prepare(0, falling_noise(COND_N, COND_RATE), eq=IrEq(bands=list(COND_BANDS[name])))
    got, sinfo = c.ir_taps(0), c.ir_shape_info(0)
    c.close()
    _check_taps_and_late(f"eq {name}", got, want)
    _check_eq_info(sinfo, winfo)


def test_damping_conditioning(gpu_lib):
    from cuda_audio_amd.engine import IrDamp

    xovers, decay, origin = COND_DAMP
    want, winfo, wdinfo = cond_damp_want()
    assert winfo["taps"] == COND_N and wdinfo == dict(xovers=1, origin=origin, damped_bands=1)
    c = _conv(COND_N_REF, COND_RATE)
    c.prepare(0, falling_noise(COND_N, COND_RATE), damp=IrDamp(xovers=xovers, decay=decay, origin=origin))
    got, sinfo, dinfo = c.ir_taps(0), c.ir_shape_info(0), c.ir_damp_info(0)
    c.close()
    _check_taps_and_late("damping 10 Hz", got, want)
    _check_eq_info(sinfo, winfo)
    assert dinfo == wdinfo


def test_decay_conditioning(gpu_lib):
    c = _conv(COND_N_REF, COND_RATE)
    c.prepare(0, falling_noise(COND_N, COND_RATE))
    taps = c.ir_taps(0)
    np.testing.assert_array_equal(taps, falling_noise(COND_N, COND_RATE))  # (a plain load: what test_ir_chunk_cpu.py checked)
    want = ir_decay_np.decay(taps, COND_RATE, **COND_DECAY)
    ir_decay_np.assert_margins(want)
    got = c.ir_decay(0, **COND_DECAY)
    c.close()
    assert got["taps"] == COND_N and got["curve"].shape == (2, 3, 33)
    ir_decay_np.check_against(got, want)
    assert not np.isnan(got["rows"][(1, "LR")]["edt"])
