"""The frequency response on the device (mc_ir_response, csrc/irresponse.hip.h) against the float64 restatement
(tests/ir_response_np.py) applied to the taps the engine stores (Convolution.ir_taps).

Tolerances (ir_response_np.check_against; its docstring has the derivation), derived, not measured, with u = 2^-53 and n_w the
window's taps:
  * Re H and Im H to (n_w + 3.3 STRETCH + 16) u A, A = sum |u x|; D to the same with A_D = sum (m - o) |u x|;
  * the group delay to 2 (tol_D + |tau| tol_H) / |H| wherever |H| >= 1000 tol_H; no case here may skip a point (a window without
    taps or without sound has status 1 and is compared exactly: H = 0, NaN delay);
  * E and A to n_w u relative; origin, N, spans and status equal; NaN where and only where the restatement has it.
The largest differences seen are printed as fractions of these bounds."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

from ir_iacc_np import pair_ir
from ir_response_np import FT, RUN, STRETCH, check_against, response

pytestmark = pytest.mark.gpu

RATE = 48000
HZ6 = (0.0, 20.0, 63.5, 1000.0, 2500.5, 9999.9)
HZ7 = HZ6 + (24000.0,)   # 0 and rate / 2 exactly; 2500.5 and 9999.9 are no short binary fractions of the rate
WATERFALL = [(64 * k, 256, 16, 64) for k in range(64)]


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irresponse", n_ref, sample_rate=rate, **kw)


def _compare(c, idx, rate, skips=0, **query):
    """ir_response of IR idx against the restatement of its stored taps."""
    want = response(c.ir_taps(idx), rate, **query)
    got = c.ir_response(idx, **query)
    check_against(got, want, skips=skips)
    return got, want


@functools.lru_cache(maxsize=None)
def _pair(n, lead=0, seed=7, t60=0.25):
    return pair_ir(n=n, lead=lead, rate=RATE, t60=t60, seed=seed)


def _spikes(d):
    """L: unit spikes at the origin and d taps later (a comb); R: one spike of a half, d taps after the origin."""
    ir = np.zeros((d + 300, 2), np.float32)
    ir[0, 0] = ir[d, 0] = 1.0
    ir[d, 1] = 0.5
    return ir


def _silent_r(n):
    ir = _pair(n).copy()
    ir[:, 1] = 0.0
    return ir


def _spread(n):
    return np.linspace(0.0, RATE / 2.0, n).astype(np.float32)


# (n_ref, the IR, query): the smallest shapes that reach every branch of the kernel and its launch
CASES = {
    "N = 1": (16384, lambda: _pair(1), dict(hz=HZ7, onset_db=0.0)),
    "N under a stretch": (16384, lambda: _pair(STRETCH - 7), dict(hz=HZ7, onset_db=0.0)),
    "N = RUN - 1": (16384, lambda: _pair(RUN - 1), dict(hz=HZ7, onset_db=0.0)),
    "N = RUN": (16384, lambda: _pair(RUN), dict(hz=HZ7, onset_db=0.0)),
    "N = RUN + 1": (16384, lambda: _pair(RUN + 1), dict(hz=HZ7, onset_db=0.0)),
    "N = 2 RUN + 1": (16384, lambda: _pair(2 * RUN + 1), dict(hz=HZ7, onset_db=0.0)),
    "origin in mid-run": (16384, lambda: _pair(6000, lead=300), dict(hz=HZ7)),
    "end in mid-run": (16384, lambda: _pair(3000), dict(hz=HZ7, end=RUN + 405, onset_db=0.0)),
    "n_freq = 1": (16384, lambda: _pair(600), dict(hz=(1000.0,))),
    "n_freq = FT - 1": (16384, lambda: _pair(600), dict(hz=_spread(FT - 1))),
    "n_freq = FT": (16384, lambda: _pair(600), dict(hz=_spread(FT))),
    "n_freq = FT + 1": (16384, lambda: _pair(600), dict(hz=_spread(FT + 1))),
    "n_freq = 1024": (16384, lambda: _pair(600), dict(hz=_spread(1024))),
    "0 and rate / 2": (16384, lambda: _pair(3000, lead=37), dict(hz=(0.0, 24000.0))),
    "window across run borders": (16384, lambda: _pair(6000, lead=37), dict(hz=HZ7, windows=[(1000, 2100, 50, 70), (1023, 2, 0, 0), (0, 1025, 0, 1)])),
    "rise + fall > L": (16384, lambda: _pair(6000, lead=37), dict(hz=HZ7, windows=[(100, 300, 200, 200)])),
    "rise = L": (16384, lambda: _pair(6000, lead=37), dict(hz=HZ7, windows=[(100, 300, 300, 50), (100, 300, 4000, 0)])),
    "windows at N and beyond": (16384, lambda: _pair(3000), dict(hz=HZ7, onset_db=0.0, windows=[(3000, 0, 0, 0), (0, 500, 0, 0), (3005, 10, 3, 3), (1 << 62, 1 << 62, 9, 9)])),
    "waterfall": (16384, lambda: _pair(6000), dict(hz=HZ7, windows=WATERFALL)),
    "spikes RUN - 1 apart": (16384, lambda: _spikes(RUN - 1), dict(hz=HZ6, onset_db=0.0)),
    "spikes RUN apart": (16384, lambda: _spikes(RUN), dict(hz=HZ6, onset_db=0.0)),
    "spikes RUN + 1 apart": (16384, lambda: _spikes(RUN + 1), dict(hz=HZ6, onset_db=0.0)),
    "silent R": (16384, lambda: _silent_r(3000), dict(hz=HZ7, windows=[None, (10, 100, 5, 5)])),
    "all zero": (16384, lambda: np.zeros((3000, 2), np.float32), dict(hz=HZ7)),
    "long carry": (524288, lambda: _pair(300000, t60=4.0), dict(hz=HZ7 + (12345.678,))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_restatement(gpu_lib, case):
    n_ref, make, query = CASES[case]
    ir = make()
    c = _conv(n_ref)
    c.prepare(0, ir)
    assert c.ir_info(0)["taps"] == len(ir)
    got, want = _compare(c, 0, RATE, **query)
    c.close()
    rows, n_win = got["rows"], len(query.get("windows", [None]))
    assert got["taps"] == (query.get("end") or len(ir))
    assert got["h"].shape == got["delay"].shape == got["db"].shape == got["phase"].shape == (n_win, 2, len(query["hz"]))
    if case == "N = 1":
        x = ir[0].astype(np.float64)
        assert got["origin"] == 0 and np.array_equal(got["h"][0], np.repeat(x[:, None], 7, axis=1) + 0j) and not got["delay"].any()
        assert rows[(0, "L")] == dict(energy=x[0] * x[0], abs_sum=abs(x[0]), status=0)
    if case == "origin in mid-run":
        assert got["origin"] >= 300 and got["spans"].tolist() == [[got["origin"], 6300]]
    if case == "end in mid-run":
        assert got["spans"].tolist() == [[0, RUN + 405]]
    if case == "window across run borders":
        o = got["origin"]
        assert got["spans"].tolist() == [[o + 1000, o + 3100], [o + 1023, o + 1025], [o, o + 1025]]
    if case == "rise + fall > L":
        assert want["spans"].tolist() == [[got["origin"] + 100, got["origin"] + 400]]
    if case == "rise = L":
        assert got["h"][0].tobytes() == got["h"][1].tobytes() and got["delay"][0].tobytes() == got["delay"][1].tobytes()  # (both clamp to 300, 0)
    if case == "windows at N and beyond":
        assert got["spans"].tolist() == [[3000, 3000], [0, 500], [3000, 3000], [3000, 3000]]
        assert [rows[(w, s)]["status"] for w in range(4) for s in "LR"] == [1, 1, 0, 0, 1, 1, 1, 1]
        assert not got["h"][[0, 2, 3]].any() and np.isnan(got["delay"][[0, 2, 3]]).all() and (got["db"][[0, 2, 3]] == -400.0).all()
    if case.startswith("spikes"):
        d = len(ir) - 300
        comb = 2.0 * np.abs(np.cos(np.pi * (np.fmod(np.array(HZ6, np.float32).astype(np.float64) * d, RATE) / RATE)))
        assert np.max(np.abs(np.abs(got["h"][0, 0]) - comb)) <= 1e-13
        assert np.max(np.abs(np.abs(got["h"][0, 1]) - 0.5)) <= 1e-13 and np.max(np.abs(got["delay"][0, 1] - d)) <= 1e-9
        assert rows[(0, "L")] == dict(energy=2.0, abs_sum=2.0, status=0) and rows[(0, "R")] == dict(energy=0.25, abs_sum=0.5, status=0)
    if case == "silent R":
        assert all(rows[(w, "R")] == dict(energy=0.0, abs_sum=0.0, status=1) and rows[(w, "L")]["status"] == 0 for w in range(2))
        assert not got["h"][:, 1].any() and np.isnan(got["delay"][:, 1]).all() and not np.isnan(got["delay"][:, 0]).any()
    if case == "all zero":
        assert all(r == dict(energy=0.0, abs_sum=0.0, status=1) for r in rows.values()) and not got["h"].any() and np.isnan(got["delay"]).all()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _bits(res, w=slice(None), f=slice(None)):
    return (res["h"][w, :, f].tobytes(), res["delay"][w, :, f].tobytes())


def _all_bits(res):
    return _bits(res) + (np.array([list(r.values()) for r in res["rows"].values()], np.float64).tobytes(), res["spans"].tobytes(), res["origin"], res["taps"])


def test_a_frequency_and_a_window_do_not_depend_on_the_others(gpu_lib):
    """2500.5 Hz asked alone, as entry 0 of 300 and as entry 299 of 300 (the second slice of the grid) gives the same bytes, and so
    does window 3 of the waterfall asked alone: rows and spans too."""
    ir = _pair(6000)
    c = _conv(16384)
    c.prepare(0, ir)
    others = np.linspace(30.0, 23000.0, 299).astype(np.float32)
    alone = c.ir_response(0, hz=(2500.5,))
    first = c.ir_response(0, hz=np.concatenate([[np.float32(2500.5)], others]))
    last = c.ir_response(0, hz=np.concatenate([others, [np.float32(2500.5)]]))
    assert _bits(alone) == _bits(first, f=slice(0, 1)) == _bits(last, f=slice(299, 300))
    assert _bits(first, f=slice(1, 300)) == _bits(last, f=slice(0, 299))
    assert alone["rows"] == first["rows"] == last["rows"]
    fall = c.ir_response(0, hz=HZ7, windows=WATERFALL)
    one = c.ir_response(0, hz=HZ7, windows=[WATERFALL[3]])
    pair = c.ir_response(0, hz=HZ7, windows=[None, WATERFALL[3]])
    c.close()
    assert _bits(one) == _bits(fall, w=slice(3, 4)) == _bits(pair, w=slice(1, 2))
    assert one["rows"][(0, "L")] == fall["rows"][(3, "L")] == pair["rows"][(1, "L")] and one["rows"][(0, "R")] == fall["rows"][(3, "R")]
    assert one["spans"][0].tolist() == fall["spans"][3].tolist() == [one["origin"] + 192, one["origin"] + 448]


def test_nothing_is_disturbed_and_two_calls_agree(gpu_lib):
    """The stored taps and ir_info are byte for byte the same before and after, a processed batch with calls in between is that of a
    run without them, and two calls return the same bits in h, delay, rows and spans."""
    from cuda_audio_amd.synth import make_input

    ir = _pair(6000, lead=37)
    x = make_input(32 * 256)
    runs, asked = [], []
    for ask in (False, True):
        c = _conv(16384, max_batch=32)
        c.prepare(0, ir)
        before = (c.ir_taps(0).tobytes(), c.ir_info(0))
        if ask:
            asked.append(c.ir_response(0, hz=HZ7, windows=WATERFALL[:5]))
            assert (c.ir_taps(0).tobytes(), c.ir_info(0)) == before
        first = c.process(x[0, :16 * 256], x[1, :16 * 256])
        if ask:
            asked.append(c.ir_response(0, hz=HZ7, windows=WATERFALL[:5]))
            asked.append(c.ir_response(0))
        second = c.process(x[0, 16 * 256:], x[1, 16 * 256:])
        runs.append((_sha(c.ir_taps(0)), _sha(first), _sha(second), c.ir_info(0)))
        c.close()
    assert runs[0] == runs[1]
    assert _all_bits(asked[0]) == _all_bits(asked[1])
    assert (asked[0]["origin"], asked[0]["taps"]) == (38, 6037)
    from cuda_audio_amd.engine import response_grid

    assert np.array_equal(asked[2]["hz"], response_grid(20.0, 20000.0, 24)) and asked[2]["h"].shape == (1, 2, 240)  # (hz=None: the default grid)


def _raw(c, idx, hz=(100.0, 1000.0, 24000.0), resp=True, rows=True, spans=True, info=True, **fields):
    """mc_ir_response with the struct's fields set directly; returns (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    q = _lib.McResponseQuery()
    L.mc_default_response_query(C.byref(q))
    q.rate, q.n_freq = RATE, 3
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(q, k)[j] = x
        else:
            setattr(q, k, v)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    h = None if hz is None else np.array(hz, np.float32)
    r, w, s, i = np.zeros(2 * 3 * 3), np.zeros(8), np.zeros(2, np.uint64), (C.c_uint64 * 2)()
    rc = L.mc_ir_response(c._h, idx, C.byref(q), None if h is None else h.ctypes.data_as(C.POINTER(C.c_float)), None, r.ctypes.data_as(dp) if resp else None,
                          w.ctypes.data_as(dp) if rows else None, s.ctypes.data_as(up) if spans else None, i if info else None)
    return rc, L.mc_last_error().decode()


NAN = float("nan")
BAD = [("struct_size", dict(struct_size=36)), ("rate", dict(rate=7999)), ("n_freq 0 outside [1, 1024]", dict(n_freq=0)), ("n_freq", dict(n_freq=1025)),
       ("n_win", dict(n_win=0)), ("n_win", dict(n_win=65)), ("flags", dict(flags=1)), ("onset_db", dict(onset_db=1.0)), ("reserved", dict(reserved=(0, 1))),
       ("hz[0]", dict(hz=(NAN, 1.0, 2.0))), ("hz[1]", dict(hz=(0.0, -1.0, 2.0))), ("hz[2]", dict(hz=(0.0, 1.0, 24001.0))), ("null win", dict(n_win=2))]


def test_refusals(gpu_lib):
    from cuda_audio_amd._lib import McError

    ir = _pair(3000)
    single = _conv(16384, form="single")
    single.prepare(0, ir)
    with pytest.raises(McError) as ex:
        single.ir_response(0, hz=HZ7)
    assert ex.value.code == -3
    single.close()
    c = _conv(16384)
    c.prepare(0, ir)
    before = c.ir_response(0, hz=HZ7)
    for idx in (1, 255, 256, 1 << 40):
        with pytest.raises(McError) as ex:
            c.ir_response(idx, hz=HZ7)
        assert ex.value.code == -1 and "IR not loaded" in str(ex.value)
    for idx in (0, 1):  # the query, the frequencies, then the pointers, come before the index
        for name, fields in BAD:
            rc, msg = _raw(c, idx, **fields)
            assert rc == -1 and name in msg, (name, rc, msg)
        names = ("hz", "resp", "rows", "spans", "info")
        for k, name in enumerate(names):
            rc, msg = _raw(c, idx, **{n: (None if n == "hz" else False) for n in names[k:]})
            assert rc == -1 and "null " + name in msg, (name, rc, msg)
    with pytest.raises(ValueError):
        c.ir_response(0, hz=np.zeros(1025, np.float32))
    with pytest.raises(ValueError):
        c.ir_response(0, hz=())
    with pytest.raises(ValueError):
        c.ir_response(0, hz=HZ7, windows=[None] * 65)
    with pytest.raises(McError):
        c.ir_response(0, hz=(30000.0,))
    assert _raw(c, 0)[0] == 0
    np.testing.assert_array_equal(c.ir_taps(0), ir)
    assert _all_bits(c.ir_response(0, hz=HZ7)) == _all_bits(before)  # the engine still answers, with the same bits
    c.close()


EQ_BANDS = (("lowcut", 120), ("peak", 2500, 6.0, 1.5))
EQ_CPU_DB = 9.43e-6


def test_an_equalised_impulse_reads_as_eq_response_predicts(gpu_lib):
    """A unit impulse of 16384 frames loaded with a low cut at 120 Hz and a 6 dB peak at 2500 Hz is the filter's impulse response,
    truncated and rounded to float32, so its measured level follows eq_response's curve.  On three points per octave from 20 Hz to
    20 kHz the restatement of tests/ir_eq_np.py's taps differs from eq_response by at most 9.43e-6 dB (at 20 Hz, 31 dB down, where
    the rounding of the taps weighs most; measured on the CPU when this test was written); the margin is four times that,
    3.77e-5 dB.  The restatement is held to it here on the CPU first; then the device equals the restatement of its own stored
    taps to the derived bounds, and reads as eq_response predicts within the margin."""
    import ir_eq_np
    from cuda_audio_amd.engine import IrEq, eq_response, response_grid

    hz = response_grid(20.0, 20000.0, 3)
    eq = IrEq(bands=list(EQ_BANDS))
    predicted = eq_response(eq, RATE, hz)
    taps = ir_eq_np.impulse_taps(EQ_BANDS, RATE, 16384)
    want = response(np.stack([taps, taps], axis=1), RATE, hz, onset_db=0.0)
    dev = float(np.max(np.abs(want["db"][0] - predicted[None, :])))
    print(f"restatement: largest deviation from eq_response {dev:.3e} dB")
    assert dev <= 4.0 * EQ_CPU_DB
    impulse = np.zeros((16384, 2), np.float32)
    impulse[0] = 1.0
    c = _conv(16384)
    c.prepare(0, impulse, eq=eq)
    got, _ = _compare(c, 0, RATE, hz=hz, onset_db=0.0)
    c.close()
    print(f"device: largest deviation from eq_response {float(np.max(np.abs(got['db'][0] - predicted[None, :]))):.3e} dB")
    assert np.max(np.abs(got["db"][0] - predicted[None, :])) <= 4.0 * EQ_CPU_DB
