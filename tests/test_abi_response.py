"""mc_response_query and mc_response_window as ctypes sees them against what include/mcconv.h documents, the defaults field by
field, every bad field, frequency and null pointer refused in the documented order before the engine is looked at, and the two
host-arithmetic entry points against the restatement, bit for bit (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np

from ir_response_np import FT, MAX_FREQ, MAX_WIN, RUN, STRETCH, grid, smooth

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")


def _default():
    from cuda_audio_amd import _lib

    q = _lib.McResponseQuery()
    _lib.load().mc_default_response_query(C.byref(q))
    return q


def test_the_structs_have_their_documented_sizes():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_response_query\) = (\d+)", src).group(1))
    assert C.sizeof(_lib.McResponseQuery) == size == _default().struct_size == 40
    assert C.sizeof(_lib.McResponseWindow) == int(re.search(r"mc_response_window;\s*/\* sizeof = (\d+)", src).group(1)) == 24
    assert int(re.search(r"#define MC_RSP_MAX_FREQ (\d+)", src).group(1)) == _lib.MC_RSP_MAX_FREQ == MAX_FREQ
    assert int(re.search(r"#define MC_RSP_MAX_WIN (\d+)", src).group(1)) == _lib.MC_RSP_MAX_WIN == MAX_WIN
    assert {"mc_default_response_query", "mc_ir_response", "mc_response_grid", "mc_response_smooth"} <= set(_lib.SYMBOLS)
    # the kernel's geometry as the restatement's tolerances and the GPU cases mirror it
    kernel = open(os.path.join(os.path.dirname(HEADER), "..", "cuda_audio_amd", "csrc", "irresponse.hip.h")).read()
    assert int(re.search(r"constexpr int RSP_RUN = (\d+);", kernel).group(1)) == RUN
    assert int(re.search(r"constexpr int RSP_STRETCH = (\d+);", kernel).group(1)) == STRETCH
    assert re.search(r"constexpr int RSP_FT = ISH_THREADS;", kernel) and FT == 256


def test_the_defaults_field_by_field():
    q = _default()
    assert (q.rate, q.n_freq, q.n_win, q.flags, q.onset_db, q.end, list(q.reserved)) == (44100, 0, 1, 0, -20.0, 0, [0, 0])


def _query(**fields):
    q = _default()
    q.rate, q.n_freq = 48000, 3
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(q, k)[j] = x
        else:
            setattr(q, k, v)
    return q


def _call(q, hz=(100.0, 1000.0, 24000.0), win=None, resp=True, rows=True, spans=True, info=True, engine=None):
    from cuda_audio_amd import _lib

    L = _lib.load()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    h = None if hz is None else np.array(tuple(hz) + (0.0,) * (MAX_FREQ - len(hz)), np.float32)
    r, w, s, i = np.zeros(MAX_WIN * 2 * MAX_FREQ * 3), np.zeros(MAX_WIN * 8), np.zeros(MAX_WIN * 2, np.uint64), (C.c_uint64 * 2)()
    rc = L.mc_ir_response(engine, 0, C.byref(q) if q is not None else None, None if h is None else h.ctypes.data_as(C.POINTER(C.c_float)), win,
                          r.ctypes.data_as(dp) if resp else None, w.ctypes.data_as(dp) if rows else None, s.ctypes.data_as(up) if spans else None,
                          i if info else None)
    return rc, L.mc_last_error().decode()


NAN = float("nan")
BAD_FIELDS = [("struct_size", dict(struct_size=36)), ("rate", dict(rate=7999)), ("rate", dict(rate=384001)), ("n_freq 0 outside [1, 1024]", dict(n_freq=0)),
              ("n_freq 1025", dict(n_freq=1025)), ("n_win 0", dict(n_win=0)), ("n_win 65", dict(n_win=65)), ("flags", dict(flags=1)),
              ("onset_db", dict(onset_db=1.0)), ("onset_db", dict(onset_db=NAN)), ("onset_db", dict(onset_db=-121.0)), ("reserved", dict(reserved=(1, 0))),
              ("reserved", dict(reserved=(0, 1)))]


def test_every_field_is_refused_before_the_engine_is_looked_at():
    rc, msg = _call(None)
    assert rc == -1 and "null query" in msg
    for name, fields in BAD_FIELDS:
        rc, msg = _call(_query(**fields))
        assert rc == -1 and name in msg, (name, fields, rc, msg)
    # in the struct's order: of two bad fields the earlier one is named; a bad field comes before a bad frequency and a null pointer
    order = [("rate", dict(rate=1)), ("n_freq", dict(n_freq=5000)), ("n_win", dict(n_win=99)), ("flags", dict(flags=4)), ("onset_db", dict(onset_db=5.0)),
             ("reserved", dict(reserved=(7, 7)))]
    for (first, a), (_, b) in zip(order, order[1:]):
        rc, msg = _call(_query(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    for name, fields in order:
        rc, msg = _call(_query(**fields), hz=(NAN, 1.0, 2.0), resp=False)
        assert rc == -1 and name in msg, (name, msg)
        rc, msg = _call(_query(**fields), hz=None)
        assert rc == -1 and name in msg, (name, msg)


def test_every_frequency_then_the_pointers_in_order():
    for f, bad in ((0, NAN), (1, -1.0), (2, 24001.0), (0, float("inf")), (2, -0.5)):
        hz = [100.0, 1000.0, 24000.0]
        hz[f] = bad
        rc, msg = _call(_query(), hz=tuple(hz), resp=False, rows=False)
        assert rc == -1 and f"hz[{f}]" in msg and "outside [0, 24000]" in msg, (f, bad, msg)
    rc, msg = _call(_query(rate=44100), hz=(0.0, 22050.0, 22051.0))
    assert rc == -1 and "hz[2]" in msg
    # frequencies past n_freq are not looked at; the edges 0 and rate / 2 pass and the call stops at the engine
    for fields, hz in ((dict(n_freq=2), (0.0, 24000.0, NAN)), (dict(n_freq=1024), (24000.0,) * 1024), (dict(n_win=64, end=1, onset_db=0.0), (1.0, 2.0, 3.0)),
                       (dict(onset_db=-120.0), (1.0, 2.0, 3.0))):
        win = None
        if fields.get("n_win", 1) > 1:
            from cuda_audio_amd import _lib

            win = (_lib.McResponseWindow * 64)()
        rc, msg = _call(_query(**fields), hz=hz, win=win)
        assert rc == -1 and "null engine" in msg, (fields, msg)
    names = ("hz", "resp", "rows", "spans", "info")
    for k, name in enumerate(names):  # every pointer from `name` on is null: `name` is the one that is named
        args = {n: (None if n == "hz" else False) for n in names[k:]}
        rc, msg = _call(_query(), **args)
        assert rc == -1 and "null " + name in msg, (name, msg)
    rc, msg = _call(_query(n_win=2), resp=False)  # (windows may be null for one window alone)
    assert rc == -1 and "null win" in msg, msg


def test_the_grid_and_the_smoothing_are_the_restatements_bit_for_bit():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import response_grid, smooth_response, waterfall_windows

    L = _lib.load()
    for lo, hi, per in ((20.0, 20000.0, 24), (20.0, 20000.0, 3), (31.5, 16000.0, 1), (10.0, 0.45 * 44100, 96), (20.0, 0.45 * 8000, 24), (0.001, 1.0, 7), (440.0, 440.0, 12)):
        want = grid(lo, hi, per)
        got = response_grid(lo, hi, per)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (lo, hi, per)
        buf = np.zeros(want.size, np.float32)
        assert L.mc_response_grid(lo, hi, per, buf.ctypes.data_as(C.POINTER(C.c_float)), want.size) == want.size and buf.tobytes() == want.tobytes()
        assert L.mc_response_grid(lo, hi, per, buf.ctypes.data_as(C.POINTER(C.c_float)), want.size - 1) == -1 and "cap" in L.mc_last_error().decode()
    buf = np.zeros(8, np.float32)
    for lo, hi, per in ((0.0, 100.0, 3), (-1.0, 100.0, 3), (200.0, 100.0, 3), (NAN, 100.0, 3), (20.0, float("inf"), 3), (20.0, 100.0, 0), (20.0, 100.0, 97)):
        assert L.mc_response_grid(lo, hi, per, buf.ctypes.data_as(C.POINTER(C.c_float)), 8) == -1, (lo, hi, per)
    assert L.mc_response_grid(20.0, 100.0, 3, None, 8) == -1 and "null hz" in L.mc_last_error().decode()

    rng = np.random.default_rng(9)
    for hz in (grid(20.0, 20000.0, 24), grid(20.0, 20000.0, 5), np.sort(rng.uniform(0.0, 24000.0, 301)).astype(np.float32),
               np.array([0.0, 0.0, 1.0, 1.0, 1.0, 2.0], np.float32), np.array([1000.0], np.float32)):
        power = rng.random(hz.size) * 10.0 ** rng.uniform(-6, 2, hz.size)
        for octaves in (0.0, 1.0 / 24, 1.0 / 3, 1.0, 1.0 + 2.0 ** -20, 3.0, 10.0):
            got = smooth_response(hz, power, octaves)
            assert got.tobytes() == smooth(hz, power, octaves).tobytes(), (hz.size, octaves)
            if octaves == 0.0:
                assert got.tobytes() == power.tobytes()
    hz, power, out = grid(20.0, 20000.0, 3), np.ones(30), np.zeros(30)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)

    def raw(h, p, n, octaves, o):
        rc = L.mc_response_smooth(None if h is None else h.ctypes.data_as(fp), None if p is None else p.ctypes.data_as(dp), n, octaves,
                                  None if o is None else o.ctypes.data_as(dp))
        return rc, L.mc_last_error().decode()

    assert raw(hz, power, 30, 1.0, out)[0] == 0 and raw(hz, power, 0, 1.0, out)[0] == 0
    for args, name in (((None, power, 30, 1.0, out), "null hz"), ((hz, None, 30, 1.0, out), "null power"), ((hz, power, 30, 1.0, None), "null out"),
                       ((hz, power, 30, -0.1, out), "octaves"), ((hz, power, 30, 10.5, out), "octaves"), ((hz, power, 30, NAN, out), "octaves"),
                       ((hz[::-1].copy(), power, 30, 1.0, out), "hz[1]"), ((np.array([1.0, NAN], np.float32), power, 2, 1.0, out), "hz[1]"),
                       ((np.array([-1.0, 2.0], np.float32), power, 2, 1.0, out), "hz[0]")):
        rc, msg = raw(*args)
        assert rc == -1 and name in msg, (name, rc, msg)
    assert waterfall_windows(3, 64, 256, 16, 64) == [(0, 256, 16, 64), (64, 256, 16, 64), (128, 256, 16, 64)]
