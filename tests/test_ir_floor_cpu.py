"""The noise-floor search as tests/ir_floor_np.py states it (no GPU): the knee lands on the analytic crossing of a decay and a
stationary floor, the late decay time is the IR's, the three statuses appear where they should, the margins of the discrete
decisions are reported, and mc_ir_tail_from_floor (host arithmetic in the library) agrees with its restatement."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import ir_floor_np
from ir_decay_np import noise_ir
from ir_floor_np import FIELDS, assert_margins, floor, noisy_ir

RATE = 8000
XOVERS = (400, 1600)


@functools.lru_cache(maxsize=None)
def _case(n, t60, floor_db, xovers=()):
    return floor(noisy_ir(n, 37, RATE, t60, floor_db=floor_db), RATE, xovers=xovers)


@pytest.mark.parametrize("n,t60,floor_db", [(6000, 0.25, -50.0), (6000, 0.25, -40.0), (6000, 0.25, -60.0), (12000, 0.5, -45.0), (3000, 0.1, -55.0)])
def test_the_knee_is_where_the_decay_meets_the_floor(n, t60, floor_db):
    res = _case(n, t60, floor_db)
    assert_margins(res)
    row = res["rows"][(0, "LR")]
    crossing = 37 + (-floor_db / 60.0) * t60 * RATE
    print(f"knee {row['knee']:.1f}, analytic crossing {crossing:.1f}, interval {row['interval']:.0f}, T {row['t']:.4f} s, "
          f"peak to noise {row['peak_to_noise_db']:.1f} dB, last change {row['last_change']}")
    assert res["origin"] == 37 and res["taps"] == n + 37 and row["status"] == 0
    assert abs(row["knee"] - crossing) <= row["interval"]
    assert abs(row["t"] / t60 - 1.0) <= 0.05
    # the noise level is the floor's: two channels of variance (0.3 * 10^(dB / 20))^2
    want = 2.0 * (0.3 * 10.0 ** (floor_db / 20.0)) ** 2
    assert abs(10.0 * math.log10(row["noise"] / want)) < 1.0
    assert row["last_change"] <= row["interval"]


def test_the_bands_have_knees_of_their_own():
    res = _case(6000, 0.25, -50.0, XOVERS)
    assert_margins(res)
    assert len(res["rows"]) == 12
    for g in range(4):
        row = res["rows"][(g, "LR")]
        assert row["status"] == 0 and 1400 < row["knee"] < 2100 and abs(row["t"] / 0.25 - 1.0) < 0.15, (g, row)
    # the broadband rows do not depend on the crossovers
    for name in ir_floor_np.SETS:
        assert res["rows"][(0, name)] == _case(6000, 0.25, -50.0)["rows"][(0, name)]


def test_a_clean_ir_has_a_knee_near_its_end_and_says_so_in_its_peak_to_noise():
    res = floor(noise_ir(6000, 37, RATE, 0.25), RATE)
    row = res["rows"][(0, "LR")]
    assert row["status"] == 0 and row["knee"] > 0.9 * 6037 and row["peak_to_noise_db"] > 150.0


def _statuses(res):
    return {int(r["status"]) for r in res["rows"].values()}


def test_the_statuses():
    quiet = noise_ir(6000, 37, RATE, 0.25).copy()
    quiet[3000:] = 0.0
    res = floor(quiet, RATE, xovers=XOVERS)
    assert _statuses(res) == {3}
    for row in res["rows"].values():
        assert row["knee"] == 6037 and row["energy"] > 0 and all(math.isnan(row[f]) for f in FIELDS if f not in ("energy", "knee", "status"))
    for ir in (np.zeros((700, 2), np.float32), noise_ir(10, 0, RATE, 0.25), noise_ir(15, 0, RATE, 0.25)):
        res = floor(ir, RATE, onset_db=0.0)
        assert _statuses(res) == {1}
        assert all(math.isnan(row[f]) for row in res["rows"].values() for f in FIELDS[1:-1])
    assert _statuses(floor(noise_ir(16, 0, RATE, 0.25), RATE, onset_db=0.0)) != {1}
    rng = np.random.default_rng(3)
    res = floor((0.1 * rng.standard_normal((5000, 2))).astype(np.float32), RATE, xovers=XOVERS)
    assert _statuses(res) == {2}


def test_every_discrete_decision_reports_its_margin():
    res = _case(6000, 0.25, -50.0)
    m = res["margins"][(0, "LR")]
    assert set(m) == {"margin", "span", "peak", "interval", "ceil"}
    # the first fit and five rounds compare with the margin, the rounds with the span; two sets of means, one rounding, five ceils
    assert [len(m[k]) for k in ("margin", "span", "peak", "interval", "ceil")] == [6, 5, 2, 1, 5]
    assert 0.0 < ir_floor_np.smallest_margin(res) < 1.0
    with pytest.raises(AssertionError):
        assert_margins(res, least=1.0)


def _c_tail(res, first=0):
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import FloorQuery, tail_from_floor

    q = res["query"]
    res = dict(res, groups=len(res["rows"]) // 3, query=FloorQuery(rate=q["rate"], xovers=q["xovers"], onset_db=q["onset_db"], end=q["end"]))
    return tail_from_floor(res, first=first, mode="cut", fade=5, length=77, seed=3, width=0.5)


@pytest.mark.parametrize("xovers", [(), XOVERS])
def test_tail_from_floor_is_its_restatement(xovers):
    res = _case(6000, 0.25, -50.0, xovers)
    got, want = _c_tail(res, first=11), ir_floor_np.tail_from_floor(res, first=11)
    assert (got.mode, got.fade, got.length, got.seed, got.width) == ("cut", 5, 77, 3, 0.5)
    assert got.xovers == tuple(float(x) for x in xovers) and list(got.knee) == want["knee"] and list(got.t60) == want["t60"]
    assert got.level_db == tuple(want["level_db"])
    for k, row in zip(got.knee, [res["rows"][(j + 1 if xovers else 0, "LR")] for j in range(len(got.knee))]):
        assert k == 11 + math.floor(row["knee"])


def test_tail_from_floor_leaves_a_band_without_a_knee_alone():
    quiet = noise_ir(6000, 37, RATE, 0.25).copy()
    quiet[3000:] = 0.0
    got = _c_tail(floor(quiet, RATE, xovers=XOVERS))
    assert got.knee == (None, None, None)
    res = _case(6000, 0.25, -50.0)
    past = dict(res, rows={k: dict(r, knee=float(res["taps"]) + 0.5) for k, r in res["rows"].items()})
    assert _c_tail(past).knee == (None,) and ir_floor_np.tail_from_floor(past)["knee"] == [None]
    # a channel without a line of its own takes half of what the pair has
    one = dict(res, rows=dict(res["rows"]))
    one["rows"][(0, "R")] = dict(res["rows"][(0, "R")], status=2.0, noise=float("nan"), knee=float("nan"), t=float("nan"))
    got, want = _c_tail(one), ir_floor_np.tail_from_floor(one)
    assert got.level_db == tuple(want["level_db"]) and got.level_db[0][1] < got.level_db[0][0] + 3.0


def test_tail_from_floor_checks_its_query():
    from cuda_audio_amd import _lib

    L = _lib.load()
    q, t = _lib.McFloorQuery(), _lib.McIrTail()
    L.mc_default_floor_query(C.byref(q))
    L.mc_default_ir_tail(C.byref(t))
    assert (q.struct_size, q.rate, q.n_xovers, q.window, q.end, q.per_decade, q.rounds, q.reserved) == (64, 44100, 0, 0, 0, 5, 5, 0)
    assert (q.onset_db, q.tail_fraction, q.margin_db, q.span_db) == (-20.0, np.float32(0.1), 10.0, 20.0)
    assert (t.struct_size, t.mode, t.n_xovers, t.fade, t.width, t.seed, t.length) == (144, 0, 0, 0, 1.0, 0, 0)
    assert list(t.knee) == [(1 << 64) - 1] * 4 and list(t.xover_hz) == [250.0, 2000.0, 8000.0]
    rows = np.zeros((1, 3, 8))
    info = (C.c_uint64 * 2)(0, 100)
    dp = rows.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mc_ir_tail_from_floor(C.byref(q), dp, info, 0, C.byref(t)) == 0
    for field, value in (("rate", 7999), ("n_xovers", 4), ("tail_fraction", 0.6), ("margin_db", 0.5), ("span_db", 61.0), ("per_decade", 0), ("rounds", 17),
                         ("reserved", 1)):
        L.mc_default_floor_query(C.byref(q))
        setattr(q, field, value)
        assert L.mc_ir_tail_from_floor(C.byref(q), dp, info, 0, C.byref(t)) == -1 and field in L.mc_last_error().decode()
    L.mc_default_floor_query(C.byref(q))
    for args in ((None, dp, info, 0, C.byref(t)), (C.byref(q), None, info, 0, C.byref(t)), (C.byref(q), dp, None, 0, C.byref(t)), (C.byref(q), dp, info, 0, None)):
        assert L.mc_ir_tail_from_floor(*args) == -1 and "null" in L.mc_last_error().decode()
