"""The interaural cross-correlation as tests/ir_iacc_np.py states it (no GPU): the bound |IACF| <= 1, equal, delayed, flipped, swapped
and scaled channels, empty windows and silent channels; mc_ir_iacc refuses every bad field in the struct's order before it looks
at the engine, and mc_ir_tail_width_from_iacc (host arithmetic in the library) clamps at both ends and refuses NaN."""
import ctypes as C
import math

import numpy as np
import pytest

from ir_decay_np import noise_ir
from ir_iacc_np import MAX_LAG, assert_margins, default_lag, iacc, pair_ir, tail_width

RATE = 8000
T = 8  # 1 ms at 8 kHz


def delayed(L, d):
    """R[m] = L[m - d], zero where L has no tap."""
    R = np.zeros_like(L)
    if d >= 0:
        R[d:] = L[:L.size - d]
    else:
        R[:d] = L[-d:]
    return np.stack([L, R], axis=1).astype(np.float32)


def mono(n=3000, seed=3):
    return noise_ir(n=n, lead=0, rate=RATE, seed=seed)[:, 0]


def test_the_default_lag_is_one_millisecond():
    assert [default_lag(r) for r in (8000, 44100, 48000, 96000)] == [8, 44, 48, 96]


def test_iacf_never_exceeds_one():
    for seed, split in ((1, 0), (2, 5), (3, 1)):
        ir = pair_ir(n=2000, seed=seed)
        ir[1000:] *= 50.0  # a loud late field behind a short early window: only pairs inside the window keep the bound
        res = iacc(ir, RATE, bands=(1000.0,), max_lag=64, split=split, onset_db=0.0)
        assert np.nanmax(np.abs(res["curve"])) <= 1.0 + 1e-12
        assert all(r["status"] == 0 for r in res["rows"].values())


def test_equal_channels_read_one_at_lag_zero():
    L = mono()
    res = iacc(np.stack([L, L], axis=1), RATE, max_lag=T, onset_db=0.0)
    assert_margins(res)
    for row in res["rows"].values():
        assert row["status"] == 0 and row["lag"] == 0 and abs(row["iacc"] - 1.0) <= 1e-15 and row["iacf"] == row["iacf0"] == row["iacc"]
        assert row["level_db"] == 0.0


@pytest.mark.parametrize("d", [-T, -1, 0, 3, T])
def test_a_delayed_channel_peaks_at_its_delay(d):
    """R = L delayed by d taps.  Over a window [a, b) the pairs at lag d are L[m] L[m] for the m with m and m + d inside, so
    C(d) = the energy of L over the window less the |d| taps at one edge, and E_R is that same sum: IACF(d) = sqrt(E_R / E_L)
    when d >= 0 (R has lost the last d taps of the window's L and gained nothing inside it: the origin is tap 0, where the
    delayed channel is silent) and, for the early window with d < 0, C(d) = sum of L^2 over [|d|, k) while R holds L over [|d|, k + |d|)."""
    L = mono().astype(np.float64)
    split = 640
    res = iacc(delayed(L, d), RATE, max_lag=T, split=split, onset_db=0.0)
    assert_margins(res)
    for row in res["rows"].values():
        assert row["status"] == 0 and row["lag"] == d and row["iacf"] > 0.9
    e = L * L
    a = abs(d)
    if d >= 0:
        EL, ER, Cd = e[:split].sum(), e[:split - a].sum(), e[:split - a].sum()
    else:
        EL, ER, Cd = e[:split].sum(), e[a:split + a].sum(), e[a:split].sum()
    early = res["rows"][(0, "early")]
    assert abs(early["iacf"] - Cd / math.sqrt(EL * ER)) <= 1e-13
    assert abs(early["energy_l"] / EL - 1.0) <= 1e-13 and abs(early["energy_r"] / ER - 1.0) <= 1e-13


def test_a_delay_past_the_lags_gives_no_peak():
    res = iacc(delayed(mono(), T + 1), RATE, max_lag=T, onset_db=0.0)
    assert all(r["status"] == 0 and r["iacc"] < 0.2 for r in res["rows"].values())


def test_a_flipped_channel_reads_minus_one():
    L = mono()
    res = iacc(np.stack([L, -L], axis=1), RATE, max_lag=T, onset_db=0.0)
    assert_margins(res)
    for row in res["rows"].values():
        assert row["lag"] == 0 and abs(row["iacf"] + 1.0) <= 1e-15 and abs(row["iacc"] - 1.0) <= 1e-15


def test_swapping_the_channels_mirrors_the_curve():
    ir = pair_ir(n=3000, seed=11)
    ir[:, 1] = np.roll(ir[:, 1], 2)
    a = iacc(ir, RATE, bands=(500.0,), max_lag=T, onset_db=0.0)
    b = iacc(ir[:, ::-1], RATE, bands=(500.0,), max_lag=T, onset_db=0.0)
    np.testing.assert_allclose(b["curve"], a["curve"][:, :, ::-1], rtol=0.0, atol=1e-14)
    for key, row in a["rows"].items():
        assert b["rows"][key]["lag"] == -row["lag"] and abs(b["rows"][key]["level_db"] + row["level_db"]) <= 1e-12


@pytest.mark.parametrize("g", [0.5, 0.1, 4.0])
def test_a_scaled_channel_reads_its_level_difference(g):
    L = mono().astype(np.float64)
    res = iacc(np.stack([L, g * L], axis=1), RATE, max_lag=T, onset_db=0.0)
    for row in res["rows"].values():
        assert abs(row["level_db"] + 20.0 * math.log10(g)) <= 1e-5  # (the taps are float32: g L is rounded)
        assert abs(row["iacc"] - 1.0) <= 1e-7 and row["lag"] == 0


@pytest.mark.parametrize("lead,onset_db", [(0, 0.0), (37, -20.0)])
def test_a_split_past_the_end_leaves_the_late_window_empty(lead, onset_db):
    ir = pair_ir(n=1500, lead=lead, seed=4)
    o_want = None
    for split in (ir.shape[0], ir.shape[0] + 5, 1 << 40):
        res = iacc(ir, RATE, max_lag=T, split=split, onset_db=onset_db)
        o_want = res["origin"] if o_want is None else o_want
        if split == ir.shape[0] and lead == 0:
            assert res["split"] == res["taps"]  # split == N - o exactly
        late, early, whole = (res["rows"][(0, w)] for w in ("late", "early", "all"))
        assert late["status"] == 1 and late["energy_l"] == 0.0 and late["energy_r"] == 0.0 and math.isnan(late["iacc"])
        assert np.isnan(res["curve"][0, 1]).all()
        assert early == whole and np.array_equal(res["curve"][0, 0], res["curve"][0, 2])
    assert (o_want > 0) == (lead > 0)


def test_a_silent_channel_is_status_one():
    ir = pair_ir(n=1500, seed=4)
    ir[:, 1] = 0.0
    res = iacc(ir, RATE, bands=(1000.0,), max_lag=T, onset_db=0.0)
    for row in res["rows"].values():
        assert row["status"] == 1 and row["energy_l"] > 0.0 and row["energy_r"] == 0.0
        assert all(math.isnan(row[f]) for f in ("iacc", "lag", "iacf", "iacf0", "level_db"))
    assert np.isnan(res["curve"]).all()


# -- the library's checks and host arithmetic (no device is touched) -------------------------------------------------
def _query(**fields):
    from cuda_audio_amd import _lib

    q = _lib.McIaccQuery()
    _lib.load().mc_default_iacc_query(C.byref(q))
    q.rate, q.max_lag = RATE, T
    for k, v in fields.items():
        if k == "reserved":
            q.reserved[0], q.reserved[1] = v
        elif k == "centre_hz":
            for j, hz in enumerate(v):
                q.centre_hz[j] = hz
        else:
            setattr(q, k, v)
    return q


def _call(q, rows=True, info=True):
    """mc_ir_iacc without an engine: (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    r = np.zeros((11 * 3, 8))
    i = (C.c_uint64 * 3)()
    rc = L.mc_ir_iacc(None, 0, C.byref(q) if q is not None else None, r.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, None, i if info else None)
    return rc, L.mc_last_error().decode()


def test_the_default_query():
    from cuda_audio_amd import _lib

    q = _lib.McIaccQuery()
    _lib.load().mc_default_iacc_query(C.byref(q))
    assert C.sizeof(_lib.McIaccQuery) == 88 and _lib.MC_IACC_MAX_LAG == MAX_LAG
    assert (q.struct_size, q.rate, q.n_bands, q.max_lag, q.q, q.onset_db, q.end, q.split, list(q.reserved)) == (
        88, 44100, 0, default_lag(44100), float(np.float32(1.41421356)), -20.0, 0, 0, [0, 0])


BAD_FIELDS = [("struct_size", dict(struct_size=84)), ("rate", dict(rate=7999)), ("rate", dict(rate=384001)), ("n_bands", dict(n_bands=11)),
              ("max_lag", dict(max_lag=1025)), ("centre_hz[1]", dict(n_bands=2, centre_hz=(100.0, 5.0))),
              ("centre_hz[0]", dict(n_bands=1, centre_hz=(3700.0,))), ("centre_hz[0]", dict(n_bands=1, centre_hz=(float("nan"),))),
              ("q 0.05", dict(q=0.05)), ("q nan", dict(q=float("nan"))), ("onset_db", dict(onset_db=1.0)), ("onset_db", dict(onset_db=-121.0)),
              ("onset_db", dict(onset_db=float("nan"))), ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, 1)))]


def test_every_field_is_refused_before_the_engine_is_looked_at():
    rc, msg = _call(None)
    assert rc == -1 and "null query" in msg
    for name, fields in BAD_FIELDS:
        rc, msg = _call(_query(**fields))
        assert rc == -1 and name in msg, (name, fields, rc, msg)
    # in the struct's order: of two bad fields the earlier one is named
    order = [("rate", dict(rate=1)), ("n_bands", dict(n_bands=99)), ("max_lag", dict(max_lag=5000)), ("q 100", dict(q=100.0)),
             ("onset_db", dict(onset_db=5.0)), ("reserved", dict(reserved=(7, 7)))]
    for (first, a), (_, b) in zip(order, order[1:]):
        rc, msg = _call(_query(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # the edges that are good pass the query and stop at the first pointer
    for fields in (dict(max_lag=0), dict(max_lag=1024), dict(n_bands=10, centre_hz=(1000.0,) * 10), dict(onset_db=-120.0), dict(onset_db=0.0),
                   dict(end=1), dict(split=1 << 60), dict(n_bands=1, centre_hz=(3599.0,))):
        rc, msg = _call(_query(**fields))
        assert rc == -1 and "null engine" in msg, (fields, msg)


def _tail(width=0.25):
    from cuda_audio_amd.engine import IrTail

    return IrTail(mode="extend", xovers=(500.0,), knee=(1000, 1500), t60=(4000, 3000), level_db=((-40.0, -41.5), (-50.25, -49.0)), fade=64, seed=3,
                  width=width)


@pytest.mark.parametrize("rho", [1.0, 0.7, 0.3, 0.0, -0.2, -1.0, 1.5, 1e-9, 0.9999999])
def test_the_width_that_continues_a_correlation(rho):
    import dataclasses

    from cuda_audio_amd.engine import tail_width_from_iacc

    want = tail_width(rho)
    assert 0.0 <= want <= 1.0 and want == float(np.float32(min(max(1.0 - rho, 0.0), 1.0)))
    got = tail_width_from_iacc(_tail(), rho)
    assert got.width == want
    assert dataclasses.asdict(dataclasses.replace(got, width=0.25)) == dataclasses.asdict(_tail())  # nothing else moved
    # the dict ir_iacc returns is read at the broadband late IACF(0)
    assert tail_width_from_iacc(_tail(), dict(rows={(0, "late"): dict(iacf0=rho), (0, "early"): dict(iacf0=-5.0)})).width == want


def test_the_width_clamps_at_both_ends():
    assert tail_width(-0.5) == 1.0 and tail_width(2.0) == 0.0 and tail_width(1.0) == 0.0 and tail_width(0.0) == 1.0


def test_the_width_refusals():
    from cuda_audio_amd import _lib
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import tail_width_from_iacc

    for rho in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            tail_width(rho)
        with pytest.raises(McError, match="rho"):
            tail_width_from_iacc(_tail(), rho)
    L = _lib.load()
    assert L.mc_ir_tail_width_from_iacc(None, 0.5) == -1 and "null" in L.mc_last_error().decode()
    c = _tail().to_c()
    c.struct_size -= 4
    assert L.mc_ir_tail_width_from_iacc(C.byref(c), 0.5) == -1 and "struct_size" in L.mc_last_error().decode()
    c = _tail().to_c()
    assert L.mc_ir_tail_width_from_iacc(C.byref(c), float("nan")) == -1 and c.width == 0.25  # (a refused call leaves the tail alone)
