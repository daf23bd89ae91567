"""The echo density as tests/ir_density_np.py states it (no GPU): a single impulse gives the window's own shape, stationary
Gaussian noise gives 1, the occupancy formula has its two known values, mc_ir_density refuses every bad field in the struct's
order before it looks at the engine, and mc_ir_tail_move_knee (host arithmetic in the library) slides a band along its line."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from ir_density_np import GAUSS_SHARE, assert_margins, density, impulse_profile, weights

RATE = 8000


def test_the_gaussian_share():
    assert GAUSS_SHARE == math.erfc(1.0 / math.sqrt(2.0))


@pytest.mark.parametrize("onset_db,d", [(0.0, 1003), (-20.0, 1003)])
def test_a_single_impulse_gives_the_window(onset_db, d):
    H, hop = 80, 16
    ir = np.zeros((3000, 2), np.float32)
    ir[d] = (0.5, -0.25)
    res = density(ir, RATE, half=H, hop=hop, onset_db=onset_db)
    assert_margins(res)
    o = d if onset_db < 0 else 0
    assert res["origin"] == o and res["centres"] == (3000 - 1 - o) // hop + 1
    t = o + np.arange(res["centres"]) * hop
    whole = (t - H >= 0) & (t + H <= 2999)
    want = impulse_profile(d, o, res["centres"], hop, H)
    for s in range(3):
        # the L + R set averages the two channels' counts: both see the impulse above sigma_LR or neither does
        np.testing.assert_allclose(res["profile"][whole, s], want[whole], rtol=1e-13, atol=0.0)
    assert np.all(res["profile"][np.abs(d - t) > H] == 0.0)
    row = res["rows"]["LR"]
    assert row["status"] == 1 and math.isnan(row["mix"]) and math.isnan(row["mean_after"])
    assert row["silent"] == np.count_nonzero(np.abs(d - t) > H)
    nearest = t[np.argmin(np.abs(d - t))]
    assert row["max_tap"] == nearest and abs(row["max"] / want.max() - 1.0) < 1e-13


def test_stationary_noise_is_fully_mixed():
    """A window of H = 80 holds (sum h)^2 / sum h^2 = 108 effective taps, so one eta has a standard deviation of
    sqrt(0.683 / (0.317 * 108)) = 0.14; 6000 taps hold 55 independent windows, so the profile's mean has 0.019: three of them."""
    rng = np.random.default_rng(5)
    res = density(rng.standard_normal((6000, 2)).astype(np.float32), RATE, half=80, hop=16, onset_db=0.0)
    h = weights(80)
    assert abs(h.sum() ** 2 / (h * h).sum() - 108.0) < 1.0
    mean = res["profile"].mean(axis=0)
    print("mean density of stationary noise:", mean)
    assert np.all(np.abs(mean - 1.0) <= 0.06)
    assert all(r["status"] == 0 and r["silent"] == 0 for r in res["rows"].values())


def test_a_fast_decay_reads_low_until_it_is_undone():
    """60 dB over nine window lengths, again and again, read in the windows that lie inside one run of the decay.  444 such
    windows hold 164 independent ones of 108 effective taps: the mean has a standard deviation of 0.14 / sqrt(164) = 0.011, the
    bound is three of them.  The two means are of the same noise, so their difference is the decay's doing alone."""
    rng = np.random.default_rng(9)
    H, n, hop = 80, 20000, 40
    t60 = 9 * (2 * H + 1)
    g = (rng.standard_normal((n, 2)) * (10.0 ** (-3.0 * (np.arange(n) % t60) / t60))[:, None]).astype(np.float32)
    t = np.arange((n - 1) // hop + 1) * hop
    inside = (t % t60 >= H) & (t % t60 < t60 - H) & (t + H < n)
    raw = density(g, RATE, half=H, hop=hop, onset_db=0.0)["profile"][inside, 2].mean()
    undone = density(g, RATE, half=H, hop=hop, onset_db=0.0, decay_t60=t60)["profile"][inside, 2].mean()
    print(f"{np.count_nonzero(inside)} windows: raw {raw:.4f}, decay undone {undone:.4f}")
    assert abs(undone - 1.0) <= 0.033 and 0.015 <= undone - raw <= 0.045


def test_density_of_occupancy():
    from cuda_audio_amd.engine import density_of_occupancy

    assert density_of_occupancy(1.0) == 1.0
    assert abs(density_of_occupancy(1.0 / 16.0) - 0.158) < 5e-4
    # the derivation, by simulation: frames sound with probability p and are scaled by 1 / sqrt p (2e6 frames: 3e-3 of 0.158 is 5 sigma)
    rng = np.random.default_rng(1)
    p = 1.0 / 16.0
    v = rng.standard_normal(2_000_000) * (rng.random(2_000_000) < p) / math.sqrt(p)
    share = np.count_nonzero(np.abs(v) > v.std()) / v.size / GAUSS_SHARE
    assert abs(share - density_of_occupancy(p)) < 3e-3


def _query(**fields):
    from cuda_audio_amd import _lib

    q = _lib.McDensityQuery()
    _lib.load().mc_default_density_query(C.byref(q))
    q.rate = RATE
    for k, v in fields.items():
        if k == "reserved":
            q.reserved[0], q.reserved[1] = v
        else:
            setattr(q, k, v)
    return q


def _call(q, rows=True, info=True):
    """mc_ir_density without an engine: (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    r = np.zeros((3, 8))
    i = (C.c_uint64 * 3)()
    rc = L.mc_ir_density(None, 0, C.byref(q) if q is not None else None, r.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, None, i if info else None)
    return rc, L.mc_last_error().decode()


def test_the_default_query():
    from cuda_audio_amd import _lib

    q = _lib.McDensityQuery()
    _lib.load().mc_default_density_query(C.byref(q))
    assert C.sizeof(_lib.McDensityQuery) == 48
    assert (q.struct_size, q.rate, q.half, q.hop, q.onset_db, q.threshold, q.end, q.decay_t60, list(q.reserved)) == (48, 44100, 0, 0, -20.0, 1.0, 0, 0, [0, 0])


# one bad value per field, in the struct's order; the last two of decay_t60 turn on the bound H 3 log2(10) / decay_t60 <= 256 with
# the default H of the rate (80 at 8000) and with a given one
BAD_FIELDS = [("struct_size", dict(struct_size=44)), ("rate", dict(rate=7999)), ("rate", dict(rate=384001)), ("half", dict(half=3)), ("half", dict(half=16385)),
              ("hop", dict(hop=(1 << 20) + 1)), ("onset_db", dict(onset_db=1.0)), ("onset_db", dict(onset_db=-121.0)), ("onset_db", dict(onset_db=float("nan"))),
              ("threshold", dict(threshold=0.0)), ("threshold", dict(threshold=2.5)), ("threshold", dict(threshold=float("nan"))),
              ("threshold", dict(threshold=float("inf"))), ("decay_t60", dict(decay_t60=3)), ("decay_t60", dict(half=16384, decay_t60=637)),
              ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, 1)))]


def test_every_field_is_refused_before_the_engine_is_looked_at():
    rc, msg = _call(None)
    assert rc == -1 and "null query" in msg
    for name, fields in BAD_FIELDS:
        rc, msg = _call(_query(**fields))
        assert rc == -1 and name in msg, (name, fields, rc, msg)
    # in the struct's order: of two bad fields the earlier one is named
    order = [("rate", dict(rate=1)), ("half", dict(half=1)), ("hop", dict(hop=1 << 21)), ("onset_db", dict(onset_db=5.0)), ("threshold", dict(threshold=-1.0)),
             ("decay_t60", dict(decay_t60=1)), ("reserved", dict(reserved=(7, 7)))]
    for (first, a), (_, b) in zip(order, order[1:]):
        rc, msg = _call(_query(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # the edges that are good pass the query and stop at the engine, then at the two arrays
    for fields in (dict(half=4, hop=1), dict(half=16384, hop=1 << 20), dict(threshold=2.0), dict(onset_db=-120.0), dict(decay_t60=4),
                   dict(half=16384, decay_t60=638), dict(end=1)):
        rc, msg = _call(_query(**fields))
        assert rc == -1 and "null engine" in msg, (fields, msg)


def _tail(**kw):
    from cuda_audio_amd.engine import IrTail

    base = dict(mode="extend", xovers=(500.0,), knee=(1000, 1500), t60=(4000, 3000), level_db=((-40.0, -41.5), (-50.25, -49.0)), fade=64, seed=3)
    base.update(kw)
    return IrTail(**base)


def test_move_knee_slides_the_levels_along_the_line():
    from cuda_audio_amd.engine import tail_move_knee

    t = _tail()
    for band, frame in ((0, 600), (1, 1501), (1, 0), (0, 123457)):
        got = tail_move_knee(t, band, frame)
        slide = 60.0 * (float(t.knee[band]) - float(frame)) / float(t.t60[band])
        want = tuple(float(np.float32(float(np.float32(v)) + slide)) for v in t.level_db[band])
        assert got.knee[band] == frame and got.level_db[band] == want, (band, frame, got, want)
        other = 1 - band
        assert got.knee[other] == t.knee[other] and got.level_db[other] == t.level_db[other] and got.t60 == t.t60
        assert (got.mode, got.xovers, got.fade, got.seed, got.width, got.length) == (t.mode, t.xovers, t.fade, t.seed, t.width, t.length)
        # there and back: the knee exactly, the levels within one float rounding
        back = tail_move_knee(got, band, t.knee[band])
        assert back.knee == t.knee
        for a, b, there in zip(back.level_db[band], t.level_db[band], want):
            assert abs(a - b) <= float(np.spacing(np.float32(max(abs(b), abs(there)))))
    # earlier is louder: 400 frames of a 4000-frame decay are 6 dB
    assert tail_move_knee(t, 0, 600).level_db[0] == (-34.0, -35.5)


def test_move_knee_refusals():
    from cuda_audio_amd import _lib
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import tail_move_knee

    for tail, band, word in ((_tail(), 2, "n_xovers"), (_tail(knee=(1000, None)), 1, "left alone"), (_tail(mode="cut"), 0, "MC_TAIL_EXTEND"),
                             (_tail(mode="off"), 0, "MC_TAIL_EXTEND")):
        with pytest.raises(McError) as ex:
            tail_move_knee(tail, band, 10)
        assert ex.value.code == -1 and word in str(ex.value), str(ex.value)
    L = _lib.load()
    assert L.mc_ir_tail_move_knee(None, 0, 10) == -1 and "null" in L.mc_last_error().decode()
    c = _tail().to_c()
    c.struct_size = 140
    assert L.mc_ir_tail_move_knee(C.byref(c), 0, 10) == -1 and "struct_size" in L.mc_last_error().decode()
    assert dataclasses.asdict(tail_move_knee(_tail(), 1, 1500)) == dataclasses.asdict(_tail())
