"""The echo density on the device (mc_ir_density, csrc/irdensity.hip.h) against the float64 restatement (tests/ir_density_np.py)
applied to the taps the engine stores (Convolution.ir_taps).

Tolerance (ir_density_np.check_against): equal integers for the mixing tap, the tap of the maximum, the silent count and the
status; 1e-10 relative for every density.  Derived, not measured: every sum is of at most 32769 non-negative doubles, so any
order of addition is within 32768 * 2^-53 = 3.7e-12 relative of any other, and the weights and the exp2 differ between libm and
the device by a few units in the last place.  Every comparison asserts first that no discrete decision of the restatement is
within 1e-9 of falling the other way (assert_margins)."""
import ctypes as C
import functools
import hashlib
import math

import numpy as np
import pytest

from ir_decay_np import noise_ir
from ir_density_np import assert_margins, check_against, density, impulse_profile

pytestmark = pytest.mark.gpu

RATE = 8000
T = 0.25
LDS_TAPS = 6144  # csrc/irdensity.hip.h's DEN_LDS_TAPS: a window of 2 H + 1 taps is staged up to H = 3071


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irdensity", n_ref, sample_rate=rate, **kw)


def _compare(c, idx, rate, margins=True, **query):
    """ir_density of IR idx against the restatement of its stored taps."""
    want = density(c.ir_taps(idx), rate, **query)
    if margins:
        assert_margins(want)
    got = c.ir_density(idx, profile=True, **query)
    for name, row in got["rows"].items():
        print(name, {k: f"{v:.9g}" for k, v in row.items()})
    check_against(got, want)
    return got, want


@functools.lru_cache(maxsize=None)
def _noise(n, lead=0, t60=T, seed=7):
    return noise_ir(n, lead, RATE, t60, seed=seed)


# (n_ref, body taps, lead of zeros, query): the smallest shapes that reach every branch of the kernel and its launch
CASES = {
    "plain": (16384, 6000, 0, dict(half=80, hop=16)),
    "hop 1": (16384, 700, 0, dict(half=40, hop=1)),
    "every window cut at both ends": (16384, 100, 0, dict(half=80, hop=7)),
    "origin in mid-run": (16384, 4000, 300, dict(half=80, hop=16, onset_db=-20.0)),
    "silent windows": (16384, 4000, 300, dict(half=80, hop=16, onset_db=0.0)),
    "end in mid-run": (65536, 40000, 0, dict(half=80, hop=16, end=33001)),
    "windows that do not touch": (16384, 6000, 0, dict(half=20, hop=400)),
    "the last hop that is staged": (16384, 6000, 0, dict(half=20, hop=40)),
    "the first hop that is not": (16384, 6000, 0, dict(half=20, hop=41)),
    "global path": (131072, 70000, 0, dict(half=16384, hop=4096)),
    "the widest staged window": (16384, 9000, 0, dict(half=(LDS_TAPS - 1) // 2, hop=500)),
    "one tap wider": (16384, 9000, 0, dict(half=(LDS_TAPS - 1) // 2 + 1, hop=500)),
    "a run the budget cuts short": (16384, 9000, 0, dict(half=3000, hop=10)),
    "default window and hop": (16384, 3000, 0, dict()),
    "decay undone, slow": (16384, 6000, 0, dict(half=80, hop=16, decay_t60=4000)),
    "decay undone, 2^16 across the window": (16384, 6000, 0, dict(half=80, hop=16, decay_t60=50)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_restatement(gpu_lib, case):
    n_ref, n, lead, query = CASES[case]
    c = _conv(n_ref)
    c.prepare(0, _noise(n, lead))
    assert c.ir_info(0)["taps"] == n + lead
    got, want = _compare(c, 0, RATE, **query)
    c.close()
    assert got["taps"] == (query.get("end") or n + lead)
    if lead:
        assert got["origin"] == (lead if query["onset_db"] < 0 else 0)
    if case == "silent windows":
        # the windows that end inside the lead of zeros
        assert got["rows"]["LR"]["silent"] == len([i for i in range(got["centres"]) if i * 16 + 80 < lead]) > 0
    if case == "plain":
        assert got["rows"]["LR"]["status"] == 0 and got["centres"] == 375 and abs(got["rows"]["LR"]["mean_after"] - 1.0) < 0.1


def test_one_tap(gpu_lib):
    """One window of one tap: sigma = |v| exactly (the square root of an exact square; the channels are equally loud, so that
    holds for sigma_LR too), and nothing is strictly above it.  The margin of that comparison is 0 by construction, which is
    why assert_margins is not asked."""
    c = _conv(16384)
    c.prepare(0, np.array([[0.25, -0.25]], np.float32))
    got, _ = _compare(c, 0, RATE, margins=False, half=80, hop=16)
    c.close()
    assert (got["origin"], got["taps"], got["centres"]) == (0, 1, 1)
    assert np.all(got["profile"] == 0.0)
    for row in got["rows"].values():
        assert row["status"] == 1 and row["silent"] == 0 and row["max"] == 0.0 and row["max_tap"] == 0 and math.isnan(row["mix"])


def test_equal_channels_give_equal_rows(gpu_lib):
    ir = np.repeat(_noise(3000)[:, :1], 2, axis=1)
    c = _conv(16384)
    c.prepare(0, ir)
    got, _ = _compare(c, 0, RATE, half=80, hop=16, decay_t60=2000)
    c.close()
    p = got["profile"]
    assert p[:, 0].tobytes() == p[:, 1].tobytes() == p[:, 2].tobytes()
    rows = [np.array(list(got["rows"][name].values())).tobytes() for name in ("L", "R", "LR")]
    assert rows[0] == rows[1] == rows[2]


def test_the_impulse_closed_form(gpu_lib):
    H, hop, d, n = 80, 16, 1003, 3000
    ir = np.zeros((n, 2), np.float32)
    ir[d] = (0.5, -0.25)
    c = _conv(16384)
    c.prepare(0, ir)
    got, _ = _compare(c, 0, RATE, half=H, hop=hop, onset_db=0.0)
    c.close()
    t = np.arange(got["centres"]) * hop
    whole = (t - H >= 0) & (t + H <= n - 1)
    want = impulse_profile(d, 0, got["centres"], hop, H)
    for s in range(3):
        assert np.all(np.abs(got["profile"][whole, s] - want[whole]) <= 1e-10 * want[whole])
    assert np.all(got["profile"][np.abs(d - t) > H] == 0.0)
    assert got["rows"]["LR"]["silent"] == np.count_nonzero(np.abs(d - t) > H)


SYNTH = dict(frames=12000, build_up=4000, t60=8000, late_gain=1.0, width=1.0)
SYNTH_QUERY = dict(half=441, hop=64, decay_t60=8000)
SYNTH_SEEDS = (2, 3, 4)


def _synth_figures(res):
    t = res["origin"] + np.arange(res["centres"]) * res["hop"]
    eta = res["profile"][:, 2]
    return float(eta[t >= 4441].mean()), float(eta[t <= 1000].max())


@pytest.mark.parametrize("seed", SYNTH_SEEDS)
def test_a_synthesised_build_up_reads_as_its_occupancy(gpu_lib, seed):
    """The late field's density is 1 where it is dense and density_of_occupancy(1 / 16) = 0.158 where the build-up starts.  A
    window of H = 441 holds about 590 effective taps: the bounds [0.95, 1.05] on the mean past the build-up and 0.30 on the
    maximum before tap 1000 are three and five standard deviations of the binomial estimate.  The seeds are ones for which the
    restatement of tests/ir_synth_np.py's frames is itself inside both bounds (checked here first, on the CPU)."""
    import ir_synth_np
    from cuda_audio_amd.engine import IrSynth, density_of_occupancy

    frames = ir_synth_np.frames(seed=seed, **SYNTH)
    mean, early = _synth_figures(density(frames, RATE, **SYNTH_QUERY))
    print(f"restatement: mean past the build-up {mean:.4f}, max before tap 1000 {early:.4f} (expected 1 and {density_of_occupancy(1 / 16):.3f})")
    assert 0.95 <= mean <= 1.05 and early <= 0.30
    c = _conv(16384)
    c.prepare_synth(0, IrSynth(seed=seed, **SYNTH))
    got, _ = _compare(c, 0, RATE, **SYNTH_QUERY)
    c.close()
    mean, early = _synth_figures(got)
    print(f"device: mean past the build-up {mean:.4f}, max before tap 1000 {early:.4f}")
    assert 0.95 <= mean <= 1.05
    assert early <= 0.30


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_nothing_is_disturbed_and_two_calls_agree(gpu_lib):
    """The SHA-256 of the stored taps and of one processed batch with ir_density calls in between, against a run without them;
    and two calls return the same bits."""
    from cuda_audio_amd.synth import make_input

    ir = _noise(6000, 37)
    x = make_input(32 * 256)
    query = dict(half=80, hop=16, decay_t60=2000, profile=True)
    runs, asked = [], []
    for ask in (False, True):
        c = _conv(16384, max_batch=32)
        c.prepare(0, ir)
        if ask:
            asked.append(c.ir_density(0, **query))
        first = c.process(x[0, :16 * 256], x[1, :16 * 256])
        if ask:
            asked.append(c.ir_density(0, **query))
            asked.append(c.ir_density(0, half=4000, hop=1000))
        second = c.process(x[0, 16 * 256:], x[1, 16 * 256:])
        runs.append((_sha(c.ir_taps(0)), _sha(first), _sha(second), c.ir_info(0)))
        c.close()
    assert runs[0] == runs[1]
    a, b = asked[0], asked[1]
    assert (a["origin"], a["taps"], a["centres"]) == (b["origin"], b["taps"], b["centres"]) == (37, 6037, 375)
    assert a["profile"].tobytes() == b["profile"].tobytes()
    for name, row in a["rows"].items():
        assert np.array(list(row.values())).tobytes() == np.array(list(b["rows"][name].values())).tobytes()


def _raw(c, idx, rows=True, info=True, **fields):
    """mc_ir_density with the struct's fields set directly; returns (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    q = _lib.McDensityQuery()
    L.mc_default_density_query(C.byref(q))
    q.rate = RATE
    for k, v in fields.items():
        setattr(q, k, v)
    r = np.zeros((3, 8))
    i = (C.c_uint64 * 3)()
    rc = L.mc_ir_density(c._h, idx, C.byref(q), r.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, None, i if info else None)
    return rc, L.mc_last_error().decode()


def test_refusals(gpu_lib):
    from cuda_audio_amd._lib import McError

    ir = _noise(3000)
    single = _conv(16384, form="single")
    single.prepare(0, ir)
    with pytest.raises(McError) as ex:
        single.ir_density(0)
    assert ex.value.code == -3
    single.close()
    c = _conv(16384)
    c.prepare(0, ir)
    before = c.ir_density(0, half=80, profile=True)
    for idx in (1, 255, 256, 1 << 40):
        with pytest.raises(McError) as ex:
            c.ir_density(idx, profile=True)
        assert ex.value.code == -1 and "IR not loaded" in str(ex.value)
    for idx in (0, 1):  # the query, then the two arrays, come before the index
        for name, fields in (("half", dict(half=3)), ("hop", dict(hop=(1 << 20) + 1)), ("threshold", dict(threshold=0.0)), ("decay_t60", dict(decay_t60=3))):
            rc, msg = _raw(c, idx, **fields)
            assert rc == -1 and name in msg, (name, rc, msg)
        for name, args in (("rows", dict(rows=False)), ("info", dict(info=False))):
            rc, msg = _raw(c, idx, **args)
            assert rc == -1 and "null " + name in msg, (name, rc, msg)
    assert _raw(c, 0)[0] == 0
    np.testing.assert_array_equal(c.ir_taps(0), ir)
    after = c.ir_density(0, half=80, profile=True)
    assert before["profile"].tobytes() == after["profile"].tobytes()
    c.close()


def test_the_work_bounds_come_after_the_index(gpu_lib):
    """600 000 taps: hop 1 makes 600 000 windows, which H = 16384 takes past 2^34 weighted taps; hop 2 halves them and passes the
    bound (it is only asked about, with `end`, not run at that size).  More than 2^22 windows need more than 2^22 taps."""
    c = _conv(1 << 20)
    c.prepare(0, _noise(600000, t60=20.0))
    rc, msg = _raw(c, 0, half=16384, hop=1)
    assert rc == -1 and "hop" in msg and "weighted taps" in msg, msg
    rc, msg = _raw(c, 1, half=16384, hop=1)
    assert rc == -1 and "IR not loaded" in msg, msg
    assert _raw(c, 0, half=16384, hop=1, end=524273)[0] == -1  # 524272 * 32769 = 2^34 - 16: 524273 windows are one too many
    assert _raw(c, 0, half=16384, hop=65536, end=524273)[0] == 0
    c.close()
    c = _conv(1 << 23)
    c.prepare(0, _noise((1 << 22) + 2, t60=100.0))
    rc, msg = _raw(c, 0, half=4, hop=1)
    assert rc == -1 and "hop" in msg and "windows" in msg, msg
    assert _raw(c, 0, half=4, hop=1 << 20, end=(1 << 22) + 1)[0] == 0
    c.close()
