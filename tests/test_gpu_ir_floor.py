"""The noise-floor search on the device (mc_ir_floor, csrc/irfloor.hip.h) against the float64 restatement (tests/ir_floor_np.py)
applied to the taps the engine stores (Convolution.ir_taps).

Tolerance (ir_floor_np.check_against): 1e-6 relative, ir_decay_np.check_against's, on its grounds: the chunked recurrence of the
bands is within 1.4e-9 relative RMS of the sequential one and the non-negative double sums add 1e-9 at most; the interval means
are differences of such sums, the knee and the decay time come from regressions over them.  Status and the interval must be
equal exactly.  Every comparison asserts first that no discrete decision of the restatement is within 1e-9 of falling the other
way (assert_margins)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from ir_decay_np import noise_ir, sign_ir
from ir_floor_np import assert_margins, check_against, floor, noisy_ir

pytestmark = pytest.mark.gpu

RATE = 8000
T = 0.25
XOVERS = (400, 1600)


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irfloor", n_ref, sample_rate=rate, **kw)


def _compare(c, idx, rate, **query):
    """ir_floor of IR idx against the restatement of its stored taps."""
    want = floor(c.ir_taps(idx), rate, **query)
    assert_margins(want)
    got = c.ir_floor(idx, **query)
    for key in sorted(got["rows"]):
        print(key, {k: f"{v:.9g}" for k, v in got["rows"][key].items()})
    check_against(got, want)
    return got, want


@pytest.mark.parametrize("xovers", [(), XOVERS])
def test_noisy_ir_against_the_restatement(gpu_lib, xovers):
    c = _conv(16384)
    c.prepare(0, noisy_ir(6000, 37, RATE, T, floor_db=-50.0))
    got, _ = _compare(c, 0, RATE, xovers=xovers)
    c.close()
    assert got["origin"] == 37 and got["taps"] == 6037 and got["groups"] == (4 if xovers else 1)
    row = got["rows"][(0, "LR")]
    assert row["status"] == 0 and abs(row["knee"] - (37 + 50.0 / 60.0 * T * RATE)) <= row["interval"]
    assert all(r["status"] == 0 for r in got["rows"].values())


@functools.lru_cache(maxsize=None)
def _edge_ir(n, lead):
    """n taps in all: `lead` zeros, then noise that would have decayed by 90 dB at the last tap over a floor at -50 dB."""
    body = n - lead
    return noisy_ir(body, lead, RATE, t60=body / 1.5 / RATE, floor_db=-50.0, seed=11 + n % 7, noise_seed=5 + n % 11)


# test_gpu_ir_decay.py's edge shapes, for its reasons: 6000 taps in 16384; 16385: one workgroup's span of the chunk passes and a
# tap; 40000: 157 chunks, more than the 128 runs of the carry pass; end = 33001 and an origin of 300 fall in mid-chunk
EDGE_CASES = [(16384, 6000, 0, 0), (65536, 16385, 0, 0), (65536, 40000, 0, 0), (65536, 40000, 0, 33001), (16384, 4300, 300, 0)]


@pytest.mark.parametrize("xovers", [(), XOVERS])
@pytest.mark.parametrize("n_ref,n,lead,end", EDGE_CASES)
def test_edges_of_the_chunking(gpu_lib, n_ref, n, lead, end, xovers):
    c = _conv(n_ref)
    c.prepare(0, _edge_ir(n, lead))
    assert c.ir_info(0)["taps"] == n
    got, _ = _compare(c, 0, RATE, xovers=xovers, end=end)
    c.close()
    assert got["taps"] == (end or n)
    if lead:
        assert got["origin"] == lead
    assert got["rows"][(0, "LR")]["status"] == 0


def test_the_statuses(gpu_lib):
    c = _conv(16384)
    quiet = noise_ir(6000, 37, RATE, T).copy()
    quiet[3000:] = 0.0
    rng = np.random.default_rng(3)
    for idx, ir in enumerate((quiet, np.zeros((700, 2), np.float32), noise_ir(10, 0, RATE, T), (0.1 * rng.standard_normal((5000, 2))).astype(np.float32))):
        c.prepare(idx, ir)
    want = (3, 1, 1, 2)
    for idx, status in enumerate(want):
        got, _ = _compare(c, idx, RATE, xovers=XOVERS if idx != 2 else ())
        row = got["rows"][(0, "LR")]
        assert row["status"] == status, (idx, row)
        assert math.isnan(row["t"]) and math.isnan(row["noise"])
        assert row["knee"] == got["taps"] if status == 3 else math.isnan(row["knee"])
    c.close()


def test_nothing_is_disturbed(gpu_lib):
    """64 periods, a batch, the stored taps and both infos with ir_floor calls in between, against a run without them; and two
    calls return the same bits."""
    from cuda_audio_amd.engine import IrShape
    from cuda_audio_amd.synth import make_input

    ir = noisy_ir(6000, 37, RATE, T)
    x = make_input(96 * 256)
    query = dict(xovers=XOVERS)
    runs = []
    for ask in (False, True):
        c = _conv(16384, max_batch=32)
        c.prepare(0, ir, shape=IrShape(fade_out=100, normalize="peak", target=0.05))
        c.prepare(1, sign_ir(3000, RATE, T) * np.float32(0.01))
        c.cc[1].value.select = 1
        out, asked = [], []
        for k in range(64):
            if ask and k in (0, 32, 33):
                asked.append(c.ir_floor(k % 2, **query))
            out.append(np.stack(c.onProcess(x[0, k * 256:(k + 1) * 256], x[1, k * 256:(k + 1) * 256])))
        if ask:
            asked.append(c.ir_floor(0, **query))
        out.append(c.process(x[0, 64 * 256:], x[1, 64 * 256:]))
        runs.append((np.concatenate(out, axis=1), c.ir_taps(0), c.ir_taps(1), c.ir_info(0), c.ir_info(1), c.ir_shape_info(0)))
        c.close()
    for a, b in zip(*runs):
        if isinstance(a, dict):
            assert a == b
        else:
            np.testing.assert_array_equal(a, b)
    assert np.abs(runs[0][0]).max() > 0.01
    first, again = asked[0], asked[3]
    assert first["origin"] == again["origin"] and first["taps"] == again["taps"]
    for key, row in first["rows"].items():
        assert np.array(list(row.values())).tobytes() == np.array(list(again["rows"][key].values())).tobytes()


def _raw(c, idx, **fields):
    """mc_ir_floor with the struct's fields set directly; returns (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    q = _lib.McFloorQuery()
    L.mc_default_floor_query(C.byref(q))
    q.rate = RATE
    for k, v in fields.items():
        if k == "xover_hz":
            for i, hz in enumerate(v):
                q.xover_hz[i] = hz
        else:
            setattr(q, k, v)
    rows = np.zeros((4, 3, 8))
    info = (C.c_uint64 * 2)()
    rc = L.mc_ir_floor(c._h, idx, C.byref(q), rows.ctypes.data_as(C.POINTER(C.c_double)), info)
    return rc, L.mc_last_error().decode()


BAD_FIELDS = [("struct_size", dict(struct_size=60)), ("rate", dict(rate=7999)), ("rate", dict(rate=384001)), ("n_xovers", dict(n_xovers=4)),
              ("xover_hz[0]", dict(n_xovers=1, xover_hz=(9.0,))), ("xover_hz[1]", dict(n_xovers=2, xover_hz=(400.0, 0.46 * RATE))),
              ("xover_hz[0]", dict(n_xovers=1, xover_hz=(float("nan"),))), ("xover_hz[1]", dict(n_xovers=2, xover_hz=(400.0, 400.0))),
              ("xover_hz[2]", dict(n_xovers=3, xover_hz=(400.0, 1600.0, 1000.0))), ("onset_db", dict(onset_db=1.0)), ("onset_db", dict(onset_db=-121.0)),
              ("tail_fraction", dict(tail_fraction=0.0)), ("tail_fraction", dict(tail_fraction=0.6)), ("tail_fraction", dict(tail_fraction=float("nan"))),
              ("margin_db", dict(margin_db=0.5)), ("margin_db", dict(margin_db=31.0)), ("span_db", dict(span_db=4.0)), ("span_db", dict(span_db=61.0)),
              ("per_decade", dict(per_decade=0)), ("per_decade", dict(per_decade=21)), ("rounds", dict(rounds=0)), ("rounds", dict(rounds=17)),
              ("reserved", dict(reserved=1))]


def test_refusals(gpu_lib):
    from cuda_audio_amd._lib import McError

    ir = noisy_ir(3000, 0, RATE, T)
    single = _conv(16384, form="single")
    single.prepare(0, ir)
    with pytest.raises(McError) as ex:
        single.ir_floor(0)
    assert ex.value.code == -3
    single.close()
    c = _conv(16384)
    c.prepare(0, ir)
    before = c.ir_floor(0, xovers=XOVERS)
    for idx in (1, 255, 256, 1 << 40):
        with pytest.raises(McError) as ex:
            c.ir_floor(idx)
        assert ex.value.code == -1 and "IR not loaded" in str(ex.value)
    for name, fields in BAD_FIELDS:
        for idx in (0, 1):  # (the query comes before the index)
            rc, msg = _raw(c, idx, **fields)
            assert rc == -1 and name in msg, (name, fields, rc, msg)
    assert _raw(c, 0)[0] == 0
    np.testing.assert_array_equal(c.ir_taps(0), ir)
    after = c.ir_floor(0, xovers=XOVERS)
    for key, row in before["rows"].items():
        assert np.array(list(row.values())).tobytes() == np.array(list(after["rows"][key].values())).tobytes()
    c.close()
