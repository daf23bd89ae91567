"""The parts step of an IR load without a GPU: the float64 restatement's own properties (tests/ir_parts_np.py), mc_ir_parts_plan and
mc_ir_parts_at against it, and the refusals of mc_load_ir_parts and mc_load_ir_sweep_parts in the documented order with a null
engine, so that no HIP call is made: a step that is off is mc_load_ir_match, refusal for refusal."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ir_parts_np as PN

FP = C.POINTER(C.c_float)
NAN = float("nan")


def _parts(**fields):
    from cuda_audio_amd import _lib

    p = _lib.McIrParts()
    _lib.load().mc_default_ir_parts(C.byref(p))
    p.mode = _lib.MC_PARTS_ON
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(p, k)[j] = x
        else:
            setattr(p, k, v)
    return p


# -- the restatement -----------------------------------------------------------------------------------------------------
def test_the_weights_sum_to_one_and_stay_in_range():
    rng = np.random.default_rng(1)
    for _ in range(200):
        F = int(rng.integers(1, 700))
        b0, b1, x = PN.random_layout(rng, F)
        w = PN.weights(F, b0, b1, x)
        assert np.abs(w.sum(axis=0) - 1.0).max() <= 1e-15
        assert w.min() >= 0.0 and w.max() <= 1.0
    w = PN.weights(10, 3, 7, (0, 0))  # hard cuts at the boundaries
    assert w[0].tolist() == [1] * 3 + [0] * 7 and w[1].tolist() == [0] * 3 + [1] * 4 + [0] * 3 and w[2].tolist() == [0] * 7 + [1] * 3
    w = PN.weights(10, 4, 8, (3, 2))  # s = 3 and 7: the fades hold frames 3, 4, 5 and 7, 8
    assert w[0, :3].tolist() == [1, 1, 1] and 0 < w[0, 5] < w[0, 4] < w[0, 3] < 1 and w[0, 6:].tolist() == [0] * 4
    assert abs(w[0, 4] - 0.5) <= 1e-16 and w[2, :7].tolist() == [0] * 7 and 0 < w[2, 7] < w[2, 8] < 1 and w[2, 9] == 1


def test_unity_parts_reproduce_the_input():
    rng = np.random.default_rng(2)
    for _ in range(200):
        F = int(rng.integers(1, 900))
        x = PN.noise(F, int(rng.integers(0, 50)))
        b0, b1, xf = PN.random_layout(rng, F)
        y, info = PN.parted(x, direct_end=b0, early_end=b1, xfade=xf)
        assert np.array_equal(y, x), (F, b0, b1, xf)
        assert info["frames_out"] == F and info["lost"] == 0


def test_width_zero_gives_equal_channels_and_swap_exchanges_them():
    x = PN.noise(500, 3)
    y, _ = PN.parted(x, direct_end=40, early_end=200, xfade=(9, 30), width=0.0, gain_db=(0.0, -4.0, 3.0))
    assert y[:, 0].tobytes() == y[:, 1].tobytes() and np.abs(y).max() > 0
    y, _ = PN.parted(x, direct_end=40, early_end=200, xfade=(9, 30), swap=PN.PARTS)
    assert np.array_equal(y, x[:, ::-1])


def test_frames_out_follows_its_rule():
    f = PN.frames_out_of
    assert f(100) == 100  # (everything is the late part)
    assert f(100, 10, 50, (4, 6), delay=(0, 0, 7)) == 107
    assert f(100, 10, 50, (4, 6), delay=(0, 0, -7)) == 93  # the early part ends at 47 + 6 = 53
    assert f(100, 10, 50, (4, 6), delay=(0, 0, -60)) == 53
    assert f(100, 10, 50, (4, 6), delay=(0, 0, -60), mute=("early",)) == 40  # the late part's 100 - 60
    assert f(100, 10, 50, (4, 6), mute=("early", "late")) == 12  # s_0 + x_0
    assert f(100, 10, 50, (4, 6), delay=(-12, 0, 0), mute=("early", "late")) == 0
    assert f(100, 10, 200, mute=("direct", "early")) == 0  # the late part is empty
    assert f(100, 0, 0, mute=("late",)) == 0  # so are the other two
    assert f(100, 10, 200, delay=(500, 0, 0)) == 510 and f(100, 300, 300) == 100
    assert f(100, 10, 50, frames_out=7) == 7


# -- the plan ------------------------------------------------------------------------------------------------------------
def _plan(p, frames=100, out=True):
    from cuda_audio_amd import _lib

    L = _lib.load()
    o, c = (C.c_double * 4)(*([-1.0] * 4)), (C.c_double * 12)(*([-1.0] * 12))
    rc = L.mc_ir_parts_plan(C.byref(p) if p is not None else None, frames, o if out else None, c)
    return rc, L.mc_last_error().decode(), list(o), np.array(c[:12]).reshape(3, 4)


def test_the_plan_agrees_with_the_restatement():
    from cuda_audio_amd.engine import IrParts, parts_plan

    rng = np.random.default_rng(3)
    for i in range(100):
        F = int(rng.integers(1, 5000))
        b0, b1, xf = PN.random_layout(rng, F)
        kw = dict(delay=tuple(int(v) for v in rng.integers(-F, F + 1, size=3)), gain_db=tuple(rng.uniform(-60, 24, 3)), width=tuple(rng.uniform(0, 2, 3)),
                  balance=tuple(rng.uniform(-1, 1, 3)), mute=tuple(n for n in PN.PARTS if rng.random() < 0.3), swap=tuple(n for n in PN.PARTS if rng.random() < 0.3),
                  invert=tuple(n for n in PN.PARTS if rng.random() < 0.3))
        Fo = PN.frames_out_of(F, b0, b1, xf, kw["delay"], kw["mute"])
        parts = IrParts(direct_end=b0, early_end=b1, xfade=xf, **kw)
        if Fo < 1:
            rc, msg, _, _ = _plan(parts.to_c(), F)
            assert rc == -1 and "every part" in msg, msg
            continue
        got = parts_plan(parts, F)
        assert got["frames_out"] == Fo and got["fade_start"] == PN.starts(b0, b1, xf) and got["device_bytes"] > 0
        want = PN.coefficients(kw["gain_db"], kw["width"], kw["balance"], kw["swap"], kw["invert"])
        assert (np.abs(got["coef"] - want) <= 1e-15 * np.abs(want)).all(), (got["coef"], want)
    # exact at 0 dB, width 0, 1 and 2, balance 0 and +-1
    for width, balance, swap, invert in itertools.product((0.0, 1.0, 2.0), (0.0, 1.0, -1.0), ((), ("early",)), ((), ("late",))):
        got = parts_plan(IrParts(width=width, balance=balance, swap=swap, invert=invert), 10)["coef"]
        assert np.array_equal(got, PN.coefficients(0.0, width, balance, swap, invert))
    assert parts_plan(IrParts(), 10)["coef"].tolist() == [[1, 0, 0, 1]] * 3
    assert parts_plan(IrParts(width=0.0, invert=("direct",)), 10)["coef"][0].tolist() == [-0.5] * 4
    assert parts_plan(IrParts(swap=("late",), balance=1.0), 10)["coef"][2].tolist() == [0, 0, 1, 0]


def test_parts_at_moves_the_boundaries_only():
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrParts, parts_at, parts_from_density

    p = parts_at(IrParts(xfade=(8, 64), gain_db=(0, -4, 0), mute=("direct",)), onset=100, rate=48000)
    assert (p.direct_end, p.early_end) == (100 + 120, 100 + 3840) and p.xfade == (8, 64) and p.gain_db == (0, -4, 0) and p.mute == ("direct",)
    L = _lib.load()
    q = _parts(delay=(1, 2, 3), frames_out=9)
    assert L.mc_ir_parts_at(C.byref(q), 5, 7, 11) == 0 and (q.direct_end, q.early_end, list(q.delay), q.frames_out) == (12, 16, [1, 2, 3], 9)
    for args, word in (((5, 8, 7), "early_frames"), (((1 << 40), 1, 2), "2^40"), ((0, 1, (1 << 40) + 1), "2^40")):
        assert L.mc_ir_parts_at(C.byref(q), *args) == -1 and word in L.mc_last_error().decode()
    assert L.mc_ir_parts_at(None, 0, 0, 0) == -1 and "null parts" in L.mc_last_error().decode()
    q.struct_size = 100
    assert L.mc_ir_parts_at(C.byref(q), 0, 0, 0) == -1 and "struct_size" in L.mc_last_error().decode()
    density = dict(origin=30, rows={"LR": dict(mix=2430.0, mix_s=0.05, status=0.0)})
    p = parts_from_density(IrParts(xfade=(0, 16)), density, first=7)
    assert (p.direct_end, p.early_end, p.xfade) == (7 + 30 + 120, 7 + 2430, (0, 16))
    with pytest.raises(ValueError):
        parts_from_density(IrParts(), dict(origin=30, rows={"LR": dict(mix=NAN, mix_s=NAN, status=1.0)}))


# -- refusals ------------------------------------------------------------------------------------------------------------
BAD_FIELDS = [("struct_size", dict(struct_size=96)), ("mode", dict(mode=2)), ("flags", dict(flags=8)), ("flags", dict(flags=0x1000)), ("reserved0", dict(reserved0=1)),
              ("direct_end", dict(direct_end=(1 << 40) + 1, early_end=(1 << 40) + 1)), ("early_end", dict(direct_end=10, early_end=9)),
              ("early_end", dict(early_end=(1 << 40) + 1)), ("xfade[0]", dict(direct_end=3, early_end=50, xfade=(8, 0))),
              ("xfade[1]", dict(direct_end=10, early_end=12, xfade=(4, 2))), ("xfade[1]", dict(direct_end=0, early_end=1, xfade=(0, 4))),
              ("delay[0]", dict(delay=((1 << 24) + 1, 0, 0))), ("delay[2]", dict(delay=(0, 0, -(1 << 24) - 1))), ("gain_db[1]", dict(gain_db=(0.0, 24.5, 0.0))),
              ("gain_db[0]", dict(gain_db=(-121.0, 0.0, 0.0))), ("gain_db[2]", dict(gain_db=(0.0, 0.0, NAN))), ("width[0]", dict(width=(-0.1, 1.0, 1.0))),
              ("width[2]", dict(width=(1.0, 1.0, 2.5))), ("width[1]", dict(width=(1.0, NAN, 1.0))), ("balance[0]", dict(balance=(1.5, 0.0, 0.0))),
              ("balance[2]", dict(balance=(0.0, 0.0, NAN))), ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, 1)))]
ORDER = [("mode", dict(mode=9)), ("flags", dict(flags=0x80)), ("reserved0", dict(reserved0=3)), ("direct_end", dict(direct_end=1 << 41)),
         ("early_end", dict(early_end=1 << 42)), ("delay[1]", dict(delay=(0, 1 << 30, 0))), ("gain_db[0]", dict(gain_db=(99.0, 0.0, 0.0))),
         ("width[0]", dict(width=(9.0, 1.0, 1.0))), ("balance[0]", dict(balance=(9.0, 0.0, 0.0))), ("reserved", dict(reserved=(7, 7)))]


def test_the_plan_refuses():
    rc, msg, _, _ = _plan(None)
    assert rc == -1 and "null parts" in msg
    for name, fields in BAD_FIELDS:
        rc, msg, out, _ = _plan(_parts(**fields))
        assert rc == -1 and name in msg and out == [-1.0] * 4, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):  # (of two bad fields the earlier one is named)
        rc, msg, _, _ = _plan(_parts(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    rc, msg, _, _ = _plan(_parts(direct_end=2, early_end=50, xfade=(8, 200)))  # (xfade[0] before xfade[1])
    assert rc == -1 and "xfade[0]" in msg, msg
    rc, msg, _, _ = _plan(_parts(), frames=0)
    assert rc == -1 and "empty IR" in msg
    rc, msg, _, _ = _plan(_parts(frames_out=100 + (1 << 24) + 1))
    assert rc == -1 and "frames_out" in msg, msg
    rc, msg, out, _ = _plan(_parts(frames_out=100 + (1 << 24)))
    assert rc == 0 and out[0] == 100.0 + (1 << 24)
    rc, msg, _, _ = _plan(_parts(flags=7))
    assert rc == -1 and "every part" in msg, msg
    rc, msg, _, _ = _plan(_parts(flags=7, frames_out=5))  # (frames_out does not rescue parts that store nothing)
    assert rc == -1 and "every part" in msg, msg
    rc, msg, out, _ = _plan(_parts(mode=0, direct_end=4, early_end=9, xfade=(2, 4)))  # (off is planned as on)
    assert rc == 0 and out[:3] == [100.0, 3.0, 7.0]
    rc, msg, _, _ = _plan(_parts(), out=False)
    assert rc == -1 and "null out" in msg


def _others():
    """A bad match, a bad filter, a bad phase, a bad tail and a bad shape."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    match = _lib.McIrMatch()
    L.mc_default_ir_match(C.byref(match))
    match.mode, match.amount = _lib.MC_MATCH_FLAT, 2.0
    filt = _lib.McIrFilter()
    L.mc_default_ir_filter(C.byref(filt))
    filt.op, filt.reg_db = _lib.MC_FILTER_CONVOLVE, 1.0
    phase = _lib.McIrPhase()
    L.mc_default_ir_phase(C.byref(phase))
    phase.mode, phase.over_log2 = _lib.MC_PHASE_MINIMUM, 0
    tail = _lib.McIrTail()
    L.mc_default_ir_tail(C.byref(tail))
    tail.mode, tail.width = _lib.MC_TAIL_EXTEND, 7.0
    shape = _lib.McIrShape()
    L.mc_default_ir_shape(C.byref(shape))
    shape.trim_db = 5.0
    return match, filt, phase, tail, shape


def _ref(x):
    return C.byref(x) if x is not None else None


def _file_args(frames=100, rates=(48000, 48000), lr=True, shape=None, tail=None, phase=None, filt=None, flr=True, fG=10, match=None, tlr=True, G=10):
    buf, fbuf, tbuf = (np.zeros((max(min(n, 1000), 1), 2), np.float32) for n in (frames, fG, G))
    args = (None, 0, buf.ctypes.data_as(FP) if lr else None, frames, 1024, rates[0], rates[1], _ref(shape), None, None, _ref(tail), _ref(phase), _ref(filt),
            fbuf.ctypes.data_as(FP) if flr else None, fG, _ref(match), tbuf.ctypes.data_as(FP) if tlr else None, G)
    return args, (buf, fbuf, tbuf)


def _sweep_args(ir_frames=900, lr=True, tail=None, phase=None, filt=None, flr=True, fG=10, match=None, tlr=True, G=10):
    from cuda_audio_amd.engine import Sweep

    rec = np.zeros((5000, 2), np.float32)
    fbuf, tbuf = (np.zeros((max(min(n, 1000), 1), 2), np.float32) for n in (fG, G))
    sw = Sweep(frames=4096, f1_hz=20.0, f2_hz=3000.0, rate=8000).to_c()
    args = (None, 0, rec.ctypes.data_as(FP) if lr else None, len(rec), 1024, C.byref(sw), 0, ir_frames, None, None, None, _ref(tail), _ref(phase), _ref(filt),
            fbuf.ctypes.data_as(FP) if flr else None, fG, _ref(match), tbuf.ctypes.data_as(FP) if tlr else None, G)
    return args, (rec, fbuf, tbuf, sw)


def _load(p, sweep=False, **kw):
    from cuda_audio_amd import _lib

    L = _lib.load()
    args, keep = (_sweep_args if sweep else _file_args)(**kw)
    rc = (L.mc_load_ir_sweep_parts if sweep else L.mc_load_ir_parts)(*args, _ref(p))
    return rc, L.mc_last_error().decode()


def test_a_step_that_is_off_refuses_what_the_match_load_refuses_message_for_message():
    """Parts NULL, and MC_PARTS_OFF with 0xA5 in every other byte: mc_load_ir_match's and mc_load_ir_sweep_match's own (rc, message),
    from the same library, row by row."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    off = _lib.McIrParts()
    C.memset(C.byref(off), 0xA5, C.sizeof(off))
    off.mode = _lib.MC_PARTS_OFF
    match, filt, phase, tail, shape = _others()
    good = _lib.McIrMatch()
    L.mc_default_ir_match(C.byref(good))
    good.mode = _lib.MC_MATCH_TARGET
    rows = []
    for m, f, p, t, s in ((match, filt, phase, tail, shape), (None, filt, phase, tail, shape), (None, None, phase, tail, shape), (None, None, None, tail, shape),
                          (None, None, None, None, shape), (None, None, None, None, None), (good, None, None, None, None)):
        for kw in (dict(), dict(rates=(0, 0)), dict(rates=(1, 2)), dict(frames=0), dict(lr=False), dict(tlr=False), dict(G=0), dict(flr=False, fG=0)):
            rows.append((L.mc_load_ir_match, L.mc_load_ir_parts, _file_args(shape=s, tail=t, phase=p, filt=f, match=m, **kw)))
        for kw in (dict(), dict(ir_frames=0), dict(lr=False), dict(tlr=False)):
            rows.append((L.mc_load_ir_sweep_match, L.mc_load_ir_sweep_parts, _sweep_args(tail=t, phase=p, filt=f, match=m, **kw)))
    seen = set()
    for wrapped, load, (args, keep) in rows:
        rc0 = wrapped(*args)
        want = L.mc_last_error().decode()
        seen.add(want)
        assert rc0 == -1
        for p in (None, C.byref(off)):
            assert load(*args, p) == rc0 and L.mc_last_error().decode() == want, want
    print(len(rows), "rows,", len(seen), "different refusals compared")
    assert len(rows) >= 36 and len(seen) >= 10


def test_the_loads_refuse_in_the_documented_order_before_the_engine_is_looked_at():
    """No engine is passed: a call that gets past the checks ends at "null argument", the load's own first check."""
    match, filt, phase, tail, shape = _others()
    for name, fields in BAD_FIELDS:
        for rates in ((0, 0), (8000, 8000), (1, 2)):  # (the parts come before the rates)
            rc, msg = _load(_parts(**fields), rates=rates)
            assert rc == -1 and name in msg, (name, msg)
        rc, msg = _load(_parts(**fields), sweep=True)
        assert rc == -1 and name in msg, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):
        rc, msg = _load(_parts(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # each bad field before a bad match field; a good parts struct lets the match speak, then the others in the wrapped call's order
    for sweep, kw in ((False, dict(rates=(8000, 8000), shape=shape, tail=tail, phase=phase, filt=filt, match=match)),
                      (True, dict(tail=tail, phase=phase, filt=filt, match=match))):
        match.amount, filt.reg_db = 2.0, 1.0
        for name, fields in BAD_FIELDS:
            rc, msg = _load(_parts(**fields), sweep=sweep, **kw)
            assert rc == -1 and name in msg and "amount" not in msg, (name, msg)
        rc, msg = _load(_parts(), sweep=sweep, **kw)
        assert rc == -1 and "amount" in msg, msg
        match.amount = 1.0
        rc, msg = _load(_parts(), sweep=sweep, **kw)
        assert rc == -1 and "reg_db" in msg, msg
    # the step's limits come after the match's: hi_hz above half the session's rate first, then frames_out, then the muted parts
    match.amount, match.hi_hz = 1.0, 30000.0
    too_long = _parts(frames_out=100 + (1 << 24) + 1)
    rc, msg = _load(too_long, match=match)
    assert rc == -1 and "hi_hz" in msg, msg
    match.hi_hz = 0.0
    rc, msg = _load(too_long, match=match)
    assert rc == -1 and "frames_out" in msg and "100 frames" in msg, msg
    rc, msg = _load(_parts(flags=7), match=match)
    assert rc == -1 and "every part" in msg, msg
    rc, msg = _load(_parts(flags=3, direct_end=20, early_end=200), match=match)  # (the late part is empty)
    assert rc == -1 and "every part" in msg, msg
    rc, msg = _load(_parts(frames_out=100 + (1 << 24)), match=match)
    assert rc == -1 and "null argument" in msg, msg
    # the step sees what the match hands on: a linear-phase match of 100 frames with a delay of 28 gives 128
    match.phase, match.delay = 1, 28
    rc, msg = _load(_parts(frames_out=128 + (1 << 24) + 1), match=match)
    assert rc == -1 and "frames_out" in msg and "128 frames" in msg, msg
    rc, msg = _load(_parts(frames_out=128 + (1 << 24)), match=match)
    assert rc == -1 and "null argument" in msg, msg
    # and without a match what the filter hands on: 100 and 29 frames give 128
    filt.reg_db = 60.0
    rc, msg = _load(_parts(frames_out=128 + (1 << 24) + 1), filt=filt, fG=29)
    assert rc == -1 and "frames_out" in msg and "128 frames" in msg, msg
    # sweeps: the limits after the lengths; the pointers last
    rc, msg = _load(_parts(frames_out=900 + (1 << 24) + 1), sweep=True)
    assert rc == -1 and "frames_out" in msg and "900 frames" in msg, msg
    rc, msg = _load(_parts(flags=7), sweep=True, ir_frames=0)
    assert rc == -1 and "every part" not in msg, msg
    rc, msg = _load(_parts(flags=7), sweep=True, lr=False)
    assert rc == -1 and "every part" in msg, msg
    rc, msg = _load(_parts(), sweep=True, lr=False)
    assert rc == -1 and "null lr" in msg, msg
    rc, msg = _load(_parts(), sweep=True)
    assert rc == -1 and "null argument" in msg, msg
    # without a tail a bad shape comes before the limits, with one after them
    rc, msg = _load(_parts(flags=7), shape=shape)
    assert rc == -1 and "trim_db" in msg, msg
    tail.width = 1.0
    rc, msg = _load(_parts(flags=7), shape=shape, tail=tail, rates=(8000, 8000))
    assert rc == -1 and "every part" in msg, msg
    rc, msg = _load(_parts(), lr=False)
    assert rc == -1 and "null argument" in msg, msg
