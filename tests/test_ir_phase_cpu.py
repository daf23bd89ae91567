"""The float64 restatement of the phase step (tests/ir_phase_np.py) against analysis, its invariants and its known answers, and
mc_ir_phase with mc_ir_phase_plan and every refusal through the ABI (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ir_phase_np as P

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")
CSRC = os.path.join(os.path.dirname(HEADER), "..", "cuda_audio_amd", "csrc")


# -- against analysis -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,r_max,oversample", [(16, 0.9, 64), (40, 0.95, 64), (16, 0.9, 8)])
def test_reflected_zeros_come_back_inside(K, r_max, oversample):
    """A product of quadratic factors with every second one reflected outside the unit circle has the magnitude response of
    the all-inside product, which is the minimum-phase sequence of that response: 1e-12 of the peak."""
    x, want = P.quadratic_product(K, r_max)
    assert np.abs(x - want).max() > 0.1 * np.abs(want).max()  # (the input is far from the answer)
    y, clamped = P.min_phase_channel(x, oversample)
    dev = np.abs(y - want).max() / np.abs(want).max()
    print(f"K {K}, r_max {r_max}, oversample {oversample}: deviation {dev:.2e} of the peak")
    assert dev <= 1e-12 and clamped == 0


# -- invariants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [127, 4096, 5000])
def test_energy_moves_to_the_front_and_stays(F):
    x = P.delayed_noise(F)
    y, info = P.min_phase64(x)
    cx, cy = P.cumulative_energy(x), P.cumulative_energy(y)
    E = cx[-1]
    worst = (cy - cx).min() / E
    print(f"F {F}: worst cumulative energy difference {worst:.2e} of E, E_out / E_in - 1 = {info['energy_out'] / info['energy_in'] - 1.0:.2e}, "
          f"centre {info['centre_in']:.1f} -> {info['centre_out']:.1f}")
    assert worst >= -1e-5
    assert info["energy_out"] / info["energy_in"] >= 1.0 - 1e-5
    assert np.abs(y[:, 0]).argmax() == 0 and np.abs(y[:, 1]).argmax() == 0
    assert info["frames"] == F and info["nfft"] == P.nfft_of(F) and info["centre_out"] < info["centre_in"] - F // 8 + 1
    assert abs(info["energy_in"] - float((x.astype(np.float64) ** 2).sum())) <= 1e-12 * info["energy_in"]


# -- known answers ----------------------------------------------------------------------------------------------------
def test_a_delayed_impulse_comes_out_at_frame_zero():
    x = np.zeros((300, 2), np.float32)
    x[123, 0], x[7, 1] = 0.5, -0.25
    y, info = P.min_phase64(x)
    want = np.zeros((300, 2))
    want[0] = (0.5, 0.25)  # (the magnitude response has no sign)
    assert np.abs(y - want).max() <= 1e-15
    assert info["centre_in"] == (123 * 0.25 + 7 * 0.0625) / 0.3125 and abs(info["centre_out"]) <= 1e-20 and info["clamped"] == (0, 0)


def test_half_one_becomes_one_half():
    """[0.5, 1] has its zero at -2; reflected to -1/2 it is [1, 0.5].  Nfft = 16: the even cepstrum -(-1/2)^|n| / (2 |n|) aliases,
    and the largest term that lands on the folded c[1] is twice that of n = -15, 2^-15 / 15 = 2.03e-6: the 2e-6 of the aliasing.
    The terms after it (n = 17 and on, and c[0]'s through y[0]) are under 5 % of it."""
    y, _ = P.min_phase_channel([0.5, 1.0], 8)
    assert P.nfft_of(2) == 16
    print("deviation", np.abs(y - [1.0, 0.5]))
    assert np.abs(y - [1.0, 0.5]).max() <= 1.05 * 2.0 ** -15 / 15.0
    y, _ = P.min_phase_channel([0.5, 1.0], 64)
    assert np.abs(y - [1.0, 0.5]).max() <= 1e-15


@pytest.mark.parametrize("F", [1, 2, 3])
def test_the_shortest_irs(F):
    x = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, -0.5]][3 - F:])
    y, info = P.min_phase64(x)
    want = np.zeros((F, 2))
    want[0] = (1.0, 0.5)
    assert np.abs(y - want).max() <= 1e-15 and info["nfft"] == (16 if F < 3 else 32) and info["frames"] == F
    assert info["energy_in"] == info["energy_out"] == 1.25 and info["centre_in"] == F - 1.0


def test_a_zero_channel_stays_zero():
    x = P.delayed_noise(500).copy()
    x[:, 1] = 0.0
    y, info = P.min_phase64(x)
    assert not y[:, 1].any() and y[:, 0].any() and info["clamped"][1] == 0
    y, info = P.min_phase64(np.zeros((40, 2)))
    assert not y.any() and info["energy_in"] == info["energy_out"] == 0.0 and info["centre_in"] == info["centre_out"] == 0.0


def test_the_floor_clamps_deep_notches():
    """[1, -1] has a zero on the unit circle at DC: bin 0 is clamped (p = 0 exactly), and the result is finite."""
    y, clamped = P.min_phase_channel([1.0, -1.0], 8, floor_db=60.0)
    assert clamped == 1 and np.isfinite(y).all() and y.any()


# -- plan and ABI -----------------------------------------------------------------------------------------------------
def _phase(**fields):
    from cuda_audio_amd import _lib

    p = _lib.McIrPhase()
    _lib.load().mc_default_ir_phase(C.byref(p))
    p.mode = _lib.MC_PHASE_MINIMUM
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def test_the_struct_has_its_documented_size_and_defaults():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_phase\) = (\d+)", src).group(1))
    p = _lib.McIrPhase()
    _lib.load().mc_default_ir_phase(C.byref(p))
    assert C.sizeof(_lib.McIrPhase) == size == p.struct_size == 16
    assert (p.mode, p.floor_db, p.over_log2) == (_lib.MC_PHASE_OFF, 120.0, 3)
    assert re.search(r"enum \{ MC_PHASE_OFF = 0, MC_PHASE_MINIMUM = 1 \};", src)
    assert {"mc_default_ir_phase", "mc_ir_phase_plan", "mc_load_ir_phase", "mc_load_ir_sweep_phase", "mc_ir_phase_info"} <= set(_lib.SYMBOLS)
    # the transform's geometry as the GPU cases mirror it
    fft = open(os.path.join(CSRC, "fft64.hip.h")).read()
    assert int(re.search(r"constexpr int F64_S_LOG2 = (\d+);", fft).group(1)) == 11
    step = open(os.path.join(CSRC, "irphase.hip.h")).read()
    assert re.search(r"constexpr uint64_t PH_MAX_FRAMES = 1ull << 21;", step) and P.MAX_FRAMES == 1 << 21 and P.MAX_NFFT == 1 << 22


def test_the_python_dataclass():
    from cuda_audio_amd.engine import IrPhase

    p = IrPhase().to_c()
    assert (p.struct_size, p.mode, p.floor_db, p.over_log2) == (16, 1, 120.0, 3)
    p = IrPhase(mode="off", floor_db=80.0, oversample=64).to_c()
    assert (p.mode, p.floor_db, p.over_log2) == (0, 80.0, 6)
    assert IrPhase(oversample=2).to_c().over_log2 == 1
    for bad in (dict(mode="linear"), dict(oversample=1), dict(oversample=3), dict(oversample=128), dict(oversample=0)):
        with pytest.raises(ValueError):
            IrPhase(**bad).to_c()


def _plan(p, frames, out=True):
    from cuda_audio_amd import _lib

    L = _lib.load()
    buf = (C.c_double * 4)(-1.0, -1.0, -1.0, -1.0)
    rc = L.mc_ir_phase_plan(C.byref(p) if p is not None else None, frames, buf if out else None)
    return rc, L.mc_last_error().decode(), list(buf)


def test_the_plan():
    from cuda_audio_amd.engine import IrPhase, phase_plan

    for F in (1, 2, 3, 16, 17, 127, 256, 257, 4096, 5000, 40000, 1 << 18, (1 << 18) + 1, 1 << 19):
        for over in (2, 8, 64):
            N = P.nfft_of(F, over)
            if N > P.MAX_NFFT:
                continue
            got = phase_plan(IrPhase(oversample=over), F)
            passes = 1 if N <= 2048 else 2
            assert got["nfft"] == N and got["passes"] == passes, (F, over, got)
            # two buffers of Nfft double2, a third when the transform has two passes, and 16 bytes of partials per 256 points
            assert got["device_bytes"] == (passes + 1) * 16 * N + 16 * ((N + 255) // 256), (F, over, got)
    rc, _, out = _plan(_phase(mode=0), 1000)  # (off is planned as if it were on)
    assert rc == 0 and out == [8192.0, 2.0, 3.0 * 16 * 8192 + 16 * 32, 0.0]


BAD_FIELDS = [("struct_size", dict(struct_size=12)), ("mode", dict(mode=2)), ("floor_db", dict(floor_db=39.9)), ("floor_db", dict(floor_db=300.5)),
              ("floor_db", dict(floor_db=float("nan"))), ("over_log2", dict(over_log2=0)), ("over_log2", dict(over_log2=7))]
ORDER = [("mode", dict(mode=9)), ("floor_db", dict(floor_db=1.0)), ("over_log2", dict(over_log2=99))]


def test_the_plan_refuses():
    rc, msg, _ = _plan(None, 100)
    assert rc == -1 and "null phase" in msg
    for name, fields in BAD_FIELDS:
        rc, msg, out = _plan(_phase(**fields), 100)
        assert rc == -1 and name in msg and out == [-1.0] * 4, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):  # (of two bad fields the earlier one is named)
        rc, msg, _ = _plan(_phase(**dict(a, **b)), 100)
        assert rc == -1 and first in msg, (first, msg)
    rc, msg, _ = _plan(_phase(), 0)
    assert rc == -1 and "empty" in msg
    rc, msg, _ = _plan(_phase(), (1 << 21) + 1)
    assert rc == -1 and "frames" in msg
    rc, msg, _ = _plan(_phase(over_log2=1), 1 << 21)
    assert rc == 0
    for F, lg in (((1 << 19) + 1, 3), (1 << 21, 2), (1 << 17, 6), ((1 << 16) + 1, 6)):
        rc, msg, _ = _plan(_phase(over_log2=lg), F)
        assert rc == -1 and "over_log2" in msg, (F, lg, msg)
    rc, msg, _ = _plan(_phase(), 100, out=False)
    assert rc == -1 and "null out" in msg


def _load(p, frames=100, rates=(0, 0), lr=True, engine=None, tail=None, shape=None):
    from cuda_audio_amd import _lib

    L = _lib.load()
    buf = np.zeros((max(min(frames, 1000), 1), 2), np.float32)
    rc = L.mc_load_ir_phase(engine, 0, buf.ctypes.data_as(C.POINTER(C.c_float)) if lr else None, frames, 1024, rates[0], rates[1], shape, None, None, tail,
                            C.byref(p) if p is not None else None)
    return rc, L.mc_last_error().decode()


def _load_sweep(p, ir_frames=900, tail=None):
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import Sweep

    L = _lib.load()
    rec = np.zeros((5000, 2), np.float32)
    sw = Sweep(frames=4096, f1_hz=20.0, f2_hz=3000.0, rate=8000).to_c()
    rc = L.mc_load_ir_sweep_phase(None, 0, rec.ctypes.data_as(C.POINTER(C.c_float)), len(rec), 1024, C.byref(sw), 0, ir_frames, None, None, None, tail,
                                  C.byref(p) if p is not None else None)
    return rc, L.mc_last_error().decode()


def test_the_loads_refuse_every_field_before_the_engine_is_looked_at():
    """No engine is passed: a call that gets past the checks ends at "null argument", the load's own first check."""
    from cuda_audio_amd import _lib

    for name, fields in BAD_FIELDS:
        for rates in ((0, 0), (8000, 8000), (1, 2)):  # (the phase comes before the rates)
            rc, msg = _load(_phase(**fields), rates=rates)
            assert rc == -1 and name in msg, (name, msg)
        rc, msg = _load_sweep(_phase(**fields))
        assert rc == -1 and name in msg, (name, msg)
    for (first, a), (_, b) in zip(ORDER, ORDER[1:]):
        rc, msg = _load(_phase(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # the phase before a bad tail and a bad shape; a good phase lets them speak
    tail = _lib.McIrTail()
    L = _lib.load()
    L.mc_default_ir_tail(C.byref(tail))
    tail.mode, tail.width = _lib.MC_TAIL_EXTEND, 7.0
    shape = _lib.McIrShape()
    L.mc_default_ir_shape(C.byref(shape))
    shape.trim_db = 5.0
    rc, msg = _load(_phase(over_log2=0), rates=(8000, 8000), tail=C.byref(tail), shape=C.byref(shape))
    assert rc == -1 and "over_log2" in msg
    rc, msg = _load(_phase(), rates=(8000, 8000), tail=C.byref(tail), shape=C.byref(shape))
    assert rc == -1 and "width" in msg
    rc, msg = _load(_phase(), shape=C.byref(shape))
    assert rc == -1 and "trim_db" in msg
    rc, msg = _load_sweep(_phase(), tail=C.byref(tail))
    assert rc == -1 and "width" in msg
    # the limits: the frames, then over_log2 with the frames; rates 0 / 0 pass without a tail, and one bad rate is named
    rc, msg = _load(_phase(), frames=(1 << 21) + 1)
    assert rc == -1 and "frames" in msg and "2097152" in msg, msg
    rc, msg = _load(_phase(over_log2=4), frames=(1 << 18) + 1)
    assert rc == -1 and "over_log2" in msg, msg
    rc, msg = _load(_phase(), frames=100000, rates=(8000, 384000))  # (the limit holds for the frames at the session's rate)
    assert rc == -1 and "frames" in msg, msg
    rc, msg = _load(_phase(), rates=(8000, 7999))
    assert rc == -1 and "session_rate" in msg, msg
    tail.width = 1.0
    rc, msg = _load(_phase(), rates=(0, 0), tail=C.byref(tail))  # (a tail needs the rate)
    assert rc == -1 and "session_rate" in msg, msg
    tail.length = (1 << 21) + 5
    rc, msg = _load(_phase(), rates=(8000, 8000), tail=C.byref(tail))  # (the frames the tail step hands on)
    assert rc == -1 and "frames" in msg and "2097157" in msg, msg
    rc, msg = _load_sweep(_phase(over_log2=6), ir_frames=(1 << 16) + 1)
    assert rc == -1 and "over_log2" in msg, msg
    for rc, msg in (_load(_phase()), _load(_phase(), lr=False), _load_sweep(_phase())):
        assert rc == -1 and "null" in msg, msg
    # off and null: the wrapped load itself, which here ends at its own null engine
    off = _phase(mode=0, struct_size=3, floor_db=float("nan"), over_log2=77)
    for p in (None, off):
        rc, msg = _load(p)
        assert rc == -1 and "null argument" in msg, msg
