"""The interaural cross-correlation on the device (mc_ir_iacc, csrc/iriacc.hip.h) against the float64 restatement
(tests/ir_iacc_np.py) applied to the taps the engine stores (Convolution.ir_taps).

Tolerances (ir_iacc_np.check_against), derived, not measured:
  * tau*, the status, the origin, N and the first late tap k are equal integers;
  * broadband rows: a sum of n products added in any order is within n 2^-53 sum |products| <= n 2^-53 sqrt(E_L E_R)
    (Cauchy-Schwarz) of any other order, so IACF differs by at most n 2^-53 = 7.8e-12 at the 70 000 taps of the longest case; the
    two energies under the square root add as much again in relative terms.  IACC, IACF(tau*), IACF(0) and every curve entry are
    held to 1e-10 absolute;
  * banded rows sit behind the chunked recurrence of DESIGN 2.8, which the decay tests hold to 1e-6 against the sequential
    loops: 1e-6 absolute;
  * the energies to 1e-6 relative and the level difference to 1e-6 dB, as the decay tests hold theirs.
Every comparison asserts first that the restatement's maximum stands out from every other lag by more than 1e-6 (assert_margins),
so that a flipped argmax cannot pass for rounding.  The largest differences seen are printed."""
import ctypes as C
import functools
import hashlib
import math

import numpy as np
import pytest

from ir_iacc_np import assert_margins, check_against, default_lag, iacc, pair_ir

pytestmark = pytest.mark.gpu

RATE = 8000
RUN = 2304  # csrc/iriacc.hip.h's IACC_RUN: the taps of a window that one workgroup sums
MAX_LAG = 1024


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("iriacc", n_ref, sample_rate=rate, **kw)


def _compare(c, idx, rate, margins=True, **query):
    """ir_iacc of IR idx, with the curve, against the restatement of its stored taps."""
    want = iacc(c.ir_taps(idx), rate, **query)
    if margins:
        assert_margins(want)
    got = c.ir_iacc(idx, curve=True, **query)
    for key, row in got["rows"].items():
        print(key, {k: f"{v:.9g}" for k, v in row.items()})
    check_against(got, want)
    return got, want


@functools.lru_cache(maxsize=None)
def _pair(n, lead=0, seed=7, t60=0.25):
    return pair_ir(n=n, lead=lead, rate=RATE, t60=t60, seed=seed)


def _delayed(n, d):
    L = _pair(n)[:, 0]
    R = np.zeros_like(L)
    if d >= 0:
        R[d:] = L[:n - d]
    else:
        R[:d] = L[-d:]
    return np.stack([L, R], axis=1)


def _flipped(n):
    L = _pair(n)[:, 0]
    return np.stack([L, -L], axis=1)


def _silent_r(n):
    ir = _pair(n).copy()
    ir[:, 1] = 0.0
    return ir


# (n_ref, the IR, query): the smallest shapes that reach every branch of the kernel and its launch
CASES = {
    "default query": (16384, lambda: _pair(6000), dict()),
    "T = 0": (16384, lambda: _pair(6000), dict(max_lag=0)),
    "T = 1024, short": (16384, lambda: _pair(700), dict(max_lag=MAX_LAG, onset_db=0.0)),  # the early window of 640 taps is shorter than T
    "T = 1024, long": (131072, lambda: _pair(70000, t60=4.0), dict(max_lag=MAX_LAG)),   # 3e8 fma
    "N a run multiple": (16384, lambda: _pair(2 * RUN), dict(max_lag=64, onset_db=0.0)),
    "N one over": (16384, lambda: _pair(2 * RUN + 1), dict(max_lag=64, onset_db=0.0)),
    "N one under": (16384, lambda: _pair(2 * RUN - 1), dict(max_lag=64, onset_db=0.0)),
    "split at a run boundary": (16384, lambda: _pair(6000), dict(max_lag=64, split=RUN, onset_db=0.0)),
    "split one past": (16384, lambda: _pair(6000), dict(max_lag=64, split=RUN + 1, onset_db=0.0)),
    "split one before": (16384, lambda: _pair(6000), dict(max_lag=64, split=RUN - 1, onset_db=0.0)),
    "split = 1": (16384, lambda: _pair(6000), dict(max_lag=8, split=1, onset_db=0.0)),
    "split past N": (16384, lambda: _pair(3000), dict(max_lag=8, split=5000)),
    "origin in mid-run": (16384, lambda: _pair(4000, lead=300), dict(max_lag=8, onset_db=-20.0)),
    "onset_db 0": (16384, lambda: _pair(4000, lead=300), dict(max_lag=8, onset_db=0.0)),
    "end in mid-run": (16384, lambda: _pair(6000), dict(max_lag=64, end=3001)),
    "delay -T": (16384, lambda: _delayed(3000, -8), dict(max_lag=8, onset_db=0.0)),
    "delay +T": (16384, lambda: _delayed(3000, 8), dict(max_lag=8, onset_db=0.0)),
    "delay T + 1": (16384, lambda: _delayed(3000, 9), dict(max_lag=8, onset_db=0.0)),
    "R = -L": (16384, lambda: _flipped(3000), dict(max_lag=8)),
    "silent R": (16384, lambda: _silent_r(3000), dict(max_lag=8)),
    "one band": (16384, lambda: _pair(6000), dict(bands=(1000.0,), max_lag=8)),
    "three bands": (16384, lambda: _pair(6000, lead=37), dict(bands=(250.0, 1000.0, 2000.0), max_lag=16)),
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
    rows = got["rows"]
    T = got["max_lag"]
    assert got["taps"] == (query.get("end") or len(ir)) and T == query.get("max_lag", default_lag(RATE))
    assert got["curve"].shape == (1 + len(query.get("bands", ())), 3, 2 * T + 1)
    if case == "default query":
        assert T == 8 and got["split"] == got["origin"] + 640 and all(r["status"] == 0 and 0.3 < r["iacc"] < 0.9 for r in rows.values())
    if case == "T = 0":
        assert all(r["lag"] == 0 and r["iacf"] == r["iacf0"] for r in rows.values())
    if "split" in query and case != "split past N":
        assert got["split"] == query["split"]
    if case == "split past N":
        assert got["split"] == got["taps"] and rows[(0, "late")]["status"] == 1 and np.isnan(got["curve"][0, 1]).all()
        assert np.array(list(rows[(0, "early")].values())).tobytes() == np.array(list(rows[(0, "all")].values())).tobytes()
    if case == "origin in mid-run":
        assert got["origin"] >= 300
    if case == "onset_db 0":
        assert got["origin"] == 0
    if case.startswith("delay"):
        d = {"delay -T": -8, "delay +T": 8}.get(case)
        if d is None:
            assert all(r["iacc"] < 0.2 for r in rows.values())
        else:
            assert all(r["lag"] == d and r["iacf"] > 0.9 for r in rows.values())
    if case == "R = -L":
        assert all(r["lag"] == 0 and abs(r["iacf"] + 1.0) <= 1e-12 for r in rows.values())
    if case == "silent R":
        assert all(r["status"] == 1 and r["energy_l"] > 0.0 and r["energy_r"] == 0.0 for r in rows.values()) and np.isnan(got["curve"]).all()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_nothing_is_disturbed_and_two_calls_agree(gpu_lib):
    """The stored taps and ir_info are byte for byte the same before and after, a processed batch with calls in between is that of a
    run without them, and two calls return the same bits in rows and curve."""
    from cuda_audio_amd.synth import make_input

    ir = _pair(6000, lead=37)
    x = make_input(32 * 256)
    query = dict(bands=(1000.0,), max_lag=64, curve=True)
    runs, asked = [], []
    for ask in (False, True):
        c = _conv(16384, max_batch=32)
        c.prepare(0, ir)
        before = (c.ir_taps(0).tobytes(), c.ir_info(0))
        if ask:
            asked.append(c.ir_iacc(0, **query))
            assert (c.ir_taps(0).tobytes(), c.ir_info(0)) == before
        first = c.process(x[0, :16 * 256], x[1, :16 * 256])
        if ask:
            asked.append(c.ir_iacc(0, **query))
            asked.append(c.ir_iacc(0, max_lag=MAX_LAG))
        second = c.process(x[0, 16 * 256:], x[1, 16 * 256:])
        runs.append((_sha(c.ir_taps(0)), _sha(first), _sha(second), c.ir_info(0)))
        c.close()
    assert runs[0] == runs[1]
    a, b = asked[0], asked[1]
    assert (a["origin"], a["taps"], a["split"]) == (b["origin"], b["taps"], b["split"]) == (38, 6037, 678)
    assert a["curve"].tobytes() == b["curve"].tobytes()
    for key, row in a["rows"].items():
        assert np.array(list(row.values())).tobytes() == np.array(list(b["rows"][key].values())).tobytes()


def _raw(c, idx, rows=True, info=True, **fields):
    """mc_ir_iacc with the struct's fields set directly; returns (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    q = _lib.McIaccQuery()
    L.mc_default_iacc_query(C.byref(q))
    q.rate, q.max_lag = RATE, 8
    for k, v in fields.items():
        if k == "reserved":
            q.reserved[0], q.reserved[1] = v
        elif k == "centre_hz":
            for j, hz in enumerate(v):
                q.centre_hz[j] = hz
        else:
            setattr(q, k, v)
    r = np.zeros((11 * 3, 8))
    i = (C.c_uint64 * 3)()
    rc = L.mc_ir_iacc(c._h, idx, C.byref(q), r.ctypes.data_as(C.POINTER(C.c_double)) if rows else None, None, i if info else None)
    return rc, L.mc_last_error().decode()


BAD = [("struct_size", dict(struct_size=84)), ("rate", dict(rate=7999)), ("n_bands", dict(n_bands=11)), ("max_lag", dict(max_lag=MAX_LAG + 1)),
       ("centre_hz[0]", dict(n_bands=1, centre_hz=(5.0,))), ("q 64", dict(q=64.0)), ("onset_db", dict(onset_db=1.0)), ("reserved", dict(reserved=(0, 1)))]


def test_refusals(gpu_lib):
    from cuda_audio_amd._lib import McError

    ir = _pair(3000)
    single = _conv(16384, form="single")
    single.prepare(0, ir)
    with pytest.raises(McError) as ex:
        single.ir_iacc(0)
    assert ex.value.code == -3
    single.close()
    c = _conv(16384)
    c.prepare(0, ir)
    before = c.ir_iacc(0, max_lag=8, curve=True)
    for idx in (1, 255, 256, 1 << 40):
        with pytest.raises(McError) as ex:
            c.ir_iacc(idx, curve=True)
        assert ex.value.code == -1 and "IR not loaded" in str(ex.value)
    for idx in (0, 1):  # the query, then the two arrays, come before the index
        for name, fields in BAD:
            rc, msg = _raw(c, idx, **fields)
            assert rc == -1 and name in msg, (name, rc, msg)
        for name, args in (("rows", dict(rows=False)), ("info", dict(info=False))):
            rc, msg = _raw(c, idx, **args)
            assert rc == -1 and "null " + name in msg, (name, rc, msg)
    with pytest.raises(McError, match="max_lag"):
        c.ir_iacc(0, max_lag=MAX_LAG + 1, curve=True)
    assert _raw(c, 0)[0] == 0
    np.testing.assert_array_equal(c.ir_taps(0), ir)
    after = c.ir_iacc(0, max_lag=8, curve=True)  # the engine still answers, with the same bits
    assert before["curve"].tobytes() == after["curve"].tobytes()
    c.close()


def test_the_work_bound_comes_after_the_index(gpu_lib):
    """3 ceil(N / 2304) (2T + 3) <= 2^23 partial sums: at T = 1024 that is 1363 runs, 3 140 352 taps.  One tap more is refused with
    a message that names max_lag; with `end` under the bound the same IR is measured (only asked about at a small `end`, not run
    at that size)."""
    n = 1363 * RUN + 1
    c = _conv(1 << 22)
    c.prepare(0, _pair(n, t60=100.0))
    rc, msg = _raw(c, 0, max_lag=MAX_LAG)
    assert rc == -1 and "max_lag" in msg and "partial sums" in msg, msg
    rc, msg = _raw(c, 1, max_lag=MAX_LAG)
    assert rc == -1 and "IR not loaded" in msg, msg
    assert _raw(c, 0, max_lag=MAX_LAG, end=n)[0] == -1
    assert _raw(c, 0, max_lag=8)[0] == 0
    assert _raw(c, 0, max_lag=MAX_LAG, end=RUN + 5)[0] == 0
    c.close()


SYNTH = dict(frames=6000, seed=2, t60=4000, late_gain=1.0, direct=0.0)


@pytest.mark.parametrize("width", [0.0, 0.3, 1.0])
def test_a_synthesised_width_reads_back(gpu_lib, width):
    """mc_ir_synth's late field is R = rho gA + sqrt(1 - rho^2) gB with rho = 1 - width, so its late broadband IACF(0) estimates rho.
    The estimate of a correlation from decaying noise has the standard error (1 - rho^2) / sqrt(N_eff), N_eff = (sum e)^2 / sum e^2
    with e = y_L^2 + y_R^2 over the late window (mc_ir_decay's e of the L + R set: the taps that carry the sum).  The restatement of
    tests/ir_synth_np.py's frames is held to 4 standard errors first, on the CPU (seed and length were chosen there); width 0
    makes L == R bit for bit, so the value is 1 to 1e-12.  The device then equals the restatement to 1e-10, and
    tail_width_from_iacc turns the reading back into the width to within those errors."""
    import ir_synth_np
    from cuda_audio_amd.engine import IrSynth, IrTail, tail_width_from_iacc

    rho = 1.0 - float(np.float32(width))
    frames = ir_synth_np.frames(width=width, **SYNTH)
    want = iacc(frames, RATE, max_lag=8, onset_db=0.0)
    y = frames[want["split"]:].astype(np.float64)
    e = (y * y).sum(axis=1)
    n_eff = float(e.sum() ** 2 / (e * e).sum())
    se = (1.0 - rho * rho) / math.sqrt(n_eff)
    read = want["rows"][(0, "late")]["iacf0"]
    print(f"restatement: late IACF(0) {read:.6f}, rho {rho:.6f}, N_eff {n_eff:.1f}, standard error {se:.4f}")
    assert abs(read - rho) <= (4.0 * se if width else 1e-12)
    c = _conv(16384)
    c.prepare_synth(0, IrSynth(width=width, **SYNTH))
    got, _ = _compare(c, 0, RATE, max_lag=8, onset_db=0.0)
    c.close()
    late = got["rows"][(0, "late")]
    assert late["status"] == 0 and abs(late["iacf0"] - read) <= 1e-10
    assert abs(late["iacf0"] - rho) <= (4.0 * se if width else 1e-12)
    tail = tail_width_from_iacc(IrTail(mode="extend"), got)
    assert tail.width == float(np.float32(min(max(1.0 - late["iacf0"], 0.0), 1.0)))
    assert abs(tail.width - float(np.float32(width))) <= 4.0 * se + 1e-7


def test_a_rendered_room_reads_its_spacing(gpu_lib):
    """tests/test_host_ir_room.py's room at 48 kHz.  With spacing 0 the two receivers are one: IACC 1 at lag 0 in every window.  With
    its own spacing (0.3 m: 42 taps at the speed of sound, inside the default 48) the device reads the restatement's values, and
    the early IACC is below 1."""
    import dataclasses

    from cuda_audio_amd.engine import IrRoom, IrSynth
    from test_host_ir_room import FRAMES, ROOM

    rate = 48000
    synth = IrSynth(frames=FRAMES, late_gain=0.0)
    c = _conv(16384, rate=rate)
    c.prepare_synth(0, synth, room=dataclasses.replace(IrRoom(**ROOM), spacing=0.0))
    got, _ = _compare(c, 0, rate)
    assert got["max_lag"] == 48
    for row in got["rows"].values():
        assert row["status"] == 0 and row["lag"] == 0 and abs(row["iacc"] - 1.0) <= 1e-12 and abs(row["level_db"]) <= 1e-9
    c.prepare_synth(0, synth, room=IrRoom(**ROOM))
    got, _ = _compare(c, 0, rate)
    c.close()
    early = got["rows"][(0, "early")]
    assert early["status"] == 0 and early["iacc"] < 0.99
