"""The speech transmission index on the device (mc_ir_sti, csrc/irsti.hip.h) against the float64 restatement (tests/ir_sti_np.py)
applied to the taps the engine stores (Convolution.ir_taps).

Tolerances (ir_sti_np.check_against), derived, not measured:
  * the status, the origin and N are equal integers;
  * broadband m: C, S and E are sums of n non-negative squares times weights of modulus <= 1, so two orders of addition differ by
    at most n 2^-53 E each; with numerator and denominator that is twice n 2^-53 = 6.7e-11 at the 300 000 taps of the longest
    case, plus the rotator's 8.2e-15 (the header of csrc/irsti.hip.h): held to 1e-10 absolute;
  * broadband MTI to 1e-9: dTI/dm = 10 / (30 ln 10 m (1 - m)) <= 5 between the clamps at m = 0.0307 and 0.9693;
  * banded rows sit behind the chunked recurrence of DESIGN 2.8, which the decay tests hold to 1e-6 against the sequential
    loops: m to 1e-6 absolute, MTI and STI to 1e-5;
  * the energies to 1e-6 relative, as the decay tests hold theirs;
  * NaN where and only where the restatement has it.
The largest differences seen are printed."""
import ctypes as C
import functools
import hashlib
import math

import numpy as np
import pytest

from ir_iacc_np import pair_ir
from ir_sti_np import ALPHA, BETA, MOD_HZ, OCTAVES, check_against, f32, schroeder, sti

pytestmark = pytest.mark.gpu

RATE = 48000
RUN = 4096     # csrc/irsti.hip.h's STI_RUN: the taps from the origin on that one workgroup sums
STRETCH = 16   # ... and STI_STRETCH: the consecutive taps of one thread


def _conv(n_ref, rate=RATE, **kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)
    kw.setdefault("max_batch", 8)
    return Convolution("irsti", n_ref, sample_rate=rate, **kw)


def _compare(c, idx, rate, **query):
    """ir_sti of IR idx against the restatement of its stored taps."""
    want = sti(c.ir_taps(idx), rate, **query)
    got = c.ir_sti(idx, **query)
    print("sti", {k: f"{v:.9g}" for k, v in got["sti"].items()})
    for key, row in got["rows"].items():
        print(key, {k: f"{v:.9g}" for k, v in row.items()})
    check_against(got, want)
    return got, want


@functools.lru_cache(maxsize=None)
def _pair(n, lead=0, seed=7, t60=0.25):
    return pair_ir(n=n, lead=lead, rate=RATE, t60=t60, seed=seed)


def _spikes(d):
    ir = np.zeros((d + 300, 2), np.float32)
    ir[0] = ir[d] = 1.0
    return ir


def _silent_r(n):
    ir = _pair(n).copy()
    ir[:, 1] = 0.0
    return ir


NONE = dict(bands=(), alpha=(), beta=())             # broadband alone
ONE = dict(bands=(1000.0,), alpha=(1.0,), beta=())   # one band: no beta term
THREE = dict(bands=(500.0, 1000.0, 2000.0), alpha=(0.3, 0.4, 0.5), beta=(0.1, 0.1))

# (n_ref, the IR, query): the smallest shapes that reach every branch of the kernel and its launch
CASES = {
    "default query": (16384, lambda: _pair(6000), dict()),
    "N two runs": (16384, lambda: _pair(2 * RUN), dict(onset_db=0.0, **ONE)),
    "N one over": (16384, lambda: _pair(2 * RUN + 1), dict(onset_db=0.0, **ONE)),
    "N one under": (16384, lambda: _pair(2 * RUN - 1), dict(onset_db=0.0, **ONE)),
    "N under a stretch": (16384, lambda: _pair(STRETCH - 7), dict(onset_db=0.0, **NONE)),
    "N = 1": (16384, lambda: _pair(1), dict(onset_db=0.0, **NONE)),
    "origin in mid-run": (16384, lambda: _pair(6000, lead=300), dict(**ONE)),
    "end in mid-run": (16384, lambda: _pair(9000), dict(end=RUN + 905, onset_db=0.0, **ONE)),
    "spikes RUN - 1 apart": (16384, lambda: _spikes(RUN - 1), dict(onset_db=0.0, **NONE)),
    "spikes RUN apart": (16384, lambda: _spikes(RUN), dict(onset_db=0.0, **NONE)),
    "spikes RUN + 1 apart": (16384, lambda: _spikes(RUN + 1), dict(onset_db=0.0, **NONE)),
    "n_mod = 1": (16384, lambda: _pair(6000), dict(mod_hz=(3.15,), **ONE)),
    "n_mod = 16": (16384, lambda: _pair(6000), dict(mod_hz=MOD_HZ + (16.0, 50.0), **ONE)),
    "no bands": (16384, lambda: _pair(6000), dict(**NONE)),
    "one band": (16384, lambda: _pair(6000), dict(**ONE)),
    "seven bands": (16384, lambda: _pair(6000, lead=37, seed=3), dict(bands=OCTAVES, alpha=ALPHA, beta=BETA, q=2.0)),
    "noise": (16384, lambda: _pair(6000), dict(snr_db=(-3.0, 6.0, 120.0), **THREE)),
    "silent R": (16384, lambda: _silent_r(3000), dict(**THREE)),
    "all zero": (16384, lambda: np.zeros((3000, 2), np.float32), dict(**ONE)),
    "long carry": (524288, lambda: _pair(300000, t60=4.0), dict(**ONE)),
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
    rows, idx = got["rows"], got["sti"]
    bands = query.get("bands", OCTAVES)
    assert got["taps"] == (query.get("end") or len(ir))
    assert got["mtf"].shape == (1 + len(bands), 3, len(query.get("mod_hz", MOD_HZ)))
    if case == "default query":
        assert all(r["status"] == 0 for r in rows.values()) and all(0.3 < v < 1.0 for v in idx.values())
    if case in ("N = 1", "N under a stretch"):
        assert got["origin"] == 0
    if case == "N = 1":
        assert np.array_equal(got["mtf"], np.ones((1, 3, 14))) and all(r["mti"] == 1.0 for r in rows.values())
    if case == "origin in mid-run":
        assert got["origin"] >= 300
    if case.startswith("spikes"):
        d = len(ir) - 300
        comb = np.abs(np.cos(np.pi * np.array([f32(F) for F in MOD_HZ]) * d / RATE))
        assert np.max(np.abs(got["mtf"][0] - comb[None, :])) <= 1e-14 and rows[(0, "L")]["energy"] == 2.0
    if case == "no bands":
        assert all(math.isnan(v) for v in idx.values()) and all(r["status"] == 0 and 0.0 < r["mti"] < 1.0 for r in rows.values())
    if case == "one band":
        assert all(idx[s] == rows[(1, s)]["mti"] for s in ("L", "R", "LR"))  # alpha 1, no beta
    if case == "noise":
        clean = sti(ir, RATE, **THREE)
        assert np.max(np.abs(got["mtf"][1] * (1.0 + 10.0 ** 0.3) - clean["mtf"][1])) <= 1e-5 and all(idx[s] < clean["sti"][s] for s in idx)
    if case == "silent R":
        assert all(rows[(g, "R")]["status"] == 1 and rows[(g, "R")]["energy"] == 0.0 and rows[(g, "L")]["status"] == 0 for g in range(4))
        assert math.isnan(idx["R"]) and np.isnan(got["mtf"][:, 1]).all()
        assert got["mtf"][:, 0].tobytes() == got["mtf"][:, 2].tobytes() and np.float64(idx["L"]).tobytes() == np.float64(idx["LR"]).tobytes()
        assert all(rows[(g, "L")] == rows[(g, "LR")] for g in range(4))
    if case == "all zero":
        assert all(r["status"] == 1 and r["energy"] == 0.0 for r in rows.values()) and np.isnan(got["mtf"]).all()
        assert all(math.isnan(v) for v in idx.values())


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _bits(res):
    return (res["mtf"].tobytes(), np.array([list(r.values()) for r in res["rows"].values()], np.float64).tobytes(),
            np.array(list(res["sti"].values())).tobytes(), res["origin"], res["taps"])


def test_nothing_is_disturbed_and_two_calls_agree(gpu_lib):
    """The stored taps and ir_info are byte for byte the same before and after, a processed batch with calls in between is that of a
    run without them, and two calls return the same bits in mtf, rows and sti."""
    from cuda_audio_amd.synth import make_input

    ir = _pair(6000, lead=37)
    x = make_input(32 * 256)
    runs, asked = [], []
    for ask in (False, True):
        c = _conv(16384, max_batch=32)
        c.prepare(0, ir)
        before = (c.ir_taps(0).tobytes(), c.ir_info(0))
        if ask:
            asked.append(c.ir_sti(0, **THREE))
            assert (c.ir_taps(0).tobytes(), c.ir_info(0)) == before
        first = c.process(x[0, :16 * 256], x[1, :16 * 256])
        if ask:
            asked.append(c.ir_sti(0, **THREE))
            asked.append(c.ir_sti(0))
        second = c.process(x[0, 16 * 256:], x[1, 16 * 256:])
        runs.append((_sha(c.ir_taps(0)), _sha(first), _sha(second), c.ir_info(0)))
        c.close()
    assert runs[0] == runs[1]
    assert _bits(asked[0]) == _bits(asked[1])
    assert (asked[0]["origin"], asked[0]["taps"]) == (38, 6037)


def _raw(c, idx, rows=True, mtf=True, sti=True, info=True, **fields):
    """mc_ir_sti with the struct's fields set directly; returns (status code, message)."""
    from cuda_audio_amd import _lib

    L = _lib.load()
    q = _lib.McStiQuery()
    L.mc_default_sti_query(C.byref(q))
    q.rate = RATE
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(q, k)[j] = x
        else:
            setattr(q, k, v)
    dp = C.POINTER(C.c_double)
    r, m, s, i = np.zeros(8 * 3 * 4), np.zeros(8 * 3 * 16), (C.c_double * 3)(), (C.c_uint64 * 2)()
    rc = L.mc_ir_sti(c._h, idx, C.byref(q), r.ctypes.data_as(dp) if rows else None, m.ctypes.data_as(dp) if mtf else None, s if sti else None,
                     i if info else None)
    return rc, L.mc_last_error().decode()


NAN = float("nan")
BAD = [("struct_size", dict(struct_size=268)), ("rate", dict(rate=7999)), ("n_bands", dict(n_bands=8)), ("n_mod", dict(n_mod=0)), ("n_mod", dict(n_mod=17)),
       ("flags", dict(flags=2)), ("centre_hz[0]", dict(centre_hz=(5.0,))), ("alpha[0]", dict(alpha=(-0.5,))), ("alpha[0]", dict(alpha=(NAN,))),
       ("beta[0]", dict(beta=(-0.5,))), ("beta[0]", dict(beta=(NAN,))), ("snr_db[0]", dict(flags=1, snr_db=(NAN,))), ("snr_db[0]", dict(flags=1, snr_db=(121.0,))),
       ("mod_hz[0]", dict(mod_hz=(0.05,))), ("mod_hz[0]", dict(mod_hz=(NAN,))), ("q 64", dict(q=64.0)), ("onset_db", dict(onset_db=1.0)),
       ("reserved", dict(reserved=(0, 1)))]


def test_refusals(gpu_lib):
    from cuda_audio_amd._lib import McError

    ir = _pair(3000)
    single = _conv(16384, form="single")
    single.prepare(0, ir)
    with pytest.raises(McError) as ex:
        single.ir_sti(0)
    assert ex.value.code == -3
    single.close()
    c = _conv(16384)
    c.prepare(0, ir)
    before = c.ir_sti(0)
    for idx in (1, 255, 256, 1 << 40):
        with pytest.raises(McError) as ex:
            c.ir_sti(idx)
        assert ex.value.code == -1 and "IR not loaded" in str(ex.value)
    for idx in (0, 1):  # the query, then the four arrays, come before the index
        for name, fields in BAD:
            rc, msg = _raw(c, idx, **fields)
            assert rc == -1 and name in msg, (name, rc, msg)
        for name in ("rows", "mtf", "sti", "info"):
            rc, msg = _raw(c, idx, **{name: False})
            assert rc == -1 and "null " + name in msg, (name, rc, msg)
    rc, msg = _raw(c, 0, rows=False, mtf=False, sti=False, info=False)
    assert rc == -1 and "null rows" in msg
    with pytest.raises(ValueError):
        c.ir_sti(0, bands=(1000.0,))
    assert _raw(c, 0)[0] == 0
    np.testing.assert_array_equal(c.ir_taps(0), ir)
    assert _bits(c.ir_sti(0)) == _bits(before)  # the engine still answers, with the same bits
    c.close()


SYNTH = dict(frames=24000, seed=2, t60=12000, late_gain=1.0, direct=0.0)


def test_a_synthesised_decay_reads_as_schroeder_predicts(gpu_lib):
    """mc_ir_synth's late field with late_gain 1 and no direct sound is noise under the envelope 10^(-3 m / t60), so its squared
    response is r^m, r = 10^(-6 / t60), times the noise's own squares, and m(F) scatters about the finite-length closed form
    |(1 - z^n) / (1 - z)| (1 - r) / (1 - r^n).  The restatement of tests/ir_synth_np.py's 24 000 frames with t60 = 12 000 frames
    differs from it by at most 0.0198 over the seeds 1 to 8 and the 14 frequencies (measured on the CPU when this test was
    written); the margin is four times that, 0.0792.  The restatement of seed 2 is held to it here on the CPU first, then the
    device equals the restatement to 1e-10."""
    import ir_synth_np
    from cuda_audio_amd.engine import IrSynth

    frames = ir_synth_np.frames(**SYNTH)
    want = sti(frames, RATE, onset_db=0.0, **NONE)
    closed = schroeder(10.0 ** (-6.0 / SYNTH["t60"]), SYNTH["frames"], [f32(F) for F in MOD_HZ], RATE)
    dev = float(np.max(np.abs(want["mtf"][0] - closed[None, :])))
    print(f"restatement: largest deviation from the closed form {dev:.4f}")
    assert dev <= 4.0 * 0.0198
    c = _conv(32768)
    c.prepare_synth(0, IrSynth(**SYNTH))
    got, _ = _compare(c, 0, RATE, onset_db=0.0, **NONE)
    c.close()
    assert np.max(np.abs(got["mtf"] - want["mtf"])) <= 1e-10
    assert np.max(np.abs(got["mtf"][0] - closed[None, :])) <= 4.0 * 0.0198
