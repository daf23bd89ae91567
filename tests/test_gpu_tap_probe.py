"""Every fp32 form of the partition sum read tap by tap (tests/tap_probe.py): the streaming MAC, the resident
MAC in its direct and fast-FIR forms, the split and the fused second-level transform, the overlap-save form, the JACK path in
both forms of its tail, and partition shards.  The parity tests feed white noise through IRs that decay by 60 dB, so they
weigh an IR's first partition a thousand times heavier than its last (tests/test_tap_probe_cpu.py has the figures); here
the IRs do not decay, the input is a handful of impulses, and the expected output is a closed form: every sample is one tap
or a sum of a few.

The bar on `worst` (the largest |got - want| over the whole stream in units of U = SIGMA AMP wet) is derived, not measured: a
tap that is missing, misplaced, doubled or weighted 10 % wrong errs by >= 0.1 x 0.5 SIGMA x 0.5 AMP = 0.025 U (asserted on the
oracle in test_tap_probe_cpu.py); float32 rounding through at most a 2^22-point transform leaves 1e-6 to 1e-5 of an output
whose RMS is about U; 1e-4 lies between.  Measured: DESIGN.md §2.5b.

Every stream runs on past the end of the last response, and its last call starts where no window of any form reaches an
impulse any more (a transform of silence is silence; a transform that holds an impulse leaves rounding noise where the exact
result is zero): the last two blocks of that call must be exact zeros."""
import numpy as np
import pytest

import tap_probe as tp
from tap_probe import BLOCK, WARM
from tap_probe_device import FUSED, OS, SPLIT, STREAM
from tap_probe_device import engine as _engine
from tap_probe_device import forms_or_skip as _forms_or_skip
from tap_probe_device import irs as _irs
from tap_probe_device import judge as _judge
from tap_probe_device import layout as _layout
from tap_probe_device import run_device as _run_device

pytestmark = pytest.mark.gpu


def _device_case(monkeypatch, tag, env, n_ref, irs, predelay, calls, imp, probed, expect, peak=0.4):
    x = tp.stream(imp, sum(calls) * BLOCK)
    got, forms, st = _run_device(monkeypatch, env, n_ref, irs, predelay, calls, x)
    for k in probed + [len(calls) - 1]:
        _forms_or_skip(forms[k] == expect, f"{tag}: call {k} of {calls[k]} blocks took {forms[k]}, not {expect}")
    _forms_or_skip((st["batches"] > 0) == (expect[0] == OS), f"{tag}: {st}")
    _judge(tag, got, irs, imp, predelay, peak)
    return got


# ---------------------------------------------------------------------------------------------------------------------------
STREAM_P = [(1, False), (2, False), (3, False), (4, False), (5, False), (15, False), (16, False), (16, True), (17, False), (31, False)]


@pytest.mark.parametrize("P,full", STREAM_P, ids=[f"P{p}{'full' if f else ''}" for p, f in STREAM_P])
def test_streaming_mac(gpu_lib, monkeypatch, P, full):
    """k_mac_stream: calls below stream_threshold, of 3 and of 7 blocks, predelay 0 and 301, impulses inside the ramp (per-slot
    gains) and after it.  (P = 31 needs 7859 taps, more than an engine of n_ref = 8192 stores: n_ref = 16384 there.)"""
    irs = _irs(P, full)
    for T in (3, 7):
        for predelay in (0, 301):
            calls, imp, probed = _layout(P, predelay, [T, T, T], T, ramp=T, seed=10 * T + predelay)
            _device_case(monkeypatch, f"stream P {P} T {T} predelay {predelay}", dict(MCCONV_OS="0"), 16384 if P > 28 else 8192, irs, predelay, calls, imp, probed,
                         (STREAM, False))


def test_a_planted_fault_fails_on_the_engine_too(gpu_lib, monkeypatch):
    """The harness itself, on the device: the engine is handed IRs whose last 3 % are 10 % low and is read against the closed form
    of the IRs as they should be; `worst` must rise above 0.025 U and lie on a tap of the last 3 %."""
    P, T = 17, 7
    irs = _irs(P)
    bad = [h.copy() for h in irs]
    for h in bad:
        h[h.shape[0] - (3 * h.shape[0]) // 100:] *= np.float32(0.9)
    calls, imp, probed = _layout(P, 0, [T, T, T], T, seed=2)
    x = tp.stream(imp, sum(calls) * BLOCK)
    got, forms, st = _run_device(monkeypatch, dict(MCCONV_OS="0"), 8192, bad, 0, calls, x)
    r = tp.compare(got, tp.want(irs, imp, got.shape[1]), irs, imp)
    print(f"planted fault: {tp.describe(r)}")
    assert r["worst"] >= 0.025
    assert any(t >= irs[imp[k][0]].shape[0] - (3 * irs[imp[k][0]].shape[0]) // 100 for k, t in r["covering"]), tp.describe(r)


@pytest.mark.parametrize("T", [8, 9, 255, 1024, 1025])
def test_resident_mac_direct_form(gpu_lib, monkeypatch, T):
    """k_mac_resident, direct form, both sides of the partition split at T < 1024: a call inside the ramp (<true>: per-slot
    gains) and calls after the warm-up (<false>: one set of gains over the window)."""
    env = dict(MCCONV_FFT2="0", MCCONV_FFA_LEVELS="0", MCCONV_OS="0")
    for P in (1, 5, 16, 17, 67):
        predelay = 301 if P in (5, 17) else 0
        calls, imp, probed = _layout(P, predelay, [T, T], T, ramp=T, warm=T, seed=T + P)
        _device_case(monkeypatch, f"resident T {T} P {P} predelay {predelay}", env, 32768, _irs(P), predelay, calls, imp, probed, (0, True))


@pytest.mark.parametrize("level,T,P,n_ref", [(1, 2048, 259, 131072), (2, 4096, 517, 262144), (3, 8192, 1029, 524288)], ids=["level1", "level2", "level3"])
def test_fast_fir_form(gpu_lib, monkeypatch, level, T, P, n_ref):
    """The fast-FIR form of the resident MAC at its smallest batch, P odd and no multiple of 2^level: every call starts at an odd
    block; the first one lies in the ramp; impulses on the last 2^level blocks of a settled call, which go through the streaming
    kernel and between them hold every residue mod 2^level.  The same stream through the direct form: their distance."""
    S = 1 << level
    irs = _irs(P)
    calls, imp, probed = _layout(P, 301, [T, T], T, lead=[3], ramp=T, settle=False, seed=level, limit=5 + S - 1,
                                 extra=lambda b: [b[-1] - k for k in range(2, S + 1)])
    assert all(sum(calls[:k]) % 2 == 1 for k in probed) and sum(calls[:2]) >= WARM + P
    peak = 0.4 if len(imp) <= 16 else 0.6  # (two groups that never overlap: at most 5 + 2^level - 1 responses at one sample)
    env = dict(MCCONV_FFT2="0", MCCONV_OS="0")
    fast = _device_case(monkeypatch, f"fast-FIR level {level} P {P}", dict(env, MCCONV_FFA_LEVELS=str(level)), n_ref, irs, 301, calls, imp, [1] + probed, (level, True), peak)
    direct = _device_case(monkeypatch, f"direct form of the same stream, P {P}", dict(env, MCCONV_FFA_LEVELS="0"), n_ref, irs, 301, calls, imp, [1] + probed, (0, True), peak)
    print(f"fast-FIR level {level} vs direct: {np.abs(fast - direct).max() / (tp.SIGMA * tp.AMP):.2e} U")


@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
def test_split_second_level_form(gpu_lib, monkeypatch, ramp):
    """k_f2_fwd / k_f2_prod at 259 partitions: a call of 768 blocks and one of 16384 - 259 + 2, one block more than a chunk, with
    impulses either side of the chunk's end; once with a first call of 768 blocks inside the ramp, which takes the form's
    per-slot-gain sequences (four per voice instead of two)."""
    P, chunk = 259, 16384 - 259 + 1
    calls, imp, probed = _layout(P, 0, [768, chunk + 1], 768, ramp=768 if ramp else 0, warm=768, seed=3 + ramp,
                                 extra=lambda b: [b[1] + chunk - 1, b[1] + chunk // 2])
    env = dict(MCCONV_FFT2="1", MCCONV_FFT2_FUSED="0", MCCONV_OS="0")
    _device_case(monkeypatch, f"split form P {P} ramp {ramp}", env, 131072, _irs(P), 0, calls, imp, ([0] if ramp else []) + probed, (SPLIT, True))


FUSED_CASES = [(16, 8192, FUSED), (17, 8192, FUSED), (345, 131072, FUSED), (5632, 2097152, FUSED), (5633, 2097152, SPLIT)]


@pytest.mark.parametrize("P,n_ref,form", FUSED_CASES, ids=[f"P{c[0]}" for c in FUSED_CASES])
def test_fused_second_level_form(gpu_lib, monkeypatch, P, n_ref, form):
    """k_g2_mac: calls of one chunk (8192 - P + 1 blocks), one chunk plus one block and three chunks, impulses on the last block of
    a chunk and the first of the next; P = 5632 is kG2Pmax, and one partition more has to take the split form."""
    chunk = 8192 - P + 1
    calls, imp, probed = _layout(P, 301 if P == 17 else 0, [chunk, chunk + 1, 3 * chunk], chunk, warm=min(chunk, 512), seed=P,
                                 extra=lambda b: [b[2] + chunk - 1, b[2] + chunk, b[1] + chunk - 1])
    env = dict(MCCONV_FFT2="1", MCCONV_FFT2_FUSED="1", MCCONV_FFT2_WORK="1", MCCONV_OS="0", MCCONV_FFA_LEVELS="0")
    irs = _irs(P)
    fused = _device_case(monkeypatch, f"fused form P {P}", env, n_ref, irs, 301 if P == 17 else 0, calls, imp, probed, (form, True))
    if P == 345:
        split = _device_case(monkeypatch, f"split form of the same stream, P {P}", dict(env, MCCONV_FFT2_FUSED="0"), n_ref, irs, 0, calls, imp, probed, (SPLIT, True))
        print(f"fused vs split, P {P}: {np.abs(fused - split).max() / (tp.SIGMA * tp.AMP):.2e} U")


OS_CASES = [(3, 8192, 0, False), (3, 8192, 256, False), (3, 8192, 301, False), (345, 131072, 301, False), (8192, 4194304, 0, True)]


@pytest.mark.parametrize("P,n_ref,predelay,full", OS_CASES, ids=[f"P{c[0]}-predelay{c[2]}" for c in OS_CASES])
def test_overlap_save_form(gpu_lib, monkeypatch, P, n_ref, predelay, full):
    """csrc/ossave.hip.h on device buffers, from 48 blocks on: a call of one segment (16384 - P blocks) and one of two segments
    plus 5 blocks, impulses either side of the segment boundary and in the call before (the history ring).  P = 8192 with
    2^21 taps exactly is the longest IR the form takes (a segment at least half new frames)."""
    hop = 16384 - P
    tail = max(48, P + 16)
    calls, imp, probed = _layout(P, predelay, [hop, 2 * hop + 5], tail, warm=40, seed=P + predelay,
                                 extra=lambda b: [b[1] + hop - 1, b[1] + hop, b[1] + 2 * hop])
    env = dict(MCCONV_OS="1", MCCONV_OS_MIN="48", MCCONV_FFA_LEVELS="0")
    _device_case(monkeypatch, f"overlap-save P {P} predelay {predelay}", env, n_ref, _irs(P, full), predelay, calls, imp, probed, (OS, True))


def test_overlap_save_form_is_not_taken_beyond_half_a_segment(gpu_lib, monkeypatch):
    """P = 8193: the overlap would be more than half a segment; the call takes the resident MAC, and its taps are right."""
    P = 8193
    calls, imp, probed = _layout(P, 0, [64, 64], 2048, warm=2048, seed=5)
    env = dict(MCCONV_OS="1", MCCONV_OS_MIN="48", MCCONV_FFA_LEVELS="0", MCCONV_FFT2="0")
    _device_case(monkeypatch, f"P {P}, no overlap-save", env, 4194304, _irs(P), 0, calls, imp, probed, (0, True))


# ---------------------------------------------------------------------------------------------------------------------------
def _jack_stream(monkeypatch, form, period, n_ref, P, predelay):
    pm = period // BLOCK
    warm = WARM * pm
    bounds = [warm + pm * j for j in range(5)]  # four consecutive periods after 170 periods of silence
    imp = tp.place_impulses(bounds, seed=P + predelay + pm, batch=2, first=warm, extra=(bounds[3], bounds[0], bounds[4] - 1, bounds[4] + pm))
    quiet = max(n for _, n, _ in imp) // BLOCK + P + -(-predelay // BLOCK) + 10
    nper = -(-quiet // pm) + 1
    irs = _irs(P)
    x = tp.stream(imp, nper * period)
    c = _engine(monkeypatch, dict(MCCONV_TAIL_FORM=form) if form else {}, n_ref, irs, predelay, 8, period=period)
    got = np.empty((2, nper * period), np.float32)
    for k in range(nper):
        s = slice(k * period, (k + 1) * period)
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
    forms = c.tail_forms()
    c.close()
    if form:
        key = dict(td="time_domain", fd="frequency_domain")[form]
        _forms_or_skip(forms[key] > 0 and sum(forms.values()) == forms[key], f"{form}: {forms} of {nper} periods")
    _judge(f"JACK {form or period} P {P} predelay {predelay}", got, irs, imp, predelay)


@pytest.mark.parametrize("form,period", [("td", 256), ("fd", 256), (None, 512), (None, 1024)], ids=["256-td", "256-fd", "512", "1024"])
def test_jack_path(gpu_lib, monkeypatch, form, period):
    """onProcess period by period: 170 periods of silence, then impulses at offsets 0 and 255 of a period and in consecutive
    periods; 256-frame periods with partition 0 of the tail forced into either of its forms (tail_forms() confirms it), 512-
    and 1024-frame periods in their one form."""
    for P in (1, 2, 3, 11):
        for predelay in (0, 100, 512):
            _jack_stream(monkeypatch, form, period, 4096, P, predelay)


@pytest.mark.parametrize("form", ["td", "fd"])
def test_jack_path_at_the_headline_length(gpu_lib, monkeypatch, form):
    """P = 1723 at n_ref = 524288, 256-frame periods: the tail kernel's sweep over every partition of the shipped operating point."""
    _jack_stream(monkeypatch, form, 256, 524288, 1723, 100)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,world", [(98, 3), (98, 4), (5, 4)], ids=["P98-3shards", "P98-4shards", "P5-4shards"])
def test_partition_shards(gpu_lib, monkeypatch, P, world):
    """part_begin / part_end engines (bounds are multiples of 16: mc_create refuses others), partial_device, a torch sum and
    finish_device: the sum of the partials is the whole IR's closed form.  98 partitions over 3 shards leave the last one two
    partitions, (96, 98); 5 over 4 leave one shard that holds them all and three empty ones."""
    import torch

    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.engine import Convolution
    from cuda_audio_amd.sharded import shard_bounds

    with pytest.raises(McError):
        Convolution("tap", 32768, part_begin=0, part_end=25)
    T, n_ref, predelay = 32, 32768, 301
    irs = _irs(P)
    calls, imp, probed = _layout(P, predelay, [T, T], T, ramp=T, seed=P + world)
    assert set(calls) == {T}
    x = tp.stream(imp, sum(calls) * BLOCK)
    bounds = [b for b in (shard_bounds(P, world, g) for g in range(world)) if b[1] > b[0]]
    assert len(bounds) == (1 if P == 5 else world) and bounds[-1][1] >= P
    shards = [_engine(monkeypatch, dict(MCCONV_OS="0"), n_ref, irs, predelay, T, whole=False, part_begin=a, part_end=b) for a, b in bounds]
    dev = torch.device("cuda:0")
    xin = torch.from_numpy(x).to(dev)
    out = torch.full((2, x.shape[1]), 7.0, device=dev)
    torch.cuda.synchronize()
    for k in range(len(calls)):
        sl, so = xin[:, k * T * BLOCK:(k + 1) * T * BLOCK], out[:, k * T * BLOCK:(k + 1) * T * BLOCK]
        parts = [torch.zeros(2 * T * BLOCK, device=dev) for _ in shards]
        torch.cuda.synchronize()
        for s, p in zip(shards, parts):
            s.partial_device(sl[0].data_ptr(), sl[1].data_ptr(), p.data_ptr(), T)
            s.sync()
        total = torch.stack(parts).sum(0)
        torch.cuda.synchronize()
        shards[0].finish_device(sl[0].data_ptr(), sl[1].data_ptr(), total.data_ptr(), so[0].data_ptr(), so[1].data_ptr(), T)
        shards[0].sync()
        for s in shards[1:]:
            s.finish_device(None, None, None, None, None, T)
    for s in shards:
        s.close()
    _judge(f"shards P {P} over {world}: {bounds}", out.cpu().numpy(), irs, imp, predelay)
