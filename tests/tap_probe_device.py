"""What the device cases of the tap probe share (tests/test_gpu_tap_probe.py, tests/test_gpu_tap_probe_moving.py,
tests/test_gpu_tap_probe_compat.py): the layout of a stream's calls and impulses, the engine in
linear mode (or, with compat=True, in compat mode), the stream through it call by call with the form
each call took, and the judgement against the closed form of tests/tap_probe.py.  A plain module: imported, not collected."""
import os

import numpy as np
import pytest

import tap_probe as tp
from tap_probe import BLOCK, WARM

WORST_BAR = 1e-4
# switches that CI legs set for the whole suite and that put another form (or another library) under every test
SUITE_WIDE = [k for k in ("MCCONV_LIB", "MCCONV_FORM", "MCCONV_NO_PARK", "MCCONV_NO_SPIN", "MCCONV_TD_FFT") if os.environ.get(k)]
STREAM, FUSED, SPLIT, OS = 0, 254, 255, 253


def irs(P, full=False):
    """Two IRs of P partitions, the last one partial (and differently so) unless `full`."""
    return [tp.probe_ir(BLOCK * P - (0 if full else 77), 1000 + 2 * P), tp.probe_ir(BLOCK * P - (0 if full else 130), 1001 + 2 * P)]


def layout(P, predelay, sizes, tail, *, lead=(), ramp=0, warm=None, extra=None, limit=8, seed=0, settle=True, window=0):
    """The calls of a stream and its impulses.  lead: calls before anything else (an odd start); ramp: a call of that many blocks
    inside the cold-start ramp with impulses of its own (forms that take per-slot gains); then silence in calls of `warm` blocks
    until block WARM + P, so that every window after it carries one set of gains; then the calls `sizes` with impulses around
    the last of them (tap_probe.place_impulses; extra(bounds) names further blocks); then calls of `tail` blocks until one
    starts beyond the reach of the last impulse - and, in compat mode, `window` = n_ref / 256 blocks more: beyond its Q1/Q2
    window too.  Returns (calls, impulses, the indices of `sizes` in calls)."""
    pdb = -(-predelay // BLOCK)
    calls, imp, pos = list(lead), [], sum(lead)
    if ramp:
        imp += tp.place_impulses([pos, pos + ramp], seed + 1, batch=0, extra=[pos + k for k in (1, 2, 5) if k < ramp - 1])
        calls.append(ramp)
        pos += ramp
    if settle:
        end = max(WARM + P, (max(n for _, n, _ in imp) // BLOCK + P + pdb + 2) if imp else 0)
        while pos < end:
            calls.append(warm or tail)
            pos += calls[-1]
    first = len(calls)
    bounds = [pos]
    for n in sizes:
        bounds.append(bounds[-1] + n)
    imp += tp.place_impulses(bounds, seed, first=pos, extra=extra(bounds) if extra else (), limit=limit)
    calls += list(sizes)
    pos = bounds[-1]
    quiet = max(n for _, n, _ in imp) // BLOCK + P + pdb + 10 + window  # (10: the fast-FIR forms reach up to 2^3 blocks further)
    while True:
        calls.append(tail)
        pos += tail
        if pos - tail >= quiet:
            break
    return calls, imp, list(range(first, first + len(sizes)))


def cut(marks, T, quiet):
    """Calls of T blocks, shortened where a block of `marks` has to start a call (a controller event, a probed call), until one
    of T blocks starts at or beyond block `quiet`.  Returns (calls, {call start: index})."""
    marks = sorted(set(int(m) for m in marks))
    calls, at, pos = [], {}, 0
    while True:
        nxt = [m for m in marks if m > pos]
        n = min(T, nxt[0] - pos) if nxt else T
        at[pos] = len(calls)
        calls.append(n)
        if pos >= quiet and n == T:
            return calls, at
        pos += n


def params(c, predelay):
    for h in (0, 1):
        c.cc[h].value.update(select=h, predelay=predelay, dry=0.0, wet=1.0, level=1.0, panWet=0.0, panDry=0.0, vsteps=0)


def engine(monkeypatch, env, n_ref, irs, predelay, max_batch, whole=True, compat=False, **kw):
    from cuda_audio_amd.engine import Convolution

    for k in ("MCCONV_OS_MIN", "MCCONV_FFT2_WORK", "MCCONV_TAIL_FORM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw.setdefault("stream_threshold", 8)
    c = Convolution("tap", n_ref, max_batch=max_batch, compat=compat, **kw)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
        assert not whole or c.ir_info(i)["partitions"] == -(-ir.shape[0] // BLOCK)
    params(c, predelay)
    return c


def events_by_call(schedule):
    """{block: {half: {field: value}}}: what a call that starts at `block` finds newly set."""
    by = {}
    for b, half, field, value in schedule:
        by.setdefault(int(b), {}).setdefault(half, {})[field] = value
    return by


def run_device(monkeypatch, env, n_ref, irs, predelay, calls, x, schedule=(), start=None, compat=False, singles=False, **kw):
    """The stream through process_device on 16-byte-aligned device buffers, call by call: the output, the form each call took
    (kernel_stats' fast_levels, resident) and the counters: os_stats(), with mac_stats() as `mac`, drop_stats() as `drop` and
    park_stats() as `park`.  schedule, start: controller events set before the call that starts at their block, and the values
    before the first call (tap_probe.controllers).  singles: a call of one block goes through onProcess (a single period)."""
    import torch

    c = engine(monkeypatch, env, n_ref, irs, predelay, max(calls), compat=compat, **kw)
    for h in (0, 1):
        if start:
            c.cc[h].value.update(**start[h])
    by = events_by_call(schedule)
    d_in = torch.from_numpy(x).to("cuda:0")
    d_out = torch.full((2, x.shape[1]), 7.0, device="cuda:0")  # (not zeros: the trailing blocks have to be written)
    torch.cuda.synchronize()
    c.enable_kernel_timing(True)
    forms, o = [], 0
    for n in calls:
        for half, kw in by.pop(o, {}).items():
            c.cc[half].value.update(**kw)
        if singles and n == 1:
            l, r = c.onProcess(x[0, o * BLOCK:(o + 1) * BLOCK], x[1, o * BLOCK:(o + 1) * BLOCK])
            d_out[:, o * BLOCK:(o + 1) * BLOCK] = torch.from_numpy(np.stack([l, r])).to("cuda:0")
            torch.cuda.synchronize()
            forms.append(None)
        else:
            c.process_device(d_in[0, o * BLOCK:].data_ptr(), d_in[1, o * BLOCK:].data_ptr(), d_out[0, o * BLOCK:].data_ptr(), d_out[1, o * BLOCK:].data_ptr(), n)
            c.sync()
            ks = c.kernel_stats()
            forms.append((ks["fast_levels"], ks["resident"]))
        o += n
    assert not by, f"events at {sorted(by)} start no call"
    st = c.os_stats()
    st["mac"], st["drop"], st["park"] = c.mac_stats(), c.drop_stats(), c.park_stats()
    c.close()
    return d_out.cpu().numpy(), forms, st


def run_jack(monkeypatch, form, period, n_ref, irs, predelay, nper, x, schedule=(), start=None, compat=False, env=None, stats=None):
    """The stream through onProcess period by period (256-frame periods: partition 0 of the tail forced into `form`, td or fd):
    the output; tail_forms() is asserted here, and returned with drop_stats() and park_stats() in `stats`, a dict, if one is given."""
    pm = period // BLOCK
    c = engine(monkeypatch, dict(env or {}, **(dict(MCCONV_TAIL_FORM=form) if form else {})), n_ref, irs, predelay, 8, compat=compat, period=period)
    for h in (0, 1):
        if start:
            c.cc[h].value.update(**start[h])
    by = events_by_call(schedule)
    got = np.empty((2, nper * period), np.float32)
    for k in range(nper):
        for half, kw in by.pop(k * pm, {}).items():
            c.cc[half].value.update(**kw)
        s = slice(k * period, (k + 1) * period)
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
    assert not by, f"events at {sorted(by)} start no period"
    forms = c.tail_forms()
    if stats is not None:
        stats.update(tail_forms=forms, drop=c.drop_stats(), park=c.park_stats())
    c.close()
    if form:
        key = dict(td="time_domain", fd="frequency_domain")[form]
        forms_or_skip(forms[key] > 0 and sum(forms.values()) == forms[key], f"{form}: {forms} of {nper} periods")
    return got


def forms_or_skip(ok, what):
    if not ok:
        if SUITE_WIDE:
            pytest.skip(f"{SUITE_WIDE} puts another form under this case: {what}")
        raise AssertionError(what)


def judge(tag, got, irs, imp, predelay, peak=0.4, states=None, compat=None):
    """`got` against the closed form: of a constant state (tap_probe.want), or under `states` (tap_probe.controllers); in compat
    mode under `states` and compat = dict(n_ref, period) (tap_probe.render_compat)."""
    if compat is not None:
        w = tp.render_compat(irs, imp, states, got.shape[1], compat["n_ref"], compat.get("period", BLOCK))
    else:
        w = tp.want(irs, imp, got.shape[1], predelay) if states is None else tp.render(irs, imp, states, got.shape[1])
    r = tp.compare(got, w, irs, imp, predelay, states=states, compat=compat)
    print(f"{tag}: {tp.describe(r)}; {len(imp)} impulses, peak {np.abs(w).max():.3f}, {got.shape[1] // BLOCK} blocks")
    assert np.abs(w).max() < peak
    assert np.abs(w[:, -2 * BLOCK:]).max() == 0
    assert r["worst"] <= WORST_BAR, f"{tag}: {tp.describe(r)}"
    assert not got[:, -2 * BLOCK:].any(), f"{tag}: the trailing blocks are not silent: {np.abs(got[:, -2 * BLOCK:]).max():.3e}"
    return r
