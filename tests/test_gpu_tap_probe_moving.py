"""The tap probe with everything the engine attaches to an input block in motion (tests/tap_probe.py: controllers, render; DESIGN.md
§2.5d): four different path gains, IRs whose lengths differ by whole partitions, a gain step at a call boundary read at the
calls either side of "one set of gains over the window", one half switching IR (two voices, the fade and the settled state),
more IRs cross-fading than there are voices (the merge), and predelay changes while responses ring (the residual rings) -
through every fp32 form of the partition sum, tap by tap against the closed form that tests/test_tap_probe_moving_cpu.py
proves on the two oracles.

Conventions as in test_gpu_tap_probe.py: compat = 0; buffers pre-filled with 7; the form of every probed call asserted
(kernel_stats(), os_stats(), tail_forms()); `worst` (the largest |got - want| over the whole stream in U = SIGMA AMP) <= 1e-4,
a bar derived there: float32 rounding leaves 1e-6 to 1e-5, and the mildest fault here - a gain 10 % wrong on a path of gain
0.25 - reads 0.006 U; the last two blocks of the last call, which starts beyond the reach of every response and of what a
flush left in the residual rings, exact zeros.  pytest -s prints every case."""
import numpy as np
import pytest

import tap_probe as tp
from tap_probe import BLOCK, WARM
from tap_probe_device import FUSED, OS, SPLIT, STREAM, WORST_BAR, cut, engine, forms_or_skip, judge, layout, run_device, run_jack

pytestmark = pytest.mark.gpu

ENV = dict(
    stream=dict(MCCONV_OS="0"),
    resident=dict(MCCONV_FFT2="0", MCCONV_FFA_LEVELS="0", MCCONV_OS="0"),
    fastfir=dict(MCCONV_FFT2="0", MCCONV_OS="0", MCCONV_FFA_LEVELS="1"),
    split=dict(MCCONV_FFT2="1", MCCONV_FFT2_FUSED="0", MCCONV_OS="0"),
    fused=dict(MCCONV_FFT2="1", MCCONV_FFT2_FUSED="1", MCCONV_FFT2_WORK="1", MCCONV_OS="0", MCCONV_FFA_LEVELS="0"),
    second=dict(MCCONV_FFT2="1", MCCONV_FFT2_FUSED="1", MCCONV_FFT2_WORK="1", MCCONV_OS="0"),  # fused where the gains allow, else split
    os=dict(MCCONV_OS="1", MCCONV_OS_MIN="48", MCCONV_FFA_LEVELS="0"),
)
DIRECT = (0, True)


def _irs(*parts, seed=0):
    """IRs of the given partitions, each with a partial last partition of its own."""
    return [tp.probe_ir(BLOCK * P - (77, 130, 5, 201, 33)[j % 5], 3000 + 10 * seed + j) for j, P in enumerate(parts)]


def _three(P):
    """P, P - 3 and P + 16 partitions, instead of equal."""
    return _irs(P, max(P - 3, 1), P + 16, seed=P)


def _gains(select=(0, 1), predelay=0):
    """Four different path gains, every one >= 0.25: L<-in1 0.328, L<-in2 0.469, R<-in1 0.656, R<-in2 0.352."""
    s = tp.start_values(predelay)
    s[0].update(select=select[0], panWet=0.5, level=0.75, wet=0.875)
    s[1].update(select=select[1], panWet=-0.25, level=0.625, wet=0.75)
    return s


def _p_end(irs, *which):
    return -(-max(-(-irs[j].shape[0] // BLOCK) for j in which) // 16) * 16


def _batch(monkeypatch, tag, env, n_ref, irs, calls, imp, schedule, start, expect, peak=0.4):
    """The stream through process_device, the forms of the calls `expect` names ({call index: (fast_levels, resident)}), the
    judgement.  Returns the forms of all calls and the counters."""
    states = tp.controllers(schedule, calls, len(irs), start=start)
    x = tp.stream(imp, sum(calls) * BLOCK)
    got, forms, st = run_device(monkeypatch, env, n_ref, irs, 0, calls, x, schedule, start)
    for k, want in sorted(expect.items()):
        forms_or_skip(forms[k] == want, f"{tag}: call {k} of {calls[k]} blocks from block {sum(calls[:k])} took {forms[k]}, not {want}")
    if len(expect) == len(calls):
        forms_or_skip(st["batches"] == sum(1 for w in expect.values() if w[0] == OS), f"{tag}: {st}")
    judge(tag, got, irs, imp, None, peak, states)
    return forms, st


def _quiet(irs, imp, schedule=(), predelay=0):
    """The block from which a call's windows reach no impulse and no flush any more."""
    last = max([n // BLOCK for _, n, _ in imp] + [b for b, _, _, _ in schedule])
    return last + _p_end(irs, *range(len(irs))) + -(-predelay // BLOCK) + 10


# ---------------------------------------------------------------------------------------------------------------------------
# a. four different path gains, settled, IRs of P, P - 3 and P + 16 partitions
SETTLED = {
    "streaming": dict(P=17, n_ref=16384, env=ENV["stream"], sizes=[7, 7, 7], expect=(STREAM, False)),
    "streaming-dry": dict(P=17, n_ref=16384, env=ENV["stream"], sizes=[7, 7, 7], expect=(STREAM, False), dry=True),
    "resident": dict(P=17, n_ref=32768, env=ENV["resident"], sizes=[9, 9], expect=DIRECT),
    "fast-fir": dict(P=259, n_ref=131072, env=ENV["fastfir"], sizes=[2048, 2048], expect=(1, True)),
    "split": dict(P=259, n_ref=131072, env=ENV["split"], sizes=[768, 768], expect=(SPLIT, True)),
    "fused": dict(P=17, n_ref=16384, env=ENV["fused"], sizes=[64, 64], expect=(FUSED, True)),
}


@pytest.mark.parametrize("form", list(SETTLED))
def test_four_path_gains_settled(gpu_lib, monkeypatch, form):
    """Each form folds the four gains {L<-in1, L<-in2, R<-in1, R<-in2} its own way; with four different ones two exchanged
    indices read 0.1 U or more.  Half 0 on the IR of P partitions and then on the one of P + 16, half 1 on the one of P - 3.
    streaming-dry adds dry = 0.25 / 0.5 panned +-0.5: the peak bar rises by AMP x the largest dry gain."""
    k = SETTLED[form]
    irs = _three(k["P"])
    T = k["sizes"][0]
    for select in ((0, 1), (2, 1)):
        start = _gains(select)
        peak = 0.4
        if k.get("dry"):
            start[0].update(dry=0.25, panDry=0.5)
            start[1].update(dry=0.5, panDry=-0.5)
            peak += tp.AMP * 0.5 * 0.625  # (half 1: dry 0.5 x pan_l(-0.5) = 1 x level 0.625)
        calls, imp, probed = layout(_p_end(irs, *select), 0, k["sizes"], T, warm=T, seed=7 * k["P"] + select[0])
        assert set(calls) == {T}
        _batch(monkeypatch, f"settled {form} select {select}", k["env"], k["n_ref"], irs, calls, imp, [], start, {j: k["expect"] for j in probed + [len(calls) - 1]}, peak)


def test_four_path_gains_settled_overlap_save(gpu_lib, monkeypatch):
    """k_os_ir_mix folds gains and IRs into A, B: calls of 64 blocks and one call of two segments plus 5 blocks (a segment hops by
    16384 blocks less the window, which is the longest voice's partitions rounded up to 16)."""
    irs = _three(3)
    for select in ((0, 1), (2, 1)):
        hop = 16384 - _p_end(irs, *select)
        calls, imp, probed = layout(_p_end(irs, *select), 0, [64, 64, 2 * hop + 5], 64, warm=40, seed=3 + select[0],
                                    extra=lambda b: [b[2] + hop - 1, b[2] + hop, b[2] + 2 * hop])
        forms, st = _batch(monkeypatch, f"settled overlap-save select {select}", ENV["os"], 8192, irs, calls, imp, [], _gains(select),
                           {j: (OS, True) for j in probed + [len(calls) - 1]})
        forms_or_skip(st["batches"] >= 4, f"{st}")


def _jack_settled_layout(pm, reach, predelay=0):
    """Impulses around four consecutive periods after 170 periods of silence, and the periods until the trailing silence."""
    warm = WARM * pm
    bounds = [warm + pm * j for j in range(5)]
    imp = tp.place_impulses(bounds, seed=reach + predelay + pm, batch=2, first=warm, extra=(bounds[3], bounds[0], bounds[4] - 1, bounds[4] + pm))
    quiet = max(n for _, n, _ in imp) // BLOCK + reach + -(-predelay // BLOCK) + 10
    return imp, -(-quiet // pm) + 1


@pytest.mark.parametrize("form,period", [("td", 256), ("fd", 256), (None, 512)], ids=["256-td", "256-fd", "512"])
def test_four_path_gains_settled_jack(gpu_lib, monkeypatch, form, period):
    """onProcess: the tail kernel folds the gains once more in each of its two forms."""
    pm = period // BLOCK
    for P in (3, 11):
        irs = _three(P)
        for select in ((0, 1), (2, 1)):
            imp, nper = _jack_settled_layout(pm, _p_end(irs, *select))
            start = _gains(select)
            states = tp.controllers([], [pm] * nper, len(irs), period, start)
            got = run_jack(monkeypatch, form, period, 8192, irs, 0, nper, tp.stream(imp, nper * period), [], start)
            judge(f"settled JACK {form or period} P {P} select {select}", got, irs, imp, None, 0.4, states)


def test_four_path_gains_settled_partition_shards(gpu_lib, monkeypatch):
    """98 (then 114) partitions over 3 shards: partial_device on each, a torch sum, finish_device."""
    import torch

    from cuda_audio_amd.sharded import shard_bounds

    T, n_ref, world = 32, 32768, 3
    irs = _three(98)
    dev = torch.device("cuda:0")
    for select in ((0, 1), (2, 1)):
        start = _gains(select)
        Pmax = max(-(-irs[j].shape[0] // BLOCK) for j in select)
        calls, imp, probed = layout(_p_end(irs, *select), 0, [T, T], T, seed=98 + select[0])
        assert set(calls) == {T}
        states = tp.controllers([], calls, len(irs), start=start)
        x = tp.stream(imp, sum(calls) * BLOCK)
        bounds = [b for b in (shard_bounds(Pmax, world, g) for g in range(world)) if b[1] > b[0]]
        assert len(bounds) == world and bounds[-1][1] >= Pmax
        shards = [engine(monkeypatch, dict(MCCONV_OS="0"), n_ref, irs, 0, T, whole=False, part_begin=a, part_end=b) for a, b in bounds]
        for s in shards:
            for h in (0, 1):
                s.cc[h].value.update(**start[h])
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
        judge(f"settled shards select {select}: {bounds}", out.cpu().numpy(), irs, imp, None, 0.4, states)


# ---------------------------------------------------------------------------------------------------------------------------
# b. a gain step at a call boundary g, read from calls that start either side of "one set of gains over the window"
def _step_case(monkeypatch, tag, env, n_ref, P, T, before, after):
    """level and panWet of both halves change at block g (a call start after the warm-up).  Impulses on g - 1 (offsets 255 and
    77) and on g (0 and 131), both inputs, and one in the probed call.  Four streams: a later call starts exactly at g + P - 1,
    g + p_end - 1, g + p_end, g + p_end + 1 (p_end: P rounded up to 16).  DESIGN.md §2.5c: per-slot gains (the form `before`)
    in calls that start before g + p_end, one set of gains (the form `after`) from there on."""
    irs = _irs(P, P, seed=P)
    p_end = _p_end(irs, 0, 1)
    g = (-(-(WARM + p_end) // T) + 1) * T  # (the call before g is settled as well)
    sched = [(g, 0, "level", 0.625), (g, 1, "level", 1.0), (g, 0, "panWet", -0.5), (g, 1, "panWet", 0.25)]
    for X in (g + P - 1, g + p_end - 1, g + p_end, g + p_end + 1):
        imp = tp.impulses_on([(0, g - 1, 255), (1, g - 1, 77), (1, g, 0), (0, g, 131), (1, X + 1 if T > 1 else X, 77)], seed=P + X)
        calls, at = cut([g, X], T, _quiet(irs, imp, sched))
        expect = {at[X]: before if X < g + p_end else after, at[g - T]: after, len(calls) - 1: after}
        _batch(monkeypatch, f"{tag} P {P}: step at {g}, a call from g + {X - g}", env, n_ref, irs, calls, imp, sched, _gains(), expect)


def test_gain_step_streaming_mac(gpu_lib, monkeypatch):
    _step_case(monkeypatch, "stream", ENV["stream"], 8192, 17, 7, (STREAM, False), (STREAM, False))


@pytest.mark.parametrize("P", [17, 67])
def test_gain_step_resident_mac(gpu_lib, monkeypatch, P):
    """k_mac_resident<true> before g + p_end, <false> from there on (kernel_stats() does not tell them apart: the taps do)."""
    _step_case(monkeypatch, "resident", ENV["resident"], 32768, P, 9, DIRECT, DIRECT)


def test_gain_step_fused_form_at_17_partitions(gpu_lib, monkeypatch):
    """The fused second-level form wants one set of gains; below 256 partitions the split form does not stand in for it (§2.5c:
    unsharded taps >= 256), so the calls before g + p_end take the resident MAC with per-slot gains."""
    _step_case(monkeypatch, "fused / resident", ENV["fused"], 8192, 17, 64, DIRECT, (FUSED, True))


def test_gain_step_split_versus_fused_form(gpu_lib, monkeypatch):
    """259 partitions, calls of 768 blocks: the split form's per-slot-gain sequences before g + p_end, the fused form after."""
    _step_case(monkeypatch, "split / fused", ENV["second"], 131072, 259, 768, (SPLIT, True), (FUSED, True))


def test_gain_step_overlap_save_and_its_fallback(gpu_lib, monkeypatch):
    """P 3, calls of 64 blocks from 48 on: os_applies refuses the call that starts before g + 16."""
    _step_case(monkeypatch, "overlap-save / resident", dict(ENV["os"], MCCONV_FFT2="0"), 8192, 3, 64, DIRECT, (OS, True))


# ---------------------------------------------------------------------------------------------------------------------------
# c. one half switches IR: voice 0 = (the old IR fading out, half 1's IR), voice 1 = (the new IR, none)
def _switch_layout(irs, frm, to, T, sel1=1, warm=None):
    """Half 0 goes from IR `frm` to IR `to` with vsteps = 3 at block s, a call start; half 1 stays on IR sel1.  Impulses on the
    block before the switch, on it, one and five blocks into the fade, and after the fade has settled: z is the first call
    start at which the test's own recurrence has had the outgoing coefficient at zero (< 1e-14) and the incoming one at wet for
    p_end blocks."""
    p_end = _p_end(irs, *range(len(irs)))
    s = -(-(WARM + p_end) // T) * T
    sched = [(s, 0, "select", to), (s, 0, "vsteps", 3)]
    start = _gains((frm, sel1))
    fade = tp.controllers(sched, [s, 400], len(irs), start=start)
    gone = next(b for b in range(s, s + 400) if fade[b]["coef"][0, frm] == 0.0)
    assert 100 < gone - s < 200 and fade[gone - 1]["coef"][0, frm] < 1e-13 and fade[s]["coef"][0, frm] == pytest.approx(0.875 * 0.875)
    gone = next(b for b in range(gone, s + 400) if fade[b]["coef"][0, to] == fade[s + 399]["coef"][0, to])  # (and the incoming one has arrived)
    assert fade[gone]["coef"][0, to] == 0.875
    z = -(-(gone + p_end) // T) * T
    places = [(0, s - 1, 255), (1, s - 1, 77), (0, s, 0), (0, s + 1, 131), (1, s + 3, 0), (0, s + 5, 255), (0, z, 77), (1, z + 1 if T > 1 else z, 131)]
    imp = tp.impulses_on(places, seed=frm + 10 * to + T)
    calls, at = cut([s, z], T, _quiet(irs, imp, sched))
    return s, z, sched, start, imp, calls, at


SWITCHED = {
    "streaming": dict(env=ENV["stream"], T=7, fade=(STREAM, False), settled=(STREAM, False)),
    "resident": dict(env=ENV["resident"], T=9, fade=DIRECT, settled=DIRECT),
    "fused": dict(env=ENV["fused"], T=64, fade=DIRECT, settled=(FUSED, True)),
    "overlap-save": dict(env=dict(ENV["os"], MCCONV_FFT2="0"), T=64, fade=DIRECT, settled=(OS, True)),
}


@pytest.mark.parametrize("frm,to", [(0, 2), (2, 0)], ids=["short-to-long", "long-to-short"])
@pytest.mark.parametrize("form", list(SWITCHED))
def test_one_half_switches_ir(gpu_lib, monkeypatch, form, frm, to):
    """IRs of 17, 5 and 33 partitions: the two voices have different p_end; the fade goes through the per-slot-gain forms
    (k_mac_stream<false>, k_mac_resident<true>), the settled two-voice state through k_mac_stream<true>, k_mac_resident<false>,
    k_g2_mac and the overlap-save fold."""
    k = SWITCHED[form]
    irs = _irs(17, 5, 33, seed=1)
    s, z, sched, start, imp, calls, at = _switch_layout(irs, frm, to, k["T"])
    expect = {at[s]: k["fade"], at[z]: k["settled"], len(calls) - 1: k["settled"]}
    _batch(monkeypatch, f"switch {frm} -> {to}, {form}: at {s}, settled at {z}", k["env"], 16384, irs, calls, imp, sched, start, expect)


@pytest.mark.parametrize("frm,to", [(0, 2), (2, 0)], ids=["short-to-long", "long-to-short"])
def test_one_half_switches_ir_split_form(gpu_lib, monkeypatch, frm, to):
    """259, 5 and 275 partitions in calls of 768 blocks: the fade takes the split form's per-slot sequences, four per voice."""
    irs = _irs(259, 5, 275, seed=2)
    s, z, sched, start, imp, calls, at = _switch_layout(irs, frm, to, 768)
    _batch(monkeypatch, f"switch {frm} -> {to}, split: at {s}, settled at {z}", ENV["split"], 131072, irs, calls, imp, sched, start,
           {at[s]: (SPLIT, True), at[z]: (SPLIT, True), len(calls) - 1: (SPLIT, True)})


@pytest.mark.parametrize("short", [True, False], ids=["a-short-voice", "two-long-voices"])
def test_one_half_switches_ir_fast_fir_form(gpu_lib, monkeypatch, short):
    """The fast-FIR form halves every voice's partitions, so the shortest sounding voice must have 256 (§2.5c, pmin).  Half 0 from
    5 to 275 partitions with half 1 on 2: voice 0 has 16 slots and keeps sounding, so no call takes the form.  Half 0 from 259 to
    275 with half 1 on 256: both voices qualify, and every call takes it, the fade (per-slot gains) and the settled state alike."""
    irs = _irs(5, 2, 275, seed=3) if short else _irs(259, 256, 275, seed=4)
    s, z, sched, start, imp, calls, at = _switch_layout(irs, 0, 2, 2048)
    want = DIRECT if short else (1, True)
    _batch(monkeypatch, f"switch, fast-FIR, short {short}: at {s}, settled at {z}", ENV["fastfir"], 131072, irs, calls, imp, sched, start,
           {j: want for j in range(at[s], len(calls))})


@pytest.mark.parametrize("frm,to", [(0, 2), (2, 0)], ids=["short-to-long", "long-to-short"])
@pytest.mark.parametrize("form", ["td", "fd"])
def test_one_half_switches_ir_jack(gpu_lib, monkeypatch, form, frm, to):
    irs = _irs(17, 5, 33, seed=1)
    s, z, sched, start, imp, calls, at = _switch_layout(irs, frm, to, 1)
    nper = sum(calls)
    states = tp.controllers(sched, calls, len(irs), start=start)
    got = run_jack(monkeypatch, form, 256, 16384, irs, 0, nper, tp.stream(imp, nper * BLOCK), sched, start)
    judge(f"switch {frm} -> {to}, JACK {form}: at {s}, settled at {z}", got, irs, imp, None, 0.4, states)


# ---------------------------------------------------------------------------------------------------------------------------
# d. more IRs than voices: the merge (consolidate_voices, k_mix) and the flush before it
def _sweep_layout(T):
    """Half 0 sweeps 0 -> 1 -> 2 -> 3 in successive calls of 2 blocks (vsteps 3): the fourth IR finds the half's three voices
    taken, and the engine renders what is owed, merges and restarts.  Half 1 stays on IR 4.  Impulses before the merge, on its
    call and after it.  IR 2 is the longest: its last 5 partitions lie beyond the end of every other IR of the merge."""
    irs = _irs(9, 5, 17, 12, 7, seed=5)
    s = -(-(WARM + 32) // 2) * 2
    sched = []
    for k, sel in enumerate((1, 2, 3)):
        sched += [(s + 2 * k, 0, "select", sel), (s + 2 * k, 0, "vsteps", 3)]
    m = s + 4
    places = [(0, s - 1, 255), (0, s + 1, 77), (0, s + 3, 0), (0, m, 131), (1, m, 0), (0, m + 1, 255), (0, m + 2, 77), (1, m + 5, 0), (0, m + 16, 131)]
    imp = tp.impulses_on(places, seed=77)
    marks = list(range(s, m + 18, 2))
    calls, at = cut(marks, T, _quiet(irs, imp, sched))
    return irs, s, m, sched, _gains((0, 4)), imp, calls, at


def _longest_tail(tag, got, irs, imp, states, m):
    """The taps of IR 2 beyond the end of every other IR, under the impulses from the merge on: what k_mix copies from one source."""
    w = tp.render(irs, imp, states, got.shape[1])
    others = max(irs[j].shape[0] for j in (0, 1, 3))
    worst = 0.0
    for i, n, a in imp:
        if i == 0 and n // BLOCK >= m:
            lo, hi = n + others, n + irs[2].shape[0]
            worst = max(worst, float(np.abs(got[:, lo:hi] - w[:, lo:hi]).max()) / (tp.SIGMA * tp.AMP))
    print(f"{tag}: IR 2's taps beyond the other IRs' ends, impulses from the merge on: worst {worst:.2e} U")
    assert worst <= WORST_BAR


def test_more_irs_than_voices_streaming(gpu_lib, monkeypatch):
    irs, s, m, sched, start, imp, calls, at = _sweep_layout(2)
    states = tp.controllers(sched, calls, len(irs), start=start)
    assert sum(1 for c in states[m]["coef"][0] if c != 0.0) == 4
    x = tp.stream(imp, sum(calls) * BLOCK)
    got, forms, st = run_device(monkeypatch, ENV["stream"], 8192, irs, 0, calls, x, sched, start)
    forms_or_skip(all(f == (STREAM, False) for f in forms), f"{forms}")
    judge(f"sweep over four IRs, streaming: merge at {m}", got, irs, imp, None, 0.4, states)
    _longest_tail("sweep, streaming", got, irs, imp, states, m)


@pytest.mark.parametrize("form", ["td", "fd"])
def test_more_irs_than_voices_jack(gpu_lib, monkeypatch, form):
    irs, s, m, sched, start, imp, calls, at = _sweep_layout(1)
    nper = sum(calls)
    states = tp.controllers(sched, calls, len(irs), start=start)
    got = run_jack(monkeypatch, form, 256, 8192, irs, 0, nper, tp.stream(imp, nper * BLOCK), sched, start)
    judge(f"sweep over four IRs, JACK {form}: merge at {m}", got, irs, imp, None, 0.4, states)
    _longest_tail(f"sweep, JACK {form}", got, irs, imp, states, m)


# ---------------------------------------------------------------------------------------------------------------------------
# e. predelay 0 -> 301 -> 256 while responses ring: retire_epoch, k_flush_ola, k_flush_ring
def _predelay_layout(irs, T, gap=14):
    p_end = _p_end(irs, 0, 1)
    q = -(-(WARM + p_end) // T) * T
    q2 = q + -(-gap // T) * T
    sched = [(q, 0, "predelay", 301), (q2, 0, "predelay", 256)]
    places = [(0, q - 1, 255), (1, q - 1, 77), (1, q, 0), (0, q + 1 if T > 1 else q, 131), (0, q2 - 1, 255), (1, q2, 0), (0, q2 + 2, 77)]
    imp = tp.impulses_on(places, seed=T)
    calls, at = cut([q, q2], T, _quiet(irs, imp, sched, 301))
    return q, q2, sched, imp, calls, at


@pytest.mark.parametrize("form,T", [("stream", 7), ("resident", 9)])
def test_predelay_changes_while_responses_ring(gpu_lib, monkeypatch, form, T):
    """The blocks played before a change ring out at the old offset, from the residual rings; the flush renders them with the form
    its P blocks take (below the stream threshold in launches of the streaming MAC, else the resident MAC with per-slot gains)."""
    irs = _irs(17, 17, seed=6)
    q, q2, sched, imp, calls, at = _predelay_layout(irs, T)
    want = (STREAM, False) if form == "stream" else DIRECT
    _batch(monkeypatch, f"predelay 0 -> 301 at {q} -> 256 at {q2}, {form}", ENV[form], 8192, irs, calls, imp, sched, _gains(), {j: want for j in range(len(calls))})


@pytest.mark.parametrize("form,period", [("td", 256), ("fd", 256), (None, 512)], ids=["256-td", "256-fd", "512"])
def test_predelay_changes_while_responses_ring_jack(gpu_lib, monkeypatch, form, period):
    pm = period // BLOCK
    irs = _irs(17, 17, seed=6)
    q, q2, sched, imp, calls, at = _predelay_layout(irs, pm)
    assert set(calls) == {pm}
    start = _gains()
    states = tp.controllers(sched, calls, len(irs), period, start)
    got = run_jack(monkeypatch, form, period, 8192, irs, 0, len(calls), tp.stream(imp, sum(calls) * BLOCK), sched, start)
    judge(f"predelay 0 -> 301 at {q} -> 256 at {q2}, JACK {form or period}", got, irs, imp, None, 0.4, states)


def test_overlap_save_form_waits_for_a_retired_epoch(gpu_lib, monkeypatch):
    """os_applies refuses a call while a retired epoch rings out: until (q - 1) 256 + n_ref, 127 blocks after a change at block q
    with n_ref = 32768.  Calls of 64 blocks: the calls at q and q + 64 take the resident MAC, the one at q + 128 the overlap-save
    form again, and the taps are right on both sides."""
    T, n_ref = 64, 32768
    irs = _irs(3, 3, seed=8)
    q = (-(-(WARM + 16) // T) + 1) * T  # (the call before q is settled: one entry of the gain table serves its blocks)
    sched = [(q, 0, "predelay", 301)]
    places = [(0, q - 1, 255), (1, q - 1, 77), (1, q, 0), (0, q + 1, 131), (0, q + 63, 255), (1, q + 64, 0), (0, q + 127, 77), (1, q + 128, 131)]
    imp = tp.impulses_on(places, seed=9)
    calls, at = cut([q], T, _quiet(irs, imp, sched, 301))
    assert set(calls) == {T}
    expect = {j: (OS, True) if b < q or b >= q + 128 else DIRECT for b, j in at.items() if b >= q - T}
    _batch(monkeypatch, f"overlap-save around a predelay change at {q}", dict(ENV["os"], MCCONV_FFT2="0"), n_ref, irs, calls, imp, sched, _gains(), expect)
