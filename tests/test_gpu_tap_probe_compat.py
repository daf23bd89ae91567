"""The tap probe in compat mode (tests/tap_probe.py: render_compat): the Q1/Q2 windows and the Q8 cut read frame
by frame through the forms that compute them - k_drop_fft, the one-term shape of k_fwd<true>, the time-domain tiles, the period
kernels of the JACK path with the terms a launch carries for the next period, k_corr / k_post, the prefix sums that ride with
the fused second-level transform and the ones that do not, the overlap-save schedule, the tails, k_flush_fix - against the closed
form that tests/test_tap_probe_compat_cpu.py proves on the two oracles to 1e-14 U.

Conventions as in test_gpu_tap_probe.py: buffers pre-filled with 7; the form of every probed call asserted (kernel_stats(),
os_stats(), drop_stats(), tail_forms(), park_stats()); `worst` <= 1e-4 U over the whole stream, where a window or cut edge
one frame off reads 0.02 U to 1.4 U (the CPU file's planted faults); the last two blocks of the last call, which starts beyond
every response, every Q1/Q2 window (n_ref / 256 blocks more than in linear mode) and every form's reach, exact zeros.
The IRs carry a bias (tap_probe.probe_ir_biased), so every Q1 and Q2 term is >= 0.02 U and the peak bar is 0.6.  pytest -s
prints every case."""
import numpy as np
import pytest

import tap_probe as tp
from tap_probe import BLOCK, WARM
from tap_probe_device import FUSED, OS, STREAM, WORST_BAR, cut, forms_or_skip, judge, layout, run_device, run_jack

pytestmark = pytest.mark.gpu

BIAS = 0.25
PEAK = 0.6
N_REF = 4096   # the Q8 regime: IRs of 12 partitions, 3072 - 77 and 3072 - 130 taps
P_REG = 12
ENV = dict(
    stream=dict(MCCONV_OS="0"),
    resident=dict(MCCONV_FFT2="0", MCCONV_FFA_LEVELS="0", MCCONV_OS="0"),
    fused=dict(MCCONV_FFT2="1", MCCONV_FFT2_FUSED="1", MCCONV_FFT2_WORK="1", MCCONV_OS="0", MCCONV_FFA_LEVELS="0"),
    os=dict(MCCONV_OS="1", MCCONV_OS_MIN="48", MCCONV_FFA_LEVELS="0"),
)
TILES = dict(MCCONV_TD_FFT="0")


def _irs(P, *more):
    """Two biased IRs of P partitions, the last one partial and differently so; `more`: further ones by their taps."""
    return [tp.probe_ir_biased(BLOCK * P - 77, 700 + 2 * P, BIAS), tp.probe_ir_biased(BLOCK * P - 130, 701 + 2 * P, BIAS)] + \
        [tp.probe_ir_biased(t, 702 + 2 * P + k, BIAS) for k, t in enumerate(more)]


def _drop_form(tag, st, want):
    """drop_stats(): the batches of the stream took their cut terms in the form `want` and in no other."""
    d = {k: st["drop"][k] for k in ("drop_fft", "forward_transforms", "tiles")}
    forms_or_skip(d[want] > 0 and sum(d.values()) == d[want], f"{tag}: cut terms not by {want} alone: {st['drop']}")


def _batch(monkeypatch, tag, env, n_ref, irs, predelay, calls, imp, expect, *, schedule=(), start=None, singles=False):
    """The stream through process_device in compat mode, the forms of the calls `expect` names, the judgement."""
    start = start or tp.start_values(predelay)
    states = tp.controllers(schedule, calls, len(irs), start=start)
    x = tp.stream(imp, sum(calls) * BLOCK)
    got, forms, st = run_device(monkeypatch, env, n_ref, irs, predelay, calls, x, schedule, start, compat=True, singles=singles)
    for k, want in sorted(expect.items()):
        forms_or_skip(forms[k] == want, f"{tag}: call {k} of {calls[k]} blocks from block {sum(calls[:k])} took {forms[k]}, not {want}")
    forms_or_skip((st["batches"] > 0) == any(w[0] == OS for w in expect.values()), f"{tag}: {st}")
    r = judge(tag, got, irs, imp, None, PEAK, states, compat=dict(n_ref=n_ref))
    return got, forms, st, r


# ---------------------------------------------------------------------------------------------------------------------------
# A. batches in the Q8 regime
@pytest.mark.parametrize("predelay", [1100, 2000])
def test_batches_whose_cut_terms_k_drop_fft_sums(gpu_lib, monkeypatch, predelay):
    """Unaligned and large predelay: several (kappa, partition) terms per output block, summed over the whole batch by k_drop_fft;
    calls below the streaming threshold and above it."""
    irs = _irs(P_REG)
    for T, form in ((7, (STREAM, False)), (9, (0, True))):
        calls, imp, probed = layout(P_REG, predelay, [T, T, T], T, ramp=T, warm=T, seed=predelay + T, window=N_REF // BLOCK)
        tag = f"Q8 batch T {T} predelay {predelay}"
        _, _, st, _ = _batch(monkeypatch, tag, ENV["stream"] if T == 7 else ENV["resident"], N_REF, irs, predelay, calls, imp, {k: form for k in probed + [len(calls) - 1]})
        _drop_form(tag, st, "drop_fft")


def test_batches_in_the_shipped_one_term_shape(gpu_lib, monkeypatch):
    """Predelay 1024, calls of 30 blocks (longer than the 16 blocks the one term reaches back): k_fwd<true> sums the cut terms."""
    irs = _irs(P_REG)
    calls, imp, probed = layout(P_REG, 1024, [30, 30, 30], 30, ramp=30, warm=30, seed=30, window=N_REF // BLOCK)
    _, _, st, _ = _batch(monkeypatch, "Q8 one-term shape", ENV["resident"], N_REF, irs, 1024, calls, imp, {k: (0, True) for k in probed + [len(calls) - 1]})
    _drop_form("Q8 one-term shape", st, "forward_transforms")


@pytest.mark.parametrize("predelay", [1024, 1100])
def test_batches_whose_cut_terms_the_time_domain_tiles_sum(gpu_lib, monkeypatch, predelay):
    irs = _irs(P_REG)
    calls, imp, probed = layout(P_REG, predelay, [9, 9, 9], 9, ramp=9, warm=9, seed=predelay + 1, window=N_REF // BLOCK)
    _, _, st, _ = _batch(monkeypatch, f"Q8 tiles predelay {predelay}", dict(ENV["resident"], **TILES), N_REF, irs, predelay, calls, imp,
                         {k: (0, True) for k in probed + [len(calls) - 1]})
    _drop_form(f"Q8 tiles predelay {predelay}", st, "tiles")


@pytest.mark.parametrize("sizes", [[120, 120, 60], [150, 1, 1, 148]], ids=["even", "periods_between"])
def test_batches_longer_than_the_look_back(gpu_lib, monkeypatch, sizes):
    """As test_gpu_parity.py::test_q8_history_across_long_batches: k_fwd keeps only the tail of such a batch in the input-history
    ring, and the next call - a batch or single periods through onProcess - looks back into it.  Impulses at the end of every
    batch and on the single periods."""
    irs = _irs(P_REG)
    ends = lambda b: [x - 1 for x in b[1:-1]] + [x for x in b[1:-1]]  # noqa: E731
    calls, imp, probed = layout(P_REG, 1024, sizes, 40, warm=40, seed=len(sizes), extra=ends, limit=10, window=N_REF // BLOCK)
    _batch(monkeypatch, f"Q8 long batches {sizes}", ENV["resident"], N_REF, irs, 1024, calls, imp, {}, singles=True)


# ---------------------------------------------------------------------------------------------------------------------------
# B. period calls
def _jack(monkeypatch, tag, form, period, n_ref, irs, predelay, env=None, schedule=None, places=None, start=None):
    """170 periods of silence, then impulses around four consecutive periods, in every block of one of them, at in-block offsets 0
    and 255, and one period further on (a settled stream: every period parked one call ahead); or `places` under `schedule`."""
    pm = period // BLOCK
    warm = WARM * pm
    P = max(-(-h.shape[0] // BLOCK) for h in irs)
    if places is None:
        bounds = [warm + pm * j for j in range(5)]
        imp = tp.place_impulses(bounds, seed=predelay + pm, batch=2, first=warm, limit=12,
                                extra=[bounds[3], bounds[0], bounds[4] - 1, bounds[4] + pm] + [bounds[2] + k for k in range(pm)] + [bounds[3] + pm - 1])
    else:
        imp = places
    last = max([n // BLOCK for _, n, _ in imp] + [b for b, _, _, _ in schedule or ()])
    quiet = last + P + -(-max([predelay] + [v for _, _, f, v in schedule or () if f == "predelay"]) // BLOCK) + 10 + n_ref // BLOCK
    nper = -(-quiet // pm) + 1
    start = start or tp.start_values(predelay)
    states = tp.controllers(schedule or [], [pm] * nper, len(irs), period, start)
    stats = {}
    got = run_jack(monkeypatch, form, period, n_ref, irs, predelay, nper, tp.stream(imp, nper * period), schedule or [], start, compat=True, env=env, stats=stats)
    judge(tag, got, irs, imp, None, PEAK, states, compat=dict(n_ref=n_ref, period=period))
    return stats


@pytest.mark.parametrize("form", ["td", "fd"])
@pytest.mark.parametrize("predelay", [1024, 1100])
def test_jack_256_in_the_regime(gpu_lib, monkeypatch, form, predelay):
    """k_drop_period_fft<1> until the stream settles, then the terms k_jack carries for the period after the next."""
    st = _jack(monkeypatch, f"Q8 JACK 256 {form} predelay {predelay}", form, 256, N_REF, _irs(P_REG), predelay)
    forms_or_skip(st["drop"]["carried_periods"] > 0 and st["park"]["used"] > 0, f"no carried cut terms: {st}")


def test_jack_256_with_time_domain_cut_terms(gpu_lib, monkeypatch):
    """MCCONV_TD_FFT=0: k_drop_period<1> ahead of every tail; nothing is carried."""
    st = _jack(monkeypatch, "Q8 JACK 256 time-domain cut terms", None, 256, N_REF, _irs(P_REG), 1100, env=TILES)
    assert st["drop"]["carried_periods"] == 0, st


@pytest.mark.parametrize("predelay", [256, 700, 1024])
@pytest.mark.parametrize("period", [512, 1024])
def test_jack_longer_periods_in_the_regime(gpu_lib, monkeypatch, period, predelay):
    """Calls of 2 and 4 blocks: the cut is measured from the call's start, so the blocks of a call lose different taps
    (k_drop_period_fft<2|4>, and the terms a parked k_tailp sums for itself).  1024-frame periods are in the regime at all three
    predelays (taps + 1023 + predelay > n_ref), 512-frame ones at 700 and 1024: (512, 256) reads the Q1/Q2 window alone."""
    irs = _irs(P_REG)
    st = _jack(monkeypatch, f"Q8 JACK {period} predelay {predelay}", None, period, N_REF, irs, predelay)
    if max(h.shape[0] for h in irs) + period - 1 + predelay > N_REF:
        forms_or_skip(st["drop"]["carried_periods"] > 0, f"no parked tail summed its own cut terms: {st}")
    else:
        assert st["drop"]["carried_periods"] == 0, st


# ---------------------------------------------------------------------------------------------------------------------------
# C. Q1/Q2 outside the Q8 regime: 17 partitions at n_ref 8192
@pytest.mark.parametrize("predelay", [0, 256, 301])
def test_q1_q2_windows_of_streaming_and_resident_batches(gpu_lib, monkeypatch, predelay):
    """k_corr's window sums and k_post: impulses inside the ramp and after it."""
    irs = _irs(17)
    for T, env, form in ((7, ENV["stream"], (STREAM, False)), (9, ENV["resident"], (0, True))):
        calls, imp, probed = layout(17, predelay, [T, T, T], T, ramp=T, warm=T, seed=predelay + T, window=32)
        tag = f"Q1/Q2 batch T {T} predelay {predelay}"
        _, _, st, _ = _batch(monkeypatch, tag, env, 8192, irs, predelay, calls, imp, {k: form for k in probed + [len(calls) - 1]})
        assert sum(st["drop"][k] for k in ("drop_fft", "forward_transforms", "tiles")) == 0, st


@pytest.mark.parametrize("predelay", [0, 301])
def test_q1_q2_prefix_sums_that_ride_with_the_fused_form(gpu_lib, monkeypatch, predelay):
    """k_g2_mac at 17 partitions: calls of 64 blocks and one of a chunk (8192 - 17 + 1 blocks) plus one, impulses either side of
    the chunk's end."""
    chunk = 8192 - 17 + 1
    calls, imp, probed = layout(17, predelay, [64, 64, chunk + 1], 64, warm=64, seed=predelay + 17, window=32, extra=lambda b: [b[2] + chunk - 1, b[2] + chunk])
    _batch(monkeypatch, f"Q1/Q2 fused predelay {predelay}", ENV["fused"], 8192, _irs(17), predelay, calls, imp, {k: (FUSED, True) for k in probed + [len(calls) - 1]})


def test_q1_q2_prefix_sums_of_a_batch_too_long_to_ride(gpu_lib, monkeypatch):
    """More than 160 x 256 blocks in one call (as test_gpu_parity.py::test_batch_longer_than_the_riding_prefix_chain): the prefix
    sums run as launches of their own.  Impulses at both ends of the call, either side of block 160 x 256 and in the call before."""
    T = 41216
    calls, imp, probed = layout(17, 301, [64, T], 64, warm=64, seed=41, window=32, extra=lambda b: [b[1] + 160 * 256 - 1, b[1] + 160 * 256, b[1] + 8176])
    _batch(monkeypatch, "Q1/Q2 long batch", ENV["fused"], 8192, _irs(17), 301, calls, imp, {k: (FUSED, True) for k in probed + [len(calls) - 1]})


@pytest.mark.parametrize("predelay", [256, 301])
def test_q1_q2_windows_of_the_overlap_save_schedule(gpu_lib, monkeypatch, predelay):
    """k_corr_terms, k_corr_fix and k_out_windows: calls of 64 blocks and one of two segments plus 5 blocks (a segment hops by
    16384 blocks less the 32 of the window)."""
    hop = 16384 - 32
    calls, imp, probed = layout(17, predelay, [64, 64, 2 * hop + 5], 64, warm=40, seed=predelay + 3, window=32,
                                extra=lambda b: [b[2] + hop - 1, b[2] + hop, b[2] + 2 * hop])
    _, _, st, _ = _batch(monkeypatch, f"Q1/Q2 overlap-save predelay {predelay}", ENV["os"], 8192, _irs(17), predelay, calls, imp,
                         {k: (OS, True) for k in probed + [len(calls) - 1]})
    forms_or_skip(st["batches"] >= 4, f"{st}")


@pytest.mark.parametrize("form,period", [("td", 256), ("fd", 256), (None, 512), (None, 1024)], ids=["256-td", "256-fd", "512", "1024"])
def test_q1_q2_windows_of_the_jack_tails(gpu_lib, monkeypatch, form, period):
    for predelay in (0, 301):
        st = _jack(monkeypatch, f"Q1/Q2 JACK {form or period} predelay {predelay}", form, period, 8192, _irs(17), predelay)
        assert st["drop"]["carried_periods"] == 0, st


# ---------------------------------------------------------------------------------------------------------------------------
# D. overlap-save in the Q8 regime
def test_overlap_save_in_the_shipped_q8_shape(gpu_lib, monkeypatch):
    """Predelay 1024 at n_ref 4096: the overlap-save step takes the regime only in the one-term shape, its forward transforms
    summing the cut terms."""
    hop = 16384 - 16
    calls, imp, probed = layout(P_REG, 1024, [64, 64, 2 * hop + 5], 64, warm=40, seed=12, window=N_REF // BLOCK,
                                extra=lambda b: [b[2] + hop - 1, b[2] + hop, b[2] + 2 * hop])
    _, _, st, _ = _batch(monkeypatch, "Q8 overlap-save", ENV["os"], N_REF, _irs(P_REG), 1024, calls, imp, {k: (OS, True) for k in probed + [len(calls) - 1]})
    _drop_form("Q8 overlap-save", st, "forward_transforms")


# ---------------------------------------------------------------------------------------------------------------------------
# E. moving state in the regime
def _moving(monkeypatch, tag, irs, predelay, sched, places, start=None, T=9, seed=0):
    """Batches of T blocks, cut where an event needs a call start, until one starts beyond every window."""
    imp = tp.impulses_on(places, seed)
    last = max([b for _, b, _ in places] + [b for b, _, _, _ in sched])
    pd = max([predelay] + [v for _, _, f, v in sched if f == "predelay"])
    calls, at = cut([b for b, _, _, _ in sched], T, last + max(-(-h.shape[0] // BLOCK) for h in irs) + -(-pd // BLOCK) + 10 + N_REF // BLOCK)
    return _batch(monkeypatch, tag, ENV["resident"], N_REF, irs, predelay, calls, imp, {len(calls) - 1: (0, True)}, schedule=sched, start=start)


def test_a_predelay_change_in_the_regime_batches(gpu_lib, monkeypatch):
    """1024 -> 1088 -> 1024 while responses ring: k_flush_fix moves what the residual rings hold, window sums and cut terms with
    them; impulses either side of both changes."""
    g = -(-(WARM + P_REG) // 9) * 9
    sched = [(g, 0, "predelay", 1088), (g + 27, 0, "predelay", 1024)]
    places = [(0, g - 1, 255), (1, g - 1, 77), (1, g, 0), (0, g + 1, 131), (1, g + 26, 255), (0, g + 27, 0), (1, g + 28, 77)]
    _moving(monkeypatch, "Q8 predelay change, batches", _irs(P_REG), 1024, sched, places, seed=5)


def test_a_predelay_change_in_the_regime_jack(gpu_lib, monkeypatch):
    """The same through onProcess (as test_gpu_parity.py::test_q8_parked_periods_carry_the_next_periods_cut_terms): the terms a
    launch carried for the next period are stale after the change and must not be used."""
    g = WARM + P_REG
    sched = [(g, 0, "predelay", 1088), (g + 32, 0, "predelay", 1024)]
    imp = tp.impulses_on([(0, g - 2, 0), (1, g - 1, 255), (1, g, 0), (0, g + 1, 131), (1, g + 31, 255), (0, g + 32, 0), (1, g + 33, 77)], seed=6)
    st = _jack(monkeypatch, "Q8 predelay change, JACK", None, 256, N_REF, _irs(P_REG), 1024, schedule=sched, places=imp)
    forms_or_skip(st["park"]["used"] > 40 and st["drop"]["carried_periods"] > 40, f"{st}")


def test_a_level_and_pan_step_in_the_regime(gpu_lib, monkeypatch):
    """Level and panWet of both halves step at call start g: the cut terms and the Q1/Q2 sums of blocks g - 1 and g carry different
    gains inside one output block."""
    g = -(-(WARM + P_REG) // 9) * 9
    start = tp.start_values(1100)
    start[0].update(level=0.75, panWet=0.5)
    start[1].update(level=0.875)
    sched = [(g, 0, "level", 1.0), (g, 0, "panWet", -0.25), (g, 1, "level", 0.625), (g, 1, "panWet", 0.25)]
    places = [(0, g - 1, 255), (1, g - 1, 77), (1, g, 0), (0, g, 131), (1, g + 1, 255)]
    _moving(monkeypatch, "Q8 level and pan step", _irs(P_REG), 1100, sched, places, start=start, seed=7)


def test_an_ir_switch_in_the_regime(gpu_lib, monkeypatch):
    """Half 0 goes from an IR of 3072 - 77 taps to one of 2800 over 3 + 5 steps: two voices with cut terms of their own."""
    g = -(-(WARM + P_REG) // 9) * 9
    sched = [(g, 0, "select", 2), (g, 0, "vsteps", 3)]
    places = [(0, g - 1, 255), (1, g - 1, 77), (0, g, 0), (0, g + 1, 131), (1, g + 3, 0), (0, g + 5, 255), (0, g + 30, 77)]
    _moving(monkeypatch, "Q8 IR switch", _irs(P_REG, 2800), 1100, sched, places, seed=8)


# ---------------------------------------------------------------------------------------------------------------------------
def test_a_planted_fault_fails_on_the_engine_too(gpu_lib, monkeypatch):
    """The harness itself, on the device: the engine in the regime read against the closed form with its cut one frame late;
    `worst` must rise to a whole tap, >= 0.25 U, on the frame where an impulse's cut lies."""
    irs = _irs(P_REG)
    calls, imp, probed = layout(P_REG, 1100, [9, 9, 9], 9, warm=9, seed=2, window=N_REF // BLOCK)
    x = tp.stream(imp, sum(calls) * BLOCK)
    got, forms, st = run_device(monkeypatch, ENV["resident"], N_REF, irs, 1100, calls, x, compat=True)
    states = tp.controllers([], calls, 2, start=tp.start_values(1100))
    r = tp.compare(got, tp.render_compat(irs, imp, states, got.shape[1], N_REF, plant=dict(cut_late=1)), irs, imp, states=states, compat=dict(n_ref=N_REF))
    print(f"planted fault: {tp.describe(r)}")
    assert r["worst"] >= 0.25
    assert any(what == "cut" and d == 0 for _, what, d in r["edges"]), tp.describe(r)
    assert WORST_BAR < 0.25
