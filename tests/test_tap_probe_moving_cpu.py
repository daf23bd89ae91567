"""The tap probe's closed form under a controller schedule (tests/tap_probe.py: controllers, render, want_scheduled) proved on the
CPU: gain, wet, pan, level and dry steps against the oracle's linear mode, which carries per-block gains;
IR switches and predelay changes against the numpy restatement of the reference's per-call algorithm in its linear form
(oracle/refcompat_np.py: whole spectra interpolated, each call's contribution shifted by that call's predelay - no per-IR
scalar anywhere); and five faults of the kind the device cases are there to find, planted in the closed form and read
against the clean oracle output: each must read >= 0.006 U, 60 times the bar of the device cases, at the place it was planted.

0.006 U: every path gain G c of these schedules is >= 0.25 where a fault is read, the smallest tap is 0.5 SIGMA, the smallest
impulse 0.5 AMP, and the mildest fault is a gain 10 % wrong: 0.1 x 0.25 x 0.25 U = 0.00625 U."""
import functools

import numpy as np
import pytest

import tap_probe as tp
from tap_probe import BLOCK, WARM

N_REF = 8192
CALL = 7
ORACLE_BAR = 1e-6
FAULT_FLOOR = 0.006
GPU_BAR = 1e-4
P0, P1, P2 = 17, 14, 21  # partitions of the three IRs: they differ by whole partitions; 256 P2 + 255 + 301 <= N_REF, so no Q8 cut


def _irs():
    return [tp.probe_ir(BLOCK * P0 - 77, 301), tp.probe_ir(BLOCK * P1 - 130, 302), tp.probe_ir(BLOCK * P2 - 5, 303)]


def _start(predelay=0):
    """Four different path gains: L<-in1 0.328, L<-in2 0.469, R<-in1 0.656, R<-in2 0.352 (every value a float32)."""
    s = tp.start_values(predelay)
    s[0].update(panWet=0.5, level=0.75, wet=0.875)
    s[1].update(panWet=-0.25, level=0.625, wet=0.75)
    return s


def _calls_until(irs, imp, schedule, start, period=BLOCK):
    """Calls of CALL blocks until two blocks past the end of the last response."""
    n = max(k for _, k, _ in imp) // BLOCK + 1
    while True:
        calls = [CALL] * -(-n // CALL)
        states = tp.controllers(schedule, calls, len(irs), period, start)
        need = -(-tp.reach_end(irs, imp, states) // BLOCK) + 2
        if need <= sum(calls):
            return calls, states
        n = need


def _gain_case(ramp):
    """Level and pan of both halves step at block g (a call start); 14 blocks later the wet gains, half 0 over 3 + 5 steps; 28
    blocks later a dry signal, different per half and panned.  Impulses on the block before each step and on it, both inputs."""
    g = 3 * CALL if ramp else -(-(WARM + P0) // CALL) * CALL
    irs = _irs()[:2]
    sched = [(g, 0, "level", 0.625), (g, 1, "level", 1.0), (g, 0, "panWet", -0.5), (g, 1, "panWet", 0.25),
             (g + 14, 0, "wet", 0.5), (g + 14, 0, "vsteps", 3), (g + 14, 1, "wet", 1.0),
             (g + 28, 0, "dry", 0.25), (g + 28, 0, "panDry", 0.5), (g + 28, 1, "dry", 0.5), (g + 28, 1, "panDry", -0.5)]
    imp = tp.impulses_on([(0, g - 1, 255), (1, g - 1, 77), (0, g, 0), (1, g, 131), (1, g + 13, 255), (0, g + 14, 0), (1, g + 15, 77), (0, g + 19, 131),
                          (0, g + 27, 255), (1, g + 28, 0), (0, g + 29, 77)], seed=31 + ramp)
    start = _start()
    calls, states = _calls_until(irs, imp, sched, start)
    return g, irs, sched, imp, start, calls, states


def _events(schedule):
    by = {}
    for b, half, field, value in schedule:
        by.setdefault(b, []).append((half, field, value))
    return by


def _upols(irs, x, schedule, calls, start):
    import oracle

    u = oracle.Upols(N_REF, compat=False)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
    for h in (0, 1):
        u.set(h, speed=100, **start[h])
    by, out, pos = _events(schedule), [], 0
    for n in calls:
        for half, field, value in by.get(pos, ()):
            u.set(half, **{field: value})
        out.append(u.process(x[0, pos * BLOCK:(pos + n) * BLOCK], x[1, pos * BLOCK:(pos + n) * BLOCK]))
        pos += n
    u.close()
    return np.concatenate(out, axis=1)


def _refcompat(irs, x, schedule, calls, start):
    """The reference's per-call algorithm, one call per block (the recurrence advances per block inside an engine's batch too)."""
    from oracle.refcompat_np import RefCompatNp

    r = RefCompatNp(N_REF, three_mult=False, linear=True)
    for i, ir in enumerate(irs):
        r.prepare(i, ir)
    cast = lambda f, v: int(v) if f in ("select", "vsteps", "predelay") else np.float32(v)  # noqa: E731
    for h in (0, 1):
        r.cc[h].update({f: cast(f, v) for f, v in start[h].items()})
    by, out = _events(schedule), []
    for b in range(sum(calls)):
        for half, field, value in by.get(b, ()):
            r.cc[half][field] = cast(field, value)
        out.append(r.process_block(x[0, b * BLOCK:(b + 1) * BLOCK], x[1, b * BLOCK:(b + 1) * BLOCK]))
    return np.concatenate(out, axis=1)


@functools.lru_cache(maxsize=None)
def _gain_run(ramp):
    g, irs, sched, imp, start, calls, states = _gain_case(ramp)
    x = tp.stream(imp, sum(calls) * BLOCK)
    clean = _upols(irs, x, sched, calls, start)
    clean.setflags(write=False)
    return g, irs, sched, imp, start, calls, states, clean


def _switch_case():
    """Half 0 goes from IR 0 to IR 2 over 3 + 5 steps at block s while half 1 stays on IR 1; the predelay goes 0 -> 301 at q and
    -> 256 at q2 while responses ring.  Impulses before the switch, on it, one and five blocks into the fade, and either side
    of both predelay changes."""
    s = -(-(WARM + P2) // CALL) * CALL
    q, q2 = s + 14, s + 28
    irs = _irs()
    sched = [(s, 0, "select", 2), (s, 0, "vsteps", 3), (q, 0, "predelay", 301), (q2, 0, "predelay", 256)]
    imp = tp.impulses_on([(0, s - 1, 255), (1, s - 1, 77), (0, s, 0), (0, s + 1, 131), (1, s + 3, 0), (0, s + 5, 255),
                          (0, q - 1, 77), (1, q, 0), (0, q + 1, 131), (1, q2 - 1, 255), (0, q2, 0)], seed=41)
    start = _start()
    calls, states = _calls_until(irs, imp, sched, start)
    return s, q, q2, irs, sched, imp, start, calls, states


@functools.lru_cache(maxsize=None)
def _switch_run():
    s, q, q2, irs, sched, imp, start, calls, states = _switch_case()
    x = tp.stream(imp, sum(calls) * BLOCK)
    clean = _refcompat(irs, x, sched, calls, start)
    clean.setflags(write=False)
    return s, q, q2, irs, sched, imp, start, calls, states, clean


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wet", [1.0, 0.75])
@pytest.mark.parametrize("predelay", [0, 301])
@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
def test_a_constant_schedule_is_the_plain_closed_form_bit_for_bit(ramp, predelay, wet):
    irs = _irs()[:2]
    first = 0 if ramp else WARM + P0
    imp = tp.place_impulses([first + CALL * j for j in range(4)], seed=5 + predelay, batch=1, first=first, extra=(first + 2, first + 3))
    nb = -(-tp.response_end(irs, imp, predelay) // BLOCK) + 2
    a = tp.want(irs, imp, nb * BLOCK, predelay, wet)
    b = tp.want_scheduled(irs, imp, nb * BLOCK, [], [nb], start=tp.start_values(predelay, wet))
    assert np.abs(a).max() > 0.5 * tp.SIGMA * 0.5 * tp.AMP * 0.2 * wet
    assert np.array_equal(a, b)


def test_an_event_inside_a_call_raises():
    tp.controllers([(7, 0, "level", 0.5)], [7, 7], 2)
    with pytest.raises(ValueError):
        tp.controllers([(8, 0, "level", 0.5)], [7, 7], 2)
    with pytest.raises(ValueError):
        tp.controllers([(7, 0, "speed", 3)], [7, 7], 2)
    with pytest.raises(ValueError):
        tp.controllers([], [3], 2, period=512)
    st = tp.controllers([(2, 1, "level", 0.5), (2, 0, "predelay", 301), (2, 1, "predelay", 7)], [2, 2], 2, period=512)
    assert [s["predelay"] for s in st] == [0, 0, 301, 301]  # (half 0's, as in the engine)
    assert st[0]["coef"][0, 0] == st[1]["coef"][0, 0] == pytest.approx(0.2) and st[2]["coef"][0, 0] == pytest.approx(0.36)  # once per period
    assert st[1]["G"][0][1] == 1.0 and st[2]["G"][0][1] == 0.5 and st[2]["G"][0][0] == 1.0


@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
def test_gain_steps_are_what_the_oracle_computes(oracle_mod, ramp):
    """Level, pan, wet (over vsteps + 5 steps) and dry steps against oracle.Upols(compat=False): <= 1e-6 U."""
    g, irs, sched, imp, start, calls, states, clean = _gain_run(ramp)
    w = tp.render(irs, imp, states, clean.shape[1])
    r = tp.compare(clean, w, irs, imp, states=states)
    dry_peak = tp.AMP * max(max(row) for s in states for row in s["D"])
    print(f"gain steps at block {g}: {tp.describe(r)}; {len(imp)} impulses, peak {np.abs(w).max():.3f}, {sum(calls)} blocks")
    gains = sorted({round(s["G"][c][i] * s["coef"][i, i], 6) for s in (states[g - 1], states[g]) for c in (0, 1) for i in (0, 1)})
    print(f"path gains either side of the step: {gains}")
    assert len(gains) == 8 and gains[0] >= 0.25, gains  # (all different, so no exchange reads as nothing)
    assert np.abs(w).max() < 0.4 + dry_peak  # (the wet sum as in every case, plus one dry impulse: AMP x the largest dry gain, 0.5 x 1 x 1)
    assert r["worst"] <= ORACLE_BAR, tp.describe(r)
    assert np.abs(clean[:, -2 * BLOCK:]).max() <= 1e-12


def test_ir_switch_and_predelay_changes_are_what_the_reference_algorithm_computes():
    """Select and predelay events against the numpy restatement in its linear form: <= 1e-6 U."""
    s, q, q2, irs, sched, imp, start, calls, states, clean = _switch_run()
    w = tp.render(irs, imp, states, clean.shape[1])
    r = tp.compare(clean, w, irs, imp, states=states)
    print(f"switch at {s}, predelay at {q} and {q2}: {tp.describe(r)}; {len(imp)} impulses, peak {np.abs(w).max():.3f}, {sum(calls)} blocks")
    assert states[s]["coef"][0, 0] == pytest.approx(0.875 * 0.875) and states[s]["coef"][0, 2] == pytest.approx(0.875 / 8)
    assert max(h.shape[0] for h in irs) + 255 + max(st["predelay"] for st in states) <= N_REF  # (no contribution reaches the Q8 cut)
    assert np.abs(w).max() < 0.4
    assert r["worst"] <= ORACLE_BAR, tp.describe(r)
    assert np.abs(clean[:, -2 * BLOCK:]).max() <= 1e-12


def test_the_numpy_restatement_in_its_linear_form_is_plain_convolution():
    """The switch itself: noise through one IR, constant controllers, against numpy's own convolution; and the default still has
    the Q1 / Q2 shortcuts (the goldens are made with it: tests/test_oracle.py holds them)."""
    from oracle.refcompat_np import RefCompatNp, split, unpack

    rng = np.random.default_rng(3)
    z = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    L, R = split(np.fft.fft(z))
    assert np.allclose(L, np.fft.fft(z.real), atol=1e-12) and np.allclose(R, np.fft.fft(z.imag), atol=1e-12)
    Lq, Rq = unpack(np.fft.fft(z))
    assert np.allclose(Lq[1:32], L[1:32]) and Rq[0] == 0 and Lq[32] == 0 and abs(L[32]) > 0
    ir = tp.probe_ir(700, 9)
    x = rng.uniform(-0.2, 0.2, (2, 8 * BLOCK)).astype(np.float32)
    want = np.stack([np.convolve(x[0], ir[:, c].astype(np.float64))[:8 * BLOCK] for c in (0, 1)])
    for linear, close in ((True, True), (False, False)):
        r = RefCompatNp(2048, three_mult=False, linear=linear)
        r.prepare(0, ir)
        for h in (0, 1):
            r.cc[h].update(select=0, wet=np.float32(1), dry=np.float32(0), vsteps=0)
        r.irfft = [[r.ir[0][c].copy() for c in (0, 1)] for _ in (0, 1)]  # settled
        r.cc[1]["level"] = np.float32(0)
        got = r.process(x[0], x[1])
        assert (np.abs(got - want).max() <= 1e-12) == close


# ---------------------------------------------------------------------------------------------------------------------------
def _copy(states):
    return [dict(s, G=[list(r) for r in s["G"]], D=[list(r) for r in s["D"]], coef=s["coef"].copy()) for s in states]


def _read(tag, clean, irs, imp, states, faulty):
    """The clean oracle output read against a closed form with a fault in it."""
    r0 = tp.compare(clean, tp.render(irs, imp, states, clean.shape[1]), irs, imp, states=states)
    r = tp.compare(clean, tp.render(irs, imp, faulty, clean.shape[1]), irs, imp, states=states)
    print(f"{tag}: {tp.describe(r)}")
    assert r0["worst"] <= ORACLE_BAR
    assert r["worst"] >= FAULT_FLOOR and r["worst"] > 50 * GPU_BAR, tp.describe(r)
    return r


@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
def test_exchanged_cross_gains_fail_the_probe(oracle_mod, ramp):
    """L<-in2 and R<-in1 exchanged: named on channel 0 under an impulse on input 1, or on channel 1 under one on input 0."""
    g, irs, sched, imp, start, calls, states, clean = _gain_run(ramp)
    bad = _copy(states)
    for s in bad:
        s["G"][0][1], s["G"][1][0] = s["G"][1][0], s["G"][0][1]
    r = _read("cross gains exchanged", clean, irs, imp, states, bad)
    assert any(imp[k][0] == 1 - r["channel"] for k, _ in r["covering"]), tp.describe(r)


@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
def test_a_gain_step_one_block_late_fails_the_probe(oracle_mod, ramp):
    """Block g still at the gains of g - 1: named under an impulse on block g, and nowhere near the bar otherwise."""
    g, irs, sched, imp, start, calls, states, clean = _gain_run(ramp)
    bad = _copy(states)
    bad[g]["G"] = [list(r) for r in states[g - 1]["G"]]
    r = _read("gain step one block late", clean, irs, imp, states, bad)
    assert any(imp[k][1] // BLOCK == g for k, _ in r["covering"]), tp.describe(r)


@pytest.mark.parametrize("ramp", [False, True], ids=["settled", "ramp"])
def test_the_other_halfs_dry_gain_fails_the_probe(oracle_mod, ramp):
    g, irs, sched, imp, start, calls, states, clean = _gain_run(ramp)
    bad = _copy(states)
    for s in bad:
        for c in (0, 1):
            s["D"][c][0], s["D"][c][1] = s["D"][c][1], s["D"][c][0]
    r = _read("dry gain of the other half", clean, irs, imp, states, bad)
    assert r["dry"] is not None and imp[r["dry"]][1] // BLOCK >= g + 28, tp.describe(r)


def test_an_outgoing_voice_without_its_last_partition_fails_the_probe():
    """IR 0's last partition missing for the blocks of the fade only: the worst sample lies on IR 0, partition P0 - 1, of an impulse
    of the fade on input 0."""
    s, q, q2, irs, sched, imp, start, calls, states, clean = _switch_run()
    cut = list(irs)
    cut[0] = irs[0].copy()
    cut[0][BLOCK * (P0 - 1):] = 0
    bad = _copy(states)
    fade = [b for b in range(s, len(bad)) if bad[b]["coef"][0, 0] != 0.0]
    assert fade == list(range(s, s + len(fade))) and s + 5 in fade and s - 1 not in fade
    for b in fade:
        bad[b]["irs"] = cut
    r = _read("outgoing voice without its last partition", clean, irs, imp, states, bad)
    assert any(j == 0 and t // BLOCK == P0 - 1 and imp[k][0] == 0 and imp[k][1] // BLOCK in fade for (k, t), j in zip(r["covering"], r["voices"])), tp.describe(r)


def test_a_block_played_at_the_next_calls_predelay_fails_the_probe():
    s, q, q2, irs, sched, imp, start, calls, states, clean = _switch_run()
    for at in (q, q2):
        bad = _copy(states)
        bad[at - 1]["predelay"] = states[at]["predelay"]
        r = _read(f"block {at - 1} at the predelay of block {at}", clean, irs, imp, states, bad)
        assert any(imp[k][1] // BLOCK == at - 1 for k, _ in r["covering"]), tp.describe(r)
