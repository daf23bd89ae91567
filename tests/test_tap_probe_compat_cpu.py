"""The tap probe's closed form in compat mode (tests/tap_probe.py: render_compat) proved on the CPU: against
oracle.RefCompat (C) and oracle/refcompat_np.py's RefCompatNp in its default, non-linear form, <= 1e-6 U, over 256-, 512- and
1024-frame reference calls, predelays either side of the Q8 regime, the cold-start ramp, an IR switch and a predelay change;
a condition on the inputs asserted on the oracle alone (every Q1 and Q2 term >= 0.02 U, a cut tap >= 0.25 U, peak < 0.6);
six faults planted in the closed form and read against the clean oracle; and what white noise under one RMS sees of two of them.

0.005 U, the faults' floor: the mildest fault gives a Q1 term the gains of the next block across a level step 0.75 -> 1, which
moves it by a quarter of a term that the condition holds >= 0.02 U: 0.25 x 0.02 U.  Every other fault removes, adds or exchanges
a whole Q1 term (>= 0.02 U) or a tap (>= 0.25 U under a path gain of 1), or exchanges two sums a fifth of the larger apart:
0.2 x 0.02 U on the weakest impulse alone, and `worst` reads the strongest of eight (it reads 0.14 U or more)."""
import functools

import numpy as np
import pytest

import tap_probe as tp
from tap_probe import BLOCK, WARM

ORACLE_BAR = 1e-6
GPU_BAR = 1e-4
TERM_FLOOR = 0.02
CUT_FLOOR = 0.25
FAULT_FLOOR = 0.005
PEAK = 0.6
BIAS = 0.25  # of SIGMA: every Q1 / Q2 term of the cases below >= 0.02 U (asserted), every tap >= 0.1 SIGMA, the output peak < 0.6
U = tp.SIGMA * tp.AMP


def _irs(n_ref, short):
    """In the regime: n_ref - 1024 taps exactly and 130 fewer, and a third one a partition shorter for the IR switch.  Short: a
    little over half of n_ref, 17 partitions at n_ref = 8192: taps + 1023 + 301 <= n_ref, outside the Q8 regime."""
    top = (n_ref // 2 + BLOCK) if short else n_ref - tp.COMPAT_KEEP
    return [tp.probe_ir_biased(top - (77 if short else 0), 500 + n_ref // 1024, BIAS), tp.probe_ir_biased(top - 130, 501 + n_ref // 1024, BIAS),
            tp.probe_ir_biased(top - BLOCK - 5, 502 + n_ref // 1024, BIAS)]


CASES = {
    # name: (period, predelay, short IRs, inside the ramp, moving state)
    "p256-pd0": (256, 0, False, False, None),
    "p256-pd256": (256, 256, False, False, None),
    "p256-pd1024": (256, 1024, False, False, None),
    "p256-pd1100": (256, 1100, False, False, None),
    "p256-pdmax": (256, "max", False, False, None),
    "p256-pd1024-ramp": (256, 1024, False, True, None),
    "p512-pd256": (512, 256, False, False, None),
    "p512-pd1024": (512, 1024, False, False, None),
    "p512-pd1100-ramp": (512, 1100, False, True, None),
    "p1024-pd0": (1024, 0, False, False, None),
    "p1024-pd256": (1024, 256, False, False, None),
    "p1024-pd1024": (1024, 1024, False, False, None),
    "p1024-pd1100": (1024, 1100, False, False, None),
    "p1024-pdmax-ramp": (1024, "max", False, True, None),
    "short-p256-pd0": (256, 0, True, False, None),
    "short-p256-pd301-ramp": (256, 301, True, True, None),
    "short-p1024-pd256": (1024, 256, True, False, None),
    "switch-p256": (256, 1024, False, False, "switch"),
    "switch-p512": (512, 1100, False, False, "switch"),
    "predelay-change-p256": (256, 1024, False, False, "predelay"),
    "level-step-p256": (256, 1024, False, False, "level"),
    "level-step-p1024": (1024, 1100, False, True, "level"),
}


def _case(name, n_ref):
    """The stream of a case: every reference call is one period.  Impulses on both inputs at in-call offsets 0 and 255, in the
    second and in the last block of a longer call, in consecutive calls and one at an odd in-call offset past a block boundary;
    q is the call that moving state changes at, with impulses on the call before it and on it."""
    period, pd, short, ramp, moving = CASES[name]
    pm = period // BLOCK
    if pd == "max":
        pd = n_ref - BLOCK  # (the window is one block long and nearly every tap is cut; beyond n_ref the reference's slices no longer match)
    irs = _irs(n_ref, short)
    q = 7 if ramp else -(-(WARM + 2) // pm)  # (call 7 of the ramp: coefficient 1 - 0.8^8 = 0.83)
    last = period - BLOCK
    second = BLOCK if pm > 1 else 0
    places = [(0, q - 1, 0), (1, q - 1, last + 255), (1, q, 0), (0, q, second + 77), (1, q + 1, second + 255), (0, q + 1, last + 131), (1, q + 2, last), (0, q + 3, 255)]
    start = tp.start_values(pd)
    sched = []
    if moving == "switch":
        sched = [(q * pm, 0, "select", 2), (q * pm, 0, "vsteps", 3)]
    elif moving == "predelay":
        sched = [(q * pm, 0, "predelay", 1088), ((q + 2) * pm, 0, "predelay", 1024)]
    elif moving == "level":
        for h in (0, 1):
            start[h]["level"] = 0.75
        sched = [(q * pm, 0, "level", 1.0), (q * pm, 1, "level", 1.0)]
    imp = tp.impulses_on([(i, c * pm, o) for i, c, o in places], seed=len(name) + n_ref // 1024)  # (o counts from the call's first block)
    ncalls = q + 4 + -(-(n_ref + 1088 + 2 * BLOCK) // period)
    calls = [pm] * ncalls
    states = tp.controllers(sched, calls, len(irs), period, start)
    assert ncalls * period >= tp.compat_end(irs, imp, states, n_ref, period) + 2 * BLOCK
    return dict(name=name, n_ref=n_ref, period=period, pm=pm, q=q, irs=irs, imp=imp, start=start, sched=sched, calls=calls, states=states, nframes=ncalls * period,
                regime=not short and (n_ref - tp.COMPAT_KEEP) + period - 1 + pd > n_ref)


def _events(sched):
    by = {}
    for b, half, field, value in sched:
        by.setdefault(b, []).append((half, field, value))
    return by


def _c_oracle(case):
    import oracle

    r = oracle.RefCompat(case["n_ref"], True)
    for i, ir in enumerate(case["irs"]):
        r.prepare(i, ir)
    for h in (0, 1):
        r.set(h, speed=100, **case["start"][h])
    x = tp.stream(case["imp"], case["nframes"])
    by, out, period, pm = _events(case["sched"]), [], case["period"], case["pm"]
    for k in range(len(case["calls"])):
        for half, field, value in by.get(k * pm, ()):
            r.set(half, **{field: value})
        out.append(r.process(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period], block=period))
    r.close()
    return np.concatenate(out, axis=1)


def _np_oracle(case, only=None, linear=False):
    """RefCompatNp call by call.  only: that impulse alone, and then the calls before its own advance the cross-fade only (their
    input is silence and so is their output); linear: the true split at 2 n_ref points, which neither wraps nor cuts."""
    from oracle.refcompat_np import RefCompatNp

    r = RefCompatNp(case["n_ref"] * (2 if linear else 1), three_mult=False, linear=linear)
    for i, ir in enumerate(case["irs"]):
        r.prepare(i, ir[:case["n_ref"] - tp.COMPAT_KEEP])
    cast = lambda f, v: int(v) if f in ("select", "vsteps", "predelay") else np.float32(v)  # noqa: E731
    for h in (0, 1):
        r.cc[h].update({f: cast(f, v) for f, v in case["start"][h].items()})
    imp = case["imp"] if only is None else [case["imp"][only]]
    x = tp.stream(imp, case["nframes"])
    by, period, pm = _events(case["sched"]), case["period"], case["pm"]
    first = min(n for _, n, _ in imp) // period
    out = np.zeros((2, case["nframes"]))
    for k in range(len(case["calls"])):
        for half, field, value in by.get(k * pm, ()):
            r.cc[half][field] = cast(field, value)
        if k < first:
            r._interp(0)
            r._interp(1)
        else:
            out[:, k * period:(k + 1) * period] = r.process_block(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period])
    return out


@functools.lru_cache(maxsize=None)
def _run(name, n_ref):
    case = _case(name, n_ref)
    clean = _c_oracle(case)
    clean.setflags(write=False)
    return case, clean


def _read(case, got, plant=None, tag=""):
    w = tp.render_compat(case["irs"], case["imp"], case["states"], case["nframes"], case["n_ref"], case["period"], plant)
    r = tp.compare(got, w, case["irs"], case["imp"], states=case["states"], compat=dict(n_ref=case["n_ref"], period=case["period"]))
    print(f"{case['name']} n_ref {case['n_ref']}{tag}: {tp.describe(r)}; peak {np.abs(w).max():.3f}")
    return r, w


ALL = [(name, n_ref) for n_ref in (4096, 8192) for name in CASES]
IDS = [f"{name}-{n_ref}" for name, n_ref in ALL]


# ---------------------------------------------------------------------------------------------------------------------------
def test_without_compat_terms_it_is_render_bit_for_bit():
    """IRs built of quadruples (p, q, -p, -q): every sum and alternating sum is zero exactly (the partial sums of float32 taps are
    exact in double), and short enough that nothing reaches a cut: the compat terms are zeros and the closed form is `render`'s."""
    n_ref, irs = 4096, []
    for seed in (1, 2):
        h = tp.probe_ir(2048, seed)
        h[2::4] = -h[0::4]
        h[3::4] = -h[1::4]
        irs.append(h)
        assert all(v == 0.0 for pair in tp.ir_sums(h) for v in pair)
    for period, predelay in ((256, 0), (256, 301), (1024, 700)):
        pm = period // BLOCK
        imp = tp.impulses_on([(0, 3 * pm, 0), (1, 3 * pm, 255), (1, 5 * pm + pm - 1, 77), (0, 200, 131)], seed=3)
        calls = [pm] * (240 // pm)
        start = tp.start_values(predelay)
        start[1].update(panWet=-0.25, level=0.625, dry=0.25)
        states = tp.controllers([(4 * pm, 0, "level", 0.5)], calls, 2, period, start)
        a = tp.render(irs, imp, states, 240 * BLOCK)
        b = tp.render_compat(irs, imp, states, 240 * BLOCK, n_ref, period)
        assert np.abs(a).max() > 0.1 * U and np.array_equal(a, b)
    irs[0][0] += np.float32(0.01)
    assert not np.array_equal(tp.render(irs, imp, states, 240 * BLOCK), tp.render_compat(irs, imp, states, 240 * BLOCK, n_ref, period))


def test_the_biased_probe_irs_sums_all_differ():
    """Four sums and four alternating sums of a voice: an IR's two channels a fifth of the larger apart (what an exchange has to
    read as), and so the two IRs on one channel (an exchange of halves); the other two pairings differ as well; none is small
    against the unbiased IR's; no tap below 0.1 SIGMA."""
    for n_ref in (4096, 8192):
        for short in (False, True):
            irs = _irs(n_ref, short)
            for pair in ((0, 1), (2, 1)):
                for kind in (0, 1):
                    s = [np.abs(tp.ir_sums(irs[j])[kind]) for j in pair]
                    v = sorted(float(x) for lr in s for x in lr)
                    plain = max(abs(tp.ir_sums(tp.probe_ir(irs[j].shape[0], 500 + n_ref // 1024 + j))[kind][c]) for j in pair for c in (0, 1))
                    assert all(b - a >= 0.005 * v[-1] for a, b in zip(v, v[1:])) and v[0] > 4 * plain, (n_ref, short, pair, kind, v, plain)
                    for a, b in ((s[0][0], s[0][1]), (s[1][0], s[1][1]), (s[0][0], s[1][0]), (s[0][1], s[1][1])):
                        assert abs(a - b) >= 0.2 * max(a, b), (n_ref, short, pair, kind, s)
            assert min(np.abs(h).min() for h in irs) >= 0.1 * tp.SIGMA * 0.999


@pytest.mark.parametrize("name,n_ref", ALL, ids=IDS)
def test_the_closed_form_is_what_both_oracles_compute(oracle_mod, name, n_ref):
    """render_compat against oracle.RefCompat and RefCompatNp: <= 1e-6 U over the whole stream, silence after the last window."""
    case, clean = _run(name, n_ref)
    r, w = _read(case, clean, tag=" C oracle")
    assert np.abs(w).max() < PEAK and np.abs(clean).max() < PEAK
    assert r["worst"] <= ORACLE_BAR, tp.describe(r)
    r2, _ = _read(case, _np_oracle(case), tag=" numpy oracle")
    assert r2["worst"] <= ORACLE_BAR, tp.describe(r2)
    assert np.abs(clean[:, -2 * BLOCK:]).max() <= 1e-12 and np.abs(w[:, -2 * BLOCK:]).max() == 0


@pytest.mark.parametrize("name,n_ref", ALL, ids=IDS)
def test_every_impulse_has_terms_and_cut_taps_worth_reading(name, n_ref):
    """On the oracle alone, impulse by impulse: RefCompatNp less its linear form is q1 + q2 (-1)^m over the window and nothing else
    there; |q1| >= 0.02 U on R, and on L under an impulse on input 2 (under one on input 1 the reference's DC shortcut is the
    true value on L: a structural zero); |q2| >= 0.02 U on both channels; and where the response reaches the cut, the linear
    form holds a tap >= 0.25 U past it and the reference nothing."""
    case = _case(name, n_ref)
    terms = tp.compat_terms(case["irs"], case["imp"], case["states"], n_ref, case["period"])
    cut_any = False
    for k, ((i, n, a), t) in enumerate(zip(case["imp"], terms)):
        ref, lin = _np_oracle(case, only=k), _np_oracle(case, only=k, linear=True)
        d = (ref - lin)[:, t["open"]:t["close"]] / U
        q1 = 0.5 * (d[:, 0::2].mean(axis=1) + d[:, 1::2].mean(axis=1))
        q2 = 0.5 * (d[:, 0::2].mean(axis=1) - d[:, 1::2].mean(axis=1))
        alt = 1.0 - 2.0 * (np.arange(d.shape[1]) % 2)
        assert np.abs(d - q1[:, None] - q2[:, None] * alt).max() <= 1e-9
        assert np.abs((ref - lin)[:, :t["open"]]).max() <= 1e-12
        past = np.abs(lin[:, t["close"]:]).max() / U
        print(f"{name} n_ref {n_ref} impulse {k} (input {i}, in-call offset {n - t['call']}): q1 {q1[0]:+.4f} {q1[1]:+.4f} U, q2 {q2[0]:+.4f} {q2[1]:+.4f} U, past the cut {past:.3f} U")
        assert abs(q1[1]) >= TERM_FLOOR and (abs(q1[0]) >= TERM_FLOOR if i == 1 else abs(q1[0]) <= 1e-9), (k, q1)
        assert np.abs(q2).min() >= TERM_FLOOR, (k, q2)
        assert np.abs(ref[:, t["close"]:]).max() <= 1e-12
        s = case["states"][n // BLOCK]
        ncut = max(n + s["predelay"] + case["irs"][j].shape[0] for j, c in enumerate(s["coef"][i]) if c != 0.0) - t["close"]
        assert case["regime"] or ncut <= 0
        if ncut >= 64:  # (of 64 taps one is large enough under the smallest amplitude and gain of these cases)
            cut_any = True
            assert past >= CUT_FLOOR, (k, past)
        elif ncut <= 0:
            assert past <= 1e-12
    assert cut_any == case["regime"]


# ---------------------------------------------------------------------------------------------------------------------------
def _fault(name, n_ref, plant, what):
    """The clean oracle output against the closed form with a fault planted: the reading, which must clear the floor."""
    case, clean = _run(name, n_ref)
    r0, _ = _read(case, clean)
    r, _ = _read(case, clean, plant, tag=f" [{what}]")
    assert r0["worst"] <= ORACLE_BAR
    assert r["worst"] >= FAULT_FLOOR and r["worst"] > 50 * GPU_BAR, tp.describe(r)
    return case, r


@pytest.mark.parametrize("name", ["p256-pd1024", "p1024-pd1100"])
def test_a_cut_one_frame_late_fails_the_probe(oracle_mod, name):
    case, r = _fault(name, 4096, dict(cut_late=1), "cut one frame late")
    assert r["worst"] >= CUT_FLOOR * 0.99 and any(what == "cut" and d == 0 for _, what, d in r["edges"]), tp.describe(r)


def test_a_cut_measured_from_the_block_fails_the_probe(oracle_mod):
    """1024-frame calls: the impulses in the second and the last block of a call keep up to 768 taps too many."""
    case, r = _fault("p1024-pd1024", 4096, dict(cut_from_block=True), "cut measured from the block")
    assert r["worst"] >= CUT_FLOOR, tp.describe(r)
    late = [j for j, (_, n, _) in enumerate(case["imp"]) if n % 1024 >= BLOCK]
    t = tp.compat_terms(case["irs"], case["imp"], case["states"], 4096, 1024)
    assert any(t[j]["close"] <= r["sample"] < t[j]["close"] + (case["imp"][j][1] % 1024) // BLOCK * BLOCK for j in late), tp.describe(r)


@pytest.mark.parametrize("name", ["p256-pd1100", "p512-pd1024", "short-p256-pd301-ramp"])
def test_a_q1_window_that_opens_one_frame_late_fails_the_probe(oracle_mod, name):
    case, r = _fault(name, 8192 if name.startswith("short") else 4096, dict(q1_open_late=1), "Q1 window opens one frame late")
    assert any(what == "window opens" and d == 0 for _, what, d in r["edges"]), tp.describe(r)


@pytest.mark.parametrize("name", ["p256-pd1024", "short-p1024-pd256"])
def test_a_q1_window_one_block_short_fails_the_probe(oracle_mod, name):
    case, r = _fault(name, 8192 if name.startswith("short") else 4096, dict(q1_short=BLOCK), "Q1 window one block short")
    t = tp.compat_terms(case["irs"], case["imp"], case["states"], case["n_ref"], case["period"])
    assert any(t[k]["close"] - BLOCK <= r["sample"] < t[k]["close"] for k in r["windows"]), tp.describe(r)


@pytest.mark.parametrize("name", ["p256-pd1024", "short-p256-pd0", "switch-p512"])
def test_exchanged_ir_sums_fail_the_probe(oracle_mod, name):
    case, r = _fault(name, 8192 if name.startswith("short") else 4096, dict(swap_sigma=True), "sigma_L and sigma_R exchanged")
    assert r["windows"], tp.describe(r)


@pytest.mark.parametrize("name", ["level-step-p256", "level-step-p1024"])
def test_a_q1_term_at_the_next_blocks_gains_fails_the_probe(oracle_mod, name):
    """Level 0.75 -> 1 at call q: the impulses on the last block before it read a Q1 term a third too large."""
    case, r = _fault(name, 4096, dict(q1_gain_shift=1), "Q1 term at the next block's gains")
    before = [k for k, (_, n, _) in enumerate(case["imp"]) if n // BLOCK == case["q"] * case["pm"] - 1]
    assert before and any(k in r["windows"] for k in before), tp.describe(r)


def test_the_q2_sign_of_the_in_block_offset_is_the_in_call_offset():
    """The fault the list names last - the Q2 sign from the offset inside the block instead of inside the call - cannot be
    planted: a block is 256 frames, an even number, so (-1)^(o + 256 k) = (-1)^o for every block k of a call.  Stated, not planted."""
    assert BLOCK % 2 == 0
    for n in (511, 256, 1023, 768 + 131):
        assert (n % BLOCK) % 2 == (n % 1024) % 2


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ref,taps,pd", [(4096, (2500, 3072), 1024), (4096, (3072, 3072), 2000), (16384, (15360, 9000), 8128)],
                         ids=["default_predelay", "pd2000", "max_predelay"])
def test_what_white_noise_under_one_rms_sees_of_a_late_cut_and_of_weak_cut_terms(oracle_mod, n_ref, taps, pd):
    """The input, IRs and parameters of test_gpu_parity.py::test_q8_tail_drop_is_reproduced, on the oracle alone.  The cut terms
    are Upols(compat) - RefCompat (what that test holds above 5 RMS_TOL).  An engine whose cut terms are 20 % low errs by a
    fifth of them; one that cuts one frame late keeps, per input block, the one sample the reference drops first.

    The expectation this was written to assert - both stay under RMS_TOL, so that test passes either engine - does not hold:
    its floor of 5 RMS_TOL would allow it, but its inputs put the cut terms at 41, 198 and 144 RMS_TOL, so cut terms 20 % low
    read 8 to 40 RMS_TOL, and a cut one frame late 2.7 to 7.6 RMS_TOL (one sample per block of 2e-3 to 5e-3).  What does pass:
    cut terms up to 2.4 %, 0.5 % and 0.7 % low, and a late cut on one block in 12, 58 and 8.  Asserted as measured: white noise
    sees both faults, by a margin below 50, where the impulse probe's is >= 0.25 U / 1e-4 U = 2500 for the late cut."""
    from cuda_audio_amd.synth import make_input
    from helpers import BASE, RMS_TOL, apply_params, rms

    nb = 3 * n_ref // 256 // 2 + 40
    x = make_input(nb * 256)
    rng = np.random.default_rng(5)
    irs = []
    for L in taps:
        h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
        irs.append((h * np.sqrt(0.004 / L)).astype(np.float32))
    p0, p1 = dict(BASE, predelay=pd), dict(BASE, select=1, level=0.9)
    ref, lin = oracle_mod.RefCompat(n_ref, True), oracle_mod.Upols(n_ref, True)
    for o in (ref, lin):
        for i, ir in enumerate(irs):
            o.prepare(i, ir)
        apply_params(o, p0, p1, True)
    want = ref.process(x[0], x[1])
    terms = lin.process(x[0], x[1]) - want
    assert rms(terms) > 5 * RMS_TOL
    weak = 0.2 * rms(terms)
    # one frame late: input block b's response at frame 256 b + n_ref, its first dropped one (tap n_ref - pd - o under offset o)
    late = np.zeros_like(want)
    for b in range(nb):
        n = b * 256 + n_ref
        if n >= want.shape[1]:
            break
        for i, p in ((0, p0), (1, p1)):
            h = irs[i].astype(np.float64)
            t = n_ref - pd - np.arange(256)
            ok = t < h.shape[0]
            g = tp.coefficient(b, float(np.float32(p["wet"]))) * float(np.float32(p["level"]))
            late[:, n] += g * (x[i, b * 256:(b + 1) * 256].astype(np.float64)[ok, None] * h[t[ok]]).sum(axis=0)
    print(f"n_ref {n_ref} predelay {pd}: signal rms {rms(want):.3e}, cut terms rms {rms(terms):.3e} ({rms(terms) / RMS_TOL:.1f} RMS_TOL), 20 % low: {weak:.3e}, "
          f"one frame late: rms {rms(late):.3e}, largest sample {np.abs(late).max():.3e}")
    print(f"  passes under RMS_TOL: cut terms {100 * RMS_TOL / rms(terms):.1f} % low; a late cut on one block in {(rms(late) / RMS_TOL) ** 2:.0f}")
    assert np.abs(late).max() > 100 * RMS_TOL  # (each such sample is a plain error, far above the bar a sample of the probe is held to)
    assert RMS_TOL < rms(late) < 50 * RMS_TOL
    assert RMS_TOL < weak < 50 * RMS_TOL
