"""Impulse trains that read a partitioned convolution tap by tap (numpy only).

In linear mode (compat=False) with dry 0, wet `wet`, level 1, panWet 0, vsteps 0, half 0 on IR 0 and half 1 on IR 1, the
output for a sparse input is known in closed form:

    out[:, n] = sum_k a_k c(b_k) h_{i_k}[n - n_k - predelay]

for impulses of amplitude a_k on input i_k at frame n_k = 256 b_k + o_k, with c(b) = wet (1 - 0.8^(b + 1)) the cold-start
coefficient of input block b counted from reset().  Every output sample is one tap or a sum of a few, so a
fault at one partition is not diluted by the rest of the IR, and an IR that does not decay weighs its last partition as
its first.  The unit of error is U = SIGMA AMP wet.

The same under a controller schedule: `controllers` gives what the engine attaches to every input block when
select, vsteps, wet, level, panWet, panDry, dry and predelay change at call starts - the cross-fade coefficient of every IR
per half, the four path gains, the four dry gains, the predelay - and `render` the closed form under them,

    out_c[n]   += a_k G_c,i_k(b_k) sum_j c_i_k[j](b_k) h_j[n - n_k - predelay(b_k), c]
    out_c[n_k] += a_k D_c,i_k(b_k)

in units of U = SIGMA AMP.  tests/test_tap_probe_moving_cpu.py proves it on the two oracles.

In compat mode `render_compat` adds what the reference's shortcuts add: the Q1 and Q2 constants over every
impulse's window and the Q8 cut at call start + n_ref, with IRs that carry a bias (`probe_ir_biased`) so that those terms are
large; tests/test_tap_probe_compat_cpu.py proves it on the two oracles in their default form."""
import numpy as np

BLOCK = 256
SIGMA = 0.05    # every tap of a probe IR lies in +-[0.5, 1] SIGMA
AMP = 0.9       # every impulse in +-[0.5, 1] AMP
WARM = 170      # blocks after which the cold-start coefficient is wet exactly: 0.8^170 = 3.4e-17 is below a double's resolution
OFFSETS = (0, 255, 77, 131)  # in-block offsets: both ends and two in between


def probe_ir(taps, seed):
    """sign * uniform(0.5, 1) * SIGMA, float32 [taps, 2]: no tap is near zero, so no fault can hide on one; the channels
    differ, and so do IRs of different seeds."""
    rng = np.random.default_rng(seed)
    sign = rng.integers(0, 2, (taps, 2)) * 2.0 - 1.0
    return (sign * rng.uniform(0.5, 1.0, (taps, 2)) * SIGMA).astype(np.float32)


def _advance(c, target, div):
    """One step of the cross-fade recurrence, in double, with the engine's rule for arriving: a coefficient
    closer to its target than a double's resolution, or below 1e-14 on its way to zero, is at its target."""
    c += (target - c) / div
    if abs(target - c) <= 1e-300 + 4e-16 * abs(target) or (target == 0.0 and abs(c) < 1e-14):
        c = target
    return c


def coefficient(block, wet=1.0):
    """The cold-start coefficient of input block `block`, in double: wet (1 - 0.8^(block + 1)), by the recurrence that
    `controllers` runs (the two agree to a double's rounding; sharing the steps makes a constant schedule bit-exact)."""
    c, wet = 0.0, float(wet)
    for _ in range(int(block) + 1):
        if c == wet:
            break
        c = _advance(c, wet, 5.0)
    return c


def place_impulses(bounds, seed, batch=None, first=0, extra=(), limit=8):
    """5 to 8 impulses (input, frame, amplitude) around batch `batch` (default: the last one) of a stream whose calls start at
    the blocks `bounds` (ascending, the last entry the end of the last call): on the first and the last block of the batch, on
    a block of the batch before, on one even and one odd block, at in-block offsets 0, 255 and in between, on both inputs.
    No impulse lies before block `first` (the end of a warm-up); `extra` names further blocks (an impulse inside the ramp, a
    chunk's edge, a residue class).  Blocks that coincide are kept once, so a batch gives fewer than 5 only when it has fewer
    blocks; more than `limit` are cut (8 keeps the sum of the responses below 8 SIGMA AMP = 0.36, well inside the output's clamp;
    a caller that raises it answers for the peak)."""
    bounds = [int(b) for b in bounds]
    if len(bounds) < 2 or any(b1 <= b0 for b0, b1 in zip(bounds, bounds[1:])):
        raise ValueError("bounds must ascend and hold at least one batch")
    j = len(bounds) - 2 if batch is None else int(batch)
    b0, b1 = bounds[j], bounds[j + 1]
    if b0 < first:
        raise ValueError("the batch starts inside the warm-up")
    blocks = [b0, b1 - 1]
    if j > 0 and bounds[j - 1] >= first:
        blocks.append((bounds[j - 1] + b0) // 2)  # a block of the batch before: its response crosses the seam
    inner = [b for b in range(b0 + 1, b1 - 1)]
    even = [b for b in inner if b % 2 == 0]
    odd = [b for b in inner if b % 2 == 1]
    if even:
        blocks.append(even[len(even) // 2])
    if odd:
        blocks.append(odd[len(odd) // 3])
    blocks += [int(b) for b in extra]
    seen, uniq = set(), []
    for b in blocks:
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    uniq = uniq[:limit]
    rng = np.random.default_rng(seed)
    out = []
    for k, b in enumerate(uniq):
        a = np.float32((1.0 if rng.integers(0, 2) else -1.0) * rng.uniform(0.5, 1.0) * AMP)
        out.append((k % 2, b * BLOCK + OFFSETS[k % len(OFFSETS)], float(a)))
    return out


def impulses_on(places, seed):
    """Impulses at stated places, (input, block, in-block offset) each, with amplitudes drawn as `place_impulses` draws them."""
    rng = np.random.default_rng(seed)
    return [(int(i), int(b) * BLOCK + int(o), float(np.float32((1.0 if rng.integers(0, 2) else -1.0) * rng.uniform(0.5, 1.0) * AMP))) for i, b, o in places]


def stream(impulses, nframes):
    """The two inputs, float32 [2, nframes]."""
    x = np.zeros((2, nframes), np.float32)
    for i, n, a in impulses:
        if x[i, n] != 0:
            raise ValueError("two impulses on one frame")
        x[i, n] = a
    return x


def response_end(irs, impulses, predelay):
    """The first frame after the last tap of every response."""
    return max(n + predelay + irs[i].shape[0] for i, n, a in impulses)


def want(irs, impulses, nframes, predelay=0, wet=1.0):
    """The closed form above: float64 [2, nframes]."""
    out = np.zeros((2, nframes))
    for i, n, a in impulses:
        h = np.asarray(irs[i], np.float64)
        s = n + predelay
        m = min(h.shape[0], nframes - s)
        if m > 0:
            out[:, s:s + m] += float(np.float32(a)) * coefficient(n // BLOCK, wet) * h[:m].T
    return out


FIELDS = ("select", "vsteps", "wet", "level", "panWet", "panDry", "dry", "predelay")
_WHOLE = ("select", "vsteps", "predelay")


def pan_l(p):
    return 1.0 - p if p >= 0 else 1.0


def pan_r(p):
    return 1.0 + p if p <= 0 else 1.0


def start_values(predelay=0, wet=1.0):
    """The probe's simplest state: half h on IR h, wet `wet`, level 1, no pan, no dry signal."""
    return [dict(select=h, vsteps=0, wet=wet, level=1.0, panWet=0.0, panDry=0.0, dry=0.0, predelay=predelay) for h in (0, 1)]


def _value(field, value):
    return int(value) if field in _WHOLE else float(np.float32(value))  # (the engine's controller values are float32)


def controllers(schedule, calls, nirs, period=BLOCK, start=None):
    """What the engine attaches to every input block of a stream cut into `calls` (blocks per call) under a controller schedule:
    a list of events (block, half, field, value), field one of FIELDS, on top of `start` (start_values() unless given).  The
    engine samples its controllers once per call, so an event inside a call raises; the cross-fade recurrence advances per
    block (per period, for periods of 512 and 1024 frames) inside a call:

        div = vsteps_i + 5;  c_i[j] += ([j == select_i] wet_i - c_i[j]) / div for every IR j;  vsteps_i = max(vsteps_i - 1, 0)

    Per block a dict: coef[i][j] = c_i[j]; G[c][i] = pan_c(panWet_i) level_i; D[c][i] = dry_i pan_c(panDry_i) level_i; predelay
    (read from half 0, as the engine does).  All in double, from float32 controller values."""
    pm = period // BLOCK
    starts, pos = set(), 0
    for n in calls:
        if n <= 0 or n % pm:
            raise ValueError("a call is a positive number of whole periods")
        starts.add(pos)
        pos += n
    by_block = {}
    for b, half, field, value in schedule:
        if field not in FIELDS or half not in (0, 1):
            raise ValueError(f"no controller {field!r} on half {half!r}")
        if b not in starts:
            raise ValueError(f"the event at block {b} lies inside a call: controllers are sampled at call starts only")
        by_block.setdefault(int(b), []).append((half, field, value))
    cc = [{k: _value(k, v) for k, v in half.items()} for half in (start or start_values())]
    coef = np.zeros((2, nirs))
    states = []
    for b in range(pos):
        for half, field, value in by_block.get(b, ()):
            cc[half][field] = _value(field, value)
        if b % pm == 0:
            for i in (0, 1):
                if not 0 <= cc[i]["select"] < nirs:
                    raise ValueError(f"half {i} selects IR {cc[i]['select']} of {nirs}")
                div = cc[i]["vsteps"] + 5.0
                for j in range(nirs):
                    coef[i, j] = _advance(coef[i, j], cc[i]["wet"] if j == cc[i]["select"] else 0.0, div)
                cc[i]["vsteps"] = max(cc[i]["vsteps"] - 1, 0)
        states.append(dict(coef=coef.copy(), predelay=cc[0]["predelay"],
                           G=[[pan(cc[i]["panWet"]) * cc[i]["level"] for i in (0, 1)] for pan in (pan_l, pan_r)],
                           D=[[cc[i]["dry"] * pan(cc[i]["panDry"]) * cc[i]["level"] for i in (0, 1)] for pan in (pan_l, pan_r)]))
    return states


def render(irs, impulses, states, nframes):
    """The closed form under per-block states (`controllers`), float64 [2, nframes]:

        out_c[n]   += a_k G_c,i_k(b_k) sum_j c_i_k[j](b_k) h_j[n - n_k - predelay(b_k), c]
        out_c[n_k] += a_k D_c,i_k(b_k)

    A state may carry `irs`, which then stand in for `irs` for the impulses on its block (planted faults)."""
    out = np.zeros((2, nframes))
    for i, n, a in impulses:
        s = states[n // BLOCK]
        a = float(np.float32(a))
        for j, c in enumerate(s["coef"][i]):
            if c == 0.0:
                continue
            h = np.asarray(s.get("irs", irs)[j], np.float64)
            o = n + s["predelay"]
            m = min(h.shape[0], nframes - o)
            for ch in (0, 1):
                if m > 0:
                    out[ch, o:o + m] += a * (s["G"][ch][i] * c) * h[:m, ch]
        for ch in (0, 1):
            out[ch, n] += a * s["D"][ch][i]
    return out


def want_scheduled(irs, impulses, nframes, schedule, calls, period=BLOCK, start=None):
    """`want` under a controller schedule; with no events and start_values(predelay, wet) it is `want`, bit for bit."""
    return render(irs, impulses, controllers(schedule, calls, len(irs), period, start), nframes)


def reach_end(irs, impulses, states):
    """The first frame after the last tap of every response under `states`."""
    return max(n + states[n // BLOCK]["predelay"] + irs[j].shape[0] for i, n, a in impulses for j, c in enumerate(states[n // BLOCK]["coef"][i]) if c != 0.0)


def probe_ir_biased(taps, seed, bias):
    """probe_ir's taps plus, per channel and per IR (by the seed's parity), a constant and an alternating constant:

        h[t, c] += SIGMA bias (u + v (-1)^t),  u in [0.55, 1], v in +-[0.55, 1], |u| + |v| <= 1.6, the eight values of two IRs all different

    The constant lifts the IR's sum (the Q1 term of compat mode), the alternating one its alternating sum (the Q2 term), which a
    constant leaves where it was; both are `taps` SIGMA bias u against the sqrt(taps) SIGMA of the unbiased taps.  An IR's two
    channels differ by a third of the larger in u and in |v|, so an exchanged sigma or alpha reads as an error, and the four of a
    voice (two IRs of seeds of different parity) are all different.  With bias <= 0.25 every tap stays >= 0.1 SIGMA in magnitude
    and <= 1.4 SIGMA."""
    u = ((1.0, 0.65), (0.55, 0.85))[seed % 2]
    v = ((-0.55, 0.95), (1.0, -0.6))[seed % 2]
    alt = 1.0 - 2.0 * (np.arange(taps) % 2)
    h = probe_ir(taps, seed).astype(np.float64)
    for c in (0, 1):
        h[:, c] += SIGMA * bias * (u[c] + v[c] * alt)
    return h.astype(np.float32)


COMPAT_KEEP = 1024  # compat mode stores the first n_ref - 1024 taps of an IR (the reference's prepare at its period of 1024 frames)


def ir_sums(h):
    """(sigma, alpha), float64 [2] each: the sums and the alternating sums sum_t h[t] (-1)^t of an IR's channels."""
    h = np.asarray(h, np.float64)
    alt = 1.0 - 2.0 * (np.arange(h.shape[0]) % 2)
    return h.sum(axis=0), (h * alt[:, None]).sum(axis=0)


def compat_terms(irs, impulses, states, n_ref, period=BLOCK, plant=None):
    """What compat mode adds to an impulse's response, per impulse a dict: `call` the first frame of the reference call that holds
    it, `open` = call + predelay and `close` = call + n_ref the Q1/Q2 window [open, close) (close is also the Q8 cut), and
    q1[c], q2[c]: the output gains q1[c] + q2[c] (-1)^(n - open) on every frame n of the window.  The derivation is
    render_compat's; `plant` its planted faults."""
    plant = plant or {}
    sums = [ir_sums(np.asarray(h)[:n_ref - COMPAT_KEEP]) for h in irs]
    if plant.get("swap_sigma"):
        sums = [(s[::-1], a) for s, a in sums]
    out = []
    for i, n, a in impulses:
        b = n // BLOCK
        s = states[b]
        g = states[b + plant["q1_gain_shift"]]["G"] if plant.get("q1_gain_shift") else s["G"]
        a = float(np.float32(a))
        cs = (n // period) * period
        # A[c][h] = sum_j c_h[j] sigma_j[c], B likewise of the alternating sums: the DC and the Nyquist bin of half h's spectrum
        A = [[sum(s["coef"][h][j] * sums[j][0][c] for j in range(len(irs))) for h in (0, 1)] for c in (0, 1)]
        B = [[sum(s["coef"][h][j] * sums[j][1][c] for j in range(len(irs))) for h in (0, 1)] for c in (0, 1)]
        q1 = [0.0 if i == 0 else -a * (A[1][0] * g[0][0] + A[0][1] * g[0][1]) / n_ref, -a * A[1][i] * g[1][i] / n_ref]
        sign = -1.0 if (n - cs) % 2 else 1.0
        q2 = [-a * sign * B[c][i] * s["G"][c][i] / n_ref for c in (0, 1)]
        out.append(dict(call=cs, open=cs + s["predelay"], close=cs + n_ref, q1=q1, q2=q2))
    return out


def render_compat(irs, impulses, states, nframes, n_ref, period=BLOCK, plant=None):
    """`render` in compat mode: what the reference computes (oracle/refcompat_np.py is its record), float64 [2, nframes].

    The reference transforms a whole call of `period` frames at once, at n_ref points.  z = x1 + j x2 is the call's input,
    zero-padded; h_j = h_j[:, 0] + j h_j[:, 1] the first n_ref - 1024 taps of IR j.  Its `unpack` splits the transform Z into the
    two real signals' spectra at the bins 1 .. n_ref/2 - 1 and their mirrors as the true split does, but

        bin 0:        X1 = Z[0] = S1 + j S2,  X2 = 0      (true: X1 = S1, X2 = S2;  S_i the sum of input i over the call)
        bin n_ref/2:  never written: X1 = X2 = 0          (true: X_i = A_i = sum_o x_i[o] (-1)^o, o counted from the call's start)

    and the IRs' spectra likewise: H_j,L[0] = sigma_j,L + j sigma_j,R, H_j,R[0] = 0, both zero at n_ref/2 (true: sigma_j,c and
    alpha_j,c = sum_t h_j[t, c] (-1)^t).  The cross-fade interpolates whole spectra per half, so half h carries
    sum_j c_h[j] H_j, and channel c is Y_c = (X1 H_0,c G_c,0 + X2 H_1,c G_c,1) / n_ref, H_h,c half h's spectrum.  The
    unnormalised inverse w_c[m] = sum_k Y_c[k] e^(2 pi j k m / n_ref) gets bin 0 as a constant and bin n_ref/2 as Y (-1)^m on all
    n_ref frames; the real part of seg[predelay:] += w[:n_ref - predelay] is the output.  For an impulse a on input i at offset
    o inside its call, with Sg_c,h = sum_j c_h[j] sigma_j,c and Al_c,h likewise of alpha, all at the impulse's block:

    Q8: of w only m < n_ref - predelay is kept: the response's frames >= call start + n_ref are dropped.

    Q1, on the frames predelay <= n - call start < n_ref, reference minus truth at bin 0:
        L: Re[(S1 + j S2)(Sg_L,0 + j Sg_R,0)] G_L,0 / n_ref - (S1 Sg_L,0 G_L,0 + S2 Sg_L,1 G_L,1) / n_ref
             = -S2 (Sg_R,0 G_L,0 + Sg_L,1 G_L,1) / n_ref:   0 for an impulse on input 0, -a (Sg_R,0 G_L,0 + Sg_L,1 G_L,1) / n_ref on 1
        R: 0 - (S1 Sg_R,0 G_R,0 + S2 Sg_R,1 G_R,1) / n_ref:  -a Sg_R,i G_R,i / n_ref
      (half 0's sums and gains under an impulse on input 1: the index pattern is the reference's, not a misprint here.)

    Q2, on the same frames, the true bin n_ref/2 missing:  -a (-1)^o Al_c,i G_c,i / n_ref (-1)^(n - call start - predelay).

    Where every sigma and alpha is zero and nothing reaches a cut the terms are zeros added to `render`'s sums: bit for bit
    `render` (tests/test_tap_probe_compat_cpu.py).  plant: faults for the tests that prove the probe - cut_late (frames),
    cut_from_block, q1_open_late (frames), q1_short (frames off the window's far end), swap_sigma, q1_gain_shift (blocks)."""
    plant = plant or {}
    keep = n_ref - COMPAT_KEEP
    out = np.zeros((2, nframes))
    for i, n, a in impulses:
        s = states[n // BLOCK]
        a = float(np.float32(a))
        cs = (n // BLOCK) * BLOCK if plant.get("cut_from_block") else (n // period) * period
        end = min(nframes, cs + n_ref + plant.get("cut_late", 0))
        for j, c in enumerate(s["coef"][i]):
            if c == 0.0:
                continue
            h = np.asarray(s.get("irs", irs)[j], np.float64)[:keep]
            o = n + s["predelay"]
            m = min(h.shape[0], end - o)
            for ch in (0, 1):
                if m > 0:
                    out[ch, o:o + m] += a * (s["G"][ch][i] * c) * h[:m, ch]
        for ch in (0, 1):
            out[ch, n] += a * s["D"][ch][i]
    for t in compat_terms(irs, impulses, states, n_ref, period, plant):
        lo, hi = t["open"], min(nframes, t["close"])
        if hi <= lo:
            continue
        alt = 1.0 - 2.0 * (np.arange(hi - lo) % 2)
        lo1, hi1 = lo + plant.get("q1_open_late", 0), min(hi, t["close"] - plant.get("q1_short", 0))
        for ch in (0, 1):
            out[ch, lo1:hi1] += t["q1"][ch]
            out[ch, lo:hi] += t["q2"][ch] * alt
    return out


def compat_end(irs, impulses, states, n_ref, period=BLOCK):
    """The first frame after every Q1/Q2 window, which is its impulse's cut: no response reaches further."""
    return max((n // period) * period + n_ref for _, n, _ in impulses)


def compare(got, wanted, irs, impulses, predelay=0, wet=1.0, states=None, compat=None):
    """The largest |got - wanted| over the whole stream in units of U, and what it belongs to: the channel and the sample, and of
    the impulses whose response covers the sample the one whose tap there is nearest to the response's end (the
    late partitions are where the forms have their edges) - its number, the tap, and the tap as partition and offset; `covering` lists
    (impulse, tap) for all of them.  impulse None: the sample lies outside every response and ought to be silent.
    With `states` (`controllers`) an impulse sounds through every IR whose coefficient at its block is not zero, each at that
    block's predelay: `voice` is the IR index of the tap named, `voices` the IR index of every entry of `covering`, and `dry`
    the impulse whose own frame the sample is, if it had a dry gain.  Without, the voice is the impulse's input.
    With `compat` (dict(n_ref, period); needs `states`) the taps past the Q8 cut cover nothing; `windows` lists the impulses whose
    Q1/Q2 window covers the sample, and `edges` (impulse, "window opens" | "cut", distance in frames) every window's first frame
    and every cut (the window's far end) within 2 frames of it."""
    err = np.abs(np.asarray(got, np.float64) - wanted)
    ch, n = np.unravel_index(int(np.argmax(err)), err.shape)
    r = dict(worst=float(err[ch, n]) / (SIGMA * AMP * wet), channel=int(ch), sample=int(n), block=int(n) // BLOCK, impulse=None, tap=None, partition=None,
             offset=None, covering=[], voice=None, voices=[], dry=None, windows=[], edges=[])
    left = None
    if compat is not None:
        for k, t in enumerate(compat_terms(irs, impulses, states, compat["n_ref"], compat.get("period", BLOCK))):
            if t["open"] <= int(n) < t["close"]:
                r["windows"].append(k)
            r["edges"] += [(k, what, int(n) - at) for what, at in (("window opens", t["open"]), ("cut", t["close"])) if abs(int(n) - at) <= 2]
    for k, (i, nk, a) in enumerate(impulses):
        s = states[nk // BLOCK] if states is not None else None
        if s is not None and int(n) == nk and any(s["D"][c][i] != 0.0 for c in (0, 1)):
            r["dry"] = k
        for j in ([i] if s is None else [j for j, c in enumerate(s["coef"][i]) if c != 0.0]):
            t = int(n) - nk - (predelay if s is None else s["predelay"])
            if compat is not None and (t >= compat["n_ref"] - COMPAT_KEEP or int(n) >= (nk // compat.get("period", BLOCK)) * compat.get("period", BLOCK) + compat["n_ref"]):
                continue
            if 0 <= t < irs[j].shape[0]:
                r["covering"].append((k, t))
                r["voices"].append(j)
                to_end = -t if s is None else irs[j].shape[0] - t
                if left is None or to_end < left:
                    left = to_end
                    r.update(impulse=k, tap=t, partition=t // BLOCK, offset=t % BLOCK, voice=j)
    return r


def describe(r):
    where = "outside every response" if r["impulse"] is None else f"impulse {r['impulse']}, IR {r['voice']}, tap {r['tap']} = partition {r['partition']} offset {r['offset']}"
    if r["dry"] is not None:
        where += f"; the dry frame of impulse {r['dry']}"
    if r.get("windows"):
        where += f"; inside the Q1/Q2 window of impulse{'s' if len(r['windows']) > 1 else ''} {', '.join(str(k) for k in r['windows'])}"
    for k, what, d in r.get("edges", ()):
        where += f"; {abs(d)} frame{'' if abs(d) == 1 else 's'} {'before' if d < 0 else 'past'} where impulse {k}'s {what}" if d else f"; where impulse {k}'s {what}"
    return f"worst {r['worst']:.2e} U at channel {r['channel']} sample {r['sample']} (block {r['block']}): {where}"
