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

in units of U = SIGMA AMP.  tests/test_tap_probe_moving_cpu.py proves it on the two oracles."""
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


def compare(got, wanted, irs, impulses, predelay=0, wet=1.0, states=None):
    """The largest |got - wanted| over the whole stream in units of U, and what it belongs to: the channel and the sample, and of
    the impulses whose response covers the sample the one whose tap there is nearest to the response's end (the
    late partitions are where the forms have their edges) - its number, the tap, and the tap as partition and offset; `covering` lists
    (impulse, tap) for all of them.  impulse None: the sample lies outside every response and ought to be silent.
    With `states` (`controllers`) an impulse sounds through every IR whose coefficient at its block is not zero, each at that
    block's predelay: `voice` is the IR index of the tap named, `voices` the IR index of every entry of `covering`, and `dry`
    the impulse whose own frame the sample is, if it had a dry gain.  Without, the voice is the impulse's input."""
    err = np.abs(np.asarray(got, np.float64) - wanted)
    ch, n = np.unravel_index(int(np.argmax(err)), err.shape)
    r = dict(worst=float(err[ch, n]) / (SIGMA * AMP * wet), channel=int(ch), sample=int(n), block=int(n) // BLOCK, impulse=None, tap=None, partition=None,
             offset=None, covering=[], voice=None, voices=[], dry=None)
    left = None
    for k, (i, nk, a) in enumerate(impulses):
        s = states[nk // BLOCK] if states is not None else None
        if s is not None and int(n) == nk and any(s["D"][c][i] != 0.0 for c in (0, 1)):
            r["dry"] = k
        for j in ([i] if s is None else [j for j, c in enumerate(s["coef"][i]) if c != 0.0]):
            t = int(n) - nk - (predelay if s is None else s["predelay"])
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
    return f"worst {r['worst']:.2e} U at channel {r['channel']} sample {r['sample']} (block {r['block']}): {where}"
