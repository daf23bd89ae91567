"""Impulse trains that read a partitioned convolution tap by tap (numpy only).

In linear mode (compat=False) with dry 0, wet `wet`, level 1, panWet 0, vsteps 0, half 0 on IR 0 and half 1 on IR 1, the
output for a sparse input is known in closed form:

    out[:, n] = sum_k a_k c(b_k) h_{i_k}[n - n_k - predelay]

for impulses of amplitude a_k on input i_k at frame n_k = 256 b_k + o_k, with c(b) = wet (1 - 0.8^(b + 1)) the cold-start
coefficient of input block b counted from reset().  Every output sample is one tap or a sum of a few, so a
fault at one partition is not diluted by the rest of the IR, and an IR that does not decay weighs its last partition as
its first.  The unit of error is U = SIGMA AMP wet."""
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


def coefficient(block, wet=1.0):
    """The cold-start coefficient of input block `block`, in double."""
    return float(wet) * (1.0 - 0.8 ** (int(block) + 1))


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


def compare(got, wanted, irs, impulses, predelay=0, wet=1.0):
    """The largest |got - wanted| over the whole stream in units of U, and what it belongs to: the channel and the sample, and of
    the impulses whose response covers the sample the one whose tap there is nearest to the response's end (the
    late partitions are where the forms have their edges) - its number, the tap, and the tap as partition and offset; `covering` lists
    (impulse, tap) for all of them.  impulse None: the sample lies outside every response and ought to be silent."""
    err = np.abs(np.asarray(got, np.float64) - wanted)
    ch, n = np.unravel_index(int(np.argmax(err)), err.shape)
    r = dict(worst=float(err[ch, n]) / (SIGMA * AMP * wet), channel=int(ch), sample=int(n), block=int(n) // BLOCK, impulse=None, tap=None, partition=None,
             offset=None, covering=[])
    for k, (i, nk, a) in enumerate(impulses):
        t = int(n) - nk - predelay
        if 0 <= t < irs[i].shape[0]:
            r["covering"].append((k, t))
            if r["tap"] is None or t > r["tap"]:
                r.update(impulse=k, tap=t, partition=t // BLOCK, offset=t % BLOCK)
    return r


def describe(r):
    where = "outside every response" if r["impulse"] is None else f"impulse {r['impulse']}, tap {r['tap']} = partition {r['partition']} offset {r['offset']}"
    return f"worst {r['worst']:.2e} U at channel {r['channel']} sample {r['sample']} (block {r['block']}): {where}"
