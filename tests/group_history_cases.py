"""Small batch sequences in which the Q1/Q2 history of a multi-device group matters (no GPU here).

The group driver (include/mcconv_group.h) finishes a batch of `n` blocks on every rank when n % (ranks * period / 256) == 0
and on rank 0 alone otherwise (a "ragged" batch).  The ranks that do not finish a ragged batch must still carry its Q1/Q2
prefix sums: the compat term of an output frame is a difference of two entries of that history, one reference length
(n_ref frames) plus the predelay apart, so for WINDOW + ceil(predelay / 256) blocks after a ragged batch every block a rank
>= 1 finishes reads entries of the batch it did not finish.  Those are the "window blocks" of a case.

One geometry for all cases: n_ref = 16384 (a window of 64 blocks, 60 partitions; the smallest size at which four ranks
each own a run of 16 partitions), IRs that fill it, and an input with a DC and an alternating component so that the
Q1/Q2 terms (sums of h, of h (-1)^m, of x and of x (-1)^m) are far above the parity tolerance - which
test_group_history_cases_cpu.py proves per window block with the oracle.
"""
from collections import namedtuple

import numpy as np

N_REF = 16384
WINDOW = N_REF // 256
MAX_BATCH = 128
IR_TAPS = (15000, 12000)
IR_SEEDS = (5678, 5680)

# sizes: batch lengths in blocks; changes: {index of the batch before which half 0's predelay becomes the value}
Case = namedtuple("Case", "name sizes ranks period predelay changes")

CASES = {c.name: c for c in (
    Case("ragged_then_even", (64, 37, 64, 64), (2, 4), 256, 300, {}),  # the window lies wholly in the runs of ranks >= 1
    Case("ragged_first", (37, 64), (4,), 256, 0, {}),  # the base of the first even batch is an entry the rank never finished
    Case("single_blocks", (64, 1, 1, 1, 64), (4,), 256, 300, {}),  # batches shorter than the rank count
    Case("two_ragged", (33, 35, 128), (4,), 256, 0, {}),  # the second window straddles two ragged batches
    Case("period_512", (64, 38, 64), (4,), 512, 300, {}),  # ragged: not a multiple of ranks * 2
    Case("tail_drop", (64, 37, 64), (4,), 256, 2000, {}),  # Q8 regime: predelay + taps exceeds n_ref
    Case("predelay_change", (64, 37, 64, 64), (4,), 256, 300, {2: 700}),  # the epoch retired after a ragged batch
)}

CASE_RANKS = [(name, r) for name, c in CASES.items() for r in c.ranks]


def params(case, predelay=None):
    from helpers import BASE

    pd = case.predelay if predelay is None else predelay
    return dict(BASE, predelay=pd, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)


def impulse_responses():
    from cuda_audio_amd.synth import make_ir

    return [make_ir(t, seed=s, norm=0.02) for t, s in zip(IR_TAPS, IR_SEEDS)]


def make_case_input(case):
    from cuda_audio_amd.synth import make_input

    x = make_input(sum(case.sizes) * 256)
    x[0] += 0.05  # DC and an alternating component: the Q1/Q2 sums matter
    x[1, ::2] += 0.04
    return x


def is_ragged(case, n, ranks):
    return n % (ranks * (case.period // 256)) != 0


def batches(case):
    """[(first block, blocks, index)] of the case's batches."""
    out, o = [], 0
    for i, n in enumerate(case.sizes):
        out.append((o, n, i))
        o += n
    return out


def window_blocks(case, ranks=None):
    """The blocks within WINDOW + ceil(largest predelay / 256) blocks after the end of each ragged batch (inside the run)."""
    ranks = max(case.ranks) if ranks is None else ranks
    nb = sum(case.sizes)
    pd = max([case.predelay] + list(case.changes.values()))
    reach = WINDOW + -(-pd // 256)
    blocks = set()
    for o, n, _ in batches(case):
        if is_ragged(case, n, ranks):
            blocks.update(range(o + n, min(o + n + reach, nb)))
    return sorted(blocks)


def finisher(case, ranks, block):
    """(batch index, rank that finishes the block in a group of `ranks`)."""
    for o, n, i in batches(case):
        if o <= block < o + n:
            return i, (0 if is_ragged(case, n, ranks) else (block - o) // (n // ranks))
    raise IndexError(block)


def block_rms(d):
    """RMS per 256-frame block over both channels of d [2, blocks * 256]: [blocks]."""
    d = np.asarray(d, dtype=np.float64)
    return np.sqrt(np.mean(d.reshape(2, -1, 256) ** 2, axis=(0, 2)))


def _upols(oracle_mod, case, compat, predelay=None):
    x = make_case_input(case)
    u = oracle_mod.Upols(N_REF, compat)
    for i, ir in enumerate(impulse_responses()):
        u.prepare(i, ir)
    p0, p1 = params(case, predelay)
    u.set(0, **p0)
    u.set(1, **p1)
    out = u.process(x[0], x[1])
    u.close()
    return out


def _refcompat(oracle_mod, case):
    """The single-transform restatement, one call per period, the predelay changed at the same blocks as in the case (the
    partitioned oracle models a constant predelay only)."""
    x = make_case_input(case)
    r = oracle_mod.RefCompat(N_REF, True)
    for i, ir in enumerate(impulse_responses()):
        r.prepare(i, ir)
    p0, p1 = params(case)
    r.set(0, **p0)
    r.set(1, **p1)
    out = np.zeros((2, x.shape[1]))
    for o, n, i in batches(case):
        if i in case.changes:
            r.set(0, predelay=case.changes[i])
        s = slice(o * 256, (o + n) * 256)
        out[:, s] = r.process(x[0, s], x[1, s], block=case.period)
    r.close()
    return out


_built = {}


def build(oracle_mod, name):
    """(input [2, n] float32, oracle output with compat on [2, n] float64, window blocks) of a case; computed once, read-only."""
    if name not in _built:
        case = CASES[name]
        x = make_case_input(case)
        # the partitioned oracle's state machine models one period of 256 frames, one predelay, and no Q8 tail drop
        q8 = max(IR_TAPS) + case.period - 1 + case.predelay > N_REF
        want = _refcompat(oracle_mod, case) if (case.period != 256 or case.changes or q8) else _upols(oracle_mod, case, True)
        x.setflags(write=False)
        want.setflags(write=False)
        _built[name] = (x, want, tuple(window_blocks(case)))
    return _built[name]


def compat_share(oracle_mod, name, predelay=None):
    """Per block, the RMS of what the Q1/Q2 (and Q8) terms contribute: Upols(compat on) - Upols(compat off), period-256 cases."""
    case = CASES[name]
    assert case.period == 256
    return block_rms(_upols(oracle_mod, case, True, predelay) - _upols(oracle_mod, case, False, predelay))
