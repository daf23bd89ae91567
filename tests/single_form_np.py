"""The running accumulator of the single-transform form (csrc/singlefft.hip.h) read whole and set against the reference's.

A call of that form adds n_ref wet frames into its accumulator and emits the first `nframes` of them; everything else reaches
an output only n_ref / nframes calls later.  mc_debug_read item 4 returns the accumulator as the engine keeps it and
oracle/refcompat_np.py keeps the reference's (RefCompatNp.resid, whose real part is what is heard), so what a handful of calls
wrote can be compared position by position: `acc_frames` undoes the engine's layout, `drive` runs the same calls and parameter
events through both, `acc_errors` reads the difference per row of the second inverse pass and per residue class of the first.
No GPU is needed to import this module (tests/test_single_form_np_cpu.py checks it on the CPU)."""
import numpy as np

from helpers import rms

ROW = 512  # frames [512 b, 512 b + 512) are what one b of the second inverse pass writes; s mod 512 is the a of the first


def acc_frames(raw, n_ref, base):
    """The 2 * n_ref floats of debug_read(4, ...) as [2, n_ref] in frame order: frame s counts from the next call's frame 0.
    The engine keeps a ring of N slots per channel, slot t = (base + s) mod N at [c][t mod 512][t / 512] (singlefft.hip.h,
    "S4"), and base = (calls so far x nframes) mod N."""
    M = n_ref // ROW
    ring = np.asarray(raw).reshape(2, ROW, M)
    t = (int(base) + np.arange(n_ref)) % n_ref
    return ring[:, t % ROW, t // ROW]


def ring_from_frames(frames, n_ref, base):
    """The inverse of acc_frames, written from the layout formula as flat offsets (for its test): the array the engine would hold."""
    M = n_ref // ROW
    frames = np.asarray(frames)
    raw = np.zeros(2 * n_ref, frames.dtype)
    t = (base + np.arange(n_ref)) % n_ref
    for c in range(2):
        raw[c * n_ref + (t % ROW) * M + t // ROW] = frames[c]
    return raw


def _set(cc, params):
    for k, v in params.items():
        cc[k] = np.float32(v) if isinstance(v, float) else v


def oracle_run(n_ref, irs, x, events, period):
    """x [2, ncalls * period] through RefCompatNp, `events` = {call index: ((half, params), ...)} applied before that call.
    Returns (outputs float64 [2, n], accumulator float64 [2, n_ref] after the last call)."""
    from oracle.refcompat_np import RefCompatNp

    r = RefCompatNp(n_ref, three_mult=True)
    for i, ir in enumerate(irs):
        r.prepare(i, ir)
    out = np.zeros((2, x.shape[1]))
    for q in range(x.shape[1] // period):
        for half, p in events.get(q, ()):
            _set(r.cc[half], p)
        s = slice(q * period, (q + 1) * period)
        out[:, s] = r.process_block(x[0, s], x[1, s])
    acc = np.stack([r.resid[c][:n_ref].real for c in range(2)])
    return out, acc


def engine_run(n_ref, irs, x, events, period):
    """The same calls through Convolution(form="single"), one mc_process per period.
    Returns (outputs float32 [2, n], accumulator float32 [2, n_ref] in frame order after the last call)."""
    from cuda_audio_amd.engine import Convolution

    c = Convolution("acc", n_ref, form="single", period=period, max_batch=8)
    try:
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        out = np.zeros((2, x.shape[1]), np.float32)
        ncalls = x.shape[1] // period
        for q in range(ncalls):
            for half, p in events.get(q, ()):
                c.cc[half].value.update(**p)
            s = slice(q * period, (q + 1) * period)
            out[:, s] = np.stack(c.onProcess(x[0, s], x[1, s]))
        raw = c.debug_read(4, 0, np.float32, 0, 2 * n_ref)
    finally:
        c.close()
    return out, acc_frames(raw, n_ref, (ncalls * period) % n_ref)


def drive(n_ref, irs, x, events, period, oracle=None):
    """Both runs: dict(want_out, want_acc, got_out, got_acc).  `oracle` = what oracle_run returned for these arguments,
    for the callers that share one among several engine runs."""
    want_out, want_acc = oracle if oracle is not None else oracle_run(n_ref, irs, x, events, period)
    got_out, got_acc = engine_run(n_ref, irs, x, events, period)
    return dict(want_out=want_out, want_acc=want_acc, got_out=got_out, got_acc=got_acc)


def _rms_over(a, axes):
    a = np.asarray(a, np.float64)
    return np.sqrt(np.mean(a * a, axis=axes))


def acc_errors(got, want, lo=0, hi=None):
    """got, want: accumulators [2, N] in frame order.  Errors as RMS over both channels: of the whole array (`rms`), of the
    worst of the M rows (`worst_row`, at `worst_row_at`) and of the worst of the 512 residue classes (`worst_class`, at
    `worst_class_at`).  Of `want` itself: `row_rms` [M], `class_rms` [512], `peak`, and for the rows that lie wholly inside
    the frames [lo, hi) (`live_rows`): the quietest of them (`row_floor`) and the quietest residue class taken over those rows
    alone (`class_floor`) - a class runs through every row, the empty ones at the far end included."""
    want = np.asarray(want, np.float64)
    N = want.shape[1]
    M = N // ROW
    hi = N if hi is None else hi
    err = (np.asarray(got, np.float64) - want).reshape(2, M, ROW)
    w = want.reshape(2, M, ROW)
    row_err, class_err = _rms_over(err, (0, 2)), _rms_over(err, (0, 1))
    b0, b1 = -(-lo // ROW), hi // ROW
    live = np.arange(b0, b1)
    row_rms = _rms_over(w, (0, 2))
    return dict(rms=rms(err), worst_row=float(row_err.max()), worst_row_at=int(row_err.argmax()),
                worst_class=float(class_err.max()), worst_class_at=int(class_err.argmax()),
                row_rms=row_rms, class_rms=_rms_over(w, (0, 1)), peak=float(np.abs(want).max()), live_rows=live,
                row_floor=float(row_rms[live].min()) if len(live) else 0.0,
                class_floor=float(_rms_over(w[:, b0:b1], (0, 1)).min()) if len(live) else 0.0)


def describe(r):
    return (f"rms {r['rms']:.3e}, worst row {r['worst_row']:.3e} (b = {r['worst_row_at']}), worst class {r['worst_class']:.3e} "
            f"(a = {r['worst_class_at']}); oracle: peak {r['peak']:.3f}, row floor {r['row_floor']:.4f}, class floor {r['class_floor']:.4f}")


def flat_ir(taps, seed, scale):
    """Stationary Gaussian noise, no decay envelope (make_ir decays by 60 dB, which leaves the far rows of the accumulator
    empty): float32 [taps, 2]."""
    return (np.random.default_rng(seed).standard_normal((taps, 2)) * scale).astype(np.float32)


def white_input(n, seed, amp=0.25):
    """White Gaussian noise of standard deviation amp: float32 [2, n]."""
    return (np.random.default_rng(seed).standard_normal((2, n)) * amp).astype(np.float32)
