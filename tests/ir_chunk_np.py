"""Numpy statement of the chunked linear recurrence of the IR tools (cuda_audio_amd/csrc/chunkwalk.hip.h, carry_scan and
chunk_geom of ireq.hip.h): the scheme itself, which the sequential restatements (ir_eq_np.biquad and what is built on it) leave
out on purpose.

Test infrastructure only: the product never imports it.  A lane's recurrence is a cascade of S biquad sections (S = 1: an EQ
band or one section of a decay band, k_eq_chunk; S = 2: a crossover of the damping, k_damp_chunk), its state the 2 S numbers
(s1, s2) of each section, affine over a run of taps: s' = A^len s + e.
  geometry  chunk_geom: chunks of CHUNK taps, at most RUNS runs of K = ceil(nchunks / RUNS) chunks, workgroups of WG_CHUNKS chunks;
  powers    M = A^CHUNK and MK = M^K by repeated squaring in `powers` (numpy float64 or longdouble), each rounded to float64
            once, MK raised from the unrounded M: ieq_carry and damp_carry of the headers (carry_powers);
  local     every chunk from rest, the chunks side by side (vectorised), the end states e_c kept;
  carry     carry_scan's three steps: every run scanned from rest by its lane; the runs' ends scanned by one lane with MK; every
            run scanned again from its true start, which stores the state each chunk starts with;
  fix-up    every chunk again from that state; what it writes is the result.
Everything but the powers is float64, one operation per numpy call in the order the kernels write them (no fused multiply-adds;
the device's compiler may fuse some, which moves a result by an ulp of a term and not by more).

`sequential` is the plain loop over all taps in either precision: with float64 it is ir_eq_np.biquad's arithmetic, with
longdouble the run the restatements are checked against."""
import functools

import numpy as np

import ir_decay_np

CHUNK = 256      # IEQ_CHUNK
RUNS = 128       # IEQ_RUNS
WG_CHUNKS = 64   # IEQ_WG_CHUNKS

# The conditioning cases of tests/test_gpu_ir_long_carry.py, which tests/test_ir_chunk_cpu.py runs through the model: 523 264 taps
# at 384 kHz (n_ref 524288 less the 1024 frames of a period) are 2044 chunks, K = 16, a last run of 12 chunks.
COND_RATE, COND_N_REF = 384000, 524288
COND_N = COND_N_REF - 1024
COND_BANDS = {
    "lowcut": (("lowcut", 10, 0, 32),),
    "peak": (("peak", 10, 24, 32),),
    "highcut": (("highcut", 10),),
    "three": (("lowcut", 10, 0, 32), ("peak", 10, 24, 32), ("highcut", 10)),
    "top": (("peak", 0.45 * COND_RATE, -36, 0.1),),
}
COND_DAMP = ((10,), (0, 200000), 1000)  # the band above the crossover fades out: late taps are the 10 Hz low-pass alone
COND_DECAY = dict(bands=(10,), curve_points=33)


@functools.lru_cache(maxsize=None)
def falling_noise(n, rate, amp=0.3):
    """n taps of noise that fall 60 dB over the length, float32 [n, 2]."""
    ir = ir_decay_np.noise_ir(n, 0, rate, t60=n / rate, seed=7, amp=amp)
    ir.setflags(write=False)
    return ir


def chunk_geom(n, chunk=CHUNK, runs=RUNS):
    """(workgroups of a chunk kernel, chunks, chunks per run of the carry pass): chunk_geom of ireq.hip.h."""
    nchunks = (n + chunk - 1) // chunk
    return (n + WG_CHUNKS * chunk - 1) // (WG_CHUNKS * chunk), nchunks, (nchunks + runs - 1) // runs


def _step(sections, s, v):
    """One tap v through the cascade; s = [s1, s2] per section, updated in place; returns the last section's output.
    Scalars or arrays of one shape."""
    for k, (b0, b1, b2, a1, a2) in enumerate(sections):
        y = b0 * v + s[2 * k]
        s[2 * k] = b1 * v - a1 * y + s[2 * k + 1]
        s[2 * k + 1] = b2 * v - a2 * y
        v = y
    return v


def matrix(sections):
    """A [2 S, 2 S] float64: column j = what a tap of zero makes of the unit state j (damp_matrix; S = 1: [[-a1, 1], [-a2, 0]])."""
    d = 2 * len(sections)
    A = np.zeros((d, d))
    for j in range(d):
        s = [1.0 if i == j else 0.0 for i in range(d)]
        _step(sections, s, 0.0)
        A[:, j] = s
    return A


def _matmul(a, b):
    """Row times column, the terms added first to last (ieq_matmul, damp_matmul)."""
    d = a.shape[0]
    r = np.zeros_like(a)
    for i in range(d):
        for j in range(d):
            v = a[i, 0] * b[0, j]
            for k in range(1, d):
                v = v + a[i, k] * b[k, j]
            r[i, j] = v
    return r


def matpow(a, p):
    """a^p by repeated squaring in a's own type (ieq_matpow, damp_matpow)."""
    r = np.eye(a.shape[0], dtype=a.dtype)
    while p:
        if p & 1:
            r = _matmul(r, a)
        p >>= 1
        a = _matmul(a, a)
    return r


def carry_mats(sections, K, powers=np.longdouble, chunk=CHUNK):
    """(M, MK) as float64: A^chunk and its K-th power, raised in `powers` and rounded once each."""
    M = matpow(matrix(sections).astype(powers), chunk)
    return M.astype(np.float64), matpow(M, K).astype(np.float64)


def _affine(M, s, e):
    """M s + e over states [..., d]: a row's terms added first to last, then e (ieq_mul, damp_mul and the carry's step)."""
    d = M.shape[0]
    out = np.empty_like(s)
    for i in range(d):
        v = M[i, 0] * s[..., 0]
        for k in range(1, d):
            v = v + M[i, k] * s[..., k]
        out[..., i] = v + e[..., i]
    return out


def carry_scan(e, M, MK, K, runs=RUNS):
    """e [nchunks, channels, d]: the state every chunk leaves from rest.  Returns the state every chunk starts with, by
    carry_scan's three steps, lane (run, channel) owning chunks [run K, (run + 1) K) cut at nchunks."""
    nchunks = e.shape[0]
    c0 = np.minimum(np.arange(runs) * K, nchunks)
    c1 = np.minimum(c0 + K, nchunks)
    pad = np.concatenate([e, np.zeros((1,) + e.shape[1:])])  # (a chunk past the end is read nowhere: the mask drops it)

    def scan(s, store):
        for j in range(K):
            c = c0 + j
            live = c < c1
            at = np.where(live, c, nchunks)
            if store is not None:
                store[at[live]] = s[live]
            s = np.where(live[:, None, None], _affine(M, s, pad[at]), s)
        return s

    ends = scan(np.zeros((runs,) + e.shape[1:]), None)
    r = np.zeros(e.shape[1:])
    for g in range(runs):  # lanes 0 and 1: one chain per channel
        end = ends[g].copy()
        ends[g] = r
        r = _affine(MK, r, end)
    start = np.zeros_like(e)
    scan(ends, start)
    return start


def _walk(x, sections, start):
    """x [nchunks, chunk, channels] through the cascade, every chunk from start [nchunks, channels, d] (None: rest), the
    chunks side by side.  Returns (y of x's shape, the end states)."""
    d = 2 * len(sections)
    s = [np.zeros(x[:, 0].shape) if start is None else start[..., i].copy() for i in range(d)]
    y = np.empty_like(x)
    for m in range(x.shape[1]):
        y[:, m] = _step(sections, s, x[:, m])
    return y, np.stack(s, axis=-1)


def chunked(x, sections, powers=np.longdouble, chunk=CHUNK, runs=RUNS):
    """x: float64 [n, channels] through the cascade `sections` ((b0, b1, b2, a1, a2) each, a0 = 1) from rest at tap 0 by the
    chunked scheme; returns y [n, channels].  Taps past n read as zero and are not written."""
    x = np.asarray(x, np.float64)
    n, channels = x.shape
    _, nchunks, K = chunk_geom(n, chunk, runs)
    M, MK = carry_mats(sections, K, powers, chunk)
    xp = np.zeros((nchunks * chunk, channels))
    xp[:n] = x
    xp = xp.reshape(nchunks, chunk, channels)
    _, e = _walk(xp, sections, None)
    y, _ = _walk(xp, sections, carry_scan(e, M, MK, K, runs))
    return y.reshape(-1, channels)[:n]


def sequential(x, sections, dtype=np.float64):
    """x [n, channels] through the cascade, one tap after the other, all of it in `dtype`; returns y [n, channels] in dtype.
    With float64 it is ir_eq_np.biquad section after section, bit for bit."""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype)
    for sec in sections:
        cast = float if dtype is np.float64 else dtype
        b0, b1, b2, a1, a2 = (cast(v) for v in sec)
        for ch in range(x.shape[1]):
            col = x[:, ch].tolist() if dtype is np.float64 else list(x[:, ch].astype(dtype))
            s1 = s2 = cast(0.0)
            y = []
            for v in col:
                o = b0 * v + s1
                s1 = b1 * v - a1 * o + s2
                s2 = b2 * v - a2 * o
                y.append(o)
            out[:, ch] = y
        x = out.copy()
    return out


def rel_rms(got, want, part=slice(None)):
    """rms(got - want) / rms(want) over the taps `part`, in float64 (the differences taken in want's type)."""
    d = np.asarray(got[part] - want[part], np.float64)
    w = np.asarray(want[part], np.float64)
    return float(np.sqrt(np.mean(d * d)) / np.sqrt(np.mean(w * w)))


def last_eighth(n):
    return slice(n - n // 8, n)
