"""The chunked-recurrence kernels of the IR tools (csrc/chunkwalk.hip.h and the five kernels that walk through it: k_eq_chunk,
k_damp_chunk, k_tail_chunk, k_flr_band, k_dec_sum; the carries k_eq_carry and k_damp_carry) give the bits that are on record.
tests/golden/chunk_walk_bits.json holds SHA-256 digests of what the library stored and measured for the cases below; the test
computes the same with the library under test and compares.  No tolerance: a different digest is a reordered expression.

What the digests pin: the arithmetic of the kernels and its order, with the carry matrices A^256 and (A^256)^K raised in long
double and rounded once (carry_powers of csrc/ireq.hip.h).
  "sha256"                 recorded at the commit before the five kernels shared one walk, and still what they give: eq_1, damp1_257,
                           the three tail_* cases and floor_40000 run no matrix of k_eq_carry that matters (one chunk, or the
                           damping's 4 x 4 ones, which were raised so from the start); the eq_* cases do, but their float32 taps
                           round the matrices' last bits away, so they stayed as well.
  "sha256_extended_carry"  re-recorded at the commit its "commit" field names, which raised k_eq_carry's 2 x 2 matrices in long
                           double where they had been squared in double: damp3_eq_16385, damp3_eq_40000 and decay_40000, the
                           three whose digests that moved.  No kernel changed there; tests/test_gpu_ir_long_carry.py has what
                           the change is for.

The lengths: 1 (below the recurrence's order), 257 (a chunk and a tap), 16385 (one workgroup's span and a tap), 32769 (129
chunks: the carry's runs are two chunks long), 40000 (three workgroups, 157 chunks).

The fixture is recorded by this module run as a program, in a process of its own, with MCCONV_LIB naming the library to record:
    MCCONV_LIB=<the build to record> python tests/test_gpu_chunk_walk_bits.py <output.json>
which writes every case under "sha256"; a digest that has to change moves by hand into a key of its own that names the commit.
The test itself never records and never skips."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chunk_walk_bits.json")
RATE = 48000
N_REF = 65536
BANDS = [("lowcut", 120), ("peak", 2500, 6.0, 1.5)]
EQ_LENGTHS = (1, 257, 16385, 32769, 40000)
XOVERS3 = (250, 2000, 8000)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _table(rows, fields, groups):
    """rows of ir_decay / ir_floor as float64 [groups, 3, fields]"""
    return np.array([[[rows[(g, name)][f] for f in fields] for name in ("L", "R", "LR")] for g in range(groups)], np.float64)


def digests():
    """{case: SHA-256} of the library that is loaded."""
    from cuda_audio_amd import engine
    from cuda_audio_amd.engine import Convolution, IrDamp, IrEq, IrTail
    from cuda_audio_amd.synth import make_ir
    from ir_shape_np import quiet_lead_ir

    out = {}
    c = Convolution("bits", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)
    eq = IrEq(bands=BANDS)
    for n in EQ_LENGTHS:
        c.prepare(0, make_ir(n, seed=41 + n % 7, norm=0.05), eq=eq)
        out[f"eq_{n}"] = _sha(c.ir_taps(0))
    damp3 = IrDamp(xovers=XOVERS3, decay=(0, 96000, 48000, 24000), origin=480)
    for n in (16385, 40000):
        c.prepare(0, make_ir(n, seed=43 + n % 7, norm=0.05), eq=eq, damp=damp3)
        out[f"damp3_eq_{n}"] = _sha(c.ir_taps(0))
    c.prepare(0, make_ir(257, seed=47, norm=0.05), damp=IrDamp(xovers=(1000,), decay=(0, 4800), origin=0))
    out["damp1_257"] = _sha(c.ir_taps(0))

    def tail(mode, X, n, length=0):
        bands = X + 1
        return IrTail(mode=mode, xovers=XOVERS3[:X], knee=tuple(n // 2 + 7 * j for j in range(bands)), t60=tuple(n // 2 - 11 * j for j in range(bands)),
                      level_db=tuple((-42.0 - 3.0 * j, -44.5 + 2.0 * j) for j in range(bands)), fade=32, length=length, seed=12345, width=0.75)

    c.prepare(0, make_ir(40000, seed=53, norm=0.05), tail=tail("cut", 3, 40000))
    out["tail_cut3_40000"] = _sha(c.ir_taps(0))
    c.prepare(0, make_ir(20000, seed=59, norm=0.05), tail=tail("extend", 3, 20000, length=33000))
    out["tail_extend3_20000_33000"] = _sha(c.ir_taps(0))
    c.prepare(0, make_ir(20000, seed=59, norm=0.05), tail=tail("extend", 0, 20000, length=33000))
    out["tail_extend0_20000_33000"] = _sha(c.ir_taps(0))

    c.prepare(0, quiet_lead_ir(39300, lead=700, seed=31))  # 40 000 taps, the origin past the quiet lead
    assert c.ir_info(0)["taps"] == 40000
    d = c.ir_decay(0, bands=(250, 1000, 4000), onset_db=-20.0, end=35000, curve_points=64)
    assert d["origin"] > 0 and d["taps"] == 35000
    out["decay_40000"] = _sha(_table(d["rows"], engine.DECAY_FIELDS, 4), d["curve"], np.array([d["origin"], d["taps"]], np.uint64))
    f = c.ir_floor(0, xovers=XOVERS3, onset_db=-20.0)
    assert f["origin"] > 0 and f["taps"] == 40000
    out["floor_40000"] = _sha(_table(f["rows"], engine.FLOOR_FIELDS, f["groups"]), np.array([f["origin"], f["taps"]], np.uint64))
    c.close()
    return out


def test_the_bits_are_those_before_the_shared_walk(gpu_lib):
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    want, again = fixture["sha256"], fixture["sha256_extended_carry"]["digests"]
    assert sorted(again) == ["damp3_eq_16385", "damp3_eq_40000", "decay_40000"] and not set(again) & set(want)
    want = dict(want, **again)
    got = digests()
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, differ


if __name__ == "__main__":
    import subprocess

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from cuda_audio_amd.build import hipcc as find_hipcc

        hipcc = next(l for l in subprocess.run([find_hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines() if "HIP version" in l)
    except (OSError, RuntimeError, StopIteration):
        hipcc = "unknown"
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(hipcc=hipcc.strip(), sha256=digests()), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", os.environ.get("MCCONV_LIB", "the tree's library"))
