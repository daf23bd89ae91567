"""Which form a batch's partition sums take, and the bits that come out, are on record (DESIGN.md §2.5c has the table of forms).
tests/golden/batch_forms.json holds, for every row of ROWS below and every call of the row, what the library of the commit its
"commit" field names answered: kernel_stats()'s fast_levels, resident and partitions after the call, and how far the call moved
the counters of mac_stats(), os_stats() and drop_stats(); and per row the SHA-256 of everything the calls wrote.  The test makes
the same calls with the library under test and compares.  Integers and digests: no tolerance.  Since that commit only the host
code that chooses the form and fills the launch arguments has moved, so the same launches with the same arguments must give the
same bits; a decision the counters cannot see (did the Q1/Q2 prefix sums ride along with the fused form's launch?) rests on the
digests.

A row is one engine - the MCCONV_* switches (every other MCCONV_* variable is cleared first), n_ref, the partitions P of its two
IRs, shard bounds, stream_threshold - and a short sequence of calls on one stream of seeded noise:
    ("d", n)                 process_device of n blocks
    ("d", n, 1)              the same with the first input pointer 4 bytes off 16-byte alignment
    ("s", T, first, count)   process_slice_device
An engine starts inside its cold-start ramp (the gains 1 - 0.8^(b+1) move until about block 80, and a window of p_end partitions
sees them p_end blocks longer), so the first call of a row takes per-slot gains and a call from block 80 + p_end on one set.

The rows stand either side of every comparison the choice makes (choose_form and os_applies in csrc/mcconv.hip), values as of
the recorded commit:
    T against stream_threshold                 threshold-default (47 / 48), threshold-8 (7 / 8)
    fused form, taps >= 16                     a voice's range is a multiple of 16 partitions, so "15 / 16" is none or 16:
                                               fused-taps0 (a shard beyond the IR's end) / fused-taps16 and fused-P5
    fused form, T x taps against fft2_work     fused-work: p_end = 352 partitions x 852 / 853 blocks; 869 / 870 ride along (345 x 870 =
                                               300 150: the IR's own 345 partitions are not what the product counts)
    fused form, settled gains or the ramp      the first call of fused-work, fused-P5 and fused-taps16 against their later ones
    split form, T 767 / 768 inside the ramp    split-ramp-767 / split-ramp-768
    split form, taps 240 / 256                 split-taps240 / split-taps256
    split form, a shard's T x taps             split-shard: 512 partitions x 2539 / 2540 blocks around 1 300 000
    fast-FIR levels (MCCONV_FFT2=0)            ladder-1: T 2046 / 2048; ladder-2: 4096 + 2 / 4096; ladder-3: 8192 + 4 / 8192;
                                               pmin 240 / 256 (ladder-pmin240 / ladder-1), 496 / 512 (ladder-pmin496 / -pmin512),
                                               1008 / 1024 (ladder-pmin1008 / ladder-3); ladder-shard takes no level
    run_front's whole window                   slice-851 / slice-852: one block of reach-back puts 852 + 1 blocks over fft2_work
    os_applies                                 overlap-save: 63 / 64 blocks with MCCONV_OS_MIN=64, a misaligned input, the ramp
Shapes above P = 1100 (kG2Pmax, the 2^21-tap IR) are in test_gpu_tap_probe.py and are not repeated.

The fixture is recorded by this module run as a program on the GPU, with MCCONV_LIB naming the library to record:
    MCCONV_LIB=<the build to record> python tests/test_gpu_batch_forms.py <output.json> <the commit that build is of>
It runs every row twice; a row whose two digests differ is not bit-stable, keeps its forms only ("sha256": null) and is listed
under "unstable".  The test itself never records and never skips."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_forms.json")
BLOCK = 256
NO_OS = dict(MCCONV_OS="0")
LADDER = dict(MCCONV_FFT2="0", MCCONV_OS="0")
SPLIT_ONLY = dict(MCCONV_FFT2_FUSED="0", MCCONV_OS="0")
FUSED_ANY = dict(MCCONV_FFT2_WORK="1", MCCONV_OS="0", MCCONV_FFA_LEVELS="0")


def _row(env, n_ref, P, calls, part=(0, 0), stream_threshold=0):
    return dict(env=env, n_ref=n_ref, P=P, calls=calls, part=part, stream_threshold=stream_threshold)


ROWS = {
    "threshold-default": _row(NO_OS, 8192, 5, [("d", 47), ("d", 48), ("d", 200), ("d", 47), ("d", 48)]),
    "threshold-8": _row(NO_OS, 8192, 5, [("d", 7), ("d", 8), ("d", 200), ("d", 7), ("d", 8)], stream_threshold=8),
    "fused-taps0": _row(FUSED_ANY, 8192, 5, [("d", 256), ("d", 64), ("d", 64)], part=(16, 32)),
    "fused-taps16": _row(FUSED_ANY, 8192, 17, [("d", 256), ("d", 64), ("d", 64)], part=(16, 32)),
    "fused-P5": _row(FUSED_ANY, 8192, 5, [("d", 256), ("d", 256), ("d", 64)]),
    "fused-work": _row(NO_OS, 131072, 345, [("d", 1024), ("d", 852), ("d", 853), ("d", 869), ("d", 870)]),
    "split-ramp-767": _row(NO_OS, 131072, 259, [("d", 767)]),
    "split-ramp-768": _row(NO_OS, 131072, 259, [("d", 768)]),
    "split-taps240": _row(SPLIT_ONLY, 65536, 240, [("d", 768), ("d", 768)]),
    "split-taps256": _row(SPLIT_ONLY, 65536, 241, [("d", 768), ("d", 768)]),
    "split-shard": _row(SPLIT_ONLY, 262144, 517, [("d", 2539), ("d", 2540)], part=(0, 512)),
    "ladder-1": _row(LADDER, 131072, 259, [("d", 2046), ("d", 2048)]),
    "ladder-2": _row(LADDER, 262144, 517, [("d", 4098), ("d", 4096)]),
    "ladder-3": _row(LADDER, 262144, 1024, [("d", 8196), ("d", 8192)]),
    "ladder-pmin240": _row(LADDER, 65536, 240, [("d", 2048)]),
    "ladder-pmin496": _row(LADDER, 131072, 496, [("d", 4096)]),
    "ladder-pmin512": _row(LADDER, 131072, 497, [("d", 4096)]),
    "ladder-pmin1008": _row(LADDER, 262144, 1008, [("d", 8192)]),
    "ladder-shard": _row(LADDER, 131072, 259, [("d", 2048)], part=(0, 256)),
    "slice-851": _row(NO_OS, 131072, 345, [("s", 1024, 100, 851), ("s", 1024, 100, 851)]),
    "slice-852": _row(NO_OS, 131072, 345, [("s", 1024, 100, 852), ("s", 1024, 100, 852)]),
    "overlap-save": _row(dict(MCCONV_OS_MIN="64"), 8192, 5, [("d", 64), ("d", 256), ("d", 63), ("d", 64), ("d", 64, 1), ("d", 64)]),
}


def run_row(row, setenv, delenv):
    """The row's calls on a fresh engine: ([what each call left in the statistics], the SHA-256 of the output)."""
    import torch

    from cuda_audio_amd.engine import Convolution
    from cuda_audio_amd.synth import make_input, make_ir

    for k in [k for k in os.environ if k.startswith("MCCONV_")]:
        delenv(k)
    for k, v in row["env"].items():
        setenv(k, v)
    P, blocks = row["P"], [c[1] for c in row["calls"]]
    c = Convolution("forms", row["n_ref"], max_batch=max(blocks), compat=False, part_begin=row["part"][0], part_end=row["part"][1],
                    stream_threshold=row["stream_threshold"])
    try:
        for i in (0, 1):
            c.prepare(i, make_ir(BLOCK * P - (77, 130)[i], seed=1000 + 2 * P + i, norm=0.05))
        for h in (0, 1):
            c.cc[h].value.update(select=h, predelay=0, dry=0.25, wet=0.75, level=1.0, panWet=0.0, panDry=0.0, vsteps=0)
        n = sum(blocks) * BLOCK
        d_in = torch.zeros(2, n + 4, device="cuda:0")  # (4 frames more: the misaligned calls start one frame later)
        d_in[:, :n] = torch.from_numpy(make_input(n, seed=4321 + P)).to("cuda:0")
        d_out = torch.full((2, n), 7.0, device="cuda:0")
        torch.cuda.synchronize()
        c.enable_kernel_timing(True)
        counters = lambda: dict(mac=c.mac_stats(), os=c.os_stats(), drop=c.drop_stats())  # noqa: E731
        seen, before, o = [], counters(), 0
        for call in row["calls"]:
            ptrs = [d_in[0, o:].data_ptr(), d_in[1, o:].data_ptr(), d_out[0, o:].data_ptr(), d_out[1, o:].data_ptr()]
            if call[0] == "s":
                c.process_slice_device(*ptrs, *call[1:])
            else:
                ptrs[0] += 4 * (call[2] if len(call) > 2 else 0)
                c.process_device(*ptrs, call[1])
            c.sync()
            ks, after = c.kernel_stats(), counters()
            seen.append(dict(fast_levels=int(ks["fast_levels"]), resident=int(ks["resident"]), partitions=int(ks["partitions"]),
                             **{g: {k: after[g][k] - before[g][k] for k in after[g]} for g in after}))
            before = after
            o += call[1] * BLOCK
        out = d_out.cpu().numpy()
    finally:
        c.close()
    return seen, hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def fixture():
    with open(GOLDEN) as fh:
        f = json.load(fh)
    assert f["commit"] and sorted(f["rows"]) == sorted(ROWS)
    return f


@pytest.mark.parametrize("name", list(ROWS))
def test_forms_and_bits_are_those_on_record(gpu_lib, monkeypatch, fixture, name):
    want = fixture["rows"][name]
    seen, digest = run_row(ROWS[name], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    for k, (call, got, exp) in enumerate(zip(ROWS[name]["calls"], seen, want["calls"])):
        print(f"{name} call {k} {call}: {got}")
        assert got == exp, f"{name}: call {k} {call} left {got}, on record {exp}"
    assert len(seen) == len(want["calls"])
    assert (want["sha256"] is None) == (name in fixture["unstable"])
    if want["sha256"] is not None:
        assert digest == want["sha256"], f"{name}: the output's bits moved"


if __name__ == "__main__":
    import subprocess

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from cuda_audio_amd.build import hipcc as find_hipcc

        hipcc = next(l for l in subprocess.run([find_hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines() if "HIP version" in l)
    except (OSError, RuntimeError, StopIteration):
        hipcc = "unknown"
    lib = os.environ.get("MCCONV_LIB", "the tree's library")
    from cuda_audio_amd import _lib

    _lib.load()  # (before the rows clear MCCONV_LIB from the environment)
    rows, unstable = {}, []
    for name, row in ROWS.items():
        runs = [run_row(row, os.environ.__setitem__, lambda k: os.environ.pop(k, None)) for _ in range(2)]
        assert runs[0][0] == runs[1][0], (name, runs[0][0], runs[1][0])
        if runs[0][1] != runs[1][1]:
            unstable.append(name)
        rows[name] = dict(calls=runs[0][0], sha256=None if name in unstable else runs[0][1])
        print(name, [(s["fast_levels"], s["resident"], s["partitions"]) for s in runs[0][0]], rows[name]["sha256"], flush=True)
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], hipcc=hipcc.strip(), rows=rows, unstable=unstable), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", lib)
