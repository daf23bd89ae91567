"""What the stepped IR loads store is on record: the tail, phase, filter and match steps (steps 1a to 1d of the shaped load)
through prepare(), prepare_sweep() and prepare_synth().  tests/golden/ir_load_bits.json holds one SHA-256 digest per case below
under the library of the commit its "commit" field names, the last one at which each step's run strung its own allocations,
upload and error tail together and shape_stage ran each step with a block of its own; the test computes the same with the
library under test and compares.  No tolerance: since then only host control flow has moved (one step request and one step plan
behind the entry points, one step helper in shape_stage, one owner of the spectral steps' work buffers), and every step's header
says that the same input gives the same bits, so a different digest is a launch, an argument or a note_load that changed.

A case's digest covers the stored taps' raw bytes, ir_info, every ir_*_info getter (its numbers, or the code and message with
which it says that the load had no such step: note_load must clear every kind) and ir_match_curve; of a load that the library
refuses, the code and the message.

One engine, n_ref 65536 at 48 kHz, and one of the single-transform form (which keeps no taps: load_ir's other note_load call).
The frames: 1 (the 16-point minimum transform), 200 (one transform pass) and 5000 (two passes, so the third work buffer
exists).  A step's knobs are asked for on that step's cases only:
  tail     cut and extend, alone
  phase    alone
  filter   convolve and deconvolve, stereo and mid, a filter of 1 frame and of 300; once at 44100 Hz (converted on upload)
  match    a target, linked and unlinked, minimum phase; linear phase with a delay; flat with a tilt; a target at 44100 Hz
  all four steps together, and with the IR at 44100 Hz
  prepare_sweep (a 4096-frame sweep, a 5000-frame recording): each step alone, and all four
  prepare_synth with a tail, and with a room and a tail
  a stepped load and then a plain prepare() on the same index

tests/golden/ir_load_bits_parts.json is a second fixture by the same mechanism for the parts step (step 1e), which the first
one's commit predates, under the package and the library of the commit it names: the last one at which prepare() and
prepare_sweep() chose among the entry points themselves.  Its digests cover ir_parts_info too.  Frames 200 and 5000: the parts
step alone, all five steps, all five with the IR at 44100 Hz; prepare_sweep with the parts alone and with all five; a five-step
load and then a plain prepare() on the same index.  No tolerance here either: only the callers of the library moved.

A fixture is recorded by this module run as a program, in a process of its own, with MCCONV_LIB naming the library to record,
or MCCONV_TREE the built checkout whose package and library are recorded; a third argument `parts` records the second fixture:
    MCCONV_LIB=<the build to record> python tests/test_gpu_ir_load_bits.py <output.json> <the commit that build is of>
    MCCONV_TREE=<a built checkout of the commit> python tests/test_gpu_ir_load_bits.py <output.json> <that commit> parts
The tests themselves never record and never skip."""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_load_bits.json")
RATE = 48000
N_REF = 65536
GOLDEN_PARTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_load_bits_parts.json")
FRAMES = (1, 200, 5000)
PARTS_FRAMES = (200, 5000)
GETTERS = ("shape", "damp", "synth", "room", "room_bands", "room_mics", "sweep", "tail", "phase", "filter", "match")


def _feed(h, v):
    """everything a case returns, in a fixed order: dicts by key, sequences in order, arrays and numbers as their raw bytes"""
    if isinstance(v, dict):
        for k in sorted(v, key=repr):
            h.update(repr(k).encode())
            _feed(h, v[k])
    elif isinstance(v, (tuple, list)):
        h.update(b"seq %d" % len(v))
        for x in v:
            _feed(h, x)
    elif isinstance(v, np.ndarray):
        h.update(repr(v.shape).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (bool, int, np.integer)):
        h.update(struct.pack("<q", int(v)))
    elif isinstance(v, float):
        h.update(struct.pack("<d", v))
    elif isinstance(v, str):
        h.update(v.encode())
    elif v is None:
        h.update(b"none")
    else:
        raise TypeError(f"{type(v)} in a case's result")


def _or_error(call):
    from cuda_audio_amd._lib import McError

    try:
        return call()
    except McError as e:
        return f"error {e.code}: {e}"


def _stored(c, idx, getters=GETTERS):
    """everything the engine tells of IR idx"""
    got = dict(taps=_or_error(lambda: c.ir_taps(idx)), info=_or_error(lambda: c.ir_info(idx)), curve=_or_error(lambda: c.ir_match_curve(idx)))
    for name in getters:
        got[name] = _or_error(lambda: getattr(c, f"ir_{name}_info")(idx))
    return got


def digests(verbose=False):
    """{case: SHA-256} of the library that is loaded."""
    from cuda_audio_amd.engine import Convolution, IrFilter, IrMatch, IrPhase, IrRoom, IrSynth, IrTail, Sweep
    from cuda_audio_amd.synth import make_ir

    out = {}

    def put(c, case, load):
        assert case not in out, case
        refused = _or_error(lambda: load(0))
        got = refused if refused is not None else _stored(c, 0)
        h = hashlib.sha256()
        _feed(h, got)
        out[case] = h.hexdigest()
        if verbose:
            print(case, refused if refused is not None else {k: v for k, v in got.items() if isinstance(v, str)}, flush=True)

    def tail(F, mode):
        if mode == "cut":
            return IrTail(mode="cut", knee=(F // 2,), fade=min(40, F // 4))
        return IrTail(mode="extend", knee=(F // 2,), t60=(2000,), level_db=((-60.0, -50.0),), fade=min(40, F // 4), length=F + 300, seed=9)

    # (the one-frame second IR by hand: make_ir's two channels can differ in sign alone, and their mid is then all zero)
    second = {1: np.array([[0.75, -0.25]], np.float32), 300: make_ir(300, seed=23, norm=0.3)}
    phase = IrPhase()

    def four(F):
        return dict(tail=tail(F, "extend"), phase=phase, filter=IrFilter(ir=second[300]), match=IrMatch(ir=second[300]))

    def cases(c, frames, alone, prefix=""):
        """alone: every step's own cases too, not just all four together"""
        for F in frames:
            ir = make_ir(F, seed=61 + F % 7, norm=0.05)
            steps = {}
            if alone:
                for mode in ("cut", "extend"):
                    steps[f"tail_{mode}"] = dict(tail=tail(F, mode))
                steps["phase"] = dict(phase=phase)
                for op in ("convolve", "deconvolve"):
                    for channels in ("stereo", "mid"):
                        for G in (1, 300):
                            steps[f"filter_{op}_{channels}_G{G}"] = dict(filter=IrFilter(ir=second[G], op=op, channels=channels))
                steps["filter_convolve_at_44100"] = dict(filter=IrFilter(ir=second[300], rate=44100))
                steps["match_target_linked"] = dict(match=IrMatch(ir=second[300]))
                steps["match_target_unlinked"] = dict(match=IrMatch(ir=second[300], link=False))
                steps["match_target_linear_delay64"] = dict(match=IrMatch(ir=second[300], phase="linear", delay=64))
                steps["match_flat_tilt"] = dict(match=IrMatch(tilt_db=-3.0))
                steps["match_target_at_44100"] = dict(match=IrMatch(ir=second[300], rate=44100))
            steps["all_four"] = four(F)
            for name, kw in steps.items():
                put(c, f"{prefix}{name}_{F}", lambda idx: c.prepare(idx, ir, **kw))
            put(c, f"{prefix}all_four_ir_at_44100_{F}", lambda idx: c.prepare(idx, ir, ir_rate=44100, **four(F)))

    c = Convolution("bits", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)
    cases(c, FRAMES, True)
    sweep, rec = Sweep(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=RATE), make_ir(5000, seed=41, norm=0.5)
    F = 5000 - 4096 + 1
    for name, kw in dict(tail=dict(tail=tail(F, "extend")), phase=dict(phase=phase), filter=dict(filter=IrFilter(ir=second[300], op="deconvolve")),
                         match=dict(match=IrMatch(ir=second[300], link=False)), all_four=four(F)).items():
        put(c, f"sweep_{name}", lambda idx: c.prepare_sweep(idx, rec, sweep, **kw))
    synth = IrSynth(frames=5000, seed=3, t60=4000, direct=1.0, n_early=4, early_first=100, early_last=900)
    put(c, "synth_tail", lambda idx: c.prepare_synth(idx, synth, tail=tail(5000, "cut")))
    put(c, "synth_room_tail", lambda idx: c.prepare_synth(idx, synth, room=IrRoom(), tail=tail(5000, "extend")))

    def stepped_then_plain(idx):
        c.prepare(idx, make_ir(200, seed=61, norm=0.05), **four(200))
        c.prepare(idx, make_ir(257, seed=62, norm=0.05))

    put(c, "all_four_then_plain", stepped_then_plain)
    c.close()
    c = Convolution("bits1", 16384, sample_rate=RATE, max_batch=32, form="single")
    cases(c, (200, 5000), False, "single_form_")
    c.close()
    return out


def parts_digests(verbose=False):
    """{case: SHA-256} of the library and the package that are loaded, for the cases with the parts step."""
    from cuda_audio_amd.engine import Convolution, IrFilter, IrMatch, IrParts, IrPhase, IrTail, Sweep
    from cuda_audio_amd.synth import make_ir

    out = {}
    c = Convolution("bitsparts", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)

    def put(case, load):
        assert case not in out, case
        refused = _or_error(lambda: load(0))
        got = refused if refused is not None else _stored(c, 0, GETTERS + ("parts",))
        h = hashlib.sha256()
        _feed(h, got)
        out[case] = h.hexdigest()
        if verbose:
            print(case, refused if refused is not None else {k: v for k, v in got.items() if isinstance(v, str)}, flush=True)

    second = make_ir(300, seed=23, norm=0.3)

    def parts(F):  # (boundaries inside the shortest thing that reaches the step, every knob of the step moved)
        return IrParts(direct_end=F // 20, early_end=F // 3, xfade=(F // 50, F // 10), delay=(0, 8, -16), gain_db=(-3.0, -4.0, 2.0), width=(1.0, 0.3, 1.7),
                       balance=0.25, swap=("early",), invert=("late",))

    def five(F):
        return dict(tail=IrTail(mode="extend", knee=(F // 2,), t60=(2000,), level_db=((-60.0, -50.0),), fade=min(40, F // 4), length=F + 300, seed=9),
                    phase=IrPhase(), filter=IrFilter(ir=second), match=IrMatch(ir=second), parts=parts(F))

    for F in PARTS_FRAMES:
        ir = make_ir(F, seed=61 + F % 7, norm=0.05)
        put(f"parts_{F}", lambda idx: c.prepare(idx, ir, parts=parts(F)))
        put(f"all_five_{F}", lambda idx: c.prepare(idx, ir, **five(F)))
        put(f"all_five_ir_at_44100_{F}", lambda idx: c.prepare(idx, ir, ir_rate=44100, **five(F)))
    sweep, rec = Sweep(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=RATE), make_ir(5000, seed=41, norm=0.5)
    F = 5000 - 4096 + 1
    put("sweep_parts", lambda idx: c.prepare_sweep(idx, rec, sweep, parts=parts(F)))
    put("sweep_all_five", lambda idx: c.prepare_sweep(idx, rec, sweep, **five(F)))

    def stepped_then_plain(idx):
        c.prepare(idx, make_ir(200, seed=61, norm=0.05), **five(200))
        c.prepare(idx, make_ir(257, seed=62, norm=0.05))

    put("all_five_then_plain", stepped_then_plain)
    c.close()
    return out


def _compare(golden, got):
    with open(golden) as fh:
        fixture = json.load(fh)
    want = fixture["sha256"]
    assert fixture["commit"]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, differ


def test_the_bits_are_those_before_the_step_plan(gpu_lib):
    _compare(GOLDEN, digests())


def test_the_bits_with_the_parts_step_are_those_before_the_one_call_per_source(gpu_lib):
    _compare(GOLDEN_PARTS, parts_digests())


if __name__ == "__main__":
    import subprocess

    sys.path.insert(0, os.environ.get("MCCONV_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from cuda_audio_amd.build import hipcc as find_hipcc

        hipcc = next(l for l in subprocess.run([find_hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines() if "HIP version" in l)
    except (OSError, RuntimeError, StopIteration):
        hipcc = "unknown"
    record = parts_digests if "parts" in sys.argv[3:] else digests
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], hipcc=hipcc.strip(), sha256=record(verbose=True)), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", os.environ.get("MCCONV_LIB", "the tree's library"))
