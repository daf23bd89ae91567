"""What the twelve IR load entry points that take the shape / eq / damp trio say when they refuse a call is on record:
mc_load_ir_damped, mc_load_ir_sweep and the ten stepped ones, mc_load_ir_{tail,phase,filter,match} and
mc_load_ir_sweep_{tail,phase,filter,match}.  tests/golden/ir_load_refusals.json holds SHA-256 digests of every (return code,
mc_last_error()) pair of the calls below under the library of the commit its "commit" field names, the last one at which each
stepped entry point strung its own checks together; the test makes the same calls with the library under test and compares.  No
tolerance: since then only the host code in front of load_ir has moved (one request, one plan, one body per source kind), so a
different digest is a check that moved, went missing or speaks differently.

Every call has a null engine.  All checks of these entry points come before the engine is looked at, and load_ir refuses a null
engine before it reads a pointer, so every call is refused, no call touches HIP, and the small dummy buffers behind the
non-null pointers are never read.  No message contains a pointer.

The step states, never thinned: each of tail, phase, filter and match is
  null   a null pointer
  off    the struct filled with 0xA5 bytes, struct_size included, and its switch off
  bad    on, one field out of range (the tail's width, the phase's floor_db, the filter's reg_db, the match's octaves)
  over   on and good, beyond its limit for some of the frames below: the tail takes the IR's own length (refused for no frame and
         above 2^24), the phase oversamples 64 times (beyond 2^22 points from 2^17 + 1 frames), the filter hands on 2^30 frames,
         the match delays a linear-phase correction by 2^20 frames
  good   on and good: the tail hands on 2^17 + 1 frames, which the oversampling phase state cannot take either
and the match's good state comes twice, against a target and against a flat line.  An entry point gets the product of the states
of the steps it takes: 1, 5, 25, 125 and 750 combinations.

The other arguments are drawn for ROWS rows per source kind, once, by a generator of this file's own (the same rows for every
combination and every library): each argument is its good value with probability 0.6 and otherwise one of the others, so that
some rows get past every check and many stop at each; the first row has every argument good, and two more have no rates and
neither a band nor a damping that would ask for them, so that the filter's and the match's own need of the session's rate
speaks.  A full product of them would be some 10^5 calls per combination.
  shape, eq, damp    null, bad (trim_db, freq_hz, xover_hz), good
  rates              (0, 0), (48000, 48000), (44100, 48000), (7999, 48000), (48000, 0)
  frames             0, 1000, 2^17 + 1, 2^21 + 1, 2^24 + 1, 2^40 + 1 (of the file, or ir_frames of a sweep)
  lr, filter_lr, target_lr          null, non-null
  filter_frames, target_frames      0, 10, 2^40 + 1
  the filter's and the match's rate 0, 8000 (written into the structs that are on)
  sweep              null, a rate of 100 Hz, good; its recording of 0 or 5000 frames

A combination's digest covers its rows in order.  The fixture holds one SHA-256 per entry point over everything it was asked, and per
combination the first eight hex digits of its own SHA-256, in the order of COMBOS, so that a mismatch names the combination while
the file stays small.

The fixture is recorded by this module run as a program, with MCCONV_LIB naming the library to record:
    MCCONV_LIB=<the build to record> python tests/test_ir_load_refusals_cpu.py <output.json> <the commit that build is of>
The test itself never records and never skips."""
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_load_refusals.json")
ROWS = 128
STATES = ("null", "off", "bad", "over", "good")
MATCH_STATES = ("null", "off", "bad", "over", "target", "flat")
STEPS = ("tail", "phase", "filter", "match")
ENTRIES = [(src, n) for src in ("file", "sweep") for n in range(5)]  # n = how many of STEPS the entry point takes
NAMES = {("file", 0): "mc_load_ir_damped", ("sweep", 0): "mc_load_ir_sweep"}
for _n, _step in enumerate(STEPS):
    NAMES["file", _n + 1], NAMES["sweep", _n + 1] = "mc_load_ir_" + _step, "mc_load_ir_sweep_" + _step

RATES = ((48000, 48000), (0, 0), (44100, 48000), (7999, 48000), (48000, 0))  # (the good value first, as on every axis)
FRAMES = (1000, 0, (1 << 17) + 1, (1 << 21) + 1, (1 << 24) + 1, (1 << 40) + 1)
SECOND_FRAMES = (10, 0, (1 << 40) + 1)


def combos(n):
    """the state combinations of an entry point that takes the first n steps"""
    return list(itertools.product(*[MATCH_STATES if s == "match" else STATES for s in STEPS[:n]]))


def _rows():
    """ROWS draws of the other arguments.  A linear congruential generator: the rows must be the same wherever this runs."""
    state = [20260101]

    def draw(n):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (state[0] >> 33) % n

    def pick(count):  # index 0 is the good value
        return 0 if draw(10) < 6 else 1 + draw(count - 1)

    rows = [dict(shape=0, eq=0, damp=0, rates=0, frames=0, lr=0, filter_lr=0, target_lr=0, filter_frames=0, target_frames=0, filter_rate=0, match_rate=0,
                 sweep=0, M=0)]  # (everything good)
    # (no rates, and neither a band nor a damping that would ask for them first: the filter's and the match's own need of the session's rate)
    rows.append(dict(rows[0], eq=1, damp=1, rates=1))
    rows.append(dict(rows[0], eq=1, damp=1, rates=1, filter_rate=1))
    while len(rows) < ROWS:
        rows.append(dict(shape=pick(3), eq=pick(3), damp=pick(3), rates=pick(len(RATES)), frames=pick(len(FRAMES)), lr=pick(2), filter_lr=pick(2),
                         target_lr=pick(2), filter_frames=pick(3), target_frames=pick(3), filter_rate=pick(2), match_rate=pick(2), sweep=pick(3), M=pick(2)))
    return rows


def _off(struct, switch):
    s = struct()
    C.memset(C.byref(s), 0xA5, C.sizeof(s))
    setattr(s, switch, 0)
    return s


def _step_states():
    """{step: {state: struct or None}}"""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrFilter, IrMatch, IrPhase, IrTail

    def tail(**kw):
        return IrTail(**dict(dict(mode="extend", knee=(500,), t60=(2000,), level_db=((-60.0, -60.0),), fade=40, length=(1 << 17) + 1), **kw)).to_c()

    def match(**kw):
        m = IrMatch(**kw).to_c()
        m.mode = _lib.MC_MATCH_TARGET  # (an IrMatch without an ir is flat)
        return m

    flat = IrMatch().to_c()
    assert flat.mode == _lib.MC_MATCH_FLAT
    return dict(
        tail=dict(null=None, off=_off(_lib.McIrTail, "mode"), bad=tail(width=2.0), over=tail(length=0), good=tail()),
        phase=dict(null=None, off=_off(_lib.McIrPhase, "mode"), bad=IrPhase(floor_db=10.0).to_c(), over=IrPhase(oversample=64).to_c(), good=IrPhase().to_c()),
        filter=dict(null=None, off=_off(_lib.McIrFilter, "op"), bad=IrFilter(reg_db=5.0).to_c(), over=IrFilter(frames_out=1 << 30).to_c(), good=IrFilter().to_c()),
        match=dict(null=None, off=_off(_lib.McIrMatch, "mode"), bad=match(octaves=5.0), over=match(phase="linear", delay=1 << 20), target=match(), flat=flat),
    )


def digests():
    """{entry point: (SHA-256 of everything, [the eight-digit digest of each combination])} of the library that is loaded."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import IrDamp, IrEq, IrShape, Sweep

    L = _lib.load()
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    shapes = (IrShape(trim_db=-40.0).to_c(), None, IrShape(trim_db=1.0).to_c())
    eqs = (IrEq(bands=[("peak", 500.0, 3.0)]).to_c(), None, IrEq(bands=[("peak", 5.0, 3.0)]).to_c())
    damps = (IrDamp().to_c(), None, IrDamp(xovers=(400, 300), decay=(0, 1, 2)).to_c())
    sweep = dict(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=48000)
    sweeps = (Sweep(**sweep).to_c(), None, Sweep(**dict(sweep, rate=100)).to_c())
    dummy = (C.c_float * 32)()
    lrs = (C.cast(dummy, C.POINTER(C.c_float)), None)
    states = _step_states()
    rows = _rows()
    out = {}
    for src, n in ENTRIES:
        fn = getattr(L, NAMES[src, n])
        whole, each = hashlib.sha256(), []
        for combo in combos(n):
            st = [states[step][name] for step, name in zip(STEPS, combo)]
            h = hashlib.sha256()
            for r in rows:
                trio = (ref(shapes[r["shape"]]), ref(eqs[r["eq"]]), ref(damps[r["damp"]]))
                if src == "file":
                    args = [None, 0, lrs[r["lr"]], FRAMES[r["frames"]], 1024, *RATES[r["rates"]], *trio]
                else:
                    args = [None, 0, lrs[r["lr"]], (5000, 0)[r["M"]], 1024, ref(sweeps[r["sweep"]]), 0, FRAMES[r["frames"]], *trio]
                args += [ref(s) for s in st[:2]]
                if n >= 3:
                    if combo[2] in ("bad", "over", "good"):
                        st[2].rate = (0, 8000)[r["filter_rate"]]
                    args += [ref(st[2]), lrs[r["filter_lr"]], SECOND_FRAMES[r["filter_frames"]]]
                if n >= 4:
                    if combo[3] in ("bad", "over", "target", "flat"):
                        st[3].rate = (0, 8000)[r["match_rate"]]
                    args += [ref(st[3]), lrs[r["target_lr"]], SECOND_FRAMES[r["target_frames"]]]
                rc = fn(*args)
                h.update(b"%d:%s\n" % (rc, L.mc_last_error()))
            each.append(h.hexdigest()[:8])
            whole.update(h.digest())
        out[NAMES[src, n]] = (whole.hexdigest(), each)
    return out


def test_the_refusals_are_those_before_the_step_plan():
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    assert fixture["commit"] and fixture["rows"] == ROWS
    got = digests()
    assert sorted(got) == sorted(fixture["sha256"]) == sorted(fixture["combinations"])
    differ = []
    for (src, n) in ENTRIES:
        name = NAMES[src, n]
        whole, each = got[name]
        want = fixture["combinations"][name]
        assert len(want) == 8 * len(each), name
        differ += [(name, dict(zip(STEPS, combo))) for k, combo in enumerate(combos(n)) if want[8 * k:8 * k + 8] != each[k]]
        if whole != fixture["sha256"][name] and not differ:
            differ.append((name, "the digest of all combinations"))
    assert not differ, differ[:20]


if __name__ == "__main__":
    import subprocess

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from cuda_audio_amd.build import hipcc as find_hipcc

        hipcc = next(l for l in subprocess.run([find_hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines() if "HIP version" in l)
    except (OSError, RuntimeError, StopIteration):
        hipcc = "unknown"
    got = digests()
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], hipcc=hipcc.strip(), rows=ROWS, sha256={k: v[0] for k, v in got.items()},
                       combinations={k: "".join(v[1]) for k, v in got.items()}), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", os.environ.get("MCCONV_LIB", "the tree's library"))
