"""What Convolution.prepare(), prepare_sweep() and prepare_synth() raise when a load is refused is on record.
tests/golden/ir_prepare_refusals.json holds, per method, one SHA-256 over all cases below and the first eight hex digits of each
case's own SHA-256 of "<exception type>:<its text>", under the package of the commit its "commit" field names, the last one at
which the three methods chose among the library's entry points themselves, branch by branch.  The test makes the same calls with
the package under test and compares.  No tolerance: only the route to the library has moved (the rates by one rule, one call per
source), so a different digest is a call that reaches another entry point's check, passes other rates or pointers, or evaluates
its arguments in another order.

Every call is made on a Convolution without an engine: Convolution.__new__, with _h = None, _L the loaded library and a
sample_rate.  Every check of a load comes before the engine is looked at, and a null engine is refused at the latest, so every
case must raise and none touches HIP; a case that returns fails the test.

The step states, never thinned: each of tail, phase, filter, match and parts is
  none   not given
  off    given and switched off
  on     on and good
  bad    on, one field out of range (the tail's width, the phase's floor_db, the filter's reg_db, the match's octaves, the parts'
         width)
and the filter and the match have a fifth, `rate`: on and good with a second IR at 44100 Hz.  That is 4 * 4 * 5 * 5 * 4 = 1600
combinations for prepare() and prepare_sweep(); prepare_synth() takes the tail alone.

The other arguments as a full product would be some 10^6 cases per method, so per combination ROWS rows of them are drawn, new ones for
every combination, by a generator of this file's own (the same rows everywhere), every value with the same probability:
  shape        None, everything off, trim_db=-40, trim_db=+1 (bad)
  eq           None, no band on, one band on, one band at 5 Hz (bad)
  damp         None, no crossover, one crossover, crossovers that descend (bad)
  prepare()        session rate None, 48000, 1000; ir_rate None, 44100, 48000, 5000
  prepare_sweep()  session rate None, 48000, 1000; the sweep's rate 0, 48000, 100; ir_frames None, 1000, 0
  prepare_synth()  session rate None, 48000, 1000; the synth's rate 0, 48000; each of room, mics and bands None, good, bad (mics
                   and bands also without a room)

The fixture is recorded by this module run as a program, with MCCONV_TREE naming the built checkout whose package is recorded:
    MCCONV_TREE=<a built checkout of the commit to record> python tests/test_ir_prepare_refusals_cpu.py <output.json> <that commit>
The test itself never records and never skips."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_prepare_refusals.json")
ROWS = {"prepare": 8, "prepare_sweep": 6, "prepare_synth": 1000}
STATES = ("none", "off", "on", "bad")
SECOND_STATES = STATES + ("rate",)
SESSIONS = (None, 48000, 1000)


def _lcg(seed):
    """draw(n): a linear congruential generator, because the rows must be the same wherever this runs"""
    state = [seed]

    def draw(n):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (state[0] >> 33) % n

    return draw


def _objects():
    """{argument: its states, in the order of the docstring}"""
    from cuda_audio_amd.engine import IrDamp, IrEq, IrFilter, IrMatch, IrParts, IrPhase, IrRoom, IrRoomBands, IrRoomMics, IrShape, IrTail

    second = np.zeros((10, 2), np.float32)
    second[0] = 1.0

    def tail(**kw):
        return IrTail(**dict(dict(mode="extend", knee=(500,), t60=(2000,), level_db=((-60.0, -60.0),), fade=40), **kw))

    def parts(**kw):
        return IrParts(**dict(dict(direct_end=20, early_end=640), **kw))

    return dict(
        shape=(None, IrShape(), IrShape(trim_db=-40.0), IrShape(trim_db=1.0)),
        eq=(None, IrEq(bands=[("off", 500.0)]), IrEq(bands=[("peak", 500.0, 3.0)]), IrEq(bands=[("peak", 5.0, 3.0)])),
        damp=(None, IrDamp(xovers=(), decay=()), IrDamp(xovers=(400,), decay=(0, 1600)), IrDamp(xovers=(400, 300), decay=(0, 1, 2))),
        tail=dict(none=None, off=tail(mode="off"), on=tail(), bad=tail(width=2.0)),
        phase=dict(none=None, off=IrPhase(mode="off"), on=IrPhase(), bad=IrPhase(floor_db=10.0)),
        filter=dict(none=None, off=IrFilter(ir=second, op="off"), on=IrFilter(ir=second), bad=IrFilter(ir=second, reg_db=5.0), rate=IrFilter(ir=second, rate=44100)),
        match=dict(none=None, off=IrMatch(ir=second, mode="off"), on=IrMatch(ir=second), bad=IrMatch(ir=second, octaves=5.0), rate=IrMatch(ir=second, rate=44100)),
        parts=dict(none=None, off=parts(mode="off"), on=parts(), bad=parts(width=2.5)),
        room=(None, IrRoom(), IrRoom(size=(5.0, -4.0, 3.0))),
        mics=(None, IrRoomMics.pair(), IrRoomMics(pattern=2.0)),
        bands=(None, IrRoomBands(xovers=(500.0,), beta=(0.9, 0.8)), IrRoomBands(xovers=(500.0, 400.0), beta=0.9)),
    )


def cases():
    """{method: [(name of the case, keyword arguments of the call, session rate)]}"""
    from cuda_audio_amd.engine import IrSynth, Sweep

    o = _objects()
    wav = np.zeros((1000, 2), np.float32)
    wav[3] = 0.5
    recording = np.zeros((5000, 2), np.float32)
    trio = lambda r: dict(shape=o["shape"][r[0]], eq=o["eq"][r[1]], damp=o["damp"][r[2]])  # noqa: E731
    out = {"prepare": [], "prepare_sweep": [], "prepare_synth": []}
    combos = list(itertools.product(STATES, STATES, SECOND_STATES, SECOND_STATES, STATES))
    draw = _lcg(20260201)
    for combo in combos:
        steps = {k: o[k][s] for k, s in zip(("tail", "phase", "filter", "match", "parts"), combo)}
        for r in [tuple(draw(n) for n in (4, 4, 4, 3, 4)) for _ in range(ROWS["prepare"])]:
            kw = dict(idx=0, wav=wav, ir_rate=(None, 44100, 48000, 5000)[r[4]], **trio(r), **steps)
            out["prepare"].append(("%s %s" % ("/".join(combo), r), kw, SESSIONS[r[3]]))
    draw = _lcg(20260202)
    for combo in combos:
        steps = {k: o[k][s] for k, s in zip(("tail", "phase", "filter", "match", "parts"), combo)}
        for r in [tuple(draw(n) for n in (4, 4, 4, 3, 3, 3)) for _ in range(ROWS["prepare_sweep"])]:
            sweep = Sweep(frames=4096, f1_hz=100.0, f2_hz=20000.0, rate=(0, 48000, 100)[r[4]])
            kw = dict(idx=0, recording=recording, sweep=sweep, ir_frames=(None, 1000, 0)[r[5]], **trio(r), **steps)
            out["prepare_sweep"].append(("%s %s" % ("/".join(combo), r), kw, SESSIONS[r[3]]))
    draw = _lcg(20260203)
    for _ in range(ROWS["prepare_synth"]):
        r = tuple(draw(n) for n in (4, 4, 4, 3, 2, 3, 3, 3, 4))
        synth = IrSynth(frames=2000, t60=1500, seed=3, rate=(0, 48000)[r[4]])
        kw = dict(idx=0, synth=synth, room=o["room"][r[5]], mics=o["mics"][r[6]], bands=o["bands"][r[7]], tail=o["tail"][STATES[r[8]]], **trio(r))
        out["prepare_synth"].append((str(r), kw, SESSIONS[r[3]]))
    return out


def digests():
    """{method: (SHA-256 of all its cases, [the eight-digit digest of each case], [the names of the cases that returned])} of the
    package that is imported."""
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import Convolution

    c = Convolution.__new__(Convolution)
    c._h, c._L = None, _lib.load()
    out = {}
    for method, rows in cases().items():
        whole, each, returned = hashlib.sha256(), [], []
        for name, kw, session in rows:
            c.sample_rate = session
            try:
                getattr(c, method)(**kw)
                said = "returned"
                returned.append(name)
            except Exception as e:  # noqa: BLE001 (whatever is raised is the record)
                said = "%s:%s" % (type(e).__name__, e)
            h = hashlib.sha256(said.encode())
            each.append(h.hexdigest()[:8])
            whole.update(h.digest())
        out[method] = (whole.hexdigest(), each, returned)
    return out


def test_the_three_methods_refuse_as_they_did_branch_by_branch():
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    assert fixture["commit"] and fixture["rows"] == ROWS
    got = digests()
    all_cases = cases()
    assert sorted(got) == sorted(fixture["sha256"]) == sorted(fixture["cases"])
    differ = []
    for method, (whole, each, returned) in got.items():
        assert not returned, (method, returned[:20])
        want = fixture["cases"][method]
        assert len(want) == 8 * len(each), method
        differ += [(method, all_cases[method][k][0]) for k in range(len(each)) if want[8 * k:8 * k + 8] != each[k]]
        if whole != fixture["sha256"][method] and not differ:
            differ.append((method, "the digest of all cases"))
    assert not differ, (len(differ), differ[:20])


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("MCCONV_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = digests()
    assert not any(v[2] for v in got.values()), {k: v[2][:5] for k, v in got.items()}
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], rows=ROWS, sha256={k: v[0] for k, v in got.items()}, cases={k: "".join(v[1]) for k, v in got.items()}), fh,
                  indent=1, sort_keys=True)
        fh.write("\n")
    import cuda_audio_amd

    print("recorded", sys.argv[1], "from", os.path.dirname(cuda_audio_amd.__file__), {k: len(v[1]) for k, v in got.items()})
