"""C++ host: `mcconv_host` over an index with a `room:` line at --rate 48000 (Convolution::prepareRoom: the line's metres and
seconds, the room rendered by the engine when the client starts), without and with `--ir-tail extend` (the floor measured on the
room alone, then the room rendered again with the tail), the malformed lines the index grammar refuses, each naming its key, and
the host over the stand-in engine of tests/stub, which has no room rendering and must say so."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_floor_np
import ir_room_np
import ir_tail_np
from helpers import RMS_TOL, rms
from test_host_ir_synth import _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE = 48000
LINE = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8,gain=0.2,spacing=0.3,axis=y"
ROOM = dict(beta=0.8, gain=0.2, spacing=0.3, axis=1)  # the line; 0.2 s at 48000 Hz is 9600 frames
FRAMES = 9600
LINE_B = "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2"  # half 1's IR: a tenth of a second, too short to have a floor
ROOM_B = dict(size=(6.0, 5.0, 2.5), source=(2.0, 2.0, 1.0), receiver=(4.0, 3.0, 1.5), gain=0.2)
FRAMES_B = 4800


@pytest.mark.gpu
def test_a_room_line_without_and_with_a_tail(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    n_ref, period, nper = 16384, 512, 200
    settings = _index(tmp_path, n_ref, [], [LINE, LINE_B])
    room, _, winfo = ir_room_np.frames(ROOM, RATE, frames=FRAMES, late_gain=0.0)
    room_b, _, winfo_b = ir_room_np.frames(ROOM_B, RATE, frames=FRAMES_B, late_gain=0.0)
    ir_room_np.assert_floor_margin(ir_room_np.images(ROOM, RATE, FRAMES)["tau"], FRAMES)
    ir_room_np.assert_floor_margin(ir_room_np.images(ROOM_B, RATE, FRAMES_B)["tau"], FRAMES_B)

    def run(tag, *flags):
        prefix = str(tmp_path / f"{tag}_")
        cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", str(RATE), "--period", str(period),
               "--dump", prefix, *flags]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
        assert all(len(a) == nper * period for a in io)
        return res.stdout + res.stderr, io

    def want_output(taps, io):
        ref = oracle_mod.RefCompat(n_ref, True)
        for j, t in enumerate(taps):
            ref.prepare(j, t)
        for h in range(2):
            ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
        want = ref.process(io[0], io[1], block=period)
        x = np.stack(io[:2]).astype(np.float64)
        wet = want - 0.5 * (x[0] + x[1])  # (dry 0.5, panDry 0, level 1 in both halves)
        print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
        assert np.abs(wet).max() < 0.5 and rms(want) > 0.01
        return want

    room_line = (f"IR 0 room: order {winfo['order']}, {winfo['images'][0]} and {winfo['images'][1]} images before frame {FRAMES}, direct sound at "
                 f"{winfo['direct'][0]:.2f} and {winfo['direct'][1]:.2f} frames, complete up to frame {winfo['complete']}")
    # 1. the room alone: one line per half (each half loads the index)
    out, io = run("plain")
    assert out.count(room_line) == 2 and " tail: " not in out, out[-3000:]
    assert out.count(f"IR 1 room: order {winfo_b['order']}, {winfo_b['images'][0]} and {winfo_b['images'][1]} images before frame {FRAMES_B}") == 2
    assert len(re.findall(rf"IR 0 synthesised: {FRAMES} frames, seed 0, 0 of 0 reflections kept", out)) == 2
    err = rms(np.stack(io[2:]) - want_output([room, room_b], io))
    print(f"room alone: rms err {err:.3e}")
    assert err <= RMS_TOL

    # 2. with the tail: the floor of the room alone, then the room again with the tail that floor gives
    floor = ir_floor_np.floor(room, RATE, xovers=())
    ir_floor_np.assert_margins(floor)
    assert floor["rows"][(0, "LR")]["peak_to_noise_db"] > 30.0
    tf = ir_floor_np.tail_from_floor(floor)
    fade_s, length_s, seed = 0.005, 0.3, 3
    spec = dict(xovers=(), knee=tuple(tf["knee"]), t60=tuple(tf["t60"]), level_db=tuple(tf["level_db"]), fade=int(np.rint(fade_s * RATE)),
                length=int(np.rint(length_s * RATE)), seed=seed)
    extended, tinfo = ir_tail_np.tailed(room, RATE, "extend", **spec)
    assert len(extended) == 14400 and FRAMES // 2 < tf["knee"][0] < FRAMES
    out2, io2 = run("extend", "--ir-tail", f"extend:fade={fade_s},length={length_s},seed={seed}")
    assert out2.count(room_line) == 4, out2[-3000:]
    line = f"IR 0 tail: extended, 1 of 1 bands at knees {tf['knee'][0]}, {FRAMES} frames in, 14400 out, first frame changed {tinfo['first']}"
    assert out2.count(line) == 2, out2[-3000:]
    floor_b = ir_floor_np.floor(room_b, RATE, xovers=())
    ir_floor_np.assert_margins(floor_b)
    assert floor_b["rows"][(0, "LR")]["status"] == 2  # (no decay above its own last tenth: left as it is)
    assert out2.count("IR 1 tail: peak to noise nan dB (status 2) is under 30 dB, left as it is") == 2, out2[-3000:]
    assert np.array_equal(io2[0], io[0]) and np.array_equal(io2[1], io[1])
    err = rms(np.stack(io2[2:]) - want_output([extended, room_b], io2))
    print(f"room with a tail: rms err {err:.3e}")
    assert err <= RMS_TOL
    assert not np.array_equal(io2[2], io[2])


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


GOOD = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5"


@pytest.mark.parametrize("line,names", [
    ("room:", "room:LENGTH_S"),                        # nothing
    ("room:0.2:5,4,3:1,1.5,1.2", "room:LENGTH_S"),     # no receiver
    ("room:abc:5,4,3:1,1.5,1.2:3.5,2,1.5", "LENGTH_S 'abc'"),
    ("room:0:5,4,3:1,1.5,1.2:3.5,2,1.5", "LENGTH_S '0'"),
    ("room:0.2:5,4:1,1.5,1.2:3.5,2,1.5", "LX,LY,LZ '5,4'"),
    ("room:0.2:5,4,3:1,x,1.2:3.5,2,1.5", "SX,SY,SZ '1,x,1.2'"),
    ("room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5,7", "RX,RY,RZ '3.5,2,1.5,7'"),
    (GOOD + ":", "nothing after the last colon"),      # an empty list
    (GOOD + ":beta", "'beta' is not key=value"),
    (GOOD + ":beta=0.9/0.8", "no value for beta"),     # two values: one or six
    (GOOD + ":beta=0.9/0.8/0.7/0.6/0.5/x", "no value for beta"),
    (GOOD + ":order=33", "no value for order"),
    (GOOD + ":order=2.5", "no value for order"),
    (GOOD + ":spacing=-0.1", "no value for spacing"),
    (GOOD + ":axis=w", "no value for axis"),
    (GOOD + ":speed=fast", "no value for speed"),
    (GOOD + ":gain=nan", "no value for gain"),
    (GOOD + ":last=-1", "no value for last"),
    (GOOD + ":t60=-1", "no value for t60"),
    (GOOD + ":colour=3", "unknown key 'colour'"),      # no such key, of the room's or of synth:'s
    (GOOD + ":late=-0.1", "no value for late"),        # a key of synth:'s
    (GOOD + ":early=65", "no value for early"),
    (GOOD + ":beta=0.8,", "is not key=value"),         # an empty item
    (GOOD + ":beta=0.8:gain=2", "room:LENGTH_S"),      # a sixth colon
])
def test_a_malformed_line_names_the_key(stub, line, names, tmp_path):
    """Exit status 2 and a message that quotes the line and names what is wrong with it, before any IR is loaded."""
    settings = _index(tmp_path, 16384, [], [line])
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"index line '{line}'" in res.stderr and names in res.stderr, res.stderr[-500:]
    assert "synth:LENGTH_S" not in res.stderr


def test_the_stub_host_links_and_says_the_engine_has_no_room(stub, tmp_path):
    """conv.cpp binds the room's entry points weakly: over an engine without them the host still links, and with a well-formed
    room: line stops when the client starts with a message that names what is missing."""
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _index(tmp_path, 16384, [], [LINE + ",order=3,last=0.05,t60=0.3,late=0.01,seed=7"])
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no room rendering (mc_synth_ir_room)" in res.stdout + res.stderr
