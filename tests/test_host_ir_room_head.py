"""C++ host: a `room:` line with a binaural listener (the keys head, headradius, ears and shadow of Convolution::parseRoom)
through `mcconv_host` against the oracle fed the restated taps, the log line with the ears' delays and shadow factors, each
malformed value refused by the name of its key, and the host over the stand-in engine of tests/stub, which has no head and must
say so."""
import os
import subprocess

import numpy as np
import pytest

import ir_room_head_np
import ir_room_np
from helpers import RMS_TOL, rms
from test_host_ir_room import HOST, RATE
from test_host_ir_synth import _index

LINE = "room:0.1:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8,gain=0.2,head=35,ears=100,headradius=0.09,shadow=0.8"
ROOM = dict(beta=0.8, gain=0.2)
HEAD = dict(facing=35.0, ear=100.0, radius=0.09, shadow=0.8)
FRAMES = 4800
LINE_B = "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2,head=-120,shadow=0.5"
ROOM_B = dict(size=(6.0, 5.0, 2.5), source=(2.0, 2.0, 1.0), receiver=(4.0, 3.0, 1.5), gain=0.2)
HEAD_B = dict(facing=-120.0, shadow=0.5)


@pytest.mark.gpu
def test_a_room_line_with_a_head(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    n_ref, period, nper = 16384, 512, 100
    settings = _index(tmp_path, n_ref, [], [LINE, LINE_B])  # (half h of the host selects IR h)
    taps, infos, plans = [], [], []
    for room, head in ((ROOM, HEAD), (ROOM_B, HEAD_B)):
        want, _, winfo = ir_room_head_np.frames64(room, None, None, head, RATE, frames=FRAMES, late_gain=0.0)
        ir_room_np.assert_floor_margin(winfo["tau"], FRAMES)
        taps.append(want.astype(np.float32))
        infos.append(winfo)
        plans.append(ir_room_head_np.plan(room, head, RATE, FRAMES))
    prefix = str(tmp_path / "head_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", str(RATE), "--period", str(period),
           "--dump", prefix]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    for j, (winfo, plan) in enumerate(zip(infos, plans)):
        line = (f"IR {j} head: the direct sound reaches the ears at {plan['direct'][0]:.2f} and {plan['direct'][1]:.2f} frames (right minus left "
                f"{plan['itd'] * 1e3:+.4f} ms), {plan['angle'][0]:.1f} and {plan['angle'][1]:.1f} degrees off their axes, shadow factors "
                f"{plan['shadow'][0]:+.4f} and {plan['shadow'][1]:+.4f}, shelf corner {plan['corner']:.0f} Hz")
        assert out.count(line) == 2, (line, out[-3000:])  # (each half loads the index)
        assert out.count(f"IR {j} room: order {winfo['order']}, {winfo['images'][0]} and {winfo['images'][1]} images before frame {FRAMES}") == 2
    ref = oracle_mod.RefCompat(n_ref, True)
    for j, t in enumerate(taps):
        ref.prepare(j, t)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want_out = ref.process(io[0], io[1], block=period)
    wet = want_out - 0.5 * (np.stack(io[:2]).astype(np.float64).sum(axis=0))  # (dry 0.5, panDry 0, level 1 in both halves)
    print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want_out):.4f}")
    assert 0.001 < np.abs(wet).max() < 0.5 and rms(want_out) > 0.01
    err = rms(np.stack(io[2:]) - want_out)
    print(f"room with a head: rms err {err:.3e}")
    assert err <= RMS_TOL


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


GOOD = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5"


@pytest.mark.parametrize("line,names", [
    (GOOD + ":head=north", "'north' is no value for head"),
    (GOOD + ":head=361", "no value for head"),
    (GOOD + ":head=10/20", "no value for head"),
    (GOOD + ":headradius=0.04", "no value for headradius"),
    (GOOD + ":headradius=0.2", "no value for headradius"),
    (GOOD + ":headradius=", "no value for headradius"),
    (GOOD + ":ears=59", "no value for ears"),
    (GOOD + ":ears=121", "no value for ears"),
    (GOOD + ":ears=nan", "no value for ears"),
    (GOOD + ":shadow=-0.1", "no value for shadow"),
    (GOOD + ":shadow=1.5", "no value for shadow"),
    (GOOD + ":shadow=deep", "no value for shadow"),
    (GOOD + ":head", "'head' is not key=value"),
    (GOOD + ":heads=35", "unknown key 'heads'"),
])
def test_a_malformed_value_names_the_key(stub, line, names, tmp_path):
    settings = _index(tmp_path, 16384, [], [line])
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"index line '{line}'" in res.stderr and names in res.stderr, res.stderr[-500:]


def test_the_form_names_the_new_keys(stub, tmp_path):
    settings = _index(tmp_path, 16384, [], ["room:"])
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60,
                         env=dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log")))
    assert res.returncode == 2
    for key in ("head", "headradius", "ears", "shadow"):
        assert f" {key}" in res.stderr, (key, res.stderr[-800:])


@pytest.mark.parametrize("keys", ["head=35,ears=100", "headradius=0.08", "shadow=0"])
def test_the_stub_host_says_the_engine_has_no_head(stub, keys, tmp_path):
    """conv.cpp binds the head's entry points weakly: over an engine without them the host still links, and a well-formed line
    with any of its keys stops when the client starts with a message that names what is missing."""
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _index(tmp_path, 16384, [], [GOOD + ":" + keys])
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no binaural listener in its rooms (mc_synth_ir_room_head)" in res.stdout + res.stderr
