"""C++ host: a `room:` line with directional microphones (the keys mic, aim, tilt, src, srcaim, srctilt of
Convolution::parseRoom) through `mcconv_host` against the oracle fed the restated taps, the log line with the direct sound's
factors, each malformed value refused by the name of its key, and the host over the stand-in engine of tests/stub, which has no
microphones and must say so."""
import os
import subprocess

import numpy as np
import pytest

import ir_room_mics_np
import ir_room_np
from helpers import RMS_TOL, rms
from test_host_ir_room import FRAMES, HOST, RATE
from test_host_ir_synth import _index

LINE = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8,gain=0.2,axis=y,mic=cardioid,aim=45/-45,spacing=0"
ROOM = dict(beta=0.8, gain=0.2, spacing=0.0, axis=1)
MICS = dict(pattern=0.5, az=(45.0, -45.0))
LINE_B = "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2,mic=fig8/0.75,tilt=10,aim=200,src=hypercardioid,srcaim=-30,srctilt=5"
ROOM_B = dict(size=(6.0, 5.0, 2.5), source=(2.0, 2.0, 1.0), receiver=(4.0, 3.0, 1.5), gain=0.2)
MICS_B = dict(pattern=(0.0, 0.75), az=200.0, el=10.0, source_pattern=0.25, source_az=-30.0, source_el=5.0)
FRAMES_B = 4800


@pytest.mark.gpu
def test_a_room_line_with_microphones(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    n_ref, period, nper = 16384, 512, 200
    settings = _index(tmp_path, n_ref, [], [LINE, LINE_B])
    taps, infos = [], []
    for room, mics, frames in ((ROOM, MICS, FRAMES), (ROOM_B, MICS_B, FRAMES_B)):
        ir_room_np.assert_floor_margin(ir_room_np.images(room, RATE, frames)["tau"], frames)
        want, _, winfo = ir_room_mics_np.frames64(room, mics, RATE, frames=frames, late_gain=0.0)
        taps.append(want.astype(np.float32))
        infos.append(winfo)
    prefix = str(tmp_path / "mics_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", str(RATE), "--period", str(period),
           "--dump", prefix]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    for j, (winfo, frames) in enumerate(zip(infos, (FRAMES, FRAMES_B))):
        m = winfo["mics"]
        line = (f"IR {j} microphones: the direct sound leaves the source at {m['source'][0]:.4f} and {m['source'][1]:.4f}, is received at "
                f"{m['receiver'][0]:.4f} and {m['receiver'][1]:.4f}, factors {m['factor'][0]:.4f} and {m['factor'][1]:.4f}")
        assert out.count(line) == 2, (line, out[-3000:])  # (each half loads the index)
        assert out.count(f"IR {j} room: order {winfo['order']}, {winfo['images'][0]} and {winfo['images'][1]} images before frame {frames}") == 2
    ref = oracle_mod.RefCompat(n_ref, True)
    for j, t in enumerate(taps):
        ref.prepare(j, t)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=period)
    wet = want - 0.5 * (np.stack(io[:2]).astype(np.float64).sum(axis=0))  # (dry 0.5, panDry 0, level 1 in both halves)
    print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert 0.001 < np.abs(wet).max() < 0.5 and rms(want) > 0.01
    err = rms(np.stack(io[2:]) - want)
    print(f"room with microphones: rms err {err:.3e}")
    assert err <= RMS_TOL


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


GOOD = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5"


@pytest.mark.parametrize("line,names", [
    (GOOD + ":mic=shotgun", "'shotgun' is no value for mic"),
    (GOOD + ":mic=1.5", "no value for mic"),
    (GOOD + ":mic=cardioid/", "no value for mic"),
    (GOOD + ":mic=0.5/0.5/0.5", "no value for mic"),
    (GOOD + ":aim=north", "no value for aim"),
    (GOOD + ":aim=45/-361", "no value for aim"),
    (GOOD + ":tilt=91", "no value for tilt"),
    (GOOD + ":tilt=10/nan", "no value for tilt"),
    (GOOD + ":src=-0.1", "no value for src"),
    (GOOD + ":src=cardioid/cardioid", "no value for src"),
    (GOOD + ":srcaim=400", "no value for srcaim"),
    (GOOD + ":srcaim=1/2", "no value for srcaim"),
    (GOOD + ":srctilt=-90.5", "no value for srctilt"),
    (GOOD + ":srctilt=up", "no value for srctilt"),
    (GOOD + ":mic", "'mic' is not key=value"),
    (GOOD + ":mics=cardioid", "unknown key 'mics'"),
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
    for key in ("mic", "aim", "tilt", "src", "srcaim", "srctilt"):
        assert f" {key}" in res.stderr, (key, res.stderr[-800:])


@pytest.mark.parametrize("keys", ["mic=cardioid,aim=45/-45,spacing=0", "src=cardioid", "srctilt=0"])
def test_the_stub_host_says_the_engine_has_no_microphones(stub, keys, tmp_path):
    """conv.cpp binds the microphones' entry points weakly: over an engine without them the host still links, and a
    well-formed line with any of their keys stops when the client starts with a message that names what is missing."""
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _index(tmp_path, 16384, [], [GOOD + ":" + keys])
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no directional microphones in its rooms (mc_synth_ir_room_mics)" in res.stdout + res.stderr
