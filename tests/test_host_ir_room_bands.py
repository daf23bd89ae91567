"""C++ host: a `room:` line with walls and air per frequency band (the keys xover, betas and air of Convolution::parseRoom)
through `mcconv_host` against the oracle fed the restated taps, the log line with the bands' reverberation times, each malformed
value refused by the name of its key, and the host over the stand-in engine of tests/stub, which has no bands and must say so."""
import os
import subprocess

import numpy as np
import pytest

import ir_room_bands_np
import ir_room_np
from helpers import RMS_TOL, rms
from test_host_ir_room import FRAMES, HOST, RATE
from test_host_ir_synth import _index

LINE = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5:gain=0.2,spacing=0.3,axis=y,xover=500/2000,betas=0.9/0.8/0.6,air=0/0.005/0.03"
ROOM = dict(gain=0.2, spacing=0.3, axis=1)
BANDS = dict(xovers=(500.0, 2000.0), beta=(0.9, 0.8, 0.6), air=(0.0, 0.005, 0.03))
# one value of air for both bands, the walls' six values of beta in every band, and microphones
LINE_B = "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2,beta=0.9/0.8/0.7/0.95/0.6/0.85,air=0.02,xover=1000,mic=cardioid,aim=45/-45"
ROOM_B = dict(size=(6.0, 5.0, 2.5), source=(2.0, 2.0, 1.0), receiver=(4.0, 3.0, 1.5), gain=0.2)
BANDS_B = dict(xovers=(1000.0,), beta=((0.9, 0.8, 0.7, 0.95, 0.6, 0.85),) * 2, air=0.02)
MICS_B = dict(pattern=0.5, az=(45.0, -45.0))
FRAMES_B = 4800


def _times(values):
    return " / ".join(f"{v:.3f}" for v in values)


@pytest.mark.gpu
def test_a_room_line_with_bands(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    n_ref, period, nper = 16384, 512, 200
    settings = _index(tmp_path, n_ref, [], [LINE, LINE_B])
    taps, infos, plans = [], [], []
    for room, mics, bands, frames in ((ROOM, None, BANDS, FRAMES), (ROOM_B, MICS_B, BANDS_B, FRAMES_B)):
        want, _, winfo = ir_room_bands_np.frames64(room, mics, bands, RATE, frames=frames, late_gain=0.0)
        ir_room_np.assert_floor_margin(winfo["tau"], frames)
        taps.append(want.astype(np.float32))
        infos.append(winfo)
        plans.append(ir_room_bands_np.plan(room, bands, RATE, frames))
    prefix = str(tmp_path / "bands_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", str(RATE), "--period", str(period),
           "--dump", prefix]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    for j, (winfo, plan, frames) in enumerate(zip(infos, plans, (FRAMES, FRAMES_B))):
        line = f"IR {j} bands: {plan['bands']}, low to high Sabine {_times(plan['sabine'])} s, Eyring {_times(plan['eyring'])} s"
        assert out.count(line) == 2, (line, out[-3000:])  # (each half loads the index)
        assert out.count(f"IR {j} room: order {winfo['order']}, {winfo['images'][0]} and {winfo['images'][1]} images before frame {frames}") == 2
    assert out.count("IR 1 microphones:") == 2 and out.count("IR 0 microphones:") == 0
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
    print(f"room with bands: rms err {err:.3e}")
    assert err <= RMS_TOL


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


GOOD = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5"


def _run(stub, line, tmp_path):
    settings = _index(tmp_path, 16384, [], [line])
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    return subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60,
                          env=env)


@pytest.mark.parametrize("line,names", [
    (GOOD + ":xover=low", "'low' is no value for xover"),
    (GOOD + ":xover=5", "no value for xover"),
    (GOOD + ":xover=500/", "no value for xover"),
    (GOOD + ":xover=2000/500", "no value for xover"),
    (GOOD + ":xover=500/500", "no value for xover"),
    (GOOD + ":xover=100/200/300/400", "no value for xover"),
    (GOOD + ":xover=nan", "no value for xover"),
    (GOOD + ":betas=1.5", "no value for betas"),
    (GOOD + ":betas=hard", "no value for betas"),
    (GOOD + ":betas=0.9/0.8", "'0.9/0.8' is no value for betas"),  # (two values, one band)
    (GOOD + ":betas=0.9/0.8/0.7,xover=500", "'0.9/0.8/0.7' is no value for betas"),
    (GOOD + ":xover=500/2000,betas=0.9", "'0.9' is no value for betas"),
    (GOOD + ":betas=0.9/0.8/0.7/0.6/0.5", "no value for betas"),
    (GOOD + ":air=-0.1", "no value for air"),
    (GOOD + ":air=1.5", "no value for air"),
    (GOOD + ":air=thin", "no value for air"),
    (GOOD + ":air=0/0.1", "'0/0.1' is no value for air"),
    (GOOD + ":xover=500/2000,air=0/0.1", "'0/0.1' is no value for air"),
    (GOOD + ":xover", "'xover' is not key=value"),
    (GOOD + ":xovers=500", "unknown key 'xovers'"),
])
def test_a_malformed_value_names_the_key(stub, line, names, tmp_path):
    res = _run(stub, line, tmp_path)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"index line '{line}'" in res.stderr and names in res.stderr, res.stderr[-500:]


def test_the_form_names_the_new_keys(stub, tmp_path):
    res = _run(stub, "room:", tmp_path)
    assert res.returncode == 2
    for key in ("xover", "betas", "air"):
        assert f" {key} " in res.stderr, (key, res.stderr[-800:])


@pytest.mark.parametrize("keys", ["xover=500/2000,betas=0.9/0.8/0.6,air=0/0.005/0.03", "air=0.01", "betas=0.8", "xover=1000,mic=cardioid"])
def test_the_stub_host_says_the_engine_has_no_bands(stub, keys, tmp_path):
    """conv.cpp binds the bands' entry points weakly: over an engine without them the host still links, and a well-formed line
    with any of their keys stops when the client starts with a message that names what is missing."""
    res = _run(stub, GOOD + ":" + keys, tmp_path)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no frequency bands in its rooms (mc_synth_ir_room_bands)" in res.stdout + res.stderr
