"""C++ host: `mcconv_host` over an index with `plate:` lines at --rate 48000 (Convolution::preparePlate: the line's metres,
millimetres, Hz and seconds, the plate's modes summed by the engine when the client starts), one line with every key and one with
two; the malformed lines the index grammar refuses, each with the form or the key in the message; and the host over the stand-in
engine of tests/stub, which has no plate synthesis and must say so."""
import os
import subprocess

import numpy as np
import pytest

import ir_plate_np
from helpers import RMS_TOL, rms
from test_host_ir_synth import _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE = 48000
LINE = "plate:0.15:size=1.5,0.8,thick=1,material=70/2700/0.33,drive=0.5,0.3,pick=0.2,0.2/1.2,0.6,low=30,high=1200,t60=0.5/0.1,damp=1200,gain=0.02,last=0.1"
PLATE = dict(size=(1.5, 0.8), thickness_mm=1.0, material=(70.0, 2700.0, 0.33), driver=(0.5, 0.3), pickups=((0.2, 0.2), (1.2, 0.6)), low_hz=30.0, high_hz=1200.0,
             t60=(0.5, 0.1), damp_hz=1200.0, gain=0.02, last=4800)  # the line; 0.15 s at 48000 Hz is 7200 frames, 0.1 s 4800
FRAMES = 7200
LINE_B = "plate:0.1:gain=0.02,high=400"  # half 1's IR: the default plate cut at 400 Hz
PLATE_B = dict(gain=0.02, high_hz=400.0)
FRAMES_B = 4800


def _plate_line(idx, info):
    return (f"IR {idx} plate: {info['modes']} modes from {info['lowest']:.2f} to {info['highest']:.2f} Hz, {info['sounding'][0]} and {info['sounding'][1]} "
            f"sounding, before frame {info['last']}, kappa {info['kappa']:.4f} m^2/s")


@pytest.mark.gpu
def test_plate_lines(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    n_ref, period, nper = 16384, 512, 200
    settings = _index(tmp_path, n_ref, [], [LINE, LINE_B])
    plate, winfo = ir_plate_np.frames(PLATE, RATE, frames=FRAMES, late_gain=0.0)
    plate_b, winfo_b = ir_plate_np.frames(PLATE_B, RATE, frames=FRAMES_B, late_gain=0.0)
    assert winfo["modes"] > 300 and winfo["last"] == 4800 and winfo_b["modes"] == 472 and not plate[4800:].any()
    prefix = str(tmp_path / "plate_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", str(RATE), "--period", str(period),
           "--dump", prefix]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    # one line per plate per half (each half loads the index)
    assert out.count(_plate_line(0, winfo)) == 2 and out.count(_plate_line(1, winfo_b)) == 2, out[-3000:]
    assert out.count(f"IR 0 synthesised: {FRAMES} frames, seed 0, 0 of 0 reflections kept") == 2
    ref = oracle_mod.RefCompat(n_ref, True)
    for j, t in enumerate((plate, plate_b)):
        ref.prepare(j, t)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=period)
    x = np.stack(io[:2]).astype(np.float64)
    wet = want - 0.5 * (x[0] + x[1])  # (dry 0.5, panDry 0, level 1 in both halves)
    print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert np.abs(wet).max() < 0.5 and rms(want) > 0.01 and rms(wet) > 1e-3
    err = rms(np.stack(io[2:]) - want)
    print(f"plates: rms err {err:.3e}")
    assert err <= RMS_TOL


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


def _run_stub(stub, tmp_path, line):
    settings = _index(tmp_path, 16384, [], [line])
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    return subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                          timeout=60, env=env)


GOOD = "plate:0.2"


@pytest.mark.parametrize("line,names", [
    ("plate:", "LENGTH_S ''"),                              # nothing
    ("plate:abc", "LENGTH_S 'abc'"),
    ("plate:0", "LENGTH_S '0'"),
    ("plate:-1", "LENGTH_S '-1'"),
    (GOOD + ":", "nothing after the last colon"),           # an empty list
    (GOOD + ":size", "'size' is not key=value"),
    (GOOD + ":size=2", "no value for size"),                # one number: two
    (GOOD + ":size=2,1,3", "no value for size"),
    (GOOD + ":size=2,x", "no value for size"),
    (GOOD + ":thick=thin", "no value for thick"),
    (GOOD + ":thick=-1", "no value for thick"),
    (GOOD + ":material=brass", "no value for material"),
    (GOOD + ":material=200/7850", "no value for material"),
    (GOOD + ":drive=0.5", "no value for drive"),
    (GOOD + ":drive=0.5/0.4", "no value for drive"),
    (GOOD + ":pick=0.3,0.6", "no value for pick"),          # one pickup: two
    (GOOD + ":pick=0.3,0.6/1.5", "no value for pick"),
    (GOOD + ":pick=0.3/0.6/1.5/0.3", "no value for pick"),
    (GOOD + ":low=nan", "no value for low"),
    (GOOD + ":high=-400", "no value for high"),
    (GOOD + ":t60=4", "no value for t60"),                  # one time: two
    (GOOD + ":t60=4,1", "no value for t60"),
    (GOOD + ":t60=4/-1", "no value for t60"),
    (GOOD + ":damp=inf", "no value for damp"),
    (GOOD + ":gain=1,5", "no value for gain"),
    (GOOD + ":last=-1", "no value for last"),
    (GOOD + ":colour=3", "unknown key 'colour'"),
    (GOOD + ":late=0.1", "unknown key 'late'"),             # a key of synth:'s: a plate has no late field under it
    (GOOD + ":gain=0.5,", "'' is not key=value"),           # an empty item
    (GOOD + ":,gain=0.5", "'' is not key=value"),
    (GOOD + ":gain=0.5:low=30", "plate:LENGTH_S"),          # a third colon
])
def test_a_malformed_line_names_the_key(stub, line, names, tmp_path):
    """Exit status 2 and a message that quotes the line and names what is wrong with it, before any IR is loaded."""
    res = _run_stub(stub, tmp_path, line)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"index line '{line}'" in res.stderr and names in res.stderr, res.stderr[-500:]


@pytest.mark.parametrize("line", [GOOD, LINE, LINE_B, GOOD + ":material=steel,t60=0/0", GOOD + ":size=2,1,drive=0.5,0.25,gain=2"])
def test_the_stub_host_links_and_says_the_engine_has_no_plate(stub, line, tmp_path):
    """conv.cpp binds the plate's entry points weakly: over an engine without them the host still links, and with a well-formed
    plate: line (every key among them) it stops when the client starts with a message that names what is missing."""
    res = _run_stub(stub, tmp_path, line)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no plate synthesis (mc_synth_ir_plate)" in res.stdout + res.stderr
    assert "index line" not in res.stderr
