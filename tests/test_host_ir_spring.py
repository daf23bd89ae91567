"""C++ host: `mcconv_host` over an index with `spring:` lines at --rate 48000 (Convolution::prepareSpring: the line's Hz,
milliseconds and seconds, the tank's response evaluated by the engine when the client starts), one line with every key and one
with two; the malformed lines the index grammar refuses, each with the form or the key in the message; and the host over the
stand-in engine of tests/stub, which has no spring synthesis and must say so."""
import os
import subprocess

import numpy as np
import pytest

import ir_spring_np as sp
from helpers import RMS_TOL, rms
from test_host_ir_synth import _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE = 48000
LINE = ("spring:0.15:sections=40,fc=3000,a=0.5,delay=21,27.5,33,t60=0.4,damping=0.1,lowpass=4,high=0.2,highsections=60,higha=-0.5,highdelay=0.4,hight60=0.2,"
        "stereo=0.05,gain=0.02,points=14,last=0.1")
SPRING = dict(sections=40, transition_hz=3000.0, dispersion=0.5, delay_ms=(21.0, 27.5, 33.0), t60=0.4, damping=0.1, lowpass_order=4, high_gain=0.2, high_sections=60,
              high_dispersion=-0.5, high_delay=0.4, high_t60=0.2, stereo=0.05, gain=0.02, log2_points=14, last=4800)  # the line; 0.1 s at 48000 Hz is 4800 frames
FRAMES = 7200
LINE_B = "spring:0.1:gain=0.02,delay=30"  # half 1's IR: the default tank with one spring of 30 ms
SPRING_B = dict(gain=0.02, delay_ms=(30.0,))
FRAMES_B = 4800


def _spring_line(idx, plan):
    delays = ", ".join(f"{l}/{r}" for l, r in plan["L"])
    return (f"IR {idx} spring: {plan['N']} points, K {plan['K']} (transition {plan['ft']:.1f} Hz), {plan['M']} sections, low-pass {'in' if plan['bq'] else 'out'}, "
            f"{plan['S']} springs with delays {delays} frames (L/R), before frame {plan['E']}, alias bound {plan['alias_db']:.1f} dB")


@pytest.mark.gpu
def test_spring_lines(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    n_ref, period, nper = 16384, 512, 200
    settings = _index(tmp_path, n_ref, [], [LINE, LINE_B])
    spring, plan = sp.spring64(RATE, FRAMES, **SPRING)
    spring_b, plan_b = sp.spring64(RATE, FRAMES_B, **SPRING_B)
    assert (plan["N"], plan["E"], plan["S"], plan["K"]) == (16384, 4800, 3, 8) and (plan_b["N"], plan_b["S"]) == (16384, 1) and not spring[4800:].any()
    prefix = str(tmp_path / "spring_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", str(RATE), "--period", str(period),
           "--dump", prefix]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    # one line per spring per half (each half loads the index)
    assert out.count(_spring_line(0, plan)) == 2 and out.count(_spring_line(1, plan_b)) == 2, out[-3000:]
    assert out.count(f"IR 0 synthesised: {FRAMES} frames, seed 0, 0 of 0 reflections kept") == 2
    ref = oracle_mod.RefCompat(n_ref, True)
    for j, t in enumerate((spring, spring_b)):
        ref.prepare(j, t.astype(np.float32))
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=period)
    x = np.stack(io[:2]).astype(np.float64)
    wet = want - 0.5 * (x[0] + x[1])  # (dry 0.5, panDry 0, level 1 in both halves)
    print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert np.abs(wet).max() < 0.5 and rms(want) > 0.01 and rms(wet) > 1e-3
    err = rms(np.stack(io[2:]) - want)
    print(f"springs: rms err {err:.3e}")
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


GOOD = "spring:0.2"


@pytest.mark.parametrize("line,names", [
    ("spring:", "LENGTH_S ''"),                               # nothing
    ("spring:abc", "LENGTH_S 'abc'"),
    ("spring:0", "LENGTH_S '0'"),
    ("spring:-1", "LENGTH_S '-1'"),
    (GOOD + ":", "nothing after the last colon"),             # an empty list
    (GOOD + ":delay", "'delay' is not key=value"),
    (GOOD + ":delay=", "no value for delay"),
    (GOOD + ":delay=66,x", "no value for delay"),
    (GOOD + ":delay=66,82,91,100", "no value for delay"),     # four springs: three
    (GOOD + ":delay=66,0", "no value for delay"),             # (an absent spring is one that is not named)
    (GOOD + ":delay=66/82", "no value for delay"),
    (GOOD + ":sections=many", "no value for sections"),
    (GOOD + ":sections=1.5", "no value for sections"),
    (GOOD + ":sections=-1", "no value for sections"),
    (GOOD + ":fc=nan", "no value for fc"),
    (GOOD + ":a=-0.5", "no value for a"),
    (GOOD + ":t60=inf", "no value for t60"),
    (GOOD + ":damping=-0.1", "no value for damping"),
    (GOOD + ":lowpass=x", "no value for lowpass"),
    (GOOD + ":high=-1", "no value for high"),
    (GOOD + ":highsections=2.5", "no value for highsections"),
    (GOOD + ":higha=0.5", "no value for higha"),              # the high dispersion is at most 0
    (GOOD + ":highdelay=", "no value for highdelay"),
    (GOOD + ":hight60=-1", "no value for hight60"),
    (GOOD + ":stereo=wide", "no value for stereo"),
    (GOOD + ":gain=1,5", "no value for gain"),
    (GOOD + ":points=-3", "no value for points"),
    (GOOD + ":last=-1", "no value for last"),
    (GOOD + ":colour=3", "unknown key 'colour'"),
    (GOOD + ":late=0.1", "unknown key 'late'"),               # a key of synth:'s: a spring has no late field under it
    (GOOD + ":gain=0.5,", "'' is not key=value"),             # an empty item
    (GOOD + ":,gain=0.5", "'' is not key=value"),
    (GOOD + ":gain=0.5:fc=3000", "spring:LENGTH_S"),          # a third colon
])
def test_a_malformed_line_names_the_key(stub, line, names, tmp_path):
    """Exit status 2 and a message that quotes the line and names what is wrong with it, before any IR is loaded."""
    res = _run_stub(stub, tmp_path, line)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"index line '{line}'" in res.stderr and names in res.stderr, res.stderr[-500:]


@pytest.mark.parametrize("line", [GOOD, LINE, LINE_B, GOOD + ":delay=66,82,91,t60=0", GOOD + ":high=0,lowpass=0,points=20"])
def test_the_stub_host_links_and_says_the_engine_has_no_spring(stub, line, tmp_path):
    """conv.cpp binds the spring's entry points weakly: over an engine without them the host still links, and with a well-formed
    spring: line (every key among them) it stops when the client starts with a message that names what is missing."""
    res = _run_stub(stub, tmp_path, line)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no spring synthesis (mc_synth_ir_spring)" in res.stdout + res.stderr
    assert "index line" not in res.stderr
