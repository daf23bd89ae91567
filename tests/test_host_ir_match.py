"""C++ host: `mcconv_host --ir-match FILE.wav|flat[:amount=,boost=,cut=,smooth=,lo=,hi=,link=0,phase=linear,delay=,tilt=]` and
`--ir-match-report` (Convolution::setIrMatch): the option grammar and what it refuses, the host over the stand-in engine of
tests/stub, which has no match step and must say so, and on the device the summary line, the report's lines against the curve
that Python gets for the same load, and the output against the oracle fed the taps of that load."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_match_np as MN
from helpers import RMS_TOL, rms
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 60
LINE = re.compile(r"IR (\d+) matched to (\S+): (\d+) frames and (\d+) target frames through a transform of (\d+) points, (\d+) frames kept, (\d+) points, "
                  r"gain ([-+0-9.]+) \.\. ([-+0-9.]+) dB, (\d+) clamped, level ([-+0-9.]+) dB")
POINT = re.compile(r"IR (\d+) match ([0-9.]+) Hz: before ([-+0-9.]+) ([-+0-9.]+) dB, gain ([-+0-9.]+) ([-+0-9.]+) dB")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("tail", ["", ":", ":amount", ":amount=", ":=1", ":amount=2", ":amount=-0.1", ":boost=61", ":cut=abc", ":smooth=0.01", ":smooth=3", ":lo=0.5",
                                  ":lo=500,hi=400", ":link=2", ":phase=maximum", ":delay=-1", ":delay=inf", ":tilt=13", ":tilt=nan", ":colour=3", ":amount=1,",
                                  ":amount=1:boost=3"])
@pytest.mark.parametrize("target", ["t.wav", "flat"])
def test_a_malformed_match_is_refused(stub, tmp_path, tail, target):
    """Exit status 2 and a message that names the option and quotes the argument, before a device, the target's file or the settings
    are looked at (an empty argument names no file)."""
    arg = target + tail if tail else ""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-match", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-match '{arg}'" in res.stderr and "FILE.wav|flat[:key=value,...]" in res.stderr


def test_a_target_file_that_is_not_there_is_refused(stub, tmp_path):
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-match", "nowhere.wav:amount=0.5"], capture_output=True, text=True,
                         cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2 and "cannot open nowhere.wav" in res.stderr


@pytest.mark.parametrize("arg", ["t.wav", "flat", "t.wav:amount=0.5,boost=6,cut=9,smooth=0.5,lo=30,hi=3000,link=0,phase=linear,delay=0.01", "flat:tilt=-3,link=1,phase=minimum"])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, arg):
    """conv.cpp binds the match entry points weakly: over an engine without them the host still links, runs as before, and with a
    well-formed option stops when the client starts with a message that names what is missing."""
    wavs = [("ir_a.wav", MN.decaying_noise(600, 1), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    _write_wav16(str(tmp_path / "t.wav"), MN.decaying_noise(400, 2), RATE)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _settings(tmp_path, N_REF, wavs)
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", str(RATE)]
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(base + ["--ir-match", arg, "--ir-match-report"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no match step (mc_load_ir_match)" in res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("arg,kw", [("t.wav", dict()), ("t.wav:amount=0.5,boost=3,cut=4,smooth=0.5,lo=40,hi=3500,link=0", dict(amount=0.5, boost_db=3.0, cut_db=4.0,
                                                                                                                             octaves=0.5, lo=40.0, hi=3500.0, link=False)),
                                    ("flat:tilt=-3,phase=linear,delay=0.01", dict(tilt_db=-3.0, phase="linear", delay=80))])
def test_the_report_lines_and_the_output(oracle_mod, tmp_path, arg, kw):
    """The target WAV is at 11025 Hz in a session at 8000.  The summary line and every line of the report against what Python's
    prepare(match=) reports of the decoded WAVs (tests/test_gpu_ir_match.py checks that against the restatement), the dumped
    output against the oracle fed the taps of those loads."""
    from cuda_audio_amd.engine import Convolution, IrMatch

    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", MN.coloured_noise(3000, 1, level=0.05), RATE), ("ir_b.wav", MN.coloured_noise(1000, 4, level=0.05), RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    tdec = _write_wav16(str(tmp_path / "t.wav"), MN.decaying_noise(2000, 2, right=1.0 / 3.0), 11025)
    flat = arg.startswith("flat")
    c = Convolution("hostmatch", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)
    loads = []
    for j, d in enumerate(decoded):
        c.prepare(j, d, nframes=PERIOD, match=IrMatch(ir=None if flat else tdec, rate=None if flat else 11025, **kw))
        loads.append((c.ir_taps(j), c.ir_match_info(j), c.ir_match_curve(j)))
    c.close()
    settings = _settings(tmp_path, N_REF, wavs)
    prefix = str(tmp_path / "match_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
           "--dump", prefix, "--ir-match", arg, "--ir-match-report"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == NPER * PERIOD for a in io)
    lines, points = LINE.findall(out), POINT.findall(out)
    assert len(lines) == 2 * len(wavs), out[-3000:]  # (each half loads the index)
    for j, (taps, info, curve) in enumerate(loads):
        mine = [l for l in lines if int(l[0]) == j]
        assert len(mine) == 2
        level = 10.0 * np.log10(info["energy_out"] / info["energy_in"])
        for l in mine:
            assert l[1] == ("flat" if flat else "t.wav")
            assert (int(l[2]), int(l[3]), int(l[4]), int(l[5]), int(l[6]), int(l[9])) == (info["frames"], info["target_frames"], info["nfft"], info["frames_out"],
                                                                                        info["points"], info["clamped"])
            assert abs(float(l[7]) - curve["gain_db"].min()) <= 5e-3 + 1e-6 and abs(float(l[8]) - curve["gain_db"].max()) <= 5e-3 + 1e-6
            assert abs(float(l[10]) - level) <= 5e-3 + 1e-6
        rows = np.array([[float(v) for v in p[1:]] for p in points if int(p[0]) == j])
        J = info["points"]
        assert rows.shape == (2 * J, 5)
        for half in range(2):
            r = rows[half * J:(half + 1) * J]
            assert np.abs(r[:, 0] - curve["hz"]).max() <= 5e-4 + 1e-9
            assert np.abs(r[:, 1:3] - curve["before_db"]).max() <= 5e-5 + 1e-9 and np.abs(r[:, 3:5] - curve["gain_db"]).max() <= 5e-5 + 1e-9
    ref = oracle_mod.RefCompat(N_REF, True)
    for j, (taps, _, _) in enumerate(loads):
        ref.prepare(j, taps)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=PERIOD)
    err = rms(np.stack(io[2:]) - want)
    print(f"rms err {err:.3e} of {rms(want):.3e}")
    assert err <= RMS_TOL
