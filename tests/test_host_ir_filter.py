"""C++ host: `mcconv_host --ir-filter FILE.wav[:op=deconvolve,channels=mid,reg=DB,keep=SECONDS]` (Convolution::setIrFilter): the
option grammar and what it refuses, the host over the stand-in engine of tests/stub, which has no filter step and must say so,
and on the device the report line and the output against the oracle fed the restatement (tests/ir_filter_np.py) of the decoded
WAVs, the filter at a rate of its own."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_filter_np as FN
from helpers import RMS_TOL, rms
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 60
LINE = re.compile(r"IR (\d+) (convolved with|deconvolved by) (\S+): (\d+) frames and (\d+) filter frames through a transform of (\d+) points, (\d+) frames kept, "
                  r"level ([-+0-9.]+) dB, ([-0-9.]+) dB left behind, (\d+) and (\d+) bins regularised")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("tail", ["", ":", ":op", ":op=", ":=deconvolve", ":op=divide", ":channels=right", ":reg=abc", ":reg=19", ":reg=201", ":reg=nan", ":keep=0",
                                  ":keep=-1", ":keep=inf", ":colour=3", ":op=convolve,", ":op=convolve:reg=60"])
def test_a_malformed_filter_is_refused(stub, tmp_path, tail):
    """Exit status 2 and a message that quotes the argument, before a device or the settings are looked at (an empty argument
    names no file)."""
    arg = "f.wav" + tail if tail else ""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-filter", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-filter '{arg}'" in res.stderr and "FILE.wav[:key=value,...]" in res.stderr


def test_a_filter_file_that_is_not_there_is_refused(stub, tmp_path):
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-filter", "nowhere.wav:op=deconvolve"], capture_output=True, text=True,
                         cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2 and "cannot open nowhere.wav" in res.stderr


@pytest.mark.parametrize("tail", ["", ":op=deconvolve,channels=mid,reg=90.5,keep=0.25", ":channels=left"])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, tail):
    """conv.cpp binds the filter entry points weakly: over an engine without them the host still links, runs as before, and with a
    well-formed option stops when the client starts with a message that names what is missing."""
    wavs = [("ir_a.wav", FN.decaying_noise(600, 1), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    _write_wav16(str(tmp_path / "f.wav"), FN.decaying_noise(40, 2), RATE)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _settings(tmp_path, N_REF, wavs)
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", str(RATE)]
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(base + ["--ir-filter", "f.wav" + tail], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no filter step (mc_load_ir_filter)" in res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("opts,kw", [("", dict()), (":op=deconvolve,channels=mid,reg=40,keep=0.25", dict(op="deconvolve", channels="mid", reg_db=40.0, frames_out=2000))])
def test_the_report_line_and_the_output(oracle_mod, tmp_path, opts, kw):
    """The filter WAV is at 11025 Hz in a session at 8000: the restatement is fed what the engine itself stores of that file
    loaded alone with the conversion (tests/test_gpu_ir_filter.py checks that path against its own restatement)."""
    from cuda_audio_amd.engine import Convolution

    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", FN.decaying_noise(3000, 1, level=0.05), RATE), ("ir_b.wav", FN.decaying_noise(1000, 4, level=0.05), RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    lift = FN.decaying_noise(400, 2, right=1.0 / 3.0).copy()
    lift[0] += np.float32(0.4)
    fdec = _write_wav16(str(tmp_path / "f.wav"), lift, 11025)
    c = Convolution("hostfilter", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)
    c.prepare(0, fdec, ir_rate=11025)
    f8k = c.ir_taps(0)
    c.close()
    settings = _settings(tmp_path, N_REF, wavs)
    prefix = str(tmp_path / "filter_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
           "--dump", prefix, "--ir-filter", "f.wav" + opts]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == NPER * PERIOD for a in io)
    restated = [FN.filtered(d, f8k, **kw) for d in decoded]
    lines = LINE.findall(out)
    assert len(lines) == 2 * len(wavs), out[-3000:]  # (each half loads the index)
    for j, (taps, info) in enumerate(restated):
        mine = [l for l in lines if int(l[0]) == j]
        assert len(mine) == 2
        level = 10.0 * np.log10(info["energy_out"] / info["energy_in"])
        for l in mine:
            assert l[1] == ("deconvolved by" if kw else "convolved with") and l[2] == "f.wav"
            assert (int(l[3]), int(l[4]), int(l[5]), int(l[6])) == (info["frames"], info["filter_frames"], info["nfft"], info["frames_out"])
            assert abs(float(l[7]) - level) <= 5e-3 + 1e-6 and (int(l[9]), int(l[10])) == tuple(info["regularised"])
    ref = oracle_mod.RefCompat(N_REF, True)
    for j, (taps, _) in enumerate(restated):
        ref.prepare(j, taps)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=PERIOD)
    err = rms(np.stack(io[2:]) - want)
    print(f"rms err {err:.3e} of {rms(want):.3e}")
    assert err <= RMS_TOL
