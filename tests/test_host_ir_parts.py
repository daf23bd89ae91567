"""C++ host: `mcconv_host --ir-parts direct=DB|off,early=DB|off,late=DB|off[,split=SECONDS|mix,first=,onset=,xfade=S:S,delay=S:S:S,
width=,balance=,swap,invert=]` (Convolution::setIrParts): the option grammar and what it refuses, the host over the stand-in engine
of tests/stub, which has no parts step and must say so, and on the device the summary line against what Python gets for the same
load, and the output against the oracle fed the taps of that load."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_parts_np as PN
from helpers import RMS_TOL, rms
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 60
NUM = r"([-+0-9.e]+)"
LINE = re.compile(rf"IR (\d+) parts: (\d+) frames in, (\d+) out, direct to (\d+), early to (\d+)( \(the mixing tap\))?, energies {NUM} / {NUM} / {NUM}, "
                  rf"direct to reverberant {NUM} dB, level {NUM} dB, (\d+) contributions lost \({NUM}\)")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("arg", ["", ",", "direct", "direct=", "=3", "direct=25", "early=-121", "late=loud", "late=nan", "direct=off,early=off,late=off", "split=-1",
                                 "split=soon", "split=0.001", "first=abc", "onset=-0.1", "xfade=0.01", "xfade=0.01:0.01:0.01", "xfade=0.01:-1", "delay=0.1",
                                 "delay=0:0:11", "delay=0:0:x", "width=2.5", "width=1:1", "width=1:1:-1", "balance=1.5", "balance=0:0:0:0", "swap=middle",
                                 "invert=direct:", "colour=3", "direct=0,", "direct=0,,late=0", "swap=early,invert=late:tail"])
def test_a_malformed_option_is_refused(stub, tmp_path, arg):
    """Exit status 2 and a message that names the option and quotes the argument, before a device or the settings are looked at."""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-parts", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-parts '{arg}'" in res.stderr and "key=value,..." in res.stderr


@pytest.mark.parametrize("arg", ["direct=off", "direct=-3,early=-4,late=2,split=0.05,first=0.002,onset=0.001,xfade=0.001:0.01,delay=0:0.001:-0.002,width=1:0.3:1.7,"
                                               "balance=0.25,swap,invert=direct:late", "early=off,split=mix"])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, arg):
    """conv.cpp binds the parts entry points weakly: over an engine without them the host still links, runs as before, and with a
    well-formed option stops when the client starts with a message that names what is missing."""
    wavs = [("ir_a.wav", PN.noise(600, 1), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _settings(tmp_path, N_REF, wavs)
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", str(RATE)]
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(base + ["--ir-parts", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no parts step (mc_load_ir_parts)" in res.stdout + res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("arg,kw", [
    ("direct=off", dict(direct_end=20, early_end=640, mute=("direct",))),
    ("direct=-3,early=-4,late=2,split=0.05,first=0.002,onset=0.001,xfade=0.001:0.01,delay=0:0.001:-0.002,width=1:0.3:1.7,balance=0.25,swap=early,invert=direct:late",
     dict(direct_end=8 + 16, early_end=8 + 400, xfade=(8, 80), delay=(0, 8, -16), gain_db=(-3.0, -4.0, 2.0), width=(1.0, 0.3, 1.7), balance=0.25, swap=("early",),
          invert=("direct", "late")))])
def test_the_summary_line_and_the_output(oracle_mod, tmp_path, arg, kw):
    """The summary line against what Python's prepare(parts=) reports of the decoded WAVs (tests/test_gpu_ir_parts.py checks that
    against the restatement), the dumped output against the oracle fed the taps of those loads."""
    from cuda_audio_amd.engine import Convolution, IrParts

    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", PN.noise(3000, 1, level=0.05), RATE), ("ir_b.wav", PN.noise(1000, 4, level=0.05), RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    c = Convolution("hostparts", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)
    loads = []
    for j, d in enumerate(decoded):
        c.prepare(j, d, nframes=PERIOD, parts=IrParts(**kw))
        loads.append((c.ir_taps(j), c.ir_parts_info(j)))
    c.close()
    settings = _settings(tmp_path, N_REF, wavs)
    prefix = str(tmp_path / "parts_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
           "--dump", prefix, "--ir-parts", arg]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == NPER * PERIOD for a in io)
    lines = LINE.findall(out)
    assert len(lines) == 2 * len(wavs), out[-3000:]  # (each half loads the index)
    for j, (taps, info) in enumerate(loads):
        mine = [l for l in lines if int(l[0]) == j]
        assert len(mine) == 2
        total = info["energy_direct"] + info["energy_early"] + info["energy_late"]
        for l in mine:
            assert (int(l[1]), int(l[2]), int(l[3]), int(l[4]), l[5], int(l[11])) == (info["frames"], info["frames_out"], info["direct_end"], info["early_end"], "",
                                                                                     info["lost"])
            for got, want in zip(l[6:9] + (l[12],), (info["energy_direct"], info["energy_early"], info["energy_late"], info["energy_lost"])):
                assert abs(float(got) - want) <= 1e-6 * abs(want), (got, want)
            assert abs(float(l[9]) - info["drr_db"]) <= 5e-3 + 1e-6 and abs(float(l[10]) - 10.0 * np.log10(info["energy_out"] / total)) <= 5e-3 + 1e-6
    ref = oracle_mod.RefCompat(N_REF, True)
    for j, (taps, _) in enumerate(loads):
        ref.prepare(j, taps)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=PERIOD)
    err = rms(np.stack(io[2:]) - want)
    print(f"rms err {err:.3e} of {rms(want):.3e}")
    assert err <= RMS_TOL
