"""C++ host: `mcconv_host --ir-phase minimum[:floor=DB,over=K]` (Convolution::setIrPhase): the option grammar and what it
refuses, the host over the stand-in engine of tests/stub, which has no phase step and must say so, and on the device the report
line and the output against the oracle fed the restatement (tests/ir_phase_np.py) of the decoded WAV."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_phase_np as P
from helpers import RMS_TOL, rms
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 60
LINE = re.compile(r"IR (\d+) minimum phase: (\d+) frames through a transform of (\d+) points, delay removed ([-0-9.]+) frames \(([-0-9.]+) ms\), "
                  r"([-0-9.]+) dB kept, (\d+) and (\d+) bins at the floor")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("arg", ["", "linear", "minimum:", "min", "minimum:floor", "minimum:floor=", "minimum:=3", "minimum:floor=abc", "minimum:floor=39",
                                 "minimum:floor=301", "minimum:floor=nan", "minimum:over=1", "minimum:over=3", "minimum:over=128", "minimum:over=8.5",
                                 "minimum:colour=3", "minimum:over=8,", "minimum:floor=100:over=8"])
def test_a_malformed_phase_is_refused(stub, tmp_path, arg):
    """Exit status 2 and a message that quotes the argument, before a device or the settings are looked at."""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-phase", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-phase '{arg}'" in res.stderr and "minimum[:key=value,...]" in res.stderr


@pytest.mark.parametrize("arg", ["minimum", "minimum:floor=90.5,over=64", "minimum:over=2"])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, arg):
    """conv.cpp binds the phase entry points weakly: over an engine without them the host still links, runs as before, and with a
    well-formed option stops when the client starts with a message that names what is missing."""
    wavs = [("ir_a.wav", P.delayed_noise(600), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _settings(tmp_path, N_REF, wavs)
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", str(RATE)]
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(base + ["--ir-phase", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no phase step (mc_load_ir_phase)" in res.stdout + res.stderr


@pytest.mark.gpu
def test_the_report_line_and_the_output(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", P.delayed_noise(3000, delay=400), RATE), ("ir_b.wav", P.delayed_noise(1000, delay=50, seed=4), RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    settings = _settings(tmp_path, N_REF, wavs)
    prefix = str(tmp_path / "phase_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
           "--dump", prefix, "--ir-phase", "minimum:floor=100,over=4"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == NPER * PERIOD for a in io)
    restated = [P.min_phase(d, oversample=4, floor_db=100.0) for d in decoded]
    lines = LINE.findall(out)
    assert len(lines) == 2 * len(wavs), out[-3000:]  # (each half loads the index)
    for j, (taps, info) in enumerate(restated):
        mine = [l for l in lines if int(l[0]) == j]
        assert len(mine) == 2
        removed = info["centre_in"] - info["centre_out"]
        kept = 10.0 * np.log10(info["energy_out"] / info["energy_in"])
        for l in mine:
            assert int(l[1]) == info["frames"] and int(l[2]) == info["nfft"] and (int(l[6]), int(l[7])) == tuple(info["clamped"])
            assert abs(float(l[3]) - removed) <= 0.05 + 1e-6 and abs(float(l[4]) - 1000.0 * removed / RATE) <= 5e-4 + 1e-6
            assert abs(float(l[5]) - kept) <= 5e-5 + 1e-6
        assert removed > 40.0
    ref = oracle_mod.RefCompat(N_REF, True)
    for j, (taps, _) in enumerate(restated):
        ref.prepare(j, taps)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=PERIOD)
    err = rms(np.stack(io[2:]) - want)
    print(f"rms err {err:.3e} of {rms(want):.3e}")
    assert err <= RMS_TOL
