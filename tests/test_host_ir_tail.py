"""C++ host: `mcconv_host --ir-floor-report [--ir-floor-xovers HZ,..] [--ir-tail cut|extend[:key=value,...]]`
(Convolution::setIrFloorReport / setIrFloorXovers / setIrTail): the option grammar and what it refuses, the host over the stand-in
engine of tests/stub, which has neither a floor measurement nor a tail step and must say so, and on the device the report lines
and the output of a repaired index against the restatements (tests/ir_floor_np.py, tests/ir_tail_np.py) of the decoded WAVs."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_floor_np
import ir_tail_np
from helpers import RMS_TOL, rms
from ir_shape_np import quiet_lead_ir
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 150
XOVERS = (400, 1600)
NUM = r"(nan|[-+0-9.]+|-?inf)"
REPORT = re.compile(rf"IR (\d+)( band (\d))? floor: origin (\d+), knee {NUM}, T {NUM} s, noise {NUM} dB, peak to noise {NUM} dB, interval {NUM}, status (\d)")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("arg", ["", "fade", "extend:", "shorten", "cut:fade", "cut:fade=", "cut:=3", "extend:fade=abc", "extend:fade=-0.1", "extend:length=nan",
                                 "extend:seed=-1", "extend:seed=1.5", "extend:width=1.5", "extend:colour=3", "extend:fade=0.1,", "extend:fade=0.1:seed=2"])
def test_a_malformed_tail_is_refused(stub, tmp_path, arg):
    """Exit status 2 and a message that quotes the argument, before a device or the settings are looked at."""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-tail", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-tail '{arg}'" in res.stderr and "cut|extend" in res.stderr


@pytest.mark.parametrize("arg", ["", "abc", "400,", "400,,1600", "1600,400", "400,400", "100,200,300,400", "0", "-5", "400;1600"])
def test_malformed_floor_crossovers_are_refused(stub, tmp_path, arg):
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-floor-xovers", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert "--ir-floor-xovers takes HZ[,HZ[,HZ]]" in res.stderr


@pytest.mark.parametrize("flags,message", [
    (["--ir-tail", "extend:fade=0.005,length=1,seed=3,width=0.5"], "the engine has no tail step (mc_load_ir_tail)"),
    (["--ir-tail", "cut", "--ir-floor-xovers", "400,1600"], "the engine has no tail step (mc_load_ir_tail)"),
    (["--ir-floor-report"], "the engine has no floor measurement (mc_ir_floor)"),
])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, flags, message):
    """conv.cpp binds the floor and tail entry points weakly: over an engine without them the host still links, runs as before,
    and with a well-formed option stops when the client starts with a message that names what is missing."""
    wavs = [("ir_a.wav", quiet_lead_ir(600, seed=94), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _settings(tmp_path, N_REF, wavs)
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", str(RATE)]
    res = subprocess.run(base + ["--ir-floor-xovers", "400,1600"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]  # (crossovers alone ask for nothing)
    res = subprocess.run(base + flags, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert message in res.stdout + res.stderr


def test_the_stub_host_says_so_for_a_sweep_line_too(stub, tmp_path):
    from test_host_ir_sweep import SPEC, _recording

    _recording(tmp_path)
    settings = _settings(tmp_path, N_REF, [])
    with open(tmp_path / "all.index", "a") as f:
        f.write(f"sweep:{tmp_path / 'rec.wav'}:{SPEC}\n")
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000", "--ir-tail", "extend"], capture_output=True, text=True,
                         cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2 and "the engine has no tail step (mc_load_ir_tail)" in res.stdout + res.stderr


def _near(text, want, tol):
    if np.isnan(want):
        return text == "nan"
    return text != "nan" and abs(float(text) - want) <= tol


def _check_report(out, restated, xovers):
    """One line per IR per half (each half loads the index) and row group; the values are the LR rows' to the printed precision."""
    lines = REPORT.findall(out)
    groups = 1 + (len(xovers) + 1 if xovers else 0)
    assert len(lines) == 2 * len(restated) * groups, out[-3000:]
    for j, want in enumerate(restated):
        for g in range(groups):
            mine = [l for l in lines if int(l[0]) == j and (l[1] == "" if g == 0 else l[1] != "" and int(l[2]) == g - 1)]
            assert len(mine) == 2, (j, g, lines)
            row = want["rows"][(g, "LR")]
            for l in mine:
                assert int(l[3]) == want["origin"] and int(l[9]) == int(row["status"])
                assert _near(l[4], row["knee"], 0.05 + 1e-6) and _near(l[5], row["t"], 5e-5 + 1e-9), (j, g, l, row)
                assert _near(l[6], 10.0 * np.log10(row["noise"]), 5e-3 + 1e-6) and _near(l[7], row["peak_to_noise_db"], 5e-3 + 1e-6), (j, g, l, row)
                assert _near(l[8], row["interval"], 0.0), (j, g, l, row)


@pytest.mark.gpu
def test_floor_report_and_tail(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    # a floor 50 dB down, which is repaired; one 22 dB down, under the 30 dB the search needs, which is left as it is
    wavs = [("ir_a.wav", ir_floor_np.noisy_ir(6000, 37, RATE, 0.25, floor_db=-50.0) * np.float32(0.1), RATE),
            ("ir_b.wav", ir_floor_np.noisy_ir(5000, 20, RATE, 0.3, floor_db=-22.0, seed=9, noise_seed=33) * np.float32(0.1), RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    settings = _settings(tmp_path, N_REF, wavs)

    def run(tag, *flags):
        prefix = str(tmp_path / f"{tag}_")
        cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
               "--dump", prefix, "--ir-floor-report", "--ir-floor-xovers", "400,1600", *flags]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
        assert all(len(a) == NPER * PERIOD for a in io)
        return res.stdout + res.stderr, io

    def want_output(taps, io):
        ref = oracle_mod.RefCompat(N_REF, True)
        for j, t in enumerate(taps):
            ref.prepare(j, t)
        for h in range(2):
            ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
        return ref.process(io[0], io[1], block=PERIOD)

    # 1. the report alone
    floors = [ir_floor_np.floor(d, RATE, xovers=XOVERS) for d in decoded]
    for f in floors:
        ir_floor_np.assert_margins(f)
    assert floors[0]["rows"][(0, "LR")]["peak_to_noise_db"] > 40.0 and floors[1]["rows"][(0, "LR")]["peak_to_noise_db"] < 30.0
    out, io = run("report")
    _check_report(out, floors, XOVERS)
    assert " tail: " not in out
    assert rms(np.stack(io[2:]) - want_output(decoded, io)) <= RMS_TOL

    # 2. extended: IR 0 is loaded again with the tail its floor gives, IR 1 is left as it is
    fade_s, seed = 0.005, 3
    tf = ir_floor_np.tail_from_floor(floors[0])
    spec = dict(xovers=XOVERS, knee=tuple(tf["knee"]), t60=tuple(tf["t60"]), level_db=tuple(tf["level_db"]), fade=int(np.rint(fade_s * RATE)), seed=seed)
    repaired, tinfo = ir_tail_np.tailed(decoded[0], RATE, "extend", **spec)
    out2, io2 = run("extend", "--ir-tail", f"extend:fade={fade_s},seed={seed}")
    knees = ", ".join(str(k) for k in tf["knee"])
    line = f"IR 0 tail: extended, 3 of 3 bands at knees {knees}, {len(decoded[0])} frames in, {len(decoded[0])} out, first frame changed {tinfo['first']}"
    assert out2.count(line) == 2, out2[-3000:]
    assert len(re.findall(rf"IR 1 tail: peak to noise {NUM} dB \(status 0\) is under 30 dB, left as it is", out2)) == 2, out2[-3000:]
    after = [ir_floor_np.floor(repaired, RATE, xovers=XOVERS), floors[1]]
    ir_floor_np.assert_margins(after[0])
    _check_report(out2, after, XOVERS)
    assert np.array_equal(io2[0], io[0]) and np.array_equal(io2[1], io[1])
    err = rms(np.stack(io2[2:]) - want_output([repaired, decoded[1]], io2))
    print(f"extended run: rms err {err:.3e}")
    assert err <= RMS_TOL
