"""C++ host: `mcconv_host --ir-response-report [--ir-response-smooth OCTAVES]` (Convolution::setIrResponseReport / parseResponse):
the option grammar and what it refuses, the host over the stand-in engine of tests/stub, which has no response measurement and must
say so, and on the device the report lines of a two-IR index against the restatement (tests/ir_response_np.py) of the decoded WAVs."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ir_iacc_np import pair_ir
from ir_response_np import grid, response, smooth
from ir_shape_np import quiet_lead_ir
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 48000, 16384, 512, 4
NUM = r"(nan|[-+0-9.]+)"
REPORT = re.compile(rf"IR (\d+) response (L|R): origin (\d+), 1 kHz level {NUM} dB, octaves((?: (?:nan|[-+0-9.]+))+), delay at 1 kHz {NUM} ms, status (\d)")
CENTRES = (31.5, 63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0)


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("arg", ["", "abc", "1,", "1 octave", "nan", "inf", "-0.5", "10.5", "1/3", "0x"])
def test_a_malformed_smoothing_option_is_refused(stub, tmp_path, arg):
    """Exit status 2 and a message that quotes the argument, before a device or the settings are looked at."""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-response-smooth", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-response-smooth '{arg}'" in res.stderr and "takes" in res.stderr


@pytest.mark.parametrize("flags,code,message", [
    (["--ir-response-smooth", "0.5"], 0, None),  # (the option alone asks for nothing)
    (["--ir-response-smooth", "0"], 0, None),
    (["--ir-response-smooth", "10"], 0, None),
    (["--ir-response-report"], 2, "the engine has no response measurement (mc_ir_response)"),
    (["--ir-response-report", "--ir-response-smooth", "0.333"], 2, "the engine has no response measurement (mc_ir_response)"),
])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, flags, code, message):
    """conv.cpp binds the response entry points weakly: over an engine without them the host still links, runs as before, and with
    --ir-response-report stops when the client starts with a message that names what is missing."""
    wavs = [("ir_a.wav", quiet_lead_ir(600, seed=94), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _settings(tmp_path, N_REF, wavs)
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", str(RATE), *flags], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == code, (res.returncode, res.stderr[-2000:])
    if message:
        assert message in res.stdout + res.stderr


def _nearest(hz, f):
    return min(max(int(math.floor(24.0 * math.log2(f / 20.0) + 0.5)), 0), hz.size - 1)


def _restate(res, rate, octaves):
    """Per channel what a report line prints: (origin, 1 kHz level, the octaves' levels relative to it, delay at 1 kHz in ms, status)
    from res, the restated response on the report's grid."""
    hz = res["hz"]
    k1 = _nearest(hz, 1000.0)
    out = []
    for c, name in enumerate("LR"):
        if res["rows"][(0, name)]["status"]:
            out.append((res["origin"], float("nan"), [float("nan")] * sum(f < 0.45 * rate for f in CENTRES), float("nan"), 1))
            continue
        with np.errstate(divide="ignore"):
            db = 10.0 * np.log10(smooth(hz, np.abs(res["h"][0, c]) ** 2, octaves))
        out.append((res["origin"], float(db[k1]), [float(db[_nearest(hz, f)] - db[k1]) for f in CENTRES if f < 0.45 * rate],
                    float(res["delay"][0, c, k1]) * 1000.0 / rate, 0))
    return out


def _near(text, want, tol):
    if np.isnan(want):
        return text == "nan"
    return text != "nan" and abs(float(text) - want) <= tol


def _check_report(out, restated):
    """Per IR and half (each half loads the index) one line per channel; the levels are printed to 2 decimals and held to 0.01 dB
    (half a unit of the last place printed; the device's own bound, some 1e-12 of A, is nothing beside it), the delay to 3 decimals
    and held to 0.01 ms."""
    lines = REPORT.findall(out)
    assert len(lines) == 2 * 2 * len(restated), out[-3000:]
    for j, want in enumerate(restated):
        mine = [l for l in lines if int(l[0]) == j]
        assert sorted(l[1] for l in mine) == ["L", "L", "R", "R"], (j, lines)
        for l in mine:
            origin, level, octaves, delay, status = want["LR".index(l[1])]
            assert int(l[2]) == origin and int(l[6]) == status, (j, l, want)
            assert _near(l[3], level, 0.01) and _near(l[5], delay, 0.01), (j, l, level, delay)
            assert len(l[4].split()) == len(octaves) and all(_near(t, v, 0.01) for t, v in zip(l[4].split(), octaves)), (j, l, octaves)


@pytest.mark.gpu
def test_the_report_lines(tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    # a decaying pair after a lead of zeros, and one whose right channel is silent
    a = pair_ir(6000, lead=37, rate=RATE, seed=5) * np.float32(0.1)
    b = pair_ir(3000, rate=RATE, seed=6, t60=0.1) * np.float32(0.1)
    b[:, 1] = 0.0
    wavs = [("ir_a.wav", a, RATE), ("ir_b.wav", b, RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    settings = _settings(tmp_path, N_REF, wavs)

    def run(*flags):
        cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
               "--ir-response-report", *flags]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout + res.stderr

    # 1. the default: one octave
    restated = [response(d, RATE, grid(20.0, min(20000.0, 0.45 * RATE), 24)) for d in decoded]
    want = [_restate(r, RATE, 1.0) for r in restated]
    assert want[0][0][4] == 0 and want[0][1][4] == 0 and want[1][0][4] == 0 and want[1][1][4] == 1 and len(want[0][0][2]) == 10
    _check_report(run(), want)
    # 2. a third of an octave
    _check_report(run("--ir-response-smooth", "0.3333"), [_restate(r, RATE, 0.3333) for r in restated])
