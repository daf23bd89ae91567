"""C++ host: `mcconv_host --ir-sti-report [--ir-sti-snr DB[,DB...]]` (Convolution::setIrStiReport / parseSti): the option grammar
and what it refuses, the host over the stand-in engine of tests/stub, which has no STI measurement and must say so, and on the
device the report lines of a two-IR index against the restatement (tests/ir_sti_np.py) of the decoded WAVs."""
import os
import re
import subprocess

import numpy as np
import pytest

from ir_iacc_np import pair_ir
from ir_shape_np import quiet_lead_ir
from ir_sti_np import SETS, rating, sti
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 48000, 16384, 512, 4
NUM = r"(nan|[-+0-9.]+)"
REPORT = re.compile(rf"IR (\d+) sti (LR|L|R): origin (\d+), STI {NUM} \((\w+)\), MTI((?: (?:nan|[-+0-9.]+)){{7}}), status (\d)")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("arg", ["", "abc", "10,", ",10", "10;20", "nan", "inf", "10dB", "-61", "121", "10,20", "1,2,3,4,5,6", "1,2,3,4,5,6,7,8", "1,2,3,x,5,6,7"])
def test_a_malformed_sti_option_is_refused(stub, tmp_path, arg):
    """Exit status 2 and a message that quotes the argument, before a device or the settings are looked at."""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-sti-snr", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-sti-snr '{arg}'" in res.stderr and "takes" in res.stderr


@pytest.mark.parametrize("flags,code,message", [
    (["--ir-sti-snr", "10"], 0, None),  # (the option alone asks for nothing)
    (["--ir-sti-snr", "-60,0,10,20,30,40,120"], 0, None),
    (["--ir-sti-report"], 2, "the engine has no STI measurement (mc_ir_sti)"),
    (["--ir-sti-report", "--ir-sti-snr", "15"], 2, "the engine has no STI measurement (mc_ir_sti)"),
])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, flags, code, message):
    """conv.cpp binds the STI entry points weakly: over an engine without them the host still links, runs as before, and with
    --ir-sti-report stops when the client starts with a message that names what is missing."""
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


def _near(text, want, tol=1e-4):
    if np.isnan(want):
        return text == "nan"
    return text != "nan" and abs(float(text) - want) <= tol


def _check_report(out, restated):
    """Per IR and half (each half loads the index) one line per channel set; STI and the seven MTI are printed to 4 decimals and
    held to the restatement at 1e-4 (half a unit of the last place printed and the device's 1e-5 behind the band filters)."""
    lines = REPORT.findall(out)
    assert len(lines) == 2 * 3 * len(restated), out[-3000:]
    for j, want in enumerate(restated):
        mine = [l for l in lines if int(l[0]) == j]
        assert sorted(l[1] for l in mine) == sorted(SETS * 2), (j, lines)
        for l in mine:
            s = l[1]
            mti = [want["rows"][(b, s)]["mti"] for b in range(1, 8)]
            status = int(any(want["rows"][(b, s)]["status"] for b in range(1, 8)))
            assert int(l[2]) == want["origin"] and int(l[6]) == status, (j, l)
            assert _near(l[3], want["sti"][s]), (j, l, want["sti"])
            words = {"none"} if np.isnan(want["sti"][s]) else {rating(want["sti"][s] - 1e-4), rating(want["sti"][s] + 1e-4)}  # (both, next to an edge)
            assert l[4] in words, (j, l)
            assert all(_near(t, v) for t, v in zip(l[5].split(), mti)), (j, l, mti)


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
               "--ir-sti-report", *flags]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout + res.stderr

    # 1. the defaults
    want = [sti(d, RATE) for d in decoded]
    assert not np.isnan(want[0]["sti"]["LR"]) and np.isnan(want[1]["sti"]["R"]) and want[1]["sti"]["L"] == want[1]["sti"]["LR"]
    _check_report(run(), want)
    # 2. noise: one ratio for every octave, then one per octave
    _check_report(run("--ir-sti-snr", "6"), [sti(d, RATE, snr_db=(6.0,) * 7) for d in decoded])
    snr = (-3.0, 0.0, 3.0, 6.0, 9.0, 12.0, 15.0)
    _check_report(run("--ir-sti-snr", ",".join(f"{v:g}" for v in snr)), [sti(d, RATE, snr_db=snr) for d in decoded])
    # 3. a rate that cannot hold the 8 kHz octave stops the host with the engine's words
    low = tmp_path / "r16"
    low.mkdir()
    slow = [(name, ir, 16000) for name, ir, _ in wavs]
    for name, ir, rate in slow:
        _write_wav16(str(low / name), ir, rate)
    res = subprocess.run([os.path.join(HOST, "mcconv_host"), "--settings", str(_settings(low, N_REF, slow)), "--periods", "1", "--rate", "16000", "--ir-sti-report"],
                         capture_output=True, text=True, cwd=str(low), timeout=300)
    assert res.returncode == 2 and "the STI cannot be measured: centre_hz[6]" in res.stdout + res.stderr, res.stderr[-2000:]
