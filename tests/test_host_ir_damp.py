"""C++ host: `mcconv_host --ir-damp 400,1600:0,0.1,0.0333 --ir-damp-origin 37 --ir-eq peak:2500:6:1.5 --ir-normalize energy:0.2`
over an index of two WAVs at --rate 48000 (Convolution::setIrDamp: every IR damped on load, the decay times turned into frames at
the client's rate; without --match-ir-rate the frames count as being at that rate), what the command line refuses, and the host
over the stand-in engine of tests/stub, which has no damping and must say so."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_damp_np
from helpers import RMS_TOL, rms
from ir_shape_np import quiet_lead_ir
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
XOVERS, SECONDS, ORIGIN = (400, 1600), (0.0, 0.1, 0.0333), 37
FRAMES = (0, 4800, 1598)  # round(seconds * 48000): 0.0333 * 48000 = 1598.4
BANDS = (("peak", 2500, 6.0, 1.5),)
FIELDS = dict(normalize="energy", target=0.2)


def _settings(tmp_path, n_ref, wavs):
    index = tmp_path / "all.index"
    index.write_text("".join(f"{tmp_path / name}\n" for name, _, _ in wavs))
    lines = ["conv.count 2"]
    for i in range(2):
        lines += [f"conv[{i}].fftSize {n_ref}", f"conv[{i}].maxPredelay 8192", f"conv[{i}].index {index}",
                  f"conv[{i}].input system:capture_{i + 1}", f"conv[{i}].output system:playback_{i + 1}",
                  f"conv[{i}].cc.device hw:2,0", f"conv[{i}].cc.message 176", f"conv[{i}].cc.select 21",
                  f"conv[{i}].cc.predelay 22", f"conv[{i}].cc.dry 23", f"conv[{i}].cc.wet 24", f"conv[{i}].cc.speed 25",
                  f"conv[{i}].cc.panDry 26", f"conv[{i}].cc.panWet 27", f"conv[{i}].cc.level 28",
                  f"conv[{i}].value.select {i}", f"conv[{i}].value.predelay 512", f"conv[{i}].value.dry 0.5",
                  f"conv[{i}].value.wet 0.6", f"conv[{i}].value.speed 100", f"conv[{i}].value.panDry 0",
                  f"conv[{i}].value.panWet {0.25 * i}", f"conv[{i}].value.level 1.0"]
    settings = tmp_path / "settings.txt"
    settings.write_text("\n".join(lines) + "\n")
    return settings


@pytest.mark.gpu
def test_damped_irs(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", quiet_lead_ir(3000, seed=94), 48000), ("ir_b.wav", quiet_lead_ir(3500, seed=82), 48000)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    n_ref, period, nper = 16384, 512, 300
    settings = _settings(tmp_path, n_ref, wavs)
    assert tuple(int(np.rint(s * 48000)) for s in SECONDS) == FRAMES
    restated = [ir_damp_np.damped(d, n_ref - 1024, None, 48000, XOVERS, FRAMES, ORIGIN, BANDS, **FIELDS) for d in decoded]
    prefix = str(tmp_path / "damp_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", "48000", "--period", str(period),
           "--dump", prefix, "--ir-damp", "400,1600:0,0.1,0.0333", "--ir-damp-origin", str(ORIGIN), "--ir-eq", "peak:2500:6:1.5",
           "--ir-normalize", "energy:0.2"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    # one line per damped IR per half (each half loads the index) with the decays in frames at the client's rate
    logged = re.findall(r"IR (\d+) damped: (\d+) crossovers, origin (\d+), (\d+) bands with a decay \(([0-9, ]+) frames\)", out)
    assert len(logged) == 4, out[-2000:]
    for l in logged:
        assert (int(l[1]), int(l[2]), int(l[3])) == (2, ORIGIN, 2)
        assert tuple(int(v) for v in l[4].split(",")) == FRAMES
    assert out.count("equalised: 1 bands") == 4
    shaped = re.findall(r"IR (\d+) shaped: onset (\d+), first kept frame (\d+), (\d+) taps, gain ([-+0-9.]+) dB", out)
    assert len(shaped) == 4
    for j, (_, info, _) in enumerate(restated):
        mine = [l for l in shaped if int(l[0]) == j]
        assert len(mine) == 2
        for l in mine:
            assert (int(l[1]), int(l[2]), int(l[3])) == (0, 0, info["taps"])
            assert abs(float(l[4]) - 20 * np.log10(info["gain"])) <= 0.006  # (two decimals; the gain is that of the damped, equalised taps)
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    ref = oracle_mod.RefCompat(n_ref, True)
    for j, (t, _, _) in enumerate(restated):
        ref.prepare(j, t)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    want = ref.process(io[0], io[1], block=period)
    x = np.stack(io[:2]).astype(np.float64)
    wet = want - 0.5 * (x[0] + x[1])  # (dry 0.5, panDry 0, level 1 in both halves)
    print(f"wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert np.abs(wet).max() < 0.5 and rms(want) > 0.01
    err = rms(np.stack(io[2:]) - want)
    print(f"rms err {err:.3e}")
    assert err <= RMS_TOL, f"rms {err:.3e}"


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("args", [
    ["--ir-damp", "400,1600"],                    # no decay times
    ["--ir-damp", ":1,2"],                        # no crossover
    ["--ir-damp", "400,1600:0,0.1"],              # a decay short
    ["--ir-damp", "400:0,0.1,0.2"],               # one too many
    ["--ir-damp", "250,500,1000,2000:0,0,0,0,0"],  # four crossovers
    ["--ir-damp", "400,abc:0,0.1,0.2"],
    ["--ir-damp", "400,1600:0,-0.1,0.2"],
    ["--ir-damp", "400,,1600:0,0.1,0.2"],
    ["--ir-damp-origin", "-3"],
    ["--ir-damp-origin", "12x"],
])
def test_the_command_line_refuses(stub, args, tmp_path):
    """Before any settings file is looked for: exit status 2 and a line that names the option."""
    res = subprocess.run([stub] + args, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert args[0] in res.stderr


def test_the_stub_host_links_and_says_the_engine_has_no_damping(stub, tmp_path):
    """conv.cpp binds the damping entry points weakly: over an engine without them the host still links, runs as before without
    --ir-damp, and with it stops at the first IR with a message that names what is missing."""
    wavs = [("ir_a.wav", quiet_lead_ir(600, seed=94), 48000)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    settings = _settings(tmp_path, 16384, wavs)
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"]
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(base + ["--ir-damp", "400,1600:0,0.1,0.0333"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no IR damping (mc_load_ir_damped)" in res.stdout + res.stderr


def test_seconds_become_frames_at_the_clients_rate():
    """Convolution::dampFrames is round(seconds * rate), as FRAMES assumes; the Python side of the same rule."""
    for seconds, rate, frames in ((0.1, 48000, 4800), (0.0333, 48000, 1598), (0.0333, 44100, 1469), (0.0, 48000, 0)):
        assert int(np.rint(seconds * rate)) == frames
