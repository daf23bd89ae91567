"""C++ host: `mcconv_host --write-sweep` (the sweep through WavFile::write, back to the generated floats), an index with a
`sweep:` line at --rate 48000 (Convolution::prepareSweep: the line's seconds turned into frames at the client's rate, the
recording deconvolved by the engine when the client starts), the malformed lines the index grammar refuses, and the host over
the stand-in engine of tests/stub, which has no sweep capture and must say so."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_sweep_np
from helpers import RMS_TOL, rms
from ir_shape_np import quiet_lead_ir, shape
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
SPEC = "0.085:100:20000:amp=0.25,fadein=0.001,fadeout=0.0005"
SWEEP = dict(frames=4080, f1_hz=100.0, f2_hz=20000.0, rate=48000, amplitude=0.25, fade_in=48, fade_out=24)  # SPEC at 48000 Hz, every time by rint
FIELDS = dict(normalize="energy", target=0.2)


def _read_wav24(path):
    """(rate, [frames, 2] float32) of a 44-byte-header stereo 24-bit file, decoded as WavFile decodes (s24 / 2^24)."""
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    channels, rate, bits = int.from_bytes(raw[22:24], "little"), int.from_bytes(raw[24:28], "little"), int.from_bytes(raw[34:36], "little")
    assert (channels, bits) == (2, 24) and int.from_bytes(raw[40:44], "little") == len(raw) - 44
    b = np.frombuffer(raw[44:], np.uint8).reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    return rate, (v / 16777216.0).astype(np.float32).reshape(-1, 2)


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host"])
    return os.path.join(HOST, "mcconv_host")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("spec,rate,fields", [
    (SPEC, 48000, SWEEP),
    ("0.05:20:20000", None, dict(frames=2205, f1_hz=20.0, f2_hz=20000.0, rate=44100, amplitude=0.5)),  # (full scale: the peaks clip by one step)
])
def test_write_sweep_round_trips_to_the_generated_floats(host, tmp_path, spec, rate, fields):
    """Needs no GPU: the sweep is host arithmetic.  Within the 24-bit quantisation step, 2^-24 (rounding takes half of it,
    clipping +0.5 to the largest sample a whole one)."""
    from cuda_audio_amd.engine import Sweep, sweep_frames

    path = tmp_path / "sweep.wav"
    cmd = [host, "--write-sweep", f"{path}:{spec}"] + (["--rate", str(rate)] if rate else [])
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    got_rate, got = _read_wav24(str(path))
    want = sweep_frames(Sweep(**fields))
    assert got_rate == fields["rate"] and got.shape == (fields["frames"], 2)
    np.testing.assert_array_equal(got[:, 0], got[:, 1])
    err = np.abs(got[:, 0].astype(np.float64) - want.astype(np.float64)).max()
    print(f"max err {err:.3e}, step {2.0 ** -24:.3e}")
    assert err <= 2.0 ** -24
    assert np.abs(want.astype(np.float64) - ir_sweep_np.sweep(**fields)).max() <= 2.0 ** -23 * fields["amplitude"]
    assert np.abs(got).max() > 0.99 * fields["amplitude"]


@pytest.mark.parametrize("spec", ["x.wav:0.1:100", "x.wav:0:100:20000", "x.wav:0.1:100:30000", "x.wav:0.1:100:20000:amp=0", ":0.1:100:20000"])
def test_write_sweep_refuses_a_malformed_argument(host, tmp_path, spec):
    res = subprocess.run([host, "--write-sweep", spec], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--write-sweep '{spec}'" in res.stderr and not os.path.exists(tmp_path / "x.wav")


def _index(tmp_path, n_ref, wavs, lines):
    """test_host_ir_damp's settings with `lines` appended to the index its two halves share."""
    settings = _settings(tmp_path, n_ref, wavs)
    with open(tmp_path / "all.index", "a") as f:
        f.write("".join(l + "\n" for l in lines))
    return settings


@pytest.mark.parametrize("line", [
    "sweep:",                                     # nothing
    "sweep:rec.wav",                              # no length
    "sweep:rec.wav:0.1:100",                      # no F2
    "sweep::0.1:100:20000",                       # no file
    "sweep:rec.wav:abc:100:20000",
    "sweep:rec.wav:0:100:20000",
    "sweep:rec.wav:-1:100:20000",
    "sweep:rec.wav:0.1:0.5:20000",                # F1 below 1 Hz
    "sweep:rec.wav:0.1:100:100",                  # F2 not above F1
    "sweep:rec.wav:0.1:100:20000x",
    "sweep:rec.wav:0.1:100:20000:",               # an empty list
    "sweep:rec.wav:0.1:100:20000:amp",            # no value
    "sweep:rec.wav:0.1:100:20000:amp=0",
    "sweep:rec.wav:0.1:100:20000:amp=-0.5",
    "sweep:rec.wav:0.1:100:20000:amp=0.5,",       # an empty item
    "sweep:rec.wav:0.1:100:20000:colour=3",       # no such key
    "sweep:rec.wav:0.1:100:20000:fadein=-0.01",
    "sweep:rec.wav:0.1:100:20000:fadein=0.06,fadeout=0.05",
    "sweep:rec.wav:0.1:100:20000:offset=nan",
    "sweep:rec.wav:0.1:100:20000:length=-1",
    "sweep:rec.wav:0.1:100:20000:amp=0.5:offset=0",  # a sixth colon
])
def test_a_malformed_line_is_refused(stub, line, tmp_path):
    """Exit status 2 and a message that quotes the line, before the recording is opened or any IR is loaded."""
    settings = _index(tmp_path, 16384, [], [line])
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    res = subprocess.run([stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"], capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"index line '{line}'" in res.stderr


def _recording(tmp_path, name="rec.wav"):
    """SWEEP through a two-tap room, 16 bit at 48000 Hz; returns the frames the host decodes."""
    s = ir_sweep_np.sweep(**SWEEP)
    rec = np.zeros((len(s) + 600, 2))
    rec[:len(s)] += s[:, None] * (1.0, 0.7)
    rec[250:250 + len(s)] += s[:, None] * (-0.4, 0.5)
    return _write_wav16(str(tmp_path / name), rec.astype(np.float32), 48000)


@pytest.mark.parametrize("keys", ["", ",offset=-0.002,length=0.02"])
def test_the_stub_host_links_and_says_the_engine_has_no_sweep_capture(stub, tmp_path, keys):
    """conv.cpp binds the sweep entry points weakly: over an engine without them the host still links, runs as before over
    WAVs, and with a well-formed sweep: line (Convolution::parseSweep took it, the recording was read) stops when the client
    starts with a message that names what is missing."""
    wavs = [("ir_a.wav", quiet_lead_ir(600, seed=94), 48000)]
    for name, ir, rate in wavs:
        _write_wav16(str(tmp_path / name), ir, rate)
    _recording(tmp_path)
    env = dict(os.environ, MCSTUB_LOG=str(tmp_path / "calls.log"))
    settings = _index(tmp_path, 16384, wavs, [])
    base = [stub, "--settings", str(settings), "--periods", "2", "--rate", "48000"]
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    _index(tmp_path, 16384, wavs, [f"sweep:{tmp_path / 'rec.wav'}:{SPEC}{keys}"])
    res = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2, (res.returncode, res.stderr[-2000:])
    assert "the engine has no sweep capture (mc_load_ir_sweep)" in res.stdout + res.stderr
    res = subprocess.run([stub, "--write-sweep", f"{tmp_path / 'out.wav'}:{SPEC}"], capture_output=True, text=True, cwd=str(tmp_path), timeout=60, env=env)
    assert res.returncode == 2 and "the engine has no sweep (mc_sweep_generate)" in res.stderr


@pytest.mark.gpu
def test_a_wav_and_a_captured_ir(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", quiet_lead_ir(3000, seed=94), 48000)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    rec = _recording(tmp_path)
    n_ref, period, nper = 16384, 512, 300
    offset_s, length_s = -0.002, 0.02
    settings = _index(tmp_path, n_ref, wavs, [f"sweep:{tmp_path / 'rec.wav'}:{SPEC},offset={offset_s},length={length_s}"])
    offset, F = int(np.rint(offset_s * 48000)), int(np.rint(length_s * 48000))
    assert (offset, F, int(np.rint(0.085 * 48000)), int(np.rint(0.001 * 48000)), int(np.rint(0.0005 * 48000))) == (-96, 960, 4080, 48, 24)
    captured = ir_sweep_np.deconvolve(rec, SWEEP, offset, F).astype(np.float32)
    restated = [shape(decoded[0], n_ref - 1024, None, 48000, **FIELDS), shape(captured, n_ref - 1024, None, 48000, **FIELDS)]
    prefix = str(tmp_path / "sweep_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", "48000", "--period", str(period),
           "--dump", prefix, "--ir-normalize", "energy:0.2"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    # one line per captured IR per half (each half loads the index)
    logged = re.findall(r"IR (\d+) captured: sweep (\d+) frames, recording (\d+) frames, (\d+) frames at offset (-?\d+)", out)
    assert logged == [("1", "4080", str(len(rec)), "960", "-96")] * 2, out[-2000:]
    shaped = re.findall(r"IR (\d+) shaped: onset (\d+), first kept frame (\d+), (\d+) taps, gain ([-+0-9.]+) dB", out)
    assert len(shaped) == 4
    for j, (_, info) in enumerate(restated):
        mine = [l for l in shaped if int(l[0]) == j]
        assert len(mine) == 2
        for l in mine:
            assert (int(l[1]), int(l[2]), int(l[3])) == (0, 0, info["taps"])
            assert abs(float(l[4]) - 20 * np.log10(info["gain"])) <= 0.006
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == nper * period for a in io)
    ref = oracle_mod.RefCompat(n_ref, True)
    for j, (t, _) in enumerate(restated):
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
