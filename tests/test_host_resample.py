"""C++ host: `mcconv_host --rate 48000 --period 512` over an index of WAVs, with and without --match-ir-rate
(Convolution::setMatchIrRate: every IR converted to the JACK client's sample rate on load)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import RMS_TOL, rms
from resample_np import resample

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")


def _write_wav16(path, lr, rate):
    """Stereo 16-bit PCM at `rate` Hz; returns the frames the host decodes (s16 / 65536, wav.cu's scaling)."""
    q = np.clip(np.rint(lr.astype(np.float64) * 65536.0), -32768, 32767).astype("<i2")
    data = q.tobytes()
    hdr = b"RIFF" + np.uint32(36 + len(data)).tobytes() + b"WAVEfmt " + np.uint32(16).tobytes()
    hdr += np.uint16(1).tobytes() + np.uint16(2).tobytes() + np.uint32(rate).tobytes()
    hdr += np.uint32(rate * 4).tobytes() + np.uint16(4).tobytes() + np.uint16(16).tobytes()
    open(path, "wb").write(hdr + b"data" + np.uint32(len(data)).tobytes() + data)
    return (q.astype(np.float32) / 65536.0).astype(np.float32)


def test_match_ir_rate(oracle_mod, tmp_path):
    from cuda_audio_amd.synth import make_ir

    subprocess.check_call(["make", "-C", HOST, "-s"])
    d0 = _write_wav16(str(tmp_path / "ir44.wav"), make_ir(3000, seed=81, norm=0.05), 44100)
    d1 = _write_wav16(str(tmp_path / "ir48.wav"), make_ir(3500, seed=82, norm=0.05), 48000)
    index = tmp_path / "all.index"
    index.write_text(f"{tmp_path / 'ir44.wav'}\n{tmp_path / 'ir48.wav'}\n")
    n_ref, period, nper = 16384, 512, 300
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
    for match in (True, False):
        prefix = str(tmp_path / f"m{int(match)}_")
        cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", "48000",
               "--period", str(period), "--dump", prefix]
        if match:
            cmd.append("--match-ir-rate")
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        out = res.stdout + res.stderr
        assert "sample rate 48000" in out
        # only the 44.1 kHz IR is converted (once per half: each half loads the index)
        assert out.count("44100 Hz -> 48000 Hz") == (2 if match else 0)
        assert "48000 Hz -> 48000 Hz" not in out
        io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
        assert all(len(a) == nper * period for a in io)
        taps = [resample(d0, 44100, 48000, n=n_ref - 1024).astype(np.float32) if match else d0, d1]
        ref = oracle_mod.RefCompat(n_ref, True)
        for j, t in enumerate(taps):
            ref.prepare(j, t)
        for h in range(2):
            ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
        want = ref.process(io[0], io[1], block=period)
        assert rms(want) > 0.05
        err = rms(np.stack(io[2:]) - want)
        assert err <= RMS_TOL, f"match={match}: rms {err:.3e}"
