"""C++ host: `mcconv_host --ir-trim -20:16 --ir-fade 256 --ir-normalize energy:0.2` over an index of WAVs with a quiet
lead-in, at --rate 48000 with and without --match-ir-rate (Convolution::setIrShape: every IR shaped on load)."""
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import RMS_TOL, rms
from ir_shape_np import assert_onset_margin, quiet_lead_ir, session_frames, shape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
FIELDS = dict(trim_db=-20, pre_roll=16, fade_out=256, normalize="energy", target=0.2)


def _write_wav16(path, lr, rate):
    """Stereo 16-bit PCM at `rate` Hz; returns the frames the host decodes (s16 / 65536, wav.cu's scaling)."""
    q = np.clip(np.rint(lr.astype(np.float64) * 65536.0), -32768, 32767).astype("<i2")
    data = q.tobytes()
    hdr = b"RIFF" + np.uint32(36 + len(data)).tobytes() + b"WAVEfmt " + np.uint32(16).tobytes()
    hdr += np.uint16(1).tobytes() + np.uint16(2).tobytes() + np.uint32(rate).tobytes()
    hdr += np.uint32(rate * 4).tobytes() + np.uint16(4).tobytes() + np.uint16(16).tobytes()
    open(path, "wb").write(hdr + b"data" + np.uint32(len(data)).tobytes() + data)
    return (q.astype(np.float32) / 65536.0).astype(np.float32)


def test_shaped_irs(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir44.wav", quiet_lead_ir(3000, seed=94), 44100), ("ir48.wav", quiet_lead_ir(3500, seed=82), 48000)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    index = tmp_path / "all.index"
    index.write_text("".join(f"{tmp_path / name}\n" for name, _, _ in wavs))
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
        # the frames each IR is shaped from: converted to 48 kHz with --match-ir-rate, as decoded without
        rates = [(rate, 48000) if match else (None, None) for _, _, rate in wavs]
        restated = []
        for d, (src, dst) in zip(decoded, rates):
            assert_onset_margin(session_frames(d, src, dst), 0, FIELDS["trim_db"])
            restated.append(shape(d, n_ref - 1024, src, dst, **FIELDS))
        prefix = str(tmp_path / f"m{int(match)}_")
        cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", "48000",
               "--period", str(period), "--dump", prefix, "--ir-trim", "-20:16", "--ir-fade", "256", "--ir-normalize", "energy:0.2"]
        if match:
            cmd.append("--match-ir-rate")
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        out = res.stdout + res.stderr
        assert out.count("44100 Hz -> 48000 Hz") == (2 if match else 0)
        # one line per shaped IR per half (each half loads the index), with what the restatement finds
        logged = re.findall(r"IR (\d+) shaped: onset (\d+), first kept frame (\d+), (\d+) taps, gain ([-+0-9.]+) dB", out)
        assert len(logged) == 4, out[-2000:]
        for j, (_, info) in enumerate(restated):
            mine = [l for l in logged if int(l[0]) == j]
            assert len(mine) == 2
            for l in mine:
                assert (int(l[1]), int(l[2]), int(l[3])) == (info["onset"], info["first"], info["taps"])
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
        print(f"match={match}: wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
        assert np.abs(wet).max() < 0.5 and rms(want) > 0.01
        err = rms(np.stack(io[2:]) - want)
        print(f"match={match}: rms err {err:.3e}")
        assert err <= RMS_TOL, f"match={match}: rms {err:.3e}"
