"""C++ host: `mcconv_host --ir-eq lowcut:120 --ir-eq peak:2500:6:1.5 --ir-normalize energy:0.2` over an index of two WAVs at
--rate 48000 (Convolution::setIrEq: every IR equalised on load, at the client's rate; without --match-ir-rate the frames
count as being at that rate)."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_eq_np
from helpers import RMS_TOL, rms
from ir_shape_np import quiet_lead_ir
from test_host_ir_shape import _write_wav16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
BANDS = (("lowcut", 120), ("peak", 2500, 6.0, 1.5))
FIELDS = dict(normalize="energy", target=0.2)


def test_equalised_irs(oracle_mod, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", quiet_lead_ir(3000, seed=94), 48000), ("ir_b.wav", quiet_lead_ir(3500, seed=82), 48000)]
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
    restated = [ir_eq_np.eq(d, n_ref - 1024, None, 48000, BANDS, **FIELDS) for d in decoded]
    prefix = str(tmp_path / "eq_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(nper), "--rate", "48000",
           "--period", str(period), "--dump", prefix, "--ir-eq", "lowcut:120", "--ir-eq", "peak:2500:6:1.5", "--ir-normalize", "energy:0.2"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = res.stdout + res.stderr
    # one line per equalised IR per half (each half loads the index), next to the shaped line with the gain after the bands
    at_1k = float(ir_eq_np.response_db(BANDS, 48000, [1000.0])[0])
    logged = re.findall(r"IR (\d+) equalised: (\d+) bands, ([-+0-9.]+) dB at 1 kHz", out)
    assert len(logged) == 4 and out.count("equalised: 2 bands") == 4, out[-2000:]
    assert all(abs(float(l[2]) - at_1k) <= 0.006 for l in logged)
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
