"""C++ host: `mcconv_host --ir-decay-report --ir-decay-bands 250,1000 [--ir-rt60 SECONDS]` over an index of two WAVs at --rate 8000
(Convolution::setIrDecayReport / setIrRt60): the logged decay of every loaded IR against the restatement (tests/ir_decay_np.py) of
the decoded WAVs, to the printed precision, and the output of an aimed run against the oracle fed the restated reloaded taps."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_decay_np
from helpers import RMS_TOL, rms
from ir_shape_np import shape
from test_host_ir_shape import _write_wav16

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 150
BANDS = (250, 1000)
FIELDS = dict(normalize="energy", target=0.2)
NUM = r"(nan|[-+0-9.]+)"
REPORT = re.compile(rf"IR (\d+)( band {NUM} Hz)? decay: origin (\d+), EDT {NUM} s, T20 {NUM} s, T30 {NUM} s, C50 {NUM} dB, C80 {NUM} dB, Ts {NUM} ms")


def _run(tmp_path, settings, tag, *flags):
    prefix = str(tmp_path / f"{tag}_")
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
           "--dump", prefix, "--ir-normalize", "energy:0.2", "--ir-decay-report", "--ir-decay-bands", "250,1000", *flags]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    io = [np.fromfile(f"{prefix}0.{e}", np.float32) for e in ("in1", "in2", "outL", "outR")]
    assert all(len(a) == NPER * PERIOD for a in io)
    return res.stdout + res.stderr, io


def _near(text, want, tol):
    if np.isnan(want):
        return text == "nan"
    return text != "nan" and abs(float(text) - want) <= tol


def _check_report(out, restated):
    """One line per IR per half (each half loads the index) and per band; the values are the LR rows' to the printed precision."""
    lines = REPORT.findall(out)
    assert len(lines) == 2 * len(restated) * (1 + len(BANDS)), out[-3000:]
    for j, want in enumerate(restated):
        for b in range(1 + len(BANDS)):
            mine = [l for l in lines if int(l[0]) == j and (l[2] == "" if b == 0 else l[2] != "" and float(l[2]) == BANDS[b - 1])]
            assert len(mine) == 2, (j, b, lines)
            row = want["rows"][(b, "LR")]
            for l in mine:
                assert int(l[3]) == want["origin"]
                for text, f in zip(l[4:7], ("edt", "t20", "t30")):
                    assert _near(text, row[f], 1e-4 + 1e-9), (j, b, f, text, row[f])
                for text, f in zip(l[7:9], ("c50", "c80")):
                    assert _near(text, row[f], 1e-2 + 1e-9), (j, b, f, text, row[f])
                assert _near(l[9], 1000.0 * row["ts"], 1e-2 + 1e-9), (j, b, l[9], row["ts"])


def _want_output(oracle_mod, taps, io):
    ref = oracle_mod.RefCompat(N_REF, True)
    for j, t in enumerate(taps):
        ref.prepare(j, t)
    for h in range(2):
        ref.set(h, select=h, predelay=512, dry=0.5, wet=0.6, speed=100, panDry=0.0, panWet=0.25 * h, level=1.0)
    return ref.process(io[0], io[1], block=PERIOD)


def test_decay_report_and_rt60(oracle_mod, tmp_path):
    from cuda_audio_amd.engine import decay_for_rt60

    subprocess.check_call(["make", "-C", HOST, "-s"])
    wavs = [("ir_a.wav", ir_decay_np.noise_ir(6000, 37, RATE, 0.25, seed=7, amp=0.1)), ("ir_b.wav", ir_decay_np.noise_ir(5000, 20, RATE, 0.3, seed=9, amp=0.1))]
    decoded = [_write_wav16(str(tmp_path / name), ir, RATE) for name, ir in wavs]
    index = tmp_path / "all.index"
    index.write_text("".join(f"{tmp_path / name}\n" for name, _ in wavs))
    lines = ["conv.count 2"]
    for i in range(2):
        lines += [f"conv[{i}].fftSize {N_REF}", f"conv[{i}].maxPredelay 8192", f"conv[{i}].index {index}",
                  f"conv[{i}].input system:capture_{i + 1}", f"conv[{i}].output system:playback_{i + 1}",
                  f"conv[{i}].cc.device hw:2,0", f"conv[{i}].cc.message 176", f"conv[{i}].cc.select 21",
                  f"conv[{i}].cc.predelay 22", f"conv[{i}].cc.dry 23", f"conv[{i}].cc.wet 24", f"conv[{i}].cc.speed 25",
                  f"conv[{i}].cc.panDry 26", f"conv[{i}].cc.panWet 27", f"conv[{i}].cc.level 28",
                  f"conv[{i}].value.select {i}", f"conv[{i}].value.predelay 512", f"conv[{i}].value.dry 0.5",
                  f"conv[{i}].value.wet 0.6", f"conv[{i}].value.speed 100", f"conv[{i}].value.panDry 0",
                  f"conv[{i}].value.panWet {0.25 * i}", f"conv[{i}].value.level 1.0"]
    settings = tmp_path / "settings.txt"
    settings.write_text("\n".join(lines) + "\n")
    query = dict(bands=BANDS)

    # 1. the report alone
    taps = [shape(d, N_REF - 1024, **FIELDS)[0] for d in decoded]
    restated = [ir_decay_np.decay(t, RATE, **query) for t in taps]
    for r in restated:
        ir_decay_np.assert_margins(r)
    out, io = _run(tmp_path, settings, "report")
    _check_report(out, restated)
    assert "rt60:" not in out
    err = rms(np.stack(io[2:]) - _want_output(oracle_mod, taps, io))
    print(f"report run: rms err {err:.3e}")
    assert err <= RMS_TOL

    # 2. aimed below the measured times: reloaded with the decay that takes them there
    target = 0.15
    measured = [r["rows"][(0, "LR")]["t30"] for r in restated]
    assert all(m > target + 0.05 for m in measured), measured
    frames = [decay_for_rt60(m, target, RATE) for m in measured]
    aimed = [shape(d, N_REF - 1024, decay_t60=f, **FIELDS)[0] for d, f in zip(decoded, frames)]
    re_restated = [ir_decay_np.decay(t, RATE, **query) for t in aimed]
    for r in re_restated:
        ir_decay_np.assert_margins(r)
    out2, io2 = _run(tmp_path, settings, "aimed", "--ir-rt60", str(target))
    logged = re.findall(rf"IR (\d+) rt60: measured {NUM} s, decay (\d+) frames, now {NUM} s", out2)
    assert len(logged) == 4, out2[-3000:]
    for j in range(2):
        mine = [l for l in logged if int(l[0]) == j]
        assert len(mine) == 2
        now = re_restated[j]["rows"][(0, "LR")]["t30"]
        print(f"IR {j}: measured {measured[j]:.6f} s, decay {frames[j]} frames, now {now:.6f} s; logged {mine[0][1:]}")
        for l in mine:
            assert int(l[2]) == frames[j]  # (the C++ decayForRt60 gives decay_for_rt60's number)
            assert _near(l[1], measured[j], 1e-4 + 1e-9) and _near(l[3], now, 1e-4 + 1e-9)
    _check_report(out2, re_restated)
    assert np.array_equal(io2[0], io[0]) and np.array_equal(io2[1], io[1])
    err = rms(np.stack(io2[2:]) - _want_output(oracle_mod, aimed, io2))
    print(f"aimed run: rms err {err:.3e}")
    assert err <= RMS_TOL
    assert rms(np.stack(io2[2:]) - np.stack(io[2:])) > 100 * RMS_TOL  # (the shorter IRs are heard)

    # 3. a target above the measured times leaves the IRs as they are: the output of run 1, bit for bit
    out3, io3 = _run(tmp_path, settings, "above", "--ir-rt60", "5")
    left = re.findall(rf"IR (\d+) rt60: target 5.0000 s is not below the measured {NUM} s, left as it is", out3)
    assert len(left) == 4 and "frames, now" not in out3, out3[-3000:]
    for l in left:
        assert _near(l[1], measured[int(l[0])], 1e-4 + 1e-9)
    _check_report(out3, restated)
    for a, b in zip(io3, io):
        np.testing.assert_array_equal(a, b)
