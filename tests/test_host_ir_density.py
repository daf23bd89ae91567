"""C++ host: `mcconv_host --ir-density-report [--ir-density-window S] [--ir-density-hop S] [--ir-density-t60 S|auto]` and
`--ir-tail extend:...,knee=mix` (Convolution::setIrDensityReport / parseDensity / IrTail::kneeAtMix): the option grammar and what
it refuses, the host over the stand-in engine of tests/stub, which has no density measurement and must say so, and on the device
the report lines of a two-IR index against the restatement (tests/ir_density_np.py) of the decoded WAVs and a room line whose
tail starts at the measured mixing tap."""
import os
import re
import subprocess

import numpy as np
import pytest

import ir_decay_np
from ir_density_np import assert_margins, density
from ir_shape_np import quiet_lead_ir
from test_host_ir_damp import _settings
from test_host_ir_shape import _write_wav16
from test_host_ir_synth import _index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 4
NUM = r"(nan|[-+0-9.]+|-?inf)"
REPORT = re.compile(rf"IR (\d+) density: origin (\d+), mixing {NUM} \({NUM} s\), first {NUM}, max {NUM} at {NUM}, after {NUM}, silent {NUM}, status (\d)")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_host_stub"])
    return os.path.join(HOST, "mcconv_host_stub")


@pytest.mark.parametrize("option,arg", [(o, a) for o in ("--ir-density-window", "--ir-density-hop", "--ir-density-t60")
                                        for a in ("", "abc", "0", "-0.01", "nan", "inf", "0.02s", "0.02,0.01", "5000")]
                         + [("--ir-density-window", "auto"), ("--ir-density-hop", "auto"), ("--ir-density-t60", "Auto")])
def test_a_malformed_density_option_is_refused(stub, tmp_path, option, arg):
    """Exit status 2 and a message that quotes the argument, before a device or the settings are looked at."""
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), option, arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"{option} '{arg}'" in res.stderr and "seconds" in res.stderr


@pytest.mark.parametrize("arg", ["extend:knee", "extend:knee=", "extend:knee=mixing", "extend:knee=0.5", "cut:knee=mix", "extend:knee=mix,"])
def test_a_malformed_knee_is_refused(stub, tmp_path, arg):
    res = subprocess.run([stub, "--settings", str(tmp_path / "none.txt"), "--ir-tail", arg], capture_output=True, text=True, cwd=str(tmp_path), timeout=60)
    assert res.returncode == 2, (res.returncode, res.stderr[-500:])
    assert f"--ir-tail '{arg}'" in res.stderr and "cut|extend" in res.stderr and "knee" in res.stderr


@pytest.mark.parametrize("flags,code,message", [
    (["--ir-density-window", "0.02", "--ir-density-hop", "0.0025", "--ir-density-t60", "auto"], 0, None),  # (the options alone ask for nothing)
    (["--ir-density-t60", "0.3"], 0, None),
    (["--ir-density-report"], 2, "the engine has no density measurement (mc_ir_density)"),
    (["--ir-density-report", "--ir-density-t60", "0.3", "--ir-density-window", "0.01"], 2, "the engine has no density measurement (mc_ir_density)"),
    (["--ir-tail", "extend:knee=floor"], 2, "the engine has no tail step (mc_load_ir_tail)"),
    (["--ir-tail", "extend:fade=0.005,knee=mix"], 2, "the engine has no tail step (mc_load_ir_tail)"),
])
def test_the_stub_host_links_and_says_what_the_engine_lacks(stub, tmp_path, flags, code, message):
    """conv.cpp binds the density entry points weakly: over an engine without them the host still links, runs as before, and
    with --ir-density-report stops when the client starts with a message that names what is missing."""
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


def _near(text, want, tol):
    if np.isnan(want):
        return text == "nan"
    return text != "nan" and abs(float(text) - want) <= tol


def _check_report(out, restated):
    """One line per IR per half (each half loads the index); the values are the LR rows' to the printed precision."""
    lines = REPORT.findall(out)
    assert len(lines) == 2 * len(restated), out[-3000:]
    for j, want in enumerate(restated):
        mine = [l for l in lines if int(l[0]) == j]
        assert len(mine) == 2, (j, lines)
        row = want["rows"]["LR"]
        for l in mine:
            assert int(l[1]) == want["origin"] and int(l[9]) == int(row["status"]), (j, l, row)
            assert _near(l[2], row["mix"], 0.0) and _near(l[3], row["mix_s"], 5e-5 + 1e-9) and _near(l[6], row["max_tap"], 0.0) and _near(l[8], row["silent"], 0.0), (j, l, row)
            for text, f in ((l[4], "first"), (l[5], "max"), (l[7], "mean_after")):
                assert _near(text, row[f], 5e-4 + 1e-9), (j, f, l, row)


@pytest.mark.gpu
def test_the_report_lines(tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    # decaying noise after a lead of zeros, and a sparse one that does not decay: an impulse every 40 taps, which never mixes
    sparse = np.zeros((4981, 2), np.float32)  # (the last tap is an impulse: the decay curve never gets to -35 dB)
    sparse[20::40] = 0.2 * (np.random.default_rng(9).integers(0, 2, size=(125, 2)) * 2.0 - 1.0)
    wavs = [("ir_a.wav", ir_decay_np.noise_ir(6000, 37, RATE, 0.25) * np.float32(0.1), RATE), ("ir_b.wav", sparse, RATE)]
    decoded = [_write_wav16(str(tmp_path / name), ir, rate) for name, ir, rate in wavs]
    settings = _settings(tmp_path, N_REF, wavs)

    def run(*flags):
        cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD),
               "--ir-density-report", *flags]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout + res.stderr

    # 1. the defaults: 20 ms in all (H = 80), a quarter of H between centres
    want = [density(d, RATE) for d in decoded]
    for w in want:
        assert_margins(w)
    assert want[0]["rows"]["LR"]["status"] == 0 and want[1]["rows"]["LR"]["status"] == 1 and want[0]["origin"] == 37
    _check_report(run(), want)

    # 2. a window of 10.1 ms (H = floor(40.4 + 0.5) = 40), a hop of 1 ms (8 taps), the measured T30 undone
    t60 = []
    for d in decoded:
        t30 = ir_decay_np.decay(d, RATE)["rows"][(0, "LR")]["t30"]
        if np.isnan(t30):  # (the sparse one never gets to -35 dB: auto then undoes nothing)
            t60.append(0)
            continue
        assert abs(t30 * RATE - np.rint(t30 * RATE)) < 0.49  # (the device's T30 rounds to the same tap)
        t60.append(int(np.rint(t30 * RATE)))
    assert t60[0] > 0 and t60[1] == 0, t60
    want = [density(d, RATE, half=40, hop=8, decay_t60=t) for d, t in zip(decoded, t60)]
    for w in want:
        assert_margins(w)
    _check_report(run("--ir-density-window", "0.0101", "--ir-density-hop", "0.001", "--ir-density-t60", "auto"), want)

    # 3. a window the engine does not take stops the host with the engine's words
    res = subprocess.run([os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", "1", "--rate", str(RATE), "--ir-density-report",
                          "--ir-density-window", "0.0005"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert res.returncode == 2 and "the density cannot be measured: half 2" in res.stdout + res.stderr, res.stderr[-2000:]


@pytest.mark.gpu
def test_a_room_hands_over_to_its_tail_at_the_mixing_tap(gpu_lib, tmp_path):
    """room -> density -> floor -> tail with knee=mix.  The host's log names the mixing tap the restatement finds in the rendered
    room and a first changed frame one fade before it; through the Python engine the same steps give the same tail, and the
    stored taps before that frame are bit for bit those of the load without a tail (the tail step's own promise)."""
    import ir_floor_np
    import ir_room_np
    from cuda_audio_amd.engine import Convolution, IrRoom, IrSynth, tail_from_floor, tail_move_knee
    from test_host_ir_room import FRAMES, LINE, ROOM

    subprocess.check_call(["make", "-C", HOST, "-s"])
    rate, n_ref, fade_s, length_s, seed = 48000, 16384, 0.005, 0.3, 3
    fade = int(np.rint(fade_s * rate))
    room, _, _ = ir_room_np.frames(ROOM, rate, frames=FRAMES, late_gain=0.0)
    want = density(room, rate)
    assert_margins(want)
    mix = int(want["rows"]["LR"]["mix"])
    floor = ir_floor_np.floor(room, rate, xovers=())
    ir_floor_np.assert_margins(floor)
    knee = ir_floor_np.tail_from_floor(floor)["knee"][0]
    assert want["rows"]["LR"]["status"] == 0 and want["origin"] + 2 * fade < mix < knee - 1000, (want["rows"]["LR"], knee)

    # the final load as the restatements give it: the floor's line slid to the mixing tap, the tail from there, and its density
    import ir_tail_np

    tf = ir_floor_np.tail_from_floor(floor)
    level = tuple(float(np.float32(float(np.float32(v)) + 60.0 * (float(knee) - float(mix)) / float(tf["t60"][0]))) for v in tf["level_db"][0])
    extended, tinfo = ir_tail_np.tailed(room, rate, "extend", xovers=(), knee=(mix,), t60=tuple(tf["t60"]), level_db=(level,), fade=fade,
                                        length=int(np.rint(length_s * rate)), seed=seed)
    after = density(extended, rate)
    assert_margins(after, least=1e-6)  # (the device's tail is the restatement's to a float's rounding, not to a double's)
    assert tinfo["first"] == mix - fade and len(extended) == 14400 and after["rows"]["LR"]["status"] == 0

    settings = _index(tmp_path, n_ref, [], [LINE, LINE])  # (half h plays IR h: both are the room)
    cmd = [os.path.join(HOST, "mcconv_host"), "--settings", str(settings), "--periods", "4", "--rate", str(rate), "--period", "512", "--ir-density-report",
           "--ir-tail", f"extend:fade={fade_s},length={length_s},seed={seed},knee=mix"]
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    out = res.stdout + res.stderr
    assert res.returncode == 0, res.stderr[-2000:]
    for j in range(2):
        assert out.count(f"IR {j} tail: knees moved to the mixing tap {mix}") == 2, out[-3000:]
        assert out.count(f"IR {j} tail: extended, 1 of 1 bands at knees {mix}, {FRAMES} frames in, 14400 out, first frame changed {mix - fade}") == 2, out[-3000:]
    _check_report(out, [after, after])  # (the report is of the final load)

    c = Convolution("irdensity_host", n_ref, sample_rate=rate, stream_threshold=8, max_batch=8)
    synth, iroom = IrSynth(frames=FRAMES, late_gain=0.0), IrRoom(**ROOM)
    c.prepare_synth(0, synth, room=iroom)
    plain = c.ir_taps(0)
    got = c.ir_density(0)
    assert got["rows"]["LR"]["mix"] == mix and got["rows"]["LR"]["status"] == 0
    tail = tail_from_floor(c.ir_floor(0), mode="extend", fade=fade, length=int(np.rint(length_s * rate)), seed=seed)
    assert tail.knee == (knee,)
    moved = tail_move_knee(tail, 0, mix)
    assert moved.level_db[0][0] > tail.level_db[0][0] + 5.0  # (earlier on the band's own line is louder)
    c.prepare_synth(0, synth, room=iroom, tail=moved)
    info = c.ir_tail_info(0)
    taps = c.ir_taps(0)
    c.close()
    assert info["first"] == mix - fade and info["bands"] == 1 and info["length"] == 14400
    assert taps[:mix - fade].tobytes() == plain[:mix - fade].tobytes()
    assert not np.array_equal(taps[mix - fade:FRAMES], plain[mix - fade:])
