"""C++ host: which load each measured value goes into is on record.  With a tail step, a parts step split at the mixing tap and an
rt60 aim, mcconv_host loads an IR up to four times (for the floor, for the echo density, the final load, the reload at the aimed
decay), each through its own subset of the steps, and hands the measured tail and boundaries from one to the next.
tests/golden/host_ir_load_lines.json holds, for the three command lines below and each Convolution instance (the `[id]` field of
a log line), the bodies of the log lines that begin "IR <n> " in order, stdout and stderr apart (their interleaving is not
defined), time stamp and colour codes stripped, as mcconv_host of the commit its "commit" field names printed them: the last one
at which a load read half of what it goes through from the object's members.  The test runs the host under test and compares.
The lines carry tap counts, knees, boundaries and energies to seven digits, so a load that went through another set of steps,
or got another load's tail or boundaries, shows.

8000 Hz, n_ref 16384, a period of 512; two WAVs of 3000 and 1000 frames of decaying noise 50 dB above their floor; a filter
f.wav and a match target t.wav.
  steps    --ir-tail extend:knee=mix --ir-phase minimum --ir-filter f.wav --ir-match t.wav --ir-parts direct=0,early=-3,late=-6,split=mix
  rt60     --ir-tail cut --ir-parts direct=0,early=-3,late=-6 --ir-rt60 0.05 --ir-eq peak:1000:3
  sources  an index of one WAV, a synth: line, a room: line and a sweep: line under --ir-tail extend --ir-phase minimum
           --ir-parts direct=0,early=-3,late=-6 (the generated IRs say which steps they do not have)

The fixture is recorded by this module run as a program, with the host binary to record:
    python tests/test_host_ir_load_lines.py <output.json> <the commit that build is of> <its cuda_audio_amd/host/mcconv_host>
which refuses to record when a WAV's tail or mixing tap could not be measured ("left as it is", "never reaches 1"): the noise
is chosen so that every measurement succeeds.  The test itself never records and never skips."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ir_floor_np  # noqa: E402
import ir_sweep_np  # noqa: E402
from test_host_ir_damp import _settings  # noqa: E402
from test_host_ir_shape import _write_wav16  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_ir_load_lines.json")
RATE, N_REF, PERIOD, NPER = 8000, 16384, 512, 4
PARTS = "direct=0,early=-3,late=-6"
RUNS = {
    "steps": ["--ir-tail", "extend:knee=mix", "--ir-phase", "minimum", "--ir-filter", "f.wav", "--ir-match", "t.wav", "--ir-parts", PARTS + ",split=mix"],
    "rt60": ["--ir-tail", "cut", "--ir-parts", PARTS, "--ir-rt60", "0.05", "--ir-eq", "peak:1000:3"],
    "sources": ["--ir-tail", "extend", "--ir-phase", "minimum", "--ir-parts", PARTS],
}
LINE = re.compile(r"^\d\d:\d\d:\d\d\.\d+ +\w+ +\[([^\]]*)\] (IR \d+ .*)$")
ANSI = re.compile(r"\x1b\[[0-9;]*m")


def _files(tmp):
    """The WAVs, the second IRs and the sweep's recording in tmp; returns the WAVs as _settings takes them."""
    wavs = [("ir_a.wav", ir_floor_np.noisy_ir(3000 - 37, 37, RATE, 0.08, floor_db=-50.0) * np.float32(0.1), RATE),
            ("ir_b.wav", ir_floor_np.noisy_ir(1000 - 20, 20, RATE, 0.07, floor_db=-50.0, seed=9, noise_seed=33) * np.float32(0.1), RATE)]
    for name, ir, rate in wavs:
        _write_wav16(os.path.join(tmp, name), ir, rate)
    _write_wav16(os.path.join(tmp, "f.wav"), ir_floor_np.noisy_ir(300, 5, RATE, 0.02, floor_db=-80.0, seed=3, noise_seed=5) * np.float32(0.5), RATE)
    _write_wav16(os.path.join(tmp, "t.wav"), ir_floor_np.noisy_ir(800, 10, RATE, 0.05, floor_db=-80.0, seed=4, noise_seed=6) * np.float32(0.1), RATE)
    s = ir_sweep_np.sweep(frames=4000, f1_hz=100.0, f2_hz=3500.0, rate=RATE, amplitude=0.25)
    rec = np.zeros((len(s) + 600, 2))
    rec[:len(s)] += s[:, None] * (1.0, 0.7)
    rec[250:250 + len(s)] += s[:, None] * (-0.4, 0.5)
    _write_wav16(os.path.join(tmp, "rec.wav"), rec.astype(np.float32), RATE)
    return wavs


def lines(host, tmp):
    """{run: {stream: {id: [bodies]}}} of the host binary `host`, run in the directory tmp."""
    import pathlib

    tmp = pathlib.Path(tmp)
    wavs = _files(str(tmp))
    out = {}
    for run, flags in RUNS.items():
        settings = _settings(tmp, N_REF, wavs[:1] if run == "sources" else wavs)
        if run == "sources":
            with open(tmp / "all.index", "a") as f:
                f.write("synth:0.25:0.2:seed=3,early=4,efirst=0.005,elast=0.05\n")
                f.write("room:0.25:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8\n")
                f.write("sweep:rec.wav:0.5:100:3500:amp=0.25\n")
        cmd = [host, "--settings", str(settings), "--periods", str(NPER), "--rate", str(RATE), "--period", str(PERIOD), *flags]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp), timeout=300)
        assert res.returncode == 0, (run, res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        out[run] = {}
        for stream, text in (("stdout", res.stdout), ("stderr", res.stderr)):
            by_id = out[run][stream] = {}
            for raw in text.splitlines():
                m = LINE.match(ANSI.sub("", raw))
                if m:
                    by_id.setdefault(m.group(1), []).append(m.group(2))
    return out


@pytest.mark.gpu
def test_every_load_goes_through_what_it_went_through_before_the_request(tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    assert fixture["commit"]
    want = fixture["lines"]
    got = lines(os.path.join(HOST, "mcconv_host"), str(tmp_path))
    assert sorted(got) == sorted(want)
    for run in RUNS:
        for stream in ("stdout", "stderr"):
            assert sorted(got[run][stream]) == sorted(want[run][stream]), (run, stream)
            for ident, bodies in want[run][stream].items():
                mine = got[run][stream][ident]
                first = next((k for k, (a, b) in enumerate(zip(mine, bodies)) if a != b), min(len(mine), len(bodies)))
                assert mine == bodies, (run, stream, ident, first, mine[first:first + 1], bodies[first:first + 1])


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        got = lines(os.path.abspath(sys.argv[3]), tmp)
    unmeasured = []
    for run, streams in got.items():
        for stream, by_id in streams.items():
            for ident, bodies in by_id.items():
                print(run, stream, ident, len(bodies))
                for b in bodies:
                    print("   ", b)
                    wav = int(b.split()[1]) < (1 if run == "sources" else 2)
                    if wav and ("left as it is" in b or "never reaches 1" in b):
                        unmeasured.append((run, b))
        assert streams["stdout"], run
    assert not unmeasured, unmeasured
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], lines=got), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", sys.argv[3])
