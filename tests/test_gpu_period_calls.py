"""What a sequence of period calls (mc_process: process_one for 256 frames, process_period_fused for 512 and 1024) leaves in the
engine's counters, and the bits that come out, are on record.  tests/golden/period_calls.json holds, for every row of ROWS below
and every "rec" step of the row, what the library of the commit its "commit" field names answered: park_stats(), drop_stats(),
tail_forms() with the sum of its two counts ("tails") and, where kernel timing is on, kernel_stats()'s partitions and resident;
and per row the SHA-256 of every sample the row's calls returned.  The test makes the same calls with the library under test and
compares.  Integers and digests: no tolerance.  Since that commit only the host code of the parked-period protocol has moved
(DESIGN.md §2.5e says where it lives), so the same launches with the same arguments in the same order must give the same counters and the same bits.

A row is one engine - the MCCONV_* switches (every other MCCONV_* variable is cleared first), the period, shard bounds - and a
sequence of steps on one stream of seeded noise:
    ("calls", n)        n period calls
    ("rec",)            read the counters.  park_stats() and drop_stats() are host-side; tail_forms() leaves the JACK path, so a
                        parked period is told to give up here: the steps that follow a "rec" begin with a few calls that park again
    ("wet", v)          a controller step on half 0
    ("select", i)       half 0 selects IR i: a cross-fade, two voices sounding, and process_one sweeps alone instead of parking
    ("predelay", v)     a predelay change on half 0 (retire_epoch)
    ("batch", n)        a process() batch of n blocks in between
    ("reload", i)       IR i loaded again, same taps
    ("period", frames)  set_period (a cold start when the size changes)
    ("sleep", s)        the host stays away (the pause rows: MCCONV_PARK_MS=20 against 60 ms, the relaunch step)
Parking starts once the cross-fade has converged exactly (params_steady; about 160 calls from a cold start or a controller step),
so a row settles for 180 calls before what it is about.  Every row but the pause rows sets MCCONV_PARK_MS=1000, so that a
scheduling hiccup cannot turn into a timeout: "timed_out" is 0 on record.

The fixture is recorded by this module run as a program on the GPU, with MCCONV_LIB naming the library to record:
    MCCONV_LIB=<the build to record> python tests/test_gpu_period_calls.py <output.json> <the commit that build is of>
It runs every row twice.  A field of a row (park, drop, forms, tails, ks, sha256) whose two runs differ is stored as null, listed
under "unstable" as "<row>:<field>" and not compared; any such field stops the recording (redesign the row) except the un-forced
256-frame row's digest and tail_forms: the form a 256-frame tail takes depends on whether the period had to be waited for, and
those two are listed whether or not the two runs happened to agree (of three runs of d9196e4 two read 492 frequency-domain and
101 time-domain tails at the eighth "rec" and one 493 and 100, with another digest).  That row still pins its other counters and
the number of its tails.  The test itself never records and never skips."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "period_calls.json")
FIELDS = ("park", "drop", "forms", "tails", "ks", "sha256")
TIMING_DEPENDENT = {"p256-free:sha256", "p256-free:forms"}
SETTLE = 180
OTHER = {256: 512, 512: 1024, 1024: 256}  # the size a row's set_period goes to and comes back from
LONG_PARK = dict(MCCONV_PARK_MS="1000")


def _base(period):
    return [("calls", SETTLE), ("rec",), ("calls", 5), ("rec",),
            ("calls", 4), ("wet", 0.3), ("calls", 8), ("rec",),
            ("calls", SETTLE), ("rec",),
            ("calls", 4), ("predelay", 64), ("calls", 8), ("rec",),
            ("calls", 4), ("batch", 8), ("calls", 6), ("rec",),
            ("calls", 4), ("reload", 0), ("calls", 6), ("rec",),
            ("calls", 4), ("period", OTHER[period]), ("calls", 3), ("period", period), ("calls", SETTLE), ("rec",),
            ("calls", 4), ("select", 1), ("calls", 12), ("rec",), ("calls", 40), ("rec",)]


Q8_STEPS = [("calls", SETTLE), ("rec",), ("calls", 6), ("rec",), ("calls", 4), ("wet", 0.3), ("calls", 6), ("rec",),
            ("calls", SETTLE), ("rec",), ("calls", 6), ("rec",)]
PAUSE_STEPS = [("calls", SETTLE), ("rec",), ("calls", 5), ("sleep", 0.06), ("calls", 10), ("rec",)]


def _row(period, steps=None, env=(), q8=False, timing=False, part=(0, 0), long_park=True):
    return dict(period=period, steps=steps or _base(period), env=dict(LONG_PARK if long_park else {}, **dict(env)), q8=q8, timing=timing,
                part=part)


TD, FD = dict(MCCONV_TAIL_FORM="td"), dict(MCCONV_TAIL_FORM="fd")
ROWS = {
    "p256-td": _row(256, env=TD),
    "p256-fd": _row(256, env=FD),
    "p256-free": _row(256),
    "p512": _row(512),
    "p1024": _row(1024),
    "nopark-256": _row(256, env=dict(TD, MCCONV_NO_PARK="1")),
    "nopark-512": _row(512, env=dict(MCCONV_NO_PARK="1")),
    "bar0-256": _row(256, env=dict(TD, MCCONV_BAR_IO="0")),
    "bar0-512": _row(512, env=dict(MCCONV_BAR_IO="0")),
    "nospin-256": _row(256, env=dict(TD, MCCONV_NO_SPIN="1")),
    "nospin-512": _row(512, env=dict(MCCONV_NO_SPIN="1")),
    "timing-256": _row(256, env=TD, timing=True),
    "timing-512": _row(512, timing=True),
    "q8-256": _row(256, Q8_STEPS, env=FD, q8=True),
    "q8-512": _row(512, Q8_STEPS, q8=True),
    "pause-256": _row(256, PAUSE_STEPS, env=dict(TD, MCCONV_PARK_MS="20"), long_park=False),
    "pause-512": _row(512, PAUSE_STEPS, env=dict(MCCONV_PARK_MS="20"), long_park=False),
    "shard-256": _row(256, env=TD, part=(16, 32)),
}


def _engine_and_irs(row):
    from cuda_audio_amd.engine import Convolution
    from cuda_audio_amd.synth import make_ir

    if row["q8"]:  # taps + 255 + predelay > n_ref: the reference discards what the predelay shifts past n_ref (conv.cu:94-98)
        n_ref, L = 4096, 3072
        h = np.random.default_rng(59).standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
        irs = [(h * np.sqrt(0.004 / L)).astype(np.float32)]
        params = (dict(select=0, predelay=1024, wet=0.5), dict(select=0, predelay=0, wet=0.5, level=0.9))
    else:
        n_ref = 8192
        irs = [make_ir(6000, seed=61, norm=0.05), make_ir(5000, seed=63, norm=0.05)]
        params = (dict(select=0, predelay=0, wet=0.6), dict(select=1, predelay=0, wet=0.5, level=0.9))
    c = Convolution("periods", n_ref, max_batch=8, stream_threshold=8, period=row["period"], part_begin=row["part"][0], part_end=row["part"][1])
    return c, irs, params


def run_row(row, setenv, delenv):
    """The row's steps on a fresh engine: ([what each "rec" step read], the SHA-256 of every sample returned).  An engine that
    refuses a step leaves the refusal's code and text as its last record."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.synth import make_input

    for k in [k for k in os.environ if k.startswith("MCCONV_")]:
        delenv(k)
    for k, v in row["env"].items():
        setenv(k, v)
    frames, period = 0, row["period"]
    for s in row["steps"]:
        if s[0] == "period":
            period = s[1]
        frames += s[1] * period if s[0] == "calls" else s[1] * 256 if s[0] == "batch" else 0
    x = make_input(frames, seed=31)
    c, irs, params = _engine_and_irs(row)
    seen, out, pos, period = [], [], 0, row["period"]
    try:
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        for h in (0, 1):
            c.cc[h].value.update(**dict(dict(dry=0.5, panWet=0.0, panDry=0.0, level=1.0, vsteps=0, speed=100), **params[h]))
        if row["timing"]:
            c.enable_kernel_timing(True)
        for s in row["steps"]:
            if s[0] == "calls":
                for _ in range(s[1]):
                    out.append(np.stack(c.onProcess(x[0, pos:pos + period], x[1, pos:pos + period])))
                    pos += period
            elif s[0] == "batch":
                out.append(c.process(x[0, pos:pos + s[1] * 256], x[1, pos:pos + s[1] * 256]))
                pos += s[1] * 256
            elif s[0] == "rec":
                rec = dict(park=c.park_stats(), drop=c.drop_stats())
                if row["timing"]:
                    ks = c.kernel_stats()
                    rec["ks"] = dict(partitions=int(ks["partitions"]), resident=int(ks["resident"]))
                rec["forms"] = c.tail_forms()
                rec["tails"] = sum(rec["forms"].values())
                seen.append(rec)
            elif s[0] == "wet":
                c.cc[0].value.wet = s[1]
            elif s[0] == "select":
                c.cc[0].value.select = s[1]
            elif s[0] == "predelay":
                c.cc[0].value.predelay = s[1]
            elif s[0] == "reload":
                c.prepare(s[1], irs[s[1]])
            elif s[0] == "period":
                period = s[1]
                c.set_period(period)
            elif s[0] == "sleep":
                time.sleep(s[1])
            else:
                raise AssertionError(s)
    except McError as err:
        seen.append(dict(refused=err.code, text=str(err)))
    finally:
        c.close()
    sha = hashlib.sha256()
    for o in out:
        sha.update(np.ascontiguousarray(o, np.float32).tobytes())
    return seen, sha.hexdigest()


@pytest.fixture(scope="module")
def fixture():
    with open(GOLDEN) as fh:
        f = json.load(fh)
    assert f["commit"] and sorted(f["rows"]) == sorted(ROWS)
    assert set(f["unstable"]) == TIMING_DEPENDENT
    return f


@pytest.mark.parametrize("name", list(ROWS))
def test_counters_and_bits_are_those_on_record(gpu_lib, monkeypatch, fixture, name):
    want = fixture["rows"][name]
    seen, digest = run_row(ROWS[name], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    unstable = {f for f in FIELDS if f"{name}:{f}" in fixture["unstable"]}
    for k, got in enumerate(seen):
        print(f"{name} rec {k}: {got}")
    print(f"{name} sha256 {digest}")
    assert len(seen) == len(want["recs"])
    for k, (got, exp) in enumerate(zip(seen, want["recs"])):
        assert sorted(got) == sorted(exp), f"{name}: rec {k} has {sorted(got)}, on record {sorted(exp)}"
        for f in got:
            assert (exp[f] is None) == (f in unstable)
            if f not in unstable:
                assert got[f] == exp[f], f"{name}: rec {k} read {f} = {got[f]}, on record {exp[f]}"
    assert (want["sha256"] is None) == ("sha256" in unstable)
    if want["sha256"] is not None:
        assert digest == want["sha256"], f"{name}: the output's bits moved"


if __name__ == "__main__":
    import subprocess

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from cuda_audio_amd.build import hipcc as find_hipcc

        hipcc = next(l for l in subprocess.run([find_hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines() if "HIP version" in l)
    except (OSError, RuntimeError, StopIteration):
        hipcc = "unknown"
    lib = os.environ.get("MCCONV_LIB", "the tree's library")
    from cuda_audio_amd import _lib

    _lib.load()  # (before the rows clear MCCONV_LIB from the environment)
    rows, unstable = {}, []
    for name, row in ROWS.items():
        runs = [run_row(row, os.environ.__setitem__, lambda k: os.environ.pop(k, None)) for _ in range(2)]
        assert len(runs[0][0]) == len(runs[1][0]), (name, runs)
        bad = {f for a, b in zip(runs[0][0], runs[1][0]) for f in set(a) | set(b) if a.get(f) != b.get(f)}
        if runs[0][1] != runs[1][1]:
            bad.add("sha256")
        differ = sorted(bad)
        bad |= {t.split(":")[1] for t in TIMING_DEPENDENT if t.startswith(name + ":")}
        for f in differ:
            print(name, "UNSTABLE", f, [[r.get(f) for r in run[0]] if f != "sha256" else run[1] for run in runs], flush=True)
        unstable += [f"{name}:{f}" for f in sorted(bad)]
        rows[name] = dict(recs=[{f: None if f in bad else v for f, v in rec.items()} for rec in runs[0][0]],
                          sha256=None if "sha256" in bad else runs[0][1])
        for k, rec in enumerate(runs[0][0]):
            print(name, k, rec, flush=True)
        print(name, rows[name]["sha256"], flush=True)
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], hipcc=hipcc.strip(), rows=rows, unstable=unstable), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", lib)
    assert set(unstable) <= TIMING_DEPENDENT, f"redesign these rows: {sorted(set(unstable) - TIMING_DEPENDENT)}"
