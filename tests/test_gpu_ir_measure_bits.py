"""The five measurements of a loaded IR (mc_ir_decay, mc_ir_floor, mc_ir_density, mc_ir_iacc, mc_ir_sti) give the bits that are on
record.  tests/golden/ir_measure_bits.json holds SHA-256 digests of everything each call below returned under the library of the
commit its "commit" field names, the last one at which each *_measure strung its own allocations, origin search and launches
together; the test computes the same with the library under test and compares.  No tolerance: since then only host control flow
has moved (the Measure struct of csrc/irdecay.hip.h, the `measure` helper of csrc/mcconv.hip), so a different digest is a launch or
an argument that changed.

One engine, n_ref 65536 at 48 kHz.  The lengths: 1 (below every recurrence's order), 257 (a chunk and a tap), 16385 (one
workgroup's span and a tap), 40000 (three workgroups, 157 chunks; quiet_lead_ir, so the origin lies past a quiet lead).  A digest
covers every row, curve, profile and info number of the call; of a call that the library refuses, the code and the message.
  floor    40000 taps have an origin grid of 79 workgroups, so the gather's scratch starts at 79 doubles: window 64 asks for
           3 (39300 / 64 + 1) edges and outgrows it in the first pass; window 2400 with per_decade 1 (the kept interval is then
           capped at n1 / 16 = 2456) asks for 51 in either pass and does not.
  errors   an index that is not loaded, per entry point: it is found after the query and the pointers and before the stream is
           touched.  The work bounds of density (2^34 weighted taps) and IACC (2^23 partial sums) cannot be broken on 40000 taps:
           hop 1 and H = 16384 make 40000 x 32769 = 1.3e9 weighted taps, T = 1024 and ten bands 3 x 18 x 2051 = 110754 partial
           sums.  tests/test_gpu_ir_density.py and tests/test_gpu_ir_iacc.py (the work bound comes after the index) break them on
           IRs that are long enough, and pin the order.

The fixture is recorded by this module run as a program, in a process of its own, with MCCONV_LIB naming the library to record:
    MCCONV_LIB=<the build to record> python tests/test_gpu_ir_measure_bits.py <output.json> <the commit that build is of>
The test itself never records and never skips."""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_measure_bits.json")
RATE = 48000
N_REF = 65536
LENGTHS = (1, 257, 16385, 40000)
XOVERS3 = (250, 2000, 8000)


def _feed(h, v):
    """everything a measurement returns, in a fixed order: dicts by key, arrays and numbers as their raw bytes"""
    if isinstance(v, dict):
        for k in sorted(v, key=repr):
            h.update(repr(k).encode())
            _feed(h, v[k])
    elif isinstance(v, np.ndarray):
        h.update(repr(v.shape).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (bool, int)):
        h.update(struct.pack("<q", int(v)))
    elif isinstance(v, float):
        h.update(struct.pack("<d", v))
    elif v is None:
        h.update(b"none")
    else:
        raise TypeError(f"{type(v)} in a measurement's result")


def _sha(call):
    from cuda_audio_amd._lib import McError

    h = hashlib.sha256()
    try:
        res = call()
    except McError as e:
        h.update(f"error {e.code}: {e}".encode())
        return h.hexdigest(), None
    _feed(h, {k: v for k, v in res.items() if k != "query"})  # (ir_floor hands its own query back: not a result)
    return h.hexdigest(), res


def digests():
    """{case: SHA-256} of the library that is loaded."""
    from cuda_audio_amd.engine import Convolution
    from cuda_audio_amd.synth import make_ir
    from ir_shape_np import quiet_lead_ir

    out = {}
    c = Convolution("bits", N_REF, sample_rate=RATE, stream_threshold=8, max_batch=8)

    def put(case, call):
        assert case not in out, case
        out[case], res = _sha(call)
        return res

    for n in LENGTHS:
        c.prepare(0, quiet_lead_ir(39300, lead=700, seed=31) if n == 40000 else make_ir(n, seed=61 + n % 7, norm=0.05))
        assert c.ir_info(0)["taps"] == n

        put(f"decay_{n}_broadband", lambda: c.ir_decay(0, onset_db=0.0))
        d = put(f"decay_{n}_3_bands", lambda: c.ir_decay(0, bands=(250, 1000, 4000), onset_db=-20.0))
        put(f"iacc_{n}_lag0", lambda: c.ir_iacc(0, max_lag=0))
        put(f"iacc_{n}_lag48_2_bands", lambda: c.ir_iacc(0, max_lag=48, bands=(500, 2000)))
        put(f"floor_{n}_broadband", lambda: c.ir_floor(0))
        put(f"floor_{n}_3_xovers", lambda: c.ir_floor(0, xovers=XOVERS3))
        put(f"sti_{n}_default", lambda: c.ir_sti(0))
        put(f"sti_{n}_snr", lambda: c.ir_sti(0, snr_db=(30.0, 25.0, 20.0, 15.0, 10.0, 5.0, 0.0)))
        put(f"sti_{n}_broadband", lambda: c.ir_sti(0, bands=(), alpha=(), beta=()))
        put(f"sti_{n}_1_band_1_mod", lambda: c.ir_sti(0, bands=(1000,), alpha=(1.0,), beta=(), mod_hz=(2.0,)))
        put(f"density_{n}_default", lambda: c.ir_density(0, profile=n == 257))
        if n in (257, 40000):
            put(f"density_{n}_half4_hop1", lambda: c.ir_density(0, half=4, hop=1, profile=n == 40000))
            put(f"density_{n}_half4_hop16_unstaged", lambda: c.ir_density(0, half=4, hop=16))
        if n == 40000:
            assert d["origin"] > 0 and d["taps"] == 40000
            d = put("decay_40000_end35000_curve64", lambda: c.ir_decay(0, bands=(250, 1000, 4000), onset_db=-20.0, end=35000, curve_points=64))
            assert d["origin"] > 0 and d["taps"] == 35000
            put("floor_40000_window64_grows", lambda: c.ir_floor(0, xovers=XOVERS3, window=64))
            put("floor_40000_window2400_fits", lambda: c.ir_floor(0, xovers=XOVERS3, window=2400, per_decade=1))
            put("iacc_40000_split1000_curve", lambda: c.ir_iacc(0, max_lag=48, bands=(500, 2000), split=1000, curve=True))
            i = put("iacc_40000_split_past_N", lambda: c.ir_iacc(0, max_lag=48, split=50000))
            assert i["split"] == 40000 and i["rows"][(0, "late")]["status"] == 1.0

    for name in ("decay", "floor", "density", "iacc", "sti"):
        assert put(f"{name}_not_loaded", lambda: getattr(c, "ir_" + name)(1)) is None
    c.close()
    return out


def test_the_bits_are_those_before_the_shared_measure(gpu_lib):
    with open(GOLDEN) as fh:
        fixture = json.load(fh)
    want = fixture["sha256"]
    assert fixture["commit"]
    got = digests()
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, differ


if __name__ == "__main__":
    import subprocess

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        from cuda_audio_amd.build import hipcc as find_hipcc

        hipcc = next(l for l in subprocess.run([find_hipcc(), "--version"], capture_output=True, text=True).stdout.splitlines() if "HIP version" in l)
    except (OSError, RuntimeError, StopIteration):
        hipcc = "unknown"
    with open(sys.argv[1], "w") as fh:
        json.dump(dict(commit=sys.argv[2], hipcc=hipcc.strip(), sha256=digests()), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sys.argv[1], "from", os.environ.get("MCCONV_LIB", "the tree's library"))
