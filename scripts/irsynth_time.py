"""Time of mc_synth_ir for F = 2^20 and F = 2^24 frames next to mc_load_ir_shaped of as many frames copied from the host, both
into an engine of n_ref 4194304 under the same shape (a 256-tap fade, so that both go through the shaping stage).  Warm engine:
one load of each kind and length that allocates, then REPS timed ones, alternating the two.  Prints one JSON line (median / min
ms; host clock around the call, which ends in a stream synchronise).  For k_synth's own time run this under
`rocprofv3 --kernel-trace --stats`, in a run of its own (KERNEL_ONLY=1 skips the host loads)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrShape, IrSynth  # noqa: E402

REPS = int(os.environ.get("REPS", "10"))
KERNEL_ONLY = os.environ.get("KERNEL_ONLY") == "1"
N_REF = 4194304
shape = IrShape(fade_out=256)
c = Convolution("synth", N_REF, max_batch=64, device=0, sample_rate=48000)
res = {}
for F in (1 << 20, 1 << 24):
    synth = IrSynth(frames=F, seed=5, late_start=2400, t60=min(F, 480000), build_up=4800, late_gain=0.05, direct=1.0, n_early=16, early_first=240,
                    early_last=2300, early_gain=0.5, width=0.8)
    host = None if KERNEL_ONLY else (0.01 * np.random.default_rng(1).standard_normal((F, 2))).astype(np.float32)
    c.prepare_synth(0, synth, shape=shape)  # (first loads allocate)
    if host is not None:
        c.prepare(1, host, shape=shape)
    ms = dict(synth=[], host=[])
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.prepare_synth(0, synth, shape=shape)
        ms["synth"].append((time.perf_counter() - t0) * 1e3)
        if host is not None:
            t0 = time.perf_counter()
            c.prepare(1, host, shape=shape)
            ms["host"].append((time.perf_counter() - t0) * 1e3)
    res[str(F)] = {k: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(float(np.min(v)), 3)) for k, v in ms.items() if v}
    res[str(F)]["taps"] = c.ir_info(0)["taps"]
c.close()
print(json.dumps(dict(n_ref=N_REF, reps=REPS, kernel_only=KERNEL_ONLY, **res)))
