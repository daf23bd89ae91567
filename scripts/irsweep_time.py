"""Time of mc_load_ir_sweep for a 10 s sweep against a 10 s IR at 44.1 kHz (N = F = 441000, a recording of N + F frames: 2 F N =
3.9e11 double fma in k_sweep_corr) next to the same load with a sweep of 2 frames (everything but the correlation: the
upload, the shaping stage, the transforms), into an engine of n_ref 524288.  Warm engine: one load of each kind that
allocates, then REPS timed ones, alternating the two.  Prints one JSON line (median / min ms; host clock around the call, which
ends in a stream synchronise).  For k_sweep_corr's own time run this under `rocprofv3 --kernel-trace --stats`, in a run of its
own (KERNEL_ONLY=1 skips the short loads)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, Sweep  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
KERNEL_ONLY = os.environ.get("KERNEL_ONLY") == "1"
N_REF, RATE = 524288, 44100
N = F = int(os.environ.get("FRAMES", "441000"))
rec = (0.05 * np.random.default_rng(1).standard_normal((N + F, 2))).astype(np.float32)
c = Convolution("sweep", N_REF, max_batch=64, device=0, sample_rate=RATE)
long, short = Sweep(frames=N, fade_in=441, fade_out=441), Sweep(frames=2, f1_hz=20.0, f2_hz=20000.0)
kinds = dict(long=long) if KERNEL_ONLY else dict(long=long, short=short)
for s in kinds.values():  # (first loads allocate)
    c.prepare_sweep(0, rec, s, ir_frames=F)
ms = {k: [] for k in kinds}
for _ in range(REPS):
    for k, s in kinds.items():
        t0 = time.perf_counter()
        c.prepare_sweep(0, rec, s, ir_frames=F)
        ms[k].append((time.perf_counter() - t0) * 1e3)
res = {k: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(float(np.min(v)), 3)) for k, v in ms.items()}
res["taps"] = c.ir_info(0)["taps"]
c.close()
print(json.dumps(dict(n_ref=N_REF, frames=F, sweep_frames=N, reps=REPS, kernel_only=KERNEL_ONLY, **res)))
