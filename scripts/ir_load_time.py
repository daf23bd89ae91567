"""Load time of one 441 000-frame stereo IR: mc_load_ir against mc_load_ir_resampled at 44.1 -> 48 kHz (the same frames,
480 000 taps after conversion), on one engine of n_ref 524288.  Prints one JSON line (median / min ms of REPS loads each).
Run under `rocprofv3 --kernel-trace --stats -- python scripts/ir_load_time.py` for the kernels' share."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
ir = make_ir(441000, seed=5, norm=0.05)
c = Convolution("load", 524288, max_batch=64, device=0, sample_rate=48000)
res = {}
for name, rate in (("mc_load_ir", 48000), ("mc_load_ir_resampled", 44100)):
    c.prepare(0, ir, ir_rate=rate)  # (first load allocates)
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.prepare(0, ir, ir_rate=rate)
        ms.append((time.perf_counter() - t0) * 1e3)
    res[name] = dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), taps=c.ir_info(0)["taps"])
c.close()
print(json.dumps(dict(ir_frames=441000, n_ref=524288, reps=REPS, **res)))
