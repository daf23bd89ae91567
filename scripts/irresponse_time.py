"""Time of mc_ir_response on one stereo IR of 441 000 taps at 44.1 kHz (ten seconds): 1024 frequencies over the whole span in one
window (431 runs x 4 slices of k_rsp_runs), the default grid (239 frequencies at this rate), and the 64-slice waterfall of 256-tap windows (hop
64, rise 16, fall 64) at 1024 frequencies (one run x 4 slices, 64 times over).  The engine runs on torch's current stream and HIP
events on that stream bracket each call (the call itself ends in a stream synchronise); the host clock is printed beside them.
Warm engine: one call of each kind first, then REPS timed ones, alternating.  Prints one JSON line (medians of REPS)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, waterfall_windows  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
F, RATE = 441000, 44100
c = Convolution("response", 1 << 20, max_batch=8, device=0, sample_rate=RATE)
c.use_torch_stream()
c.prepare(0, make_ir(F, seed=5, norm=0.05))
hz = np.linspace(20.0, 0.45 * RATE, 1024).astype(np.float32)
fall = waterfall_windows(64, 64, 256, 16, 64)
kinds = dict(whole_1024=lambda: c.ir_response(0, hz=hz, onset_db=0.0), whole_default_grid=lambda: c.ir_response(0, onset_db=0.0),
             waterfall_64x1024=lambda: c.ir_response(0, hz=hz, windows=fall, onset_db=0.0))
for call in kinds.values():
    call()
ev_ms, host_ms = {k: [] for k in kinds}, {k: [] for k in kinds}
for _ in range(REPS):
    for k, call in kinds.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        b.synchronize()
        host_ms[k].append((time.perf_counter() - t0) * 1e3)
        ev_ms[k].append(a.elapsed_time(b))
got = c.ir_response(0, hz=hz, onset_db=0.0)
taps = c.ir_info(0)["taps"]
c.close()
res = {k: dict(event_median_ms=round(float(np.median(ev_ms[k])), 3), event_min_ms=round(float(np.min(ev_ms[k])), 3),
               host_median_ms=round(float(np.median(host_ms[k])), 3)) for k in kinds}
print(json.dumps(dict(taps=taps, origin=got["origin"], rate=RATE, reps=REPS, db_1khz=round(float(got["db"][0, 0, np.argmin(np.abs(hz - 1000.0))]), 2), **res)), flush=True)
