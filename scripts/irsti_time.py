"""Time of mc_ir_sti on one stereo IR of 2^20 taps at 48 kHz with the default query (seven octave bands, 14 modulation
frequencies: eight row groups, each a band filter and one k_sti_runs of 256 workgroups), next to the broadband group alone and
to mc_ir_decay with the same seven bands, which pays for the same filters.  The engine runs on torch's current stream and HIP
events on that stream bracket each call (the call itself ends in a stream synchronise); the host clock is printed beside them.
Warm engine: one call of each kind first, then REPS timed ones, alternating.  Prints one JSON line (medians of REPS)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
F, RATE = 1 << 20, 48000
OCTAVES = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0)
c = Convolution("sti", 2 * F, max_batch=8, device=0, sample_rate=RATE)
c.use_torch_stream()
c.prepare(0, make_ir(F, seed=5, norm=0.05))
kinds = dict(sti_7_bands=lambda: c.ir_sti(0), sti_broadband=lambda: c.ir_sti(0, bands=(), alpha=(), beta=()),
             decay_7_bands=lambda: c.ir_decay(0, bands=OCTAVES))
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
got = c.ir_sti(0)
taps = c.ir_info(0)["taps"]
c.close()
res = {k: dict(event_median_ms=round(float(np.median(ev_ms[k])), 3), event_min_ms=round(float(np.min(ev_ms[k])), 3),
               host_median_ms=round(float(np.median(host_ms[k])), 3)) for k in kinds}
print(json.dumps(dict(taps=taps, origin=got["origin"], rate=RATE, reps=REPS, sti={k: round(v, 4) for k, v in got["sti"].items()}, **res)), flush=True)
