"""Time of one synthesised load with a spring tank (mc_synth_ir_spring): the default tank at 48 kHz over 4 s (192 000 frames, a
transform of 2^19 points), next to the same load without the spring (k_synth, the shaping stage, the transforms): the difference
is k_spring_bins, the inverse transform in double, k_spring_acc and k_synth_room's reads.  With CAP=1 (the default) the largest
load is timed too: 2^21 frames, a transform of 2^22 points.  The engine runs on torch's current stream and HIP events on that
stream bracket each load (the load itself ends in a stream synchronise); the host clock is printed beside them.  Warm engine: one
load of each kind that allocates, then REPS timed ones, alternating.  Prints one JSON line.  For the split between k_spring_bins
and the transform run this under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrSpring, IrSynth, spring_plan  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
CAP = int(os.environ.get("CAP", "1"))
F, F_cap, RATE = 4 * 48000, 1 << 21, 48000
spring = IrSpring()
plan, plan_cap = spring_plan(spring, RATE, F), spring_plan(spring, RATE, F_cap)
synth, synth_cap = IrSynth(frames=F, late_gain=0.0), IrSynth(frames=F_cap, late_gain=0.0)
c = Convolution("spring", 1 << 19, max_batch=8, device=0, sample_rate=RATE)
c.use_torch_stream()

kinds = dict(plain=lambda: c.prepare_synth(0, synth), spring=lambda: c.prepare_synth(0, synth, spring=spring))
if CAP:
    kinds.update(plain_cap=lambda: c.prepare_synth(0, synth_cap), spring_cap=lambda: c.prepare_synth(0, synth_cap, spring=spring))
for call in kinds.values():  # (first calls allocate)
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
c.close()
res = {k: dict(event_median_ms=round(float(np.median(ev_ms[k])), 3), event_min_ms=round(float(np.min(ev_ms[k])), 3),
               host_median_ms=round(float(np.median(host_ms[k])), 3)) for k in kinds}
out = dict(frames=F, points=plan["points"], reps=REPS, spring_less_plain_ms=round(res["spring"]["event_median_ms"] - res["plain"]["event_median_ms"], 3))
if CAP:
    out.update(frames_cap=F_cap, points_cap=plan_cap["points"],
               spring_cap_less_plain_ms=round(res["spring_cap"]["event_median_ms"] - res["plain_cap"]["event_median_ms"], 3))
print(json.dumps(dict(out, **res)), flush=True)
