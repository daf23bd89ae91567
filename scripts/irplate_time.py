"""Time of one synthesised load with a plate (mc_synth_ir_plate): the default plate to 20 kHz at 48 kHz over 4 s (25 697 modes x
192 000 frames, 4.9e9 pairs), next to the same load without the plate (k_synth, the shaping stage, the transforms): the
difference is the table's upload, the accumulator's zeroing, k_plate and k_synth_room's reads.  With CAP=1 (the default) the
largest load the work cap allows is timed too: the same plate over as many frames as 2^36 pairs hold.  The engine runs on torch's
current stream and HIP events on that stream bracket each load (the load itself ends in a stream synchronise); the host clock is
printed beside them.  Warm engine: one load of each kind that allocates, then REPS timed ones, alternating.  Prints one JSON
line.  For k_plate's own time run this under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrPlate, IrSynth, plate_plan  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
CAP = int(os.environ.get("CAP", "1"))
F, RATE = 4 * 48000, 48000
plate = IrPlate()
plan = plate_plan(plate, RATE, F)
F_cap = min((1 << 36) // plan["modes"], 1 << 24)
synth, synth_cap = IrSynth(frames=F, late_gain=0.0), IrSynth(frames=F_cap, late_gain=0.0)
c = Convolution("plate", 1 << 19, max_batch=8, device=0, sample_rate=RATE)
c.use_torch_stream()

kinds = dict(plain=lambda: c.prepare_synth(0, synth), plate=lambda: c.prepare_synth(0, synth, plate=plate))
if CAP:
    kinds.update(plain_cap=lambda: c.prepare_synth(0, synth_cap), plate_cap=lambda: c.prepare_synth(0, synth_cap, plate=plate))
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
less = res["plate"]["event_median_ms"] - res["plain"]["event_median_ms"]
out = dict(frames=F, modes=plan["modes"], pairs=plan["pairs"], reps=REPS, plate_less_plain_ms=round(less, 3), pairs_per_s=round(plan["pairs"] / (less * 1e-3), -6))
if CAP:
    less_cap = res["plate_cap"]["event_median_ms"] - res["plain_cap"]["event_median_ms"]
    out.update(frames_cap=F_cap, pairs_cap=F_cap * plan["modes"], plate_cap_less_plain_ms=round(less_cap, 3),
               pairs_per_s_cap=round(F_cap * plan["modes"] / (less_cap * 1e-3), -6))
print(json.dumps(dict(out, **res)), flush=True)
