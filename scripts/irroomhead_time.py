"""Time of one synthesised load of the default room (1 s at 48 kHz, images up to 0.5 s: the automatic order is then 29; the
whole second would need order 58, above the library's 32) with a binaural listener in it
(mc_synth_ir_room_head: k_room's HEAD instantiation, two accumulators, and the head's pass) next to the same load without a head
(mc_synth_ir_room).  The engine runs on torch's current stream and HIP events on that stream bracket each load (the load itself
ends in a stream synchronise); the host clock is printed beside them.  Warm engine: one load of each kind that allocates, then
REPS timed ones, alternating.  Prints one JSON line.  For k_room's and k_room_head's own times run this under
`rocprofv3 --kernel-trace --stats`, in a run of its own: the headed scatter does twice the atomics, so a ratio near 2 for k_room
is what the code predicts."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrRoom, IrRoomHead, IrSynth  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
F, RATE = 48000, 48000
room, head = IrRoom(last=F // 2), IrRoomHead()
synth = IrSynth(frames=F, late_gain=0.0)
c = Convolution("roomhead", 1 << 17, max_batch=8, device=0, sample_rate=RATE)
c.use_torch_stream()
kinds = dict(head=lambda: c.prepare_synth(0, synth, room=room, head=head), room=lambda: c.prepare_synth(0, synth, room=room))
for call in kinds.values():  # (first calls allocate)
    call()
ev_ms, host_ms, infos = {k: [] for k in kinds}, {k: [] for k in kinds}, {}
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
        infos[k] = c.ir_room_info(0)
c.close()
res = {k: dict(event_median_ms=round(float(np.median(ev_ms[k])), 3), event_min_ms=round(float(np.min(ev_ms[k])), 3),
               host_median_ms=round(float(np.median(host_ms[k])), 3), order=infos[k]["order"], images_kept=infos[k]["images"]) for k in kinds}
print(json.dumps(dict(frames=F, reps=REPS, head_over_room=round(res["head"]["event_median_ms"] / res["room"]["event_median_ms"], 3), **res)), flush=True)
