"""Time of one synthesised load with the reflections of a room (mc_synth_ir_room) at the largest lattice, order 32 (2.2 M
images), F = 2^20 frames, 48 kHz, next to the same load without the room (k_synth, the shaping stage, the transforms): the
difference is the accumulator's zeroing, k_room and k_synth_room's reads; and the load with a cardioid pair in the room
(mc_synth_ir_room_mics, k_room's other instantiation), and the load with 1, 2 and 4 frequency bands in the room
(mc_synth_ir_room_bands: k_room once per band, from the second band on with air, and the join).  The engine runs on torch's current stream and HIP
events on that stream bracket each load (the load itself ends in a stream synchronise); the host clock is printed beside them.
Warm engine: one load of each kind that allocates, then REPS timed ones, alternating.  Prints one JSON line.  For k_room's own
time run this under `rocprofv3 --kernel-trace --stats`, in a run of its own.  LAST=frames leaves out images from that frame on."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrRoom, IrRoomBands, IrRoomMics, IrSynth  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
F, RATE = 1 << 20, 48000
room = IrRoom(order=32, last=int(os.environ.get("LAST", "0")))
synth = IrSynth(frames=F, late_gain=0.0)
c = Convolution("room", 2 * F, max_batch=8, device=0, sample_rate=RATE)
c.use_torch_stream()
mics = IrRoomMics.pair()  # XY: cardioids at +45 and -45 degrees

def banded(B):  # walls that soften and air that thickens with the band; band 0 has no air
    bands = IrRoomBands(xovers=(250.0, 1000.0, 4000.0)[:B - 1], beta=tuple(0.9 - 0.1 * j for j in range(B)), air=tuple(0.01 * j for j in range(B)))
    return lambda: c.prepare_synth(0, synth, room=room, bands=bands)


kinds = dict(plain=lambda: c.prepare_synth(0, synth), mics=lambda: c.prepare_synth(0, synth, room=room, mics=mics), bands1=banded(1), bands2=banded(2),
             bands4=banded(4), room=lambda: c.prepare_synth(0, synth, room=room))
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
info = c.ir_room_info(0)
c.close()
res = {k: dict(event_median_ms=round(float(np.median(ev_ms[k])), 3), event_min_ms=round(float(np.min(ev_ms[k])), 3),
               host_median_ms=round(float(np.median(host_ms[k])), 3)) for k in kinds}
print(json.dumps(dict(frames=F, order=info["order"], images_kept=info["images"], last=info["last"], reps=REPS,
                      room_less_plain_ms=round(res["room"]["event_median_ms"] - res["plain"]["event_median_ms"], 3),
                      mics_less_room_ms=round(res["mics"]["event_median_ms"] - res["room"]["event_median_ms"], 3), **res)), flush=True)
