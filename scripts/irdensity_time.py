"""Time of mc_ir_density on one 441 000-tap stereo IR (BASELINE config 3, n_ref 524288) at 48 kHz: the default window and hop
(H = 480, hop 120: 3675 windows of 961 taps, staged in LDS), hop 1 (441 000 windows) and H = 16384 (windows of 32 769 taps read from
global memory, the default hop 4096), next to mc_load_ir and mc_ir_decay of the same IR.  Warm engine: one call first, then REPS
timed ones.  Prints one JSON line (median / min ms; host clock around `Convolution.ir_density` / `ir_decay` / `prepare`)."""
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
c = Convolution("density", 524288, max_batch=64, device=0, sample_rate=48000)


def timed(call):
    call()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3))


res = dict(load=timed(lambda: c.prepare(0, ir)), decay_0_bands=timed(lambda: c.ir_decay(0)))
t30 = c.ir_decay(0)["rows"][(0, "LR")]["t30"]
t60 = 0 if np.isnan(t30) else int(round(t30 * 48000))
res.update(density_default=timed(lambda: c.ir_density(0)), density_default_t60=timed(lambda: c.ir_density(0, decay_t60=t60)),
           density_default_profile=timed(lambda: c.ir_density(0, profile=True)), density_hop_1=timed(lambda: c.ir_density(0, hop=1)),
           density_half_16384=timed(lambda: c.ir_density(0, half=16384)))
d = c.ir_density(0, decay_t60=t60)
row = d["rows"]["LR"]
taps = c.ir_info(0)["taps"]
c.close()
print(json.dumps(dict(ir_frames=441000, taps=taps, n_ref=524288, rate=48000, reps=REPS, t30_s=round(float(t30), 4), centres=d["centres"], mix=row["mix"],
                      mean_after=round(row["mean_after"], 4), **res)))
