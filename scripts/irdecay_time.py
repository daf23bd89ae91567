"""Time of mc_ir_decay on one 441 000-tap stereo IR (BASELINE config 3, n_ref 524288): the broadband row alone and with 10
band-passed rows (the octaves 31.5 Hz .. 16 kHz), next to mc_load_ir of the same IR.  Warm engine: one call first, then REPS
timed ones.  Prints one JSON line (median / min ms; host clock around `Convolution.ir_decay` / `Convolution.prepare`)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
OCTAVES = (31.5, 63, 125, 250, 500, 1000, 2000, 4000, 8000, 16000)
ir = make_ir(441000, seed=5, norm=0.05)
c = Convolution("decay", 524288, max_batch=64, device=0, sample_rate=48000)


def timed(call):
    call()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3))


res = dict(load=timed(lambda: c.prepare(0, ir)), decay_0_bands=timed(lambda: c.ir_decay(0)),
           decay_10_bands=timed(lambda: c.ir_decay(0, bands=OCTAVES)), decay_10_bands_curve=timed(lambda: c.ir_decay(0, bands=OCTAVES, curve_points=1024)))
row = c.ir_decay(0)["rows"][(0, "LR")]
taps = c.ir_info(0)["taps"]
c.close()
print(json.dumps(dict(ir_frames=441000, taps=taps, n_ref=524288, rate=48000, reps=REPS, t30_s=round(row["t30"], 4), **res)))
