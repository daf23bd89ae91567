"""Load time of one 441 000-frame stereo IR (BASELINE config 3, n_ref 524288): mc_load_ir against mc_load_ir_shaped with
trim -20 dB : 16 + reverse + decay 6000 + fade 512 + energy 0.25, at equal rates and converted 44.1 -> 48 kHz.  Prints one
JSON line (median / min ms of REPS loads each after one that allocates; host clock around `Convolution.prepare`)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrShape  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
ir = make_ir(441000, seed=5, norm=0.05)
shape = IrShape(trim_db=-20, pre_roll=16, reverse=True, decay_t60=6000, fade_out=512, normalize="energy", target=0.25)
c = Convolution("load", 524288, max_batch=64, device=0, sample_rate=48000)
res = {}
for name, rate, sh in (("mc_load_ir", 48000, None), ("mc_load_ir_shaped", 48000, shape), ("mc_load_ir_resampled", 44100, None),
                       ("mc_load_ir_shaped_resampled", 44100, shape)):
    c.prepare(0, ir, ir_rate=rate, shape=sh)  # (first load allocates)
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.prepare(0, ir, ir_rate=rate, shape=sh)
        ms.append((time.perf_counter() - t0) * 1e3)
    res[name] = dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), taps=c.ir_info(0)["taps"])
c.close()
print(json.dumps(dict(ir_frames=441000, n_ref=524288, reps=REPS, **res)))
