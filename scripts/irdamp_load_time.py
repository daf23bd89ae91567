"""Load time of one 441 000-frame stereo IR (BASELINE config 3, n_ref 524288) through mc_load_ir_damped with one crossover and
with three, next to the same load with damping off (mc_load_ir_eq with no band on, which is mc_load_ir: the yardstick), with
two EQ bands (what three crossovers are expected to cost about as much as) and with three crossovers under eight bands.  Warm
engine: one load that allocates, then REPS timed ones.  Prints one JSON line (median / min ms; host clock around
`Convolution.prepare`)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrDamp, IrEq  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
ir = make_ir(441000, seed=5, norm=0.05)
bands8 = IrEq(bands=[("lowcut", 60, 0, 1.0), ("lowshelf", 200, 6.0), ("peak", 400, -12.0, 4.0), ("peak", 1000, 6.0, 2.0),
                     ("peak", 2500, 3.5, 0.3), ("peak", 5200, -18.0, 16.0), ("highshelf", 6000, -9.0, 0.5), ("highcut", 15000, 0, 0.9)])
bands2 = IrEq(bands=[("lowcut", 120), ("peak", 2500, 6.0, 1.5)])
damp1 = IrDamp(xovers=(1000,), decay=(0, 48000), origin=480)
damp3 = IrDamp(xovers=(250, 2000, 8000), decay=(0, 96000, 48000, 24000), origin=480)
c = Convolution("load", 524288, max_batch=64, device=0, sample_rate=48000)
res = {}
for name, eq, damp in (("damping_off", IrEq(), None), ("2_bands", bands2, None), ("1_xover", None, damp1), ("3_xovers", None, damp3),
                       ("3_xovers_8_bands", bands8, damp3)):
    c.prepare(0, ir, eq=eq, damp=damp)  # (first load allocates)
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        c.prepare(0, ir, eq=eq, damp=damp)
        ms.append((time.perf_counter() - t0) * 1e3)
    res[name] = dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3), taps=c.ir_info(0)["taps"])
c.close()
print(json.dumps(dict(ir_frames=441000, n_ref=524288, rate=48000, reps=REPS, **res)))
