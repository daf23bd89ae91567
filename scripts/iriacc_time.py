"""Time of mc_ir_iacc on one 441 000-tap stereo IR (BASELINE config 3, n_ref 524288) at 48 kHz: the default lag (T = 48: 97 lags),
T = 1024 (2049 lags, 1.8e9 fma) and ten octave bands at the default lag, next to mc_load_ir and the broadband mc_ir_decay of the
same IR.  Warm engine: one call first, then REPS timed ones.  Prints one JSON line (median / min ms; host clock around
`Convolution.ir_iacc` / `ir_decay` / `prepare`)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution  # noqa: E402
from cuda_audio_amd.synth import make_ir  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
BANDS = (31.5, 63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0, 16000.0)
ir = make_ir(441000, seed=5, norm=0.05)
c = Convolution("iacc", 524288, max_batch=64, device=0, sample_rate=48000)


def timed(call):
    call()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(float(np.min(ms)), 3))


res = dict(load=timed(lambda: c.prepare(0, ir)), decay_0_bands=timed(lambda: c.ir_decay(0)))
res.update(iacc_default=timed(lambda: c.ir_iacc(0)), iacc_default_curve=timed(lambda: c.ir_iacc(0, curve=True)),
           iacc_lag_1024=timed(lambda: c.ir_iacc(0, max_lag=1024)), iacc_10_bands=timed(lambda: c.ir_iacc(0, bands=BANDS)),
           decay_10_bands=timed(lambda: c.ir_decay(0, bands=BANDS)))
a = c.ir_iacc(0)
taps = c.ir_info(0)["taps"]
c.close()
print(json.dumps(dict(ir_frames=441000, taps=taps, n_ref=524288, rate=48000, reps=REPS, max_lag=a["max_lag"], origin=a["origin"],
                      iacc={w: round(a["rows"][(0, w)]["iacc"], 4) for w in ("early", "late", "all")}, **res)))
