"""Time of mc_ir_floor with three crossovers (five row groups) and of an extending tail load (mc_load_ir_tail, four bands) at
F' = 2^20 and 2^24 frames, 48 kHz, next to the same load without the tail step (the upload, the shaping stage, the transforms).
Warm engine: one call of each kind that allocates, then REPS timed ones, alternating.  Prints one JSON line per size (median /
min ms; host clock around the call, which ends in a stream synchronise).  For k_tail_chunk's own time run this under
`rocprofv3 --kernel-trace --stats`, in a run of its own.  SIZES=20 (or 24, or 20,24) picks the sizes; MODE=cut times a cutting
tail in place of the extending one (k_tail_chunk without the noise)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_audio_amd.engine import Convolution, IrTail  # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
MODE = os.environ.get("MODE", "extend")
RATE = 48000
XOVERS = (250, 2000, 8000)
for log2 in (int(s) for s in os.environ.get("SIZES", "20,24").split(",")):
    F = 1 << log2
    rng = np.random.default_rng(1)
    m = np.arange(F, dtype=np.float64)
    ir = (0.05 * rng.standard_normal((F, 2)) * (10.0 ** (-4.0 * m / F) + 10.0 ** -2.5)[:, None]).astype(np.float32)  # 80 dB over its length, a floor at -50
    c = Convolution("tail", 2 * F, max_batch=8, device=0, sample_rate=RATE)
    tail = IrTail(mode=MODE, xovers=XOVERS, knee=(F // 2,) * 4, t60=(F // 4,) * 4, level_db=((-75.0, -75.0),) * 4, fade=RATE // 100, seed=1)
    kinds = {"plain": lambda: c.prepare(0, ir), MODE: lambda: c.prepare(0, ir, tail=tail), "floor": lambda: c.ir_floor(0, xovers=XOVERS)}
    for call in kinds.values():  # (first calls allocate)
        call()
    ms = {k: [] for k in kinds}
    for _ in range(REPS):
        for k, call in kinds.items():
            t0 = time.perf_counter()
            call()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    res = {k: dict(median_ms=round(float(np.median(v)), 3), min_ms=round(float(np.min(v)), 3)) for k, v in ms.items()}
    floor = c.ir_floor(0, xovers=XOVERS)["rows"][(0, "LR")]
    info = c.ir_tail_info(0)
    c.close()
    print(json.dumps(dict(frames=F, n_ref=2 * F, reps=REPS, bands=info["bands"], knee_found=round(floor["knee"], 1), **res)), flush=True)
