"""What the six mc_ir_*_info getters remember is the LAST load's: a plain mc_load_ir onto an index whose load went through every
source and step leaves none of it behind.  (Each tool's own test file checks its getter after its own load; none reloads across
all six kinds.)  A sweep and a synthesis cannot be one load, so two indices carry the six kinds between them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE = 48000
KINDS = ("shape", "damp", "synth", "sweep", "tail", "room")


def _known(c, idx):
    """the kinds whose getter answers for IR idx; every other one must say MC_ERR_STATE"""
    from cuda_audio_amd._lib import McError

    known = set()
    for kind in KINDS:
        try:
            getattr(c, f"ir_{kind}_info")(idx)
            known.add(kind)
        except McError as ex:
            assert ex.code == -3, (kind, ex)
    return known


@pytest.mark.parametrize("form", ["partitioned", "single"])
def test_a_plain_reload_forgets_all_six_kinds_of_facts(gpu_lib, form):
    from cuda_audio_amd.engine import Convolution, IrDamp, IrRoom, IrSynth, IrTail, Sweep, sweep_frames

    c = Convolution("reload", 4096, sample_rate=RATE, max_batch=8, form=form)
    tail = IrTail(mode="extend", knee=(200,), t60=(300,), level_db=((-60.0, -62.0),), fade=16, seed=5)
    c.prepare_synth(0, IrSynth(frames=800, seed=3, t60=300, late_gain=0.3, direct=1.0), room=IrRoom(order=2), damp=IrDamp(), tail=tail)
    sw = Sweep(frames=256, f1_hz=100.0, f2_hz=20000.0, rate=RATE)
    rec = np.zeros((600, 2), np.float32)
    rec[10:266, 0] = rec[10:266, 1] = sweep_frames(sw)
    c.prepare_sweep(1, rec, sw, ir_frames=300)
    assert _known(c, 0) == {"shape", "damp", "synth", "tail", "room"} and _known(c, 1) == {"shape", "sweep"}
    plain = np.zeros((300, 2), np.float32)
    plain[0] = 1.0
    for idx in (0, 1):
        c.prepare(idx, plain)
        assert _known(c, idx) == set()
        assert c.ir_info(idx)["taps"] == 300
    c.close()
