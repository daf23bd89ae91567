"""mc_ir_parts as ctypes sees it against what include/mcconv.h documents: the size, every offset, the defaults field by field, the
flag macros, and mc_ir_parts_info's MC_ERR_STATE (no GPU for the layout; the getter needs an engine)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")

OFFSETS = dict(struct_size=0, mode=4, flags=8, reserved0=12, direct_end=16, early_end=24, xfade=32, delay=40, gain_db=52, width=64, balance=76,
               frames_out=88, reserved=96)


def test_the_struct_has_its_documented_layout_and_defaults():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_ir_parts\) = (\d+)", src).group(1))
    p = _lib.McIrParts()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    _lib.load().mc_default_ir_parts(C.byref(p))
    assert C.sizeof(_lib.McIrParts) == size == p.struct_size == 104 and size % 8 == 0 and C.alignment(_lib.McIrParts) == 8
    assert {n: getattr(_lib.McIrParts, n).offset for n, _ in _lib.McIrParts._fields_} == OFFSETS
    assert (p.mode, p.flags, p.reserved0, p.direct_end, p.early_end, list(p.xfade), list(p.delay)) == (_lib.MC_PARTS_OFF, 0, 0, 0, 0, [0, 0], [0, 0, 0])
    assert (list(p.gain_db), list(p.width), list(p.balance), p.frames_out, list(p.reserved)) == ([0.0] * 3, [1.0] * 3, [0.0] * 3, 0, [0, 0])
    assert re.search(r"enum \{ MC_PARTS_OFF = 0, MC_PARTS_ON = 1 \};", src)
    assert re.search(r"#define MC_PARTS_MUTE\(p\) \(1u << \(p\)\)", src) and re.search(r"#define MC_PARTS_SWAP\(p\) \(1u << \(4 \+ \(p\)\)\)", src)
    assert re.search(r"#define MC_PARTS_INVERT\(p\) \(1u << \(8 \+ \(p\)\)\)", src)
    assert re.search(r"#define MC_ABI_VERSION 1\b", src)
    assert {"mc_default_ir_parts", "mc_ir_parts_plan", "mc_ir_parts_at", "mc_load_ir_parts", "mc_load_ir_sweep_parts", "mc_ir_parts_info"} <= set(_lib.SYMBOLS)
    # the struct's fields in the header's order, as the refusals name them
    body = re.search(r"typedef struct \{([^}]*)\} mc_ir_parts;", src).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert names == [n for n, _ in _lib.McIrParts._fields_]
    # values only: no field is a pointer
    assert not re.search(r"\*", re.sub(r"/\*.*?\*/", "", body))
    _lib.load().mc_default_ir_parts(None)  # (a null pointer is left alone)


def test_the_python_dataclass_fills_the_struct():
    from cuda_audio_amd.engine import IrParts

    p = IrParts(direct_end=5, early_end=90, xfade=(4, 10), delay=(0, -3, 20), gain_db=-4.0, width=(1.0, 0.3, 1.7), balance=0.25, mute=("direct",),
                swap=("early", "late"), invert="late", frames_out=77).to_c()
    assert (p.mode, p.flags, p.direct_end, p.early_end, list(p.xfade), list(p.delay), p.frames_out) == (1, 0x1 | 0x60 | 0x400, 5, 90, [4, 10], [0, -3, 20], 77)
    assert list(p.gain_db) == [-4.0] * 3 and list(p.balance) == [0.25] * 3 and np.allclose(list(p.width), [1.0, 0.3, 1.7], rtol=1e-7)
    assert IrParts(mode="off").to_c().mode == 0 and not IrParts(mode="off").on()
    for bad in (dict(mute=("middle",)), dict(mode="maybe"), dict(delay=(1, 2))):
        with pytest.raises(ValueError):
            IrParts(**bad).to_c()


@pytest.mark.gpu
def test_the_info_getter_needs_a_load_with_the_step_on(gpu_lib):
    from cuda_audio_amd import _lib
    from cuda_audio_amd.engine import Convolution, IrParts, IrShape

    c = Convolution("abiparts", 16384, sample_rate=48000, stream_threshold=8, max_batch=8)
    x = np.zeros((300, 2), np.float32)
    x[3] = 1.0
    out = (C.c_double * 10)()
    assert c._L.mc_ir_parts_info(c._h, 0, out) == -1 and "not loaded" in c._L.mc_last_error().decode()
    c.prepare(0, x, shape=IrShape(fade_out=10))
    assert c._L.mc_ir_parts_info(c._h, 0, out) == _lib.load().mc_ir_parts_info(c._h, 0, out) == -3
    assert "was not loaded with a parts step" in c._L.mc_last_error().decode()
    c.prepare(0, x, parts=IrParts(mode="off"))
    with pytest.raises(_lib.McError) as err:
        c.ir_parts_info(0)
    assert err.value.code == -3
    c.prepare(0, x, parts=IrParts(direct_end=10, early_end=10))
    info = c.ir_parts_info(0)
    assert (info["frames"], info["frames_out"], info["direct_end"], info["early_end"], info["lost"]) == (300, 300, 10, 10, 0)
    assert info["energy_direct"] == 2.0 and info["energy_early"] == info["energy_late"] == 0.0 and info["energy_out"] == 2.0
    c.prepare(0, x)  # a plain load takes the information away again
    with pytest.raises(_lib.McError):
        c.ir_parts_info(0)
    c.close()
