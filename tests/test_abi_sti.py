"""mc_sti_query as ctypes sees it against what include/mcconv.h documents, the defaults field by field, and every bad field
refused in the struct's order before the engine is looked at (no GPU: the library's checks touch no device)."""
import ctypes as C
import os
import re

import numpy as np

from ir_sti_np import ALPHA, BETA, MAX_BANDS, MAX_MOD, MOD_HZ, OCTAVES, f32

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcconv.h")


def _default():
    from cuda_audio_amd import _lib

    q = _lib.McStiQuery()
    _lib.load().mc_default_sti_query(C.byref(q))
    return q


def test_the_struct_has_its_documented_size():
    from cuda_audio_amd import _lib

    src = open(HEADER).read()
    size = int(re.search(r"sizeof\(mc_sti_query\) = (\d+)", src).group(1))
    assert C.sizeof(_lib.McStiQuery) == size == _default().struct_size == 272
    assert int(re.search(r"#define MC_STI_MAX_BANDS (\d+)", src).group(1)) == _lib.MC_STI_MAX_BANDS == MAX_BANDS
    assert int(re.search(r"#define MC_STI_MAX_MOD (\d+)", src).group(1)) == _lib.MC_STI_MAX_MOD == MAX_MOD
    assert {"mc_default_sti_query", "mc_ir_sti"} <= set(_lib.SYMBOLS)


def test_the_defaults_field_by_field():
    q = _default()
    assert (q.rate, q.n_bands, q.n_mod, q.flags, q.end, list(q.reserved)) == (44100, 7, 14, 0, 0, [0, 0])
    assert (q.q, q.onset_db) == (f32(1.41421356), -20.0)
    assert list(q.centre_hz) == [f32(v) for v in OCTAVES]
    assert list(q.alpha) == list(ALPHA)
    assert list(q.beta) == list(BETA)
    assert list(q.snr_db) == [0.0] * 7
    assert list(q.mod_hz) == [f32(v) for v in MOD_HZ] + [0.0, 0.0]
    assert abs(sum(q.alpha) - sum(q.beta) - 1.0) <= 1e-12  # (the weights' one internal check)


def _query(**fields):
    q = _default()
    q.rate = 48000
    for k, v in fields.items():
        if isinstance(v, tuple):
            for j, x in enumerate(v):
                getattr(q, k)[j] = x
        else:
            setattr(q, k, v)
    return q


def _call(q, rows=True, mtf=True, sti=True, info=True, engine=None):
    from cuda_audio_amd import _lib

    L = _lib.load()
    dp = C.POINTER(C.c_double)
    r, m, s, i = np.zeros(8 * 3 * 4), np.zeros(8 * 3 * 16), (C.c_double * 3)(), (C.c_uint64 * 2)()
    rc = L.mc_ir_sti(engine, 0, C.byref(q) if q is not None else None, r.ctypes.data_as(dp) if rows else None, m.ctypes.data_as(dp) if mtf else None,
                     s if sti else None, i if info else None)
    return rc, L.mc_last_error().decode()


NAN = float("nan")
BAD_FIELDS = [("struct_size", dict(struct_size=268)), ("rate", dict(rate=7999)), ("n_bands", dict(n_bands=8)), ("n_mod", dict(n_mod=0)),
              ("n_mod", dict(n_mod=17)), ("flags", dict(flags=2)), ("flags", dict(flags=3)), ("centre_hz[0]", dict(centre_hz=(5.0,))),
              ("centre_hz[6]", dict(rate=16000)), ("alpha[0]", dict(alpha=(-0.1,))), ("alpha[0]", dict(alpha=(NAN,))), ("beta[0]", dict(beta=(-0.1,))),
              ("beta[0]", dict(beta=(float("inf"),))), ("snr_db[0]", dict(flags=1, snr_db=(NAN,))), ("snr_db[0]", dict(flags=1, snr_db=(-61.0,))),
              ("snr_db[6]", dict(flags=1, snr_db=(0.0,) * 6 + (121.0,))), ("mod_hz[0]", dict(mod_hz=(0.05,))), ("mod_hz[0]", dict(mod_hz=(NAN,))),
              ("mod_hz[13]", dict(mod_hz=tuple(MOD_HZ[:13]) + (50.5,))), ("q 0.05", dict(q=0.05)), ("q nan", dict(q=NAN)), ("onset_db", dict(onset_db=1.0)),
              ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, 1)))]


def test_every_field_is_refused_before_the_engine_is_looked_at():
    rc, msg = _call(None)
    assert rc == -1 and "null query" in msg
    for name, fields in BAD_FIELDS:
        rc, msg = _call(_query(**fields))
        assert rc == -1 and name in msg, (name, fields, rc, msg)
    # in the struct's order: of two bad fields the earlier one is named
    order = [("rate", dict(rate=1)), ("n_bands", dict(n_bands=99)), ("n_mod", dict(n_mod=99)), ("flags", dict(flags=4)), ("centre_hz[0]", dict(centre_hz=(1.0,))),
             ("alpha[1]", dict(alpha=(0.1, -1.0))), ("beta[2]", dict(beta=(0.1, 0.1, -1.0))), ("mod_hz[3]", dict(mod_hz=(1.0, 1.0, 1.0, 99.0))),
             ("q 100", dict(q=100.0)), ("onset_db", dict(onset_db=5.0)), ("reserved", dict(reserved=(7, 7)))]
    for (first, a), (_, b) in zip(order, order[1:]):
        rc, msg = _call(_query(**dict(a, **b)))
        assert rc == -1 and first in msg, (first, msg)
    # what is not used is not looked at; the good edges pass the query and stop at the engine
    for fields in (dict(n_bands=0, centre_hz=(NAN,), alpha=(NAN,)), dict(n_bands=1, beta=(NAN,)), dict(snr_db=(NAN,)), dict(n_mod=1, mod_hz=(0.1, 99.0)),
                   dict(n_mod=16, mod_hz=(50.0,) * 16), dict(flags=1, snr_db=(-60.0, 120.0)), dict(alpha=(0.0,), beta=(0.0,)), dict(end=1)):
        rc, msg = _call(_query(**fields))
        assert rc == -1 and "null engine" in msg, (fields, msg)
