"""The transforms of long settled batches read bin by bin against the oracle (tests/spectral_probe.py): the overlap-save form
(csrc/ossave.hip.h, fast_levels 253: one 512 x 8192-point transform per segment), the fused second-level transform (k_g2_mac,
254: 256 bins x 8192 points along the block axis) and the split one (k_f2_fwd / k_f2_prod, 255: 256 bins x 16384 points).
Their other tests feed white noise and assert one whole-signal RMS, in which a fault at one bin or one pair of bins of a
2^22-point transform is diluted by 2048; here the stream carries narrow-band probes at the rows, columns and partners where
the index algebra of these passes can go wrong, once as they are and once mirrored, and the error is read at each line.

The bar on `worst` (the largest error line in units of S, the rms of the wet lines) is derived, not measured: every wet line
is at least 0.1 S (asserted on the oracle), so a coefficient that is structurally wrong - a wrong partner, a wrong conjugate,
a wrong table entry - errs by the order of the line, >= 0.1; float32 rounding through a 2^22-point transform leaves about 1e-6;
1e-4 lies two decades from either.  Measured: DESIGN.md §2.5a.  Every case also holds every block of the window to the
oracle (whole-window RMS <= RMS_TOL, the worst 256-frame block <= 2 RMS_TOL)."""
import functools

import numpy as np
import pytest

from helpers import BASE, RMS_TOL, _dry, rms
from spectral_probe import (AMP, DC, LARGE_BINS, LARGE_D, N_OS, NOISE_AMP, SEED, SMALL_BINS, dc_heavy_stream, describe, probe_errors,
                            probe_stream)

pytestmark = pytest.mark.gpu

WORST_BAR = 1e-4
P0, P1 = dict(BASE, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)
# n_ref, IRs (taps, seed), P16, probe bins, window = N / d frames: the last 16384 / d blocks of the stream
TIERS = {
    # the smallest shape at which these kernels run (a segment is 2^22 frames whatever the batch); the window holds the seam
    # between the two long batches and a segment's wrap
    "small": dict(n_ref=8192, irs=((7000, 11), (6500, 22)), p16=32, bins=SMALL_BINS, d=1),
    # 345 partitions: the split form takes IRs from 256 partitions on (fft2_applies), and the overlap of the segments differs
    "large": dict(n_ref=131072, irs=((88200, 5678), (80000, 5680)), p16=352, bins=LARGE_BINS, d=LARGE_D),
}
FORMS = {
    "overlap_save": (253, dict(MCCONV_OS="1", MCCONV_FFA_LEVELS="0")),
    "fused": (254, dict(MCCONV_OS="0", MCCONV_FFT2="1", MCCONV_FFT2_FUSED="1", MCCONV_FFT2_WORK="1", MCCONV_FFA_LEVELS="0")),
    "split": (255, dict(MCCONV_OS="0", MCCONV_FFT2="1", MCCONV_FFT2_FUSED="0", MCCONV_FFA_LEVELS="0")),
}


def _sizes(tier):
    hop = 16384 - TIERS[tier]["p16"]
    return [TIERS[tier]["p16"] + 400, hop, hop]  # (the first one: the cold-start ramp leaves the window)


def _irs(tier):
    from cuda_audio_amd.synth import make_ir

    return [make_ir(taps, seed=seed, norm=0.02) for taps, seed in TIERS[tier]["irs"]]


@functools.lru_cache(maxsize=2)
def _stream_and_window(tier, kind):
    """The stream ("plain", "mirrored": the probes; "dc_heavy": the goldens' inputs scaled up), the oracle's window at its end
    and the dry mix there, computed once per stream."""
    import oracle

    t = TIERS[tier]
    nb, win = sum(_sizes(tier)), 16384 // t["d"]
    if kind == "dc_heavy":
        x = dc_heavy_stream(nb * 256)
    else:
        x = probe_stream(nb * 256, t["bins"], N_OS, AMP, NOISE_AMP, DC, SEED, mirror=kind == "mirrored")
    u = oracle.Upols(t["n_ref"], True)
    for i, ir in enumerate(_irs(tier)):
        u.prepare(i, ir)
    u.set(0, **P0)
    u.set(1, **P1)
    want = u.range(x[0], x[1], nb - win, win)
    u.close()
    dry = _dry(x[:, (nb - win) * 256:], P0, P1)
    for a in (x, want, dry):
        a.setflags(write=False)
    return x, want, dry


def _engine_window(monkeypatch, tier, form, x):
    """The stream through the engine as three device-resident batches; the window at its end, the form each batch took and
    the overlap-save counters."""
    import torch

    from cuda_audio_amd.engine import Convolution

    for k, v in FORMS[form][1].items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MCCONV_OS_MIN", raising=False)
    t, sizes = TIERS[tier], _sizes(tier)
    c = Convolution("probe", t["n_ref"], max_batch=max(sizes), stream_threshold=8)
    for i, ir in enumerate(_irs(tier)):
        c.prepare(i, ir)
    c.cc[0].value.update(**P0)
    c.cc[1].value.update(**P1)
    d_in = torch.from_numpy(x).to("cuda:0")
    d_out = torch.zeros(2, x.shape[1], device="cuda:0")
    c.enable_kernel_timing(True)
    levels, o = [], 0
    for n in sizes:
        c.process_device(d_in[0, o * 256:].data_ptr(), d_in[1, o * 256:].data_ptr(), d_out[0, o * 256:].data_ptr(), d_out[1, o * 256:].data_ptr(), n)
        c.sync()
        levels.append(c.kernel_stats()["fast_levels"])
        o += n
    st = c.os_stats()
    c.close()
    win = 16384 // t["d"]
    return d_out[:, (o - win) * 256:].cpu().numpy(), levels, st


def _check(monkeypatch, tier, form, kind):
    t = TIERS[tier]
    x, want, dry = _stream_and_window(tier, kind)
    bins = [] if kind == "dc_heavy" else t["bins"]
    # 1. the oracle alone: every read-out line stands clear of zero, the reference's clamp of the wet sum (Q4) stays out
    wet = want - dry
    r0 = probe_errors(want.astype(np.float32), want, dry, bins, N_OS, t["d"])
    print(f"oracle: floor {r0['floor']:.3f}, S {r0['S']:.3e}, wet peak {np.abs(wet).max():.3f}, rms(want) {rms(want):.4f}")
    assert r0["floor"] >= 0.1
    assert np.abs(wet).max() < 0.5
    assert rms(want) > 0.01
    got, levels, st = _engine_window(monkeypatch, tier, form, x)
    assert levels[1:] == [FORMS[form][0]] * 2, levels
    assert st["batches"] >= 2 if form == "overlap_save" else st["batches"] == 0, st
    r = probe_errors(got, want, dry, bins, N_OS, t["d"], Ww=r0["Ww"])
    print(f"{tier} {form} {kind}: {describe(r)}")
    # 2. bin by bin
    assert r["worst"] <= WORST_BAR, describe(r)
    # 3. every block of the window
    assert r["rms"] <= RMS_TOL and r["worst_block"] <= 2 * RMS_TOL, describe(r)


# (ordered by stream: the oracle's window is computed once per (tier, stream) and shared by the forms)
CASES = [(tier, form, kind) for tier in TIERS for kind in ("plain", "mirrored") for form in FORMS if tier == "large" or form != "split"]


@pytest.mark.parametrize("tier,form,kind", CASES, ids=["-".join(c) for c in CASES])
def test_probed_bins_match_the_oracle(oracle_mod, gpu_lib, monkeypatch, tier, form, kind):
    _check(monkeypatch, tier, form, kind)


@pytest.mark.parametrize("tier", list(TIERS))
def test_overlap_save_with_heavy_dc_and_alternating_inputs(oracle_mod, gpu_lib, monkeypatch, tier):
    """in1 = 0.2 + noise, in2 = 0.2 (-1)^n + noise: the Q1/Q2 block sums {S1, S2, A1, A2} are about 50 instead of about 3, and
    the column pass's sixteen partial sums and the prefix kernels carry the result.  The error lines at bins 0 and N/2 in units
    of the wet line at bin 0 (the reference leaves its Nyquist bin unwritten: the oracle's wet line at N/2 is null, and the
    engine's has to be)."""
    _check(monkeypatch, tier, "overlap_save", "dc_heavy")
