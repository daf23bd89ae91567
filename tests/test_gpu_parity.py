"""GPU parity tests: HIP engine (through the C ABI) vs the float64 oracle.

Sizes are chosen so the oracle finishes in seconds; BASELINE-size cases use the
partitioned oracle form (proven equal to the single-FFT restatement to 1e-16 in
tests/test_oracle.py) and size-independent properties.
"""
import os

import numpy as np
import pytest

from helpers import BASE, RMS_TOL, apply_params, rms

pytestmark = pytest.mark.gpu


def _conv(**kw):
    from cuda_audio_amd.engine import Convolution

    # tests keep batches short for the oracle's sake: lower the stream/resident switch-over (default 96 blocks)
    # so that batches of >= 8 blocks run the resident kernel and shorter ones / single periods the streaming one
    kw.setdefault("stream_threshold", 8)
    return Convolution("test", **kw)


def test_abi_loads_and_creates(gpu_lib):
    assert gpu_lib.mc_abi_version() == 1
    c = _conv(fftSize=4096, max_batch=8)
    assert c.num_irs() == 0
    c.close()


def test_ir_spectra_match_numpy(gpu_lib):
    """prepare(): per-partition 512-point spectra vs numpy rfft (conv.cu:207-253 restated per partition)."""
    from cuda_audio_amd.synth import make_ir

    ir = make_ir(1000, seed=3)
    c = _conv(fftSize=4096, max_batch=8)
    c.prepare(0, ir)
    H = c.ir_spectra(0)  # [2][P][256]
    P = H.shape[1]
    assert P == 4
    for ch in range(2):
        for p in range(P):
            seg = np.zeros(512)
            part = ir[p * 256 : (p + 1) * 256, ch]
            seg[: len(part)] = part
            ref = np.fft.rfft(seg)
            got = H[ch, p]
            assert abs(got[0].real - ref[0].real) < 2e-5  # packed DC
            assert abs(got[0].imag - ref[256].real) < 2e-5  # packed Nyquist
            assert np.abs(got[1:] - ref[1:256]).max() < 2e-5
    info = c.ir_info(0)
    assert info["taps"] == 1000 and info["partitions"] == 4
    np.testing.assert_allclose(info["sigma"], ir.astype(np.float64).sum(axis=0), rtol=1e-12)
    c.close()


CASES = {
    "defaults": (dict(BASE), dict(BASE, select=1)),
    "unequal": (
        dict(BASE, predelay=300, wet=0.7, dry=0.3, panWet=0.25, panDry=-0.5, level=0.9),
        dict(BASE, select=1, predelay=17, wet=0.4, dry=0.6, panWet=-0.75, panDry=0.1, level=0.8),
    ),
    "predelay1024": (dict(BASE, predelay=1024), dict(BASE, select=1)),
    "hardpan": (dict(BASE, panWet=1.0, panDry=-1.0), dict(BASE, select=1, panWet=-1.0, panDry=1.0)),
    "slowfade": (dict(BASE, vsteps=20), dict(BASE, select=1, vsteps=7)),
}


def _small_setup(oracle_mod, n_ref, nb, case, taps=(2500, 2800), three_mult=True):
    # taps + 255 <= n_ref - predelay for every case here: the reference's tail drop (Q8) is tested separately
    from cuda_audio_amd.synth import make_input, make_ir

    x = make_input(nb * 256)
    irs = [make_ir(taps[0], seed=11, norm=0.05), make_ir(taps[1], seed=22, norm=0.05)]
    p0, p1 = CASES[case]
    ref = oracle_mod.RefCompat(n_ref, three_mult)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    return x, irs, (p0, p1), ref.process(x[0], x[1])


@pytest.mark.parametrize("case", list(CASES))
def test_batch_matches_refcompat(oracle_mod, gpu_lib, case):
    """Resident (batch) kernel path vs the single-FFT restatement, cold start, N_ref = 4096."""
    nb = 96
    x, irs, (p0, p1), want = _small_setup(oracle_mod, 4096, nb, case)
    c = _conv(fftSize=4096, max_batch=48)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    apply_params(c, p0, p1, False)
    got = c.process(x[0], x[1])
    assert c.kernel_stats()["launches"] == 0
    err = rms(got - want)
    assert err <= RMS_TOL, f"{case}: rms {err:.3e} (signal {rms(want):.3e})"
    c.close()


@pytest.mark.parametrize("case", ["defaults", "unequal", "slowfade"])
def test_jack_path_matches_refcompat(oracle_mod, gpu_lib, case):
    """onProcess (one block per call, streaming MAC kernel) vs the restatement."""
    nb = 40
    x, irs, (p0, p1), want = _small_setup(oracle_mod, 4096, nb, case)
    c = _conv(fftSize=4096, max_batch=4)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    apply_params(c, p0, p1, False)
    got = np.zeros((2, nb * 256), np.float32)
    for b in range(nb):
        s = slice(b * 256, (b + 1) * 256)
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
    err = rms(got - want)
    assert err <= RMS_TOL, f"{case}: rms {err:.3e}"
    assert c.avgRuntime() > 0
    c.close()


def _golden():
    import glob
    import os

    return sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))


@pytest.mark.parametrize("path", _golden(), ids=[p.split("/")[-1][:-4] for p in _golden()])
@pytest.mark.parametrize("max_batch", [24, 1])
def test_engine_matches_golden_vectors(gpu_lib, path, max_batch):
    """Committed golden vectors (numpy restatement of conv.cu) through both MAC kernels."""
    import json

    z = np.load(path, allow_pickle=False)
    p0, p1 = json.loads(str(z["params"]))
    c = _conv(fftSize=int(z["n_ref"]), max_batch=max_batch, stream_threshold=8)
    c.prepare(0, z["ir0"])
    c.prepare(1, z["ir1"])
    apply_params(c, p0, p1, False)
    got = c.process(z["x"][0], z["x"][1])
    err = rms(got - z["expected"])
    assert err <= RMS_TOL, f"rms {err:.3e}"
    c.close()


def test_batch_split_invariance(gpu_lib):
    """Same stream cut into different batch sizes (incl. ragged and stream-kernel sizes) gives the same output."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = 150
    x = make_input(nb * 256)
    ir = make_ir(3000, seed=5, norm=0.05)
    outs = []
    for mb in (64, 37, 5):
        c = _conv(fftSize=8192, max_batch=mb)
        c.prepare(0, ir)
        outs.append(c.process(x[0], x[1]))
        c.close()
    assert rms(outs[0] - outs[1]) < 2e-7
    assert rms(outs[0] - outs[2]) < 2e-7


def test_linear_mode_matches_direct_convolution(oracle_mod, gpu_lib):
    """compat=0, config-1 shape: 1024-tap IR, exact time-domain convolution as ground truth."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = 40
    x = make_input(nb * 256)
    ir = make_ir(1024, seed=9, norm=0.05)
    c = _conv(fftSize=4096, max_batch=40, compat=False)
    c.prepare(0, ir)
    c.cc[0].value.update(dry=0.0, wet=1.0, vsteps=0)
    c.cc[1].value.update(dry=0.0, wet=1.0, vsteps=0)
    # settle the cross-fade (Q7) on silence, then run the signal
    z = np.zeros(80 * 256, np.float32)
    c.process(z, z)
    got = c.process(x[0], x[1])
    n = nb * 256
    wantL = oracle_mod.direct_conv(x[0], ir[:, 0])[:n] + oracle_mod.direct_conv(x[1], ir[:, 0])[:n]
    wantR = oracle_mod.direct_conv(x[0], ir[:, 1])[:n] + oracle_mod.direct_conv(x[1], ir[:, 1])[:n]
    assert rms(got[0] - wantL) <= RMS_TOL and rms(got[1] - wantR) <= RMS_TOL
    c.close()


def test_config2_2s_ir(oracle_mod, gpu_lib):
    """BASELINE config 2: stereo, 2 s IR (88 200 taps), N_ref = 131072; oracle = partitioned form."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = 600
    x = make_input(nb * 256)
    ir = make_ir(88200, seed=5678, norm=0.02)
    o = oracle_mod.Upols(131072, True)
    o.prepare(0, ir)
    want = o.process(x[0], x[1])
    c = _conv(fftSize=131072, max_batch=256)
    c.prepare(0, ir)
    got = c.process(x[0], x[1])
    assert np.abs(want).max() < 1.0
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    c.close()


def test_config3_10s_ir(oracle_mod, gpu_lib):
    """BASELINE config 3 (headline): stereo, 10 s IR (441 000 taps, P = 1723), N_ref = 524288."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = 768
    x = make_input(nb * 256)
    ir = make_ir(441000, seed=5678, norm=0.02)
    o = oracle_mod.Upols(524288, True)
    o.prepare(0, ir)
    want = o.process(x[0], x[1])
    c = _conv(fftSize=524288, max_batch=256)
    c.prepare(0, ir)
    assert c.ir_info(0)["partitions"] == 1723
    assert c.algorithmic_bytes_per_block() == 6 * 1723 * 2048
    got = c.process(x[0], x[1])
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    c.close()


def test_sharded_partials_sum_to_unsharded(gpu_lib):
    """§8(e): G virtual shards on one device — sum of partial wet blocks then finish == unsharded engine."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    nb, T = 128, 64
    x = make_input(nb * 256)
    ir = make_ir(20000, seed=7, norm=0.02)  # 79 partitions -> shards of 32
    full = _conv(fftSize=32768, max_batch=T)
    full.prepare(0, ir)
    want = full.process(x[0], x[1])
    full.close()
    shards = [_conv(fftSize=32768, max_batch=T, part_begin=b, part_end=b + 32) for b in (0, 32, 64)]
    for s in shards:
        s.prepare(0, ir)
    dev = torch.device("cuda:0")
    got = np.zeros_like(want)
    for o in range(0, nb, T):
        xin = torch.from_numpy(x[:, o * 256 : (o + T) * 256].copy()).to(dev)
        parts = [torch.zeros(2 * T * 256, device=dev) for _ in shards]
        for s, p in zip(shards, parts):
            s.partial_device(xin[0].data_ptr(), xin[1].data_ptr(), p.data_ptr(), T)
            s.sync()
        total = parts[0] + parts[1] + parts[2]
        out = torch.zeros(2, T * 256, device=dev)
        for s in shards:
            s.finish_device(xin[0].data_ptr(), xin[1].data_ptr(), total.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), T)
            s.sync()
        got[:, o * 256 : (o + T) * 256] = out.cpu().numpy()
    for s in shards:
        s.close()
    assert rms(got - want) < 5e-7


def test_two_batches_in_flight_and_retire_only(gpu_lib):
    """Sharded pipeline: partial(k+1) may be issued before finish(k); a rank that does not need the output
    retires batches with NULL buffers.  Results equal the plain batch call."""
    import torch

    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.synth import make_input, make_ir

    nb, T = 96, 32
    x = make_input(nb * 256)
    ir = make_ir(6000, seed=7, norm=0.02)
    plain = _conv(fftSize=16384, max_batch=T)
    plain.prepare(0, ir)
    want = plain.process(x[0], x[1])
    plain.close()
    dev = torch.device("cuda:0")
    a = _conv(fftSize=16384, max_batch=T)  # keeps the output
    b = _conv(fftSize=16384, max_batch=T)  # "non-root": retires only
    for c in (a, b):
        c.prepare(0, ir)
    xin = torch.from_numpy(x).to(dev)
    parts = [torch.zeros(2 * T * 256, device=dev) for _ in range(2)]
    out = torch.zeros(2, nb * 256, device=dev)
    nbat = nb // T
    for k in range(nbat + 1):
        if k < nbat:
            s = xin[:, k * T * 256:(k + 1) * T * 256]
            for c in (a, b):
                c.partial_device(s[0].data_ptr(), s[1].data_ptr(), parts[k % 2].data_ptr(), T)
                c.sync()
        if k >= 1:
            j = k - 1
            s = xin[:, j * T * 256:(j + 1) * T * 256]
            o = out[:, j * T * 256:(j + 1) * T * 256]
            a.finish_device(s[0].data_ptr(), s[1].data_ptr(), parts[j % 2].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T)
            b.finish_device(None, None, None, None, None, T)
            a.sync()
    assert a.blocks_processed() == nb and b.blocks_processed() == nb
    assert rms(out.cpu().numpy() - want) < 1e-7
    # a third partial without a finish is refused
    s = xin[:, : T * 256]
    a.partial_device(s[0].data_ptr(), s[1].data_ptr(), parts[0].data_ptr(), T)
    a.partial_device(s[0].data_ptr(), s[1].data_ptr(), parts[1].data_ptr(), T)
    with pytest.raises(McError):
        a.partial_device(s[0].data_ptr(), s[1].data_ptr(), parts[0].data_ptr(), T)
    a.close()
    b.close()


def test_jack_path_pan_change_is_exact(oracle_mod, gpu_lib):
    """panWet / level / dry changes between periods: the streaming path keeps per-block pans with the delay
    line (and speculates the next period's sweep), so it follows the reference exactly, where the values
    current at block t scale the whole contribution of input block t (conv.cu:386-401)."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref = 60, 8192
    x = make_input(nb * 256)
    irs = [make_ir(5000, seed=11, norm=0.05), make_ir(4000, seed=22, norm=0.05)]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=4)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    ref.set(1, select=1)
    c.cc[1].value.select = 1
    events = {12: (0, dict(panWet=0.5)), 20: (1, dict(panWet=-0.25, level=0.7)), 33: (0, dict(dry=0.1, panDry=0.75)),
              41: (0, dict(panWet=-1.0))}
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    for b in range(nb):
        if b in events:
            half, kw = events[b]
            ref.set(half, **kw)
            c.cc[half].value.update(**kw)
        s = slice(b * 256, (b + 1) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e}"
    c.close()


def test_speculative_sweep_is_invisible(gpu_lib):
    """The next period's partition sweep is launched speculatively after each period; an IR switch, a batch call
    or a reset in between must invalidate it.  The same events played twice give identical samples (both runs
    speculate: the library has no switch that turns speculation off)."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = 50
    x = make_input(nb * 256)
    irs = [make_ir(5000, seed=11, norm=0.05), make_ir(4000, seed=22, norm=0.05)]

    def run():
        c = _conv(fftSize=8192, max_batch=8)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        out = np.zeros((2, nb * 256), np.float32)
        b = 0
        while b < nb:
            if b == 10:
                c.cc[0].value.select = 1  # IR switch: the speculated sweep used the old IR
            if b == 20:  # a batch call in the middle of single periods
                s = slice(b * 256, (b + 6) * 256)
                out[:, s] = c.process(x[0, s], x[1, s])
                b += 6
                continue
            if b == 35:
                c.prepare(1, irs[0])  # reload an IR in place
            s = slice(b * 256, (b + 1) * 256)
            out[0, s], out[1, s] = c.onProcess(x[0, s], x[1, s])
            b += 1
        c.close()
        return out

    a, bb = run(), run()
    assert np.abs(a).max() > 0.01
    assert rms(a - bb) < 1e-7


@pytest.mark.parametrize("taps,n_ref", [(441000, 524288), (1323000, 2097152)], ids=["10s_P1723", "30s_P5168"])
def test_full_length_impulse_response(gpu_lib, taps, n_ref):
    """Size-independent property at BASELINE sizes (configs 3 and 5 shapes, true-stereo 2x2 IR matrix):
    a unit impulse on input 1 resp. input 2 returns the selected IR's L/R taps, scaled by the cold-start
    cross-fade coefficient wet/5 (Q7, conv.cu:27), over every one of the P partitions.  compat=0 (linear)."""
    from cuda_audio_amd.synth import make_ir

    P = (taps + 255) // 256
    nb = P + 3
    irs = [make_ir(taps, seed=5678), make_ir(taps, seed=5680)]
    c = _conv(fftSize=n_ref, max_batch=512, compat=False)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    assert c.ir_info(0)["partitions"] == P
    for h in (0, 1):
        c.cc[h].value.update(select=h, dry=0.0, wet=1.0, level=1.0, panWet=0.0, vsteps=0)
    for inp in (0, 1):
        c.reset()
        x = np.zeros((2, nb * 256), np.float32)
        x[inp, 5] = 1.0
        y = c.process(x[0], x[1])
        want = np.zeros((2, nb * 256))
        want[:, 5 : 5 + taps] = 0.2 * irs[inp].T.astype(np.float64)  # e(0) = wet / 5
        err = np.abs(y - want).max()
        assert err < 2e-6, f"input {inp}: max err {err:.3e} (IR peak {np.abs(irs[inp]).max():.3e})"
        # the tail partitions really carry signal
        assert np.abs(y[:, (P - 2) * 256 :]).max() > 1e-7
    c.close()


def test_config4_eight_channels_sharded(oracle_mod, gpu_lib):
    """BASELINE config 4 shape: 8 channels = 4 stereo `Convolution` pairs (main.cu:31-39 makes one object per
    pair), each with IR partitions sharded over G engines whose partial blocks are summed.  One GPU, virtual
    shards; checked per pair against the oracle."""
    import torch

    from cuda_audio_amd.sharded import shard_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    nb, T, n_ref, G = 64, 32, 32768, 4
    dev = torch.device("cuda:0")
    for pair in range(4):
        x = make_input(nb * 256, seed=100 + 10 * pair)
        ir = make_ir(25000, seed=40 + pair, norm=0.02)  # 98 partitions
        o = oracle_mod.Upols(n_ref, True)
        o.prepare(0, ir)
        want = o.process(x[0], x[1])
        bounds = [shard_bounds(98, G, g) for g in range(G)]
        shards = [_conv(fftSize=n_ref, max_batch=T, part_begin=a, part_end=b) for a, b in bounds if b > a]
        for s in shards:
            s.prepare(0, ir)
        got = np.zeros_like(want)
        xin = torch.from_numpy(x).to(dev)
        for k in range(nb // T):
            sl = xin[:, k * T * 256 : (k + 1) * T * 256]
            parts = [torch.zeros(2 * T * 256, device=dev) for _ in shards]
            for s, p in zip(shards, parts):
                s.partial_device(sl[0].data_ptr(), sl[1].data_ptr(), p.data_ptr(), T)
                s.sync()
            total = torch.stack(parts).sum(0)
            out = torch.zeros(2, T * 256, device=dev)
            shards[0].finish_device(sl[0].data_ptr(), sl[1].data_ptr(), total.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), T)
            shards[0].sync()
            for s in shards[1:]:
                s.finish_device(None, None, None, None, None, T)
            got[:, k * T * 256 : (k + 1) * T * 256] = out.cpu().numpy()
        for s in shards:
            s.close()
        err = rms(got - want)
        assert err <= RMS_TOL, f"pair {pair}: rms {err:.3e}"


@pytest.mark.parametrize("n_ref,taps,pd", [(4096, (2500, 3072), 1024), (4096, (3072, 3072), 2000), (16384, (15360, 9000), 8128)],
                         ids=["default_predelay", "pd2000", "max_predelay"])
@pytest.mark.parametrize("jack", [False, True, "tiles"], ids=["batch", "jack", "batch_time_domain"])
def test_q8_tail_drop_is_reproduced(oracle_mod, gpu_lib, n_ref, taps, pd, jack, monkeypatch):
    """Q8: with taps + 255 + predelay > N_ref the reference discards what the predelay shifts past N_ref
    (conv.cu:94-98).  The shipped defaults are in that regime (predelay 1024, IRs truncated to N-1024).
    Slowly decaying IRs so that the discarded tail is far above the tolerance.  Batches recompute the cut terms in the
    frequency domain (k_drop_fft; partition sums over the last partitions), single periods and MCCONV_TD_FFT=0 in the
    time domain (tiles): all three against the same oracle."""
    from cuda_audio_amd.synth import make_input

    if jack == "tiles":
        monkeypatch.setenv("MCCONV_TD_FFT", "0")  # (read when the engine is created)
        jack = False

    nb = 3 * n_ref // 256 // 2 + 40
    x = make_input(nb * 256)
    rng = np.random.default_rng(5)
    irs = []
    for L in taps:
        h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
        irs.append((h * np.sqrt(0.004 / L)).astype(np.float32))
    p0, p1 = dict(BASE, predelay=pd), dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=37)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    want = ref.process(x[0], x[1])
    if jack:
        got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256]))
                              for b in range(nb)], axis=1)
    else:
        got = c.process(x[0], x[1])
    # the discarded part is well above the bar: a linear engine would fail here
    lin = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        lin.prepare(i, ir)
    apply_params(lin, p0, p1, True)
    assert rms(lin.process(x[0], x[1]) - want) > 5 * RMS_TOL
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    c.close()


def test_q8_parked_periods_carry_the_next_periods_cut_terms(oracle_mod, gpu_lib):
    """JACK path in the Q8 regime once the parameters are steady (the cold-start ramp takes ~160 calls): every period is
    parked one call ahead, and the launch that carries it also sums the cut terms of the period after it (k_jack's last
    workgroup) - no launch of their own.  A controller change in between (predelay 1024 -> 1088 -> 1024: a new epoch, the
    carried terms are stale) must fall back to k_drop_period_fft; the samples are the oracle's throughout."""
    from cuda_audio_amd.synth import make_input

    n_ref, L, nb = 4096, 3072, 300
    x = make_input(nb * 256, seed=53)
    rng = np.random.default_rng(59)
    h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
    ir = (h * np.sqrt(0.004 / L)).astype(np.float32)
    p0, p1 = dict(BASE, predelay=1024), dict(BASE, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=8)
    ref.prepare(0, ir)
    c.prepare(0, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    events = {230: 1088, 262: 1024}
    for b in range(nb):
        if b in events:
            ref.set(0, predelay=events[b])
            c.cc[0].value.predelay = events[b]
        s = slice(b * 256, (b + 1) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
    stats, parks = c.drop_stats(), c.park_stats()
    c.close()
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e}) {stats} {parks}"
    if not any(os.environ.get(k) for k in ("MCCONV_NO_PARK", "MCCONV_NO_SPIN", "MCCONV_TD_FFT")):
        assert parks["used"] > 40 and stats["carried_periods"] > 40, (stats, parks)


def test_q8_carried_cut_terms_do_not_survive_a_park_timeout(oracle_mod, gpu_lib, monkeypatch):
    """Round-3 advice (medium): in the Q8 regime the launch parked for period b also sums the cut terms of period b + 2 into the
    buffer of b's parity.  When the host stays away longer than the park time, the tail of b gives up and is launched again -
    and that launch's own cut terms (k_drop_period_fft for block b) overwrite the same buffer, while the engine still held the
    carried terms of b + 2 to be valid: two calls later b + 2 was finished with b's terms (wrong by a whole Q8 term).  unpark()
    now forgets the carried terms.  Settled stream, pauses of 60 ms against a park time of 20 ms, the oracle's samples throughout."""
    import time

    from cuda_audio_amd.synth import make_input

    monkeypatch.setenv("MCCONV_PARK_MS", "20")
    n_ref, L, nb = 4096, 3072, 260
    x = make_input(nb * 256, seed=57)
    rng = np.random.default_rng(61)
    h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
    ir = (h * np.sqrt(0.004 / L)).astype(np.float32)
    p0, p1 = dict(BASE, predelay=1024), dict(BASE, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=8)
    ref.prepare(0, ir)
    c.prepare(0, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    for b in range(nb):
        if b in (200, 215, 230):
            time.sleep(0.06)
        s = slice(b * 256, (b + 1) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
    stats, parks = c.drop_stats(), c.park_stats()
    c.close()
    per_block = np.sqrt(((got - want) ** 2).reshape(2, nb, 256).mean(axis=(0, 2)))
    assert per_block.max() <= 2 * RMS_TOL, f"worst block {int(per_block.argmax())}: {per_block.max():.3e} {stats} {parks}"
    assert rms(got - want) <= RMS_TOL
    if not any(os.environ.get(k) for k in ("MCCONV_NO_PARK", "MCCONV_NO_SPIN", "MCCONV_TD_FFT")):
        assert parks["timed_out"] >= 1 and stats["carried_periods"] > 10, (stats, parks)


@pytest.mark.parametrize("period,pd", [(1024, 256), (512, 700), (1024, 0)])
@pytest.mark.parametrize("jack", [False, True], ids=["batch", "jack"])
def test_q8_begins_earlier_for_longer_calls(oracle_mod, gpu_lib, period, pd, jack):
    """The reference transforms a whole call at once: a call of pm blocks contributes taps + 256 pm - 1 frames, and what passes
    n_ref frames after the START of the call is cut.  With taps = n_ref - 1024 and a 1024-frame period that happens from predelay 1
    on - not from 770 on, as for calls of one block, which is where the engine switched its pass on until tests/fuzz/fuzz_q8.py ran
    longer periods against the oracle (11 of 141 runs off by up to 5e-4).  (1024, 0): the boundary, nothing cut."""
    from cuda_audio_amd.synth import make_input

    n_ref, L, pm = 4096, 3072, period // 256
    ncalls = (3 * n_ref // 256 // 2 + 24) // pm
    x = make_input(ncalls * period, seed=41)
    rng = np.random.default_rng(43)
    irs = []
    for k in range(2):
        h = rng.standard_normal((L - 40 * k, 2)) * np.exp(-np.arange(L - 40 * k) / (2.0 * L))[:, None]
        irs.append((h * np.sqrt(0.004 / L)).astype(np.float32))
    p0, p1 = dict(BASE, predelay=pd), dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=6 * pm, period=period)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    want = ref.process(x[0], x[1], block=period)
    step = 1 if jack else 5
    parts = []
    for k in range(0, ncalls, step):
        s = slice(k * period, min(k + step, ncalls) * period)
        parts.append(np.stack(c.onProcess(x[0, s], x[1, s])) if jack else c.process(x[0, s], x[1, s]))
    got = np.concatenate(parts, axis=1)
    c.close()
    if pd:  # the cut terms are well above the bar: an engine that does not see the regime fails
        lin = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            lin.prepare(i, ir)
        apply_params(lin, p0, p1, True)
        assert rms(lin.process(x[0], x[1], block=period) - want) > 5 * RMS_TOL
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("jack", [False, True], ids=["batch", "jack"])
def test_q8_one_voice_with_irs_of_different_length(oracle_mod, gpu_lib, jack):
    """A voice pairs half 0's IR with half 1's.  Here one is 60 partitions long and the other 40, at n_ref = 16384 with an
    unaligned predelay of 4736 frames: the cut terms of the long one run over partitions 44 .. 59, which the short one does not
    have - and its partition-major copy of the last partitions (k_h_tail: 48 of them) ends 11 partitions earlier.  Found by
    tests/fuzz/fuzz_q8.py (seed 5002: a memory access fault - the sum reads both IRs' entries unconditionally and must take the
    short one's from the zero-padded bank there)."""
    from cuda_audio_amd.synth import make_input

    n_ref, pd, taps = 16384, 4736, (10000, 15360)
    nb = n_ref // 256 + 70
    x = make_input(nb * 256, seed=29)
    rng = np.random.default_rng(31)
    irs = []
    for L in taps:
        h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (1.5 * L))[:, None]
        irs.append((h * np.sqrt(0.003 / L)).astype(np.float32))
    p0, p1 = dict(BASE, predelay=pd), dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=40)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    want = ref.process(x[0], x[1])
    if jack:
        got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256])) for b in range(nb)], axis=1)
    else:
        got = np.concatenate([c.process(x[0, o * 256:min(o + 40, nb) * 256], x[1, o * 256:min(o + 40, nb) * 256]) for o in range(0, nb, 40)], axis=1)
    c.close()
    lin = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        lin.prepare(i, ir)
    apply_params(lin, p0, p1, True)
    assert rms(lin.process(x[0], x[1]) - want) > 5 * RMS_TOL  # (the cut terms matter)
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("sizes", [[120, 120, 60], [150, 1, 1, 148], [70, 230]], ids=["even", "periods_between", "short_then_long"])
def test_q8_history_across_long_batches(oracle_mod, gpu_lib, sizes):
    """Q8 with batches longer than the look-back of the pass (one reference length + the largest predelay):
    k_fwd keeps only the tail of such a batch in the input-history ring; the next call - a batch or single
    periods - must find everything it looks back to."""
    from cuda_audio_amd.synth import make_input

    n_ref, taps, pd = 4096, (2500, 3072), 1024
    nb = sum(sizes)
    x = make_input(nb * 256)
    rng = np.random.default_rng(5)
    irs = []
    for L in taps:
        h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
        irs.append((h * np.sqrt(0.004 / L)).astype(np.float32))
    p0, p1 = dict(BASE, predelay=pd), dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=max(sizes))
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    want = ref.process(x[0], x[1])
    parts, o = [], 0
    for n in sizes:
        seg = x[:, o * 256:(o + n) * 256]
        parts.append(np.stack(c.onProcess(seg[0], seg[1])) if n == 1 else c.process(seg[0], seg[1]))
        o += n
    got = np.concatenate(parts, axis=1)
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    c.close()


@pytest.mark.parametrize("period,form,pd", [(256, "fft", 1100), (512, "fft", 1100), (1024, "fft", 1100), (512, "tiles", 1100), (256, "fft", 1024)])
def test_q8_with_crossfading_irs_and_longer_periods(oracle_mod, gpu_lib, period, form, pd, monkeypatch):
    """The Q8 regime with everything that shapes its cut terms at once: two IRs of different length cross-fading on one half
    (two voices with their own gains per block), an unaligned predelay (three slices of the last partitions' segments
    contribute), and reference calls of 2 and 4 blocks (the cut is measured from the start of the CALL: block distances
    differ inside a call).  Batches of whole calls, both forms of the cut terms, against oracle.RefCompat run call by call.
    Predelay 1024 with calls of one block is the shipped shape - every output block loses ONE term of ONE source block, here of two
    cross-fading voices with gains per block - which the forward transforms sum themselves (k_fwd<true>)."""
    from cuda_audio_amd.synth import make_input

    if form == "tiles":
        monkeypatch.setenv("MCCONV_TD_FFT", "0")
    n_ref, pm = 4096, period // 256
    ncalls = (3 * n_ref // 256 // 2 + 44) // pm
    x = make_input(ncalls * period, seed=91)
    rng = np.random.default_rng(17)
    irs = []
    for L in (3072, 2800, 3000):
        h = rng.standard_normal((L, 2)) * np.exp(-np.arange(L) / (2.0 * L))[:, None]
        irs.append((h * np.sqrt(0.004 / L)).astype(np.float32))
    p0, p1 = dict(BASE, predelay=pd, speed=9), dict(BASE, select=1, level=0.9, speed=14)
    ref = oracle_mod.RefCompat(n_ref, True)
    per = 6 if pd != 1024 else 30  # (calls per batch; the one-term shape needs batches longer than its 16 blocks of reach)
    c = _conv(fftSize=n_ref, max_batch=per * pm, period=period)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    switches = {ncalls // 2 - 3: (0, 2), ncalls // 2 + 4: (1, 0), ncalls - 20 // pm: (0, 1)}  # call index -> (half, IR)
    got = np.zeros((2, ncalls * period), np.float32)
    want = np.zeros((2, ncalls * period))
    k = 0
    while k < ncalls:
        if k in switches:
            half, ir = switches[k]
            ref.set(half, select=ir, vsteps=(p0, p1)[half]["speed"])
            c.cc[half].value.update(select=ir, vsteps=(p0, p1)[half]["speed"])
        n = min(per - 1, ncalls - k, min([q for q in switches if q > k] + [ncalls]) - k)
        s = slice(k * period, (k + n) * period)
        want[:, s] = ref.process(x[0, s], x[1, s], block=period)
        got[:, s] = c.process(x[0, s], x[1, s])
        k += n
    stats = c.drop_stats()
    c.close()
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    # the form under test is the form that ran
    if os.environ.get("MCCONV_TD_FFT") == "0" and form != "tiles":
        form = "tiles"  # (the whole suite under that switch)
    if form == "tiles":
        assert stats["tiles"] > 0 and stats["drop_fft"] == stats["forward_transforms"] == 0, stats
    elif form == "fft" and pd == 1024:
        assert stats["forward_transforms"] > 0 and stats["tiles"] == 0, stats
    else:
        assert stats["drop_fft"] > 0 and stats["forward_transforms"] == stats["tiles"] == 0, stats


@pytest.mark.parametrize("jack", [False, True], ids=["batch", "jack"])
def test_live_ir_switch_crossfade(oracle_mod, gpu_lib, jack):
    """select CCs while audio runs.  The reference pulls its live spectra towards the newly
    selected IR over `speed` blocks (f_interpolate, conv.cu:15-32, 255-276, 339-353); the engine runs the
    outgoing and incoming IRs as two voices whose coefficients follow the same recurrence.  Includes a
    switch back before the first fade has finished, different speeds per half and a wet change mid-fade."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref = 140, 8192
    x = make_input(nb * 256)
    irs = [make_ir(5000, seed=11, norm=0.05), make_ir(4000, seed=22, norm=0.05), make_ir(6000, seed=33, norm=0.05)]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=16)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    cmap = (21, 22, 23, 24, 25, 26, 27, 28)
    # (block, half, controller, value): select = v * 3 / 128 -> IR index; speed = v * 1024 / 128
    events = [(0, 0, 25, 2), (0, 1, 25, 1), (10, 0, 21, 64), (30, 1, 21, 100), (38, 0, 21, 0), (50, 0, 24, 90),
              (70, 0, 21, 127), (70, 1, 21, 0)]
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))

    class Dev:
        pass

    dev = Dev()
    for half in (0, 1):
        cc = c.cc[half]
        cc.device, cc.message = dev, 176
        cc.select, cc.predelay, cc.dry, cc.wet, cc.speed, cc.panDry, cc.panWet, cc.level = cmap
    step = 1 if jack else 5
    b = 0
    while b < nb:
        n = 1 if jack else min(step, nb - b)
        if not jack:
            # a batch may not straddle an event: cut it at the next one
            nxt = min([ev[0] for ev in events if ev[0] > b] + [nb])
            n = min(n, nxt - b)
        for ev in events:
            if ev[0] == b:
                _, half, ctl, val = ev
                oracle_mod.handle_cc(ref.cc(half), cmap, ctl, val, ref.num_irs())
                # one physical controller per half here: address the half directly through the C ABI
                import ctypes as C

                arr = (C.c_uint8 * 8)(*cmap)
                assert c._L.mc_handle_cc(c._h, half, arr, ctl, val) == 0
        s = slice(b * 256, (b + n) * 256)
        for k in range(n):
            ss = slice((b + k) * 256, (b + k + 1) * 256)
            want[:, ss] = ref.process(x[0, ss], x[1, ss])
        if jack:
            got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        else:
            got[:, s] = c.process(x[0, s], x[1, s])
        b += n
    assert ref.cc(0).select == 2 and ref.cc(1).select == 0
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    c.close()


# fp16 storage of spectra and delay line (BASELINE config 5): stated separately from the fp32 bar.
# Half has an 11-bit significand: each stored value carries <= 2^-11 relative error, products of two
# stored values ~7e-4, and the errors of the ~P*4 terms of a bin are independent, so the output error is
# ~1e-3 of the signal.  Bar: RMS error <= 2e-3 x RMS signal.
FP16_REL_TOL = 2e-3


def test_config5_fp16_streaming_mac_parity(oracle_mod, gpu_lib):
    """True-stereo 2x2 IR matrix, fp16 spectra + delay line, fp32 accumulation, vs the float64 oracle."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref = 420, 131072
    x = make_input(nb * 256)
    irs = [make_ir(88200, seed=5678, norm=0.02), make_ir(88200, seed=5680, norm=0.02)]
    o = oracle_mod.Upols(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=32, precision="fp16")
    for i, ir in enumerate(irs):
        o.prepare(i, ir)
        c.prepare(i, ir)
    o.set(1, select=1)
    c.cc[1].value.select = 1
    want = o.process(x[0], x[1])
    got = c.process(x[0], x[1])
    assert c.algorithmic_bytes_per_block() == 6 * 345 * 256 * 4
    wet_err = rms(got - want)
    # compare against the wet part only (the dry half of the output is exact in either precision)
    wet = want - 0.5 * (x[0] + x[1])
    assert wet_err <= FP16_REL_TOL * rms(wet), f"rms err {wet_err:.3e} vs wet rms {rms(wet):.3e}"
    assert wet_err > 1e-7  # it really is the reduced-precision path
    # one period at a time through the same storage (JACK path) agrees with the batch
    c.reset()
    nj = 40
    gj = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256]))
                         for b in range(nj)], axis=1)
    assert rms(gj - want[:, : nj * 256]) <= FP16_REL_TOL * rms(wet[:, : nj * 256]) + 1e-6
    c.close()


def test_config5_fp16_full_length_30s(gpu_lib):
    """30 s IRs (P = 5168), fp16 storage: an impulse returns the IR within the fp16 bar over its whole length."""
    from cuda_audio_amd.synth import make_ir

    taps, n_ref = 1323000, 2097152
    P = (taps + 255) // 256
    nb = P + 3
    irs = [make_ir(taps, seed=5678), make_ir(taps, seed=5680)]
    c = _conv(fftSize=n_ref, max_batch=256, compat=False, precision="fp16")
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    for h in (0, 1):
        c.cc[h].value.update(select=h, dry=0.0, wet=1.0, level=1.0, panWet=0.0, vsteps=0)
    x = np.zeros((2, nb * 256), np.float32)
    x[1, 7] = 1.0
    y = c.process(x[0], x[1])
    want = np.zeros((2, nb * 256))
    want[:, 7 : 7 + taps] = 0.2 * irs[1].T.astype(np.float64)
    assert rms(y - want) <= FP16_REL_TOL * rms(want)
    tail = slice((P - 200) * 256, P * 256)  # the -60 dB end of the IR keeps its relative accuracy (per-IR scaling)
    assert rms(y[:, tail] - want[:, tail]) <= 4 * FP16_REL_TOL * rms(want[:, tail])
    c.close()


def test_fp16_engines_take_the_overlap_save_form_for_long_batches(gpu_lib, monkeypatch):
    """mc_config.precision = 1 keeps IR spectra and delay line in fp16 for the partition sweep (single periods, short batches).
    A long settled batch runs as overlap-save segments in either precision - the form's spectra are built from the fp32 taps - so an
    fp16 engine's long batches are the fp32 engine's (1e-6), and the periods that follow go back to the fp16 sweep on the
    delay-line slots the form left (fp16 tolerance)."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    monkeypatch.setenv("MCCONV_OS", "1")  # (the suite is also run with the measurement switches set)
    n_ref, taps, T = 131072, 88200, 13000
    x = make_input((3 * T + 4) * 256)
    ir = make_ir(taps, seed=5678)
    dx = torch.from_numpy(x).cuda()
    outs, levels, per = [], [], []
    for prec in ("fp32", "fp16"):
        c = _conv(fftSize=n_ref, max_batch=T, precision=prec)
        c.prepare(0, ir)
        apply_params(c, dict(BASE), dict(BASE), False)
        c.enable_kernel_timing(True)
        o = torch.zeros(3, 2, T * 256, device="cuda")
        lv = []
        for k in range(3):
            c.process_device(dx[0, k * T * 256:].data_ptr(), dx[1, k * T * 256:].data_ptr(), o[k, 0].data_ptr(), o[k, 1].data_ptr(), T)
            c.sync()
            lv.append(c.kernel_stats()["fast_levels"])
        outs.append(o.cpu().numpy())
        levels.append(lv)
        a = 3 * T * 256
        per.append(np.concatenate([np.stack(c.onProcess(x[0, a + 256 * j:a + 256 * (j + 1)], x[1, a + 256 * j:a + 256 * (j + 1)])) for j in range(4)], axis=1))
        c.close()
    assert levels[0][1:] == [253, 253] and levels[1][1:] == [253, 253], levels
    wet = rms(per[0]) * 0.5
    assert rms(outs[1][1:] - outs[0][1:]) <= 1e-6
    assert rms(per[1] - per[0]) <= FP16_REL_TOL * wet + 1e-6


def test_error_behaviour_and_edge_cases(oracle_mod, gpu_lib):
    """Boundary behaviour of the C ABI: wrong period length, missing IR, oversize batch, oversize IR capacity,
    IR longer than N_ref - 1024 (truncated like conv.cu:239), reset."""
    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.synth import make_input, make_ir

    c = _conv(fftSize=4096, max_batch=8)
    x = make_input(16 * 256)
    with pytest.raises(McError) as ei:  # no IR loaded yet
        c.onProcess(x[0, :256], x[1, :256])
    assert ei.value.code == -3
    ir = make_ir(5000, seed=3, norm=0.05)  # longer than 4096 - 1024: truncated to 3072 taps / 12 partitions
    c.prepare(0, ir)
    assert c.ir_info(0)["taps"] == 3072 and c.ir_info(0)["partitions"] == 12
    with pytest.raises(McError) as ei:  # the engine is built for 256-frame periods (the reference mis-computes > 1024)
        c.onProcess(x[0, :128], x[1, :128])
    assert ei.value.code == -1
    with pytest.raises(McError):
        c.process_device(1, 1, 1, 1, 9)  # more blocks than max_batch
    c.cc[0].value.select = 7
    with pytest.raises(McError):
        c.onProcess(x[0, :256], x[1, :256])  # selected IR not loaded
    c.cc[0].value.select = 0
    ref = oracle_mod.RefCompat(4096, True)
    ref.prepare(0, ir)
    want = ref.process(x[0], x[1])
    got = c.process(x[0], x[1])
    assert rms(got - want) <= RMS_TOL
    # reset returns to the cold state: same input, same output again
    c.reset()
    assert c.blocks_processed() == 0
    assert rms(c.process(x[0], x[1]) - want) <= RMS_TOL
    # silence in, silence out (no DC offsets, no NaNs)
    c.reset()
    z = np.zeros(8 * 256, np.float32)
    out = c.process(z, z)
    assert np.all(out == 0.0)
    c.close()
    with pytest.raises(McError):  # IR needs more partitions than the engine was sized for
        d = _conv(fftSize=8192, max_batch=4, max_partitions=4)
        d.prepare(0, make_ir(3000, seed=1))


def test_ir_cycling_reuses_voice_slots(oracle_mod, gpu_lib):
    """Four IRs selected in turn with three voice slots: a slot is reused once its IR has decayed and its
    last sounding block has left every window; results still follow the reference's interpolated spectra."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref, gap = 520, 8192, 80
    x = make_input(nb * 256)
    irs = [make_ir(3000 + 500 * j, seed=50 + j, norm=0.05) for j in range(4)]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=40)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    for eng_set in (lambda h, **kw: ref.set(h, **kw), lambda h, **kw: c.cc[h].value.update(**kw)):
        eng_set(0, speed=0, vsteps=0)
        eng_set(1, speed=0, vsteps=0, select=1)
    want = np.zeros((2, nb * 256))
    got = np.zeros((2, nb * 256), np.float32)
    for b0 in range(0, nb, 40):
        if b0 and b0 % gap == 0:
            sel = (b0 // gap) % 4
            ref.set(0, select=sel)
            c.cc[0].value.select = sel
            if (b0 // gap) % 2 == 0:
                ref.set(1, select=(sel + 2) % 4)
                c.cc[1].value.select = (sel + 2) % 4
        s = slice(b0 * 256, (b0 + 40) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        got[:, s] = c.process(x[0, s], x[1, s])
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e}"
    c.close()


def test_full_size_resident_vs_streaming_with_events(gpu_lib):
    """BASELINE config-3 size (two 441 000-tap IRs, P = 1723): the resident kernels (uniform and gain-per-slot)
    and the streaming kernel are independent implementations of the same sum; on a 2600-block stream with pan /
    level / wet changes and a live IR switch (two voices sounding for a whole IR length) they must agree."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = 2600
    x = make_input(nb * 256)
    irs = [make_ir(441000, seed=5678), make_ir(441000, seed=5680), make_ir(300000, seed=5690)]
    events = {300: (0, dict(panWet=0.5)), 700: (1, dict(level=0.8, wet=0.4)), 1200: (0, dict(select=2, vsteps=40)),
              1900: (1, dict(panWet=-0.5)), 2300: (0, dict(dry=0.2))}

    def run(max_batch, thr):
        c = _conv(fftSize=524288, max_batch=max_batch, stream_threshold=thr)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        c.cc[1].value.select = 1
        out = np.zeros((2, nb * 256), np.float32)
        b = 0
        while b < nb:
            if b in events:
                half, kw = events[b]
                c.cc[half].value.update(**kw)
            nxt = min([e for e in events if e > b] + [nb])
            n = min(max_batch, nxt - b)
            s = slice(b * 256, (b + n) * 256)
            out[:, s] = c.process(x[0, s], x[1, s])
            b += n
        c.close()
        return out

    res = run(512, 1)       # resident kernels only
    stm = run(100, 101)     # streaming kernel only
    assert np.abs(res).max() > 0.05
    err = rms(res - stm)
    assert err < 2e-6, f"resident vs streaming rms {err:.3e} (signal {rms(res):.3e})"


@pytest.mark.parametrize("period", [512, 1024])
@pytest.mark.parametrize("pd,taps", [(300, (2500, 2800)), (1024, (3072, 3072))], ids=["pd300", "pd1024_taildrop"])
def test_longer_jack_periods(oracle_mod, gpu_lib, period, pd, taps):
    """The reference's run scripts start jackd with 512- (x86) and 1024-frame (Jetson) periods.  Its per-call
    semantics then change — one cross-fade step per call, DC/Nyquist (Q1/Q2) and tail-drop (Q8) windows
    measured from the call start — while the convolution itself is the same.  Engine: 2 / 4 internal blocks per
    period sharing the call's gains and window origin; onProcess and batch calls; cold start included."""
    from cuda_audio_amd.synth import make_input, make_ir

    n_ref, ncalls = 4096, 80
    n = ncalls * period
    x = make_input(n)
    irs = [make_ir(taps[0], seed=11, norm=0.05), make_ir(taps[1], seed=22, norm=0.05)]
    p0 = dict(BASE, predelay=pd, wet=0.7, panWet=0.25, vsteps=9)
    p1 = dict(BASE, select=1, level=0.8)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    want = ref.process(x[0], x[1], block=period)
    # one period per call (what JACK does)
    c = _conv(fftSize=n_ref, max_batch=16, period=period)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    apply_params(c, p0, p1, False)
    got = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period]))
                          for k in range(ncalls)], axis=1)
    err = rms(got - want)
    assert err <= RMS_TOL, f"onProcess: rms {err:.3e}"
    # batches of whole periods through the resident kernel
    c.set_period(256)
    c.set_period(period)  # resets to the cold state
    apply_params(c, p0, p1, False)
    got2 = c.process(x[0], x[1])
    assert rms(got2 - want) <= RMS_TOL
    c.close()
    # an engine declared as a partition shard (here: one shard holding every partition) keeps the batch kernels
    # for its periods, with zero-copy I/O and the completion word raised by k_post
    c = _conv(fftSize=n_ref, max_batch=16, period=period, part_begin=0, part_end=16)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
    apply_params(c, p0, p1, False)
    got3 = np.concatenate([np.stack(c.onProcess(x[0, k * period:(k + 1) * period], x[1, k * period:(k + 1) * period]))
                           for k in range(ncalls)], axis=1)
    assert rms(got3 - want) <= RMS_TOL
    from cuda_audio_amd._lib import McError

    with pytest.raises(McError):
        c.onProcess(x[0, :256], x[1, :256])  # wrong period length
    c.close()


def _run_with_predelay_events(oracle_mod, n_ref, nb, taps, events, mode, period=256, compat=True, p_extra=None, max_batch=None):
    """events: {call index: predelay}.  mode 'jack' = one period per mc_process call, 'batch' = mc_process_batch
    calls cut at the events.  Returns (got, want)."""
    from cuda_audio_amd.synth import make_input, make_ir

    pm = period // 256
    ncalls = nb // pm
    x = make_input(nb * 256)
    irs = [make_ir(taps[0], seed=11, norm=0.05), make_ir(taps[1], seed=22, norm=0.05)]
    p0 = dict(BASE, wet=0.7, panWet=0.25, **(p_extra or {}))
    p1 = dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True) if compat else None
    c = _conv(fftSize=n_ref, max_batch=max_batch or (pm if mode == "jack" else 16 * pm), period=period, compat=compat)
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
        if ref:
            ref.prepare(i, ir)
    apply_params(c, p0, p1, False)
    if ref:
        apply_params(ref, p0, p1, True)
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    q = 0
    while q < ncalls:
        if q in events:
            c.cc[0].value.predelay = events[q]
            if ref:
                ref.set(0, predelay=events[q])
        n = 1
        if mode == "batch":
            nxt = min([e for e in events if e > q] + [ncalls])
            n = min(16, nxt - q)
        s = slice(q * period, (q + n) * period)
        if ref:
            want[:, s] = ref.process(x[0, s], x[1, s], block=period)
        if mode == "jack":
            got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        else:
            got[:, s] = c.process(x[0, s], x[1, s])
        q += n
    c.close()
    return x, irs, (p0, p1), got, want


@pytest.mark.parametrize("mode", ["jack", "batch"])
@pytest.mark.parametrize("period", [256, 512])
def test_predelay_change_keeps_old_blocks_at_their_offset(oracle_mod, gpu_lib, mode, period):
    """A predelay CC while audio runs.  The reference shifts each call's contribution by the predelay current at
    that call (conv.cu:411-415): blocks already played ring out at the old offset.  Up, down, back to zero, and
    two changes closer together than the IR length."""
    nb, n_ref = 120, 8192
    pm = period // 256
    events = {0: 300, 20 // pm: 1500, 50 // pm: 64, 58 // pm: 0, 90 // pm: 4096}
    _, _, _, got, want = _run_with_predelay_events(oracle_mod, n_ref, nb, (5000, 4000), events, mode, period)
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("mode", ["jack", "batch", "batch_time_domain"])
def test_predelay_change_in_the_tail_drop_regime(oracle_mod, gpu_lib, mode, monkeypatch):
    """Predelay changes with taps + 255 + predelay > N_ref (Q8 active before and after; the shipped defaults)."""
    if mode == "batch_time_domain":
        monkeypatch.setenv("MCCONV_TD_FFT", "0")
        mode = "batch"
    nb, n_ref = 100, 4096
    events = {0: 1024, 30: 2000, 55: 1024, 75: 0}
    _, _, _, got, want = _run_with_predelay_events(oracle_mod, n_ref, nb, (3072, 3072), events, mode)
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


def test_predelay_knob_sweep(oracle_mod, gpu_lib):
    """A controller sweep: a new predelay on every period for 40 periods (handleCC steps of 64 frames)."""
    nb, n_ref = 110, 8192
    events = {10 + k: 64 * (k + 1) for k in range(40)}
    events.update({70 + k: 64 * (40 - 3 * k) for k in range(12)})
    _, _, _, got, want = _run_with_predelay_events(oracle_mod, n_ref, nb, (6000, 5000), events, "jack", p_extra=dict(vsteps=7))
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


def test_predelay_change_linear_mode_and_streaming_flush(oracle_mod, gpu_lib):
    """compat = 0 (plain linear convolution): output = sum over epochs of conv(input of the epoch) delayed by the
    epoch's predelay.  max_batch 4 makes the retirement run the streaming MAC in many chunks."""
    nb, n_ref = 64, 8192
    events = {0: 100, 25: 2000, 40: 7}
    x, irs, (p0, p1), got, _ = _run_with_predelay_events(oracle_mod, n_ref, nb, (5000, 4000), events, "jack", compat=False,
                                                        max_batch=4)
    # direct model in float64: settled gains only after the cold-start ramp, so build it from per-block gains
    n = nb * 256
    edges = sorted(events) + [nb]
    want = np.zeros((2, n + 16384))
    e = [0.0, 0.0]
    for b in range(nb):
        pd = [events[k] for k in sorted(events) if k <= b][-1]
        for half, (p, ir) in enumerate(((p0, irs[0]), (p1, irs[1]))):
            v = p["vsteps"] if b == 0 else max(p["vsteps"] - b, 0)
            e[half] += (p["wet"] - e[half]) / (v + 5)
            pw = p["panWet"]
            gl = (1 - pw if pw >= 0 else 1) * p["level"] * e[half]
            gr = (1 + pw if pw <= 0 else 1) * p["level"] * e[half]
            xb = x[half, b * 256:(b + 1) * 256].astype(np.float64)
            yl = np.convolve(xb, ir[:, 0].astype(np.float64))
            yr = np.convolve(xb, ir[:, 1].astype(np.float64))
            o = b * 256 + pd
            want[0, o:o + len(yl)] += gl * yl
            want[1, o:o + len(yr)] += gr * yr
    want = np.clip(want[:, :n], -1, 1)
    for half, p in enumerate((p0, p1)):
        pdry = p["panDry"]
        want[0] += x[half] * p["dry"] * (1 - pdry if pdry >= 0 else 1) * p["level"]
        want[1] += x[half] * p["dry"] * (1 + pdry if pdry <= 0 else 1) * p["level"]
    assert edges[0] == 0
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


def test_predelay_change_sharded(oracle_mod, gpu_lib):
    """Three virtual shards: every shard retires its own partition share; the sum of the partials still equals
    the reference after predelay changes (the partial carries the predelay and the retired tails)."""
    import torch

    from cuda_audio_amd.sharded import partitions_for, shard_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref, T = 96, 16384, 8
    x = make_input(nb * 256)
    irs = [make_ir(12000, seed=11, norm=0.05), make_ir(9000, seed=22, norm=0.05)]
    P = partitions_for(12000, n_ref)
    world = 3
    p0, p1 = dict(BASE, predelay=500, wet=0.7), dict(BASE, select=1)
    ref = oracle_mod.RefCompat(n_ref, True)
    shards = []
    for r in range(world):
        pb, pe = shard_bounds(P, world, r)
        s = _conv(fftSize=n_ref, max_batch=T, part_begin=pb, part_end=pe)
        s.use_torch_stream()
        shards.append(s)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        for s in shards:
            s.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    for s in shards:
        apply_params(s, p0, p1, False)
    events = {24: 3000, 56: 0, 64: 1024}
    dx = torch.from_numpy(x).cuda()
    out = torch.zeros(2, nb * 256, device="cuda")
    want = np.zeros((2, nb * 256))
    parts = [torch.zeros(2 * T * 256, device="cuda") for _ in range(world)]
    for b in range(0, nb, T):
        if b in events:
            ref.set(0, predelay=events[b])
            for s in shards:
                s.cc[0].value.predelay = events[b]
        sl = slice(b * 256, (b + T) * 256)
        want[:, sl] = ref.process(x[0, sl], x[1, sl])
        xin = dx[:, sl].contiguous()
        for s, p in zip(shards, parts):
            s.partial_device(xin[0].data_ptr(), xin[1].data_ptr(), p.data_ptr(), T)
        total = parts[0] + parts[1] + parts[2]
        o = torch.zeros(2, T * 256, device="cuda")
        shards[0].finish_device(xin[0].data_ptr(), xin[1].data_ptr(), total.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T)
        for s in shards[1:]:
            s.finish_device(None, None, None, None, None, T)
        out[:, sl] = o
    torch.cuda.synchronize()
    err = rms(out.cpu().numpy() - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    for s in shards:
        s.close()


@pytest.mark.parametrize("n_ref,taps,pd,period,world,T", [(8192, (5000, 4000), 0, 256, 3, 48), (8192, (5000, 4000), 700, 256, 3, 48),
                                                          (4096, (3072, 3072), 1024, 256, 3, 48), (8192, (6000, 4000), 300, 512, 3, 48),
                                                          (16384, (9000, 15000), 8192, 256, 3, 48),
                                                          (4096, (3072, 3072), 1024, 256, 4, 256), (4096, (2500, 3000), 0, 256, 8, 256)],
                         ids=["pd0", "pd700", "pd1024_taildrop", "period512", "max_predelay", "long_batches_taildrop", "long_batches_8way"])
def test_block_sliced_engines_tile_the_output(oracle_mod, gpu_lib, n_ref, taps, pd, period, world, T):
    """Block-sliced operation (throughput scaling without a collective): three engines are fed the same batches and
    each finishes its slice of the output blocks.  The concatenation equals the reference - through the cold-start
    ramp (per-slot gains), an IR switch with cross-fade and a wet change, for slices that start inside the batch.
    With batches longer than the reference length plus the largest predelay an engine transforms only the blocks its
    windows can reach (the long_batches cases)."""
    import torch

    from cuda_audio_amd._lib import McError
    from cuda_audio_amd.sharded import slice_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    pm = period // 256
    nbat = 5 if T < 100 else 3
    nb = T * nbat
    x = make_input(nb * 256)
    irs = [make_ir(taps[0], seed=11, norm=0.05), make_ir(taps[1], seed=22, norm=0.05), make_ir(taps[0] - 500, seed=33, norm=0.05)]
    p0 = dict(BASE, predelay=pd, wet=0.7, panWet=0.25, speed=20)
    p1 = dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    # slice + reach-back (predelay / 256 + 1 blocks) must fit max_batch
    engines = [_conv(fftSize=n_ref, max_batch=T + 16, period=period) for _ in range(world)]
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        for c in engines:
            c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    for c in engines:
        apply_params(c, p0, p1, False)
        c.use_torch_stream()
    dx = torch.from_numpy(x).cuda()
    out = torch.zeros(2, nb * 256, device="cuda")
    want = np.zeros((2, nb * 256))
    for k in range(nbat):
        if k == 2:  # select CC on half 0 (cross-fade over `speed` calls) and a wet change on half 1
            ref.set(0, select=2, vsteps=20)
            ref.set(1, wet=0.3)
            for c in engines:
                c.cc[0].value.update(select=2, vsteps=20)
                c.cc[1].value.wet = 0.3
        sl = slice(k * T * 256, (k + 1) * T * 256)
        want[:, sl] = ref.process(x[0, sl], x[1, sl], block=period)
        xin = dx[:, sl].contiguous()
        for r, c in enumerate(engines):
            first, count = slice_bounds(T, world, r, pm)
            o = torch.zeros(2, count * 256, device="cuda")
            c.process_slice_device(xin[0].data_ptr(), xin[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T, first, count)
            out[:, (k * T + first) * 256:(k * T + first + count) * 256] = o
    torch.cuda.synchronize()
    err = rms(out.cpu().numpy() - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    # a sliced engine refuses whole-batch and single-period calls and predelay changes until it is reset
    c = engines[1]
    xin = dx[:, : T * 256].contiguous()
    o = torch.zeros(2, T * 256, device="cuda")
    with pytest.raises(McError):
        c.process_device(xin[0].data_ptr(), xin[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T)
    c.cc[0].value.predelay = (pd + 64) % 8192
    with pytest.raises(McError):
        c.process_slice_device(xin[0].data_ptr(), xin[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T, 0, T // 3)
    c.reset()
    c.process_device(xin[0].data_ptr(), xin[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T)
    for c in engines:
        c.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("mode,period,nirs", [("jack", 256, 3), ("batch", 256, 3), ("jack", 512, 3), ("jack", 256, 6),
                                              ("batch", 256, 6), ("jack", 1024, 6)],
                         ids=["jack", "batch", "jack512", "jack_6irs", "batch_6irs", "jack1024_6irs"])
def test_random_controller_traffic(oracle_mod, gpu_lib, seed, mode, period, nirs):
    """Randomised live control: every few calls a random controller message (select, predelay, dry, wet, speed, pans,
    level) on a random half, applied to the restatement and to the engine through handleCC.  With three IRs the
    engine's three voices hold every IR that is still sounding; with six they overflow and merge."""
    import ctypes as C

    from cuda_audio_amd.synth import make_input, make_ir

    rng = np.random.default_rng(seed)
    pm = period // 256
    ncalls, n_ref = 260 // pm, 4096
    nb = ncalls * pm
    x = make_input(nb * 256)
    irs = [make_ir(2500, seed=11, norm=0.05), make_ir(3072, seed=22, norm=0.05), make_ir(1800, seed=33, norm=0.05),
           make_ir(2900, seed=44, norm=0.05), make_ir(900, seed=55, norm=0.05), make_ir(2200, seed=66, norm=0.05)][:nirs]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=16 * pm, period=period)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    cmap = (21, 22, 23, 24, 25, 26, 27, 28)
    arr = (C.c_uint8 * 8)(*cmap)
    events = {}
    q = 0
    while q < ncalls:
        ctl = int(rng.choice(cmap))
        val = int(rng.integers(0, 128))
        if ctl == 25:
            val = int(rng.integers(0, 4))   # speed: cross-fades of at most 24 calls
        if ctl == 28:
            val = int(rng.integers(64, 128))  # level: keep the wet sum inside the clamp (Q4)
        events.setdefault(q, []).append((int(rng.integers(0, 2)), ctl, val))
        q += int(rng.integers(1, 9))
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    q = 0
    while q < ncalls:
        for half, ctl, val in events.get(q, []):
            oracle_mod.handle_cc(ref.cc(half), cmap, ctl, val, ref.num_irs())
            assert c._L.mc_handle_cc(c._h, half, arr, ctl, val) == 0
        n = 1
        if mode == "batch":
            n = min(16, min([e for e in events if e > q] + [ncalls]) - q)
        s = slice(q * period, (q + n) * period)
        want[:, s] = ref.process(x[0, s], x[1, s], block=period)
        if mode == "jack":
            got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        else:
            got[:, s] = c.process(x[0, s], x[1, s])
        q += n
    c.close()
    assert np.abs(want).max() < 1.5
    err = rms(got - want)
    assert err <= RMS_TOL, f"seed {seed}: rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("mode", ["jack", "batch"])
def test_more_irs_crossfading_than_voices(oracle_mod, gpu_lib, mode):
    """A select controller swept across seven IRs faster than any of them can fade out (speed 100 calls): the
    reference blends all of them in its live spectra.  The engine has three voices per half; when a fourth IR
    arrives it renders what the blocks played so far still owe, merges the half's deselected IRs into one spectrum
    (they all decay by the same factor from then on) and carries on - still the reference's output."""
    import ctypes as C

    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref = 260, 8192
    x = make_input(nb * 256)
    irs = [make_ir(3000 + 450 * j, seed=60 + j, norm=0.05) for j in range(7)]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=16)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    cmap = (21, 22, 23, 24, 25, 26, 27, 28)
    arr = (C.c_uint8 * 8)(*cmap)
    # speed 100 on both halves; half 0 sweeps up through the IRs every 5 calls and back, half 1 hops around;
    # a predelay and a wet change in between
    events = {0: [(0, 25, 13), (1, 25, 13), (0, 22, 5)]}
    for k, sel in enumerate([1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1, 0]):
        events.setdefault(10 + 5 * k, []).append((0, 21, int(np.ceil(sel * 128 / 7))))
    for k, sel in enumerate([3, 6, 1, 4, 0, 5, 2]):
        events.setdefault(20 + 9 * k, []).append((1, 21, int(np.ceil(sel * 128 / 7))))
    events.setdefault(57, []).append((0, 22, 40))
    events.setdefault(90, []).append((1, 24, 100))
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    q = 0
    while q < nb:
        for half, ctl, val in events.get(q, []):
            oracle_mod.handle_cc(ref.cc(half), cmap, ctl, val, ref.num_irs())
            assert c._L.mc_handle_cc(c._h, half, arr, ctl, val) == 0
        n = 1 if mode == "jack" else min(16, min([e for e in events if e > q] + [nb]) - q)
        s = slice(q * 256, (q + n) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        if mode == "jack":
            got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        else:
            got[:, s] = c.process(x[0, s], x[1, s])
        q += n
    c.close()
    assert ref.cc(0).select == 0 and ref.cc(1).select == 2
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("max_batch", [256, 4])
def test_predelay_change_and_voice_merge_at_headline_size(oracle_mod, gpu_lib, max_batch):
    """Config-3 size (10 s IRs, P = 1723, N_ref = 524288): predelay changes and a fourth cross-fading IR while
    audio runs, one period per call, against the single-FFT restatement.  The history is re-rendered in launches
    of at least 256 blocks whatever max_batch is (1.3 ms per change here)."""
    import time

    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref = 44, 524288
    x = make_input(nb * 256)
    irs = [make_ir(441000, seed=5678 + j, norm=0.02) for j in range(4)]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=max_batch)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    for half in (0, 1):
        ref.set(half, speed=100, vsteps=0, select=half)
        c.cc[half].value.update(speed=100, vsteps=0, select=half)
    events = {8: dict(predelay=3000), 14: dict(select=2, vsteps=100), 20: dict(select=3, vsteps=100), 26: dict(predelay=0),
              32: dict(select=1, vsteps=100)}  # half 0: IRs 0, 2, 3 sounding -> IR 1 is the fourth
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    worst = 0.0
    for b in range(nb):
        if b in events:
            ref.set(0, **events[b])
            c.cc[0].value.update(**events[b])
        s = slice(b * 256, (b + 1) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        t0 = time.perf_counter()
        got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        if b in events:
            worst = max(worst, time.perf_counter() - t0)
    c.close()
    err = rms(got - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"
    print(f"longest call with a re-render (max_batch {max_batch}): {worst * 1e3:.2f} ms")


@pytest.mark.parametrize("mode", ["jack", "batch"])
def test_fp16_storage_with_predelay_changes_and_voice_merges(oracle_mod, gpu_lib, mode):
    """fp16 storage mode through the history re-renders: predelay changes and a select sweep over five IRs (the
    merged spectrum gets its own fp16 copy and scale).  Bar: the fp16 tolerance of config 5."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb, n_ref = 160, 16384
    x = make_input(nb * 256)
    irs = [make_ir(9000 + 1200 * j, seed=70 + j, norm=0.05) for j in range(5)]
    ref = oracle_mod.RefCompat(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=16, precision="fp16")
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    for half in (0, 1):
        ref.set(half, speed=60, vsteps=0, select=half, dry=0.0)
        c.cc[half].value.update(speed=60, vsteps=0, select=half, dry=0.0)
    events = {12: (0, dict(predelay=1500)), 20: (0, dict(select=2, vsteps=60)), 28: (0, dict(select=3, vsteps=60)),
              36: (0, dict(select=4, vsteps=60)), 44: (1, dict(select=0, vsteps=60)), 52: (1, dict(select=3, vsteps=60)),
              60: (1, dict(select=2, vsteps=60)), 90: (0, dict(predelay=64)), 120: (0, dict(select=1, vsteps=60))}
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    q = 0
    while q < nb:
        if q in events:
            half, kw = events[q]
            ref.set(half, **kw)
            c.cc[half].value.update(**kw)
        n = 1 if mode == "jack" else min(16, min([e for e in events if e > q] + [nb]) - q)
        s = slice(q * 256, (q + n) * 256)
        want[:, s] = ref.process(x[0, s], x[1, s])
        if mode == "jack":
            got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        else:
            got[:, s] = c.process(x[0, s], x[1, s])
        q += n
    c.close()
    err = rms(got - want)  # dry = 0: the output is the wet signal
    assert err <= FP16_REL_TOL * rms(want), f"rms err {err:.3e} vs wet rms {rms(want):.3e}"
    assert err > 1e-7


@pytest.mark.parametrize("levels,n_ref,taps,sizes", [(1, 131072, (88200, 80000, 70000), [3, 4098, 4096]),
                                                      (2, 262144, (140000, 150000, 135000), [3, 4100, 4096]),
                                                      (3, 524288, (280000, 300000, 270000), [5, 8200, 8192])],
                         ids=["one_level_P345", "two_levels_P586", "three_levels_P1172"])
def test_fast_fir_form_of_the_resident_mac(oracle_mod, gpu_lib, monkeypatch, levels, n_ref, taps, sizes):
    """Long batches run the resident MAC in fast-FIR form: the convolution along the block axis is split into the
    polyphase components of the block sequence - three half-rate convolutions (3/4 of the multiply-adds), or nine
    at a quarter of the rate for long IRs (9/16).  Same output as the direct form and as the oracle: through the
    cold-start ramp (per-slot gains), for a batch that starts at an odd block, for a batch length that is not a
    multiple of the tile, and with two voices (IR switch)."""
    from cuda_audio_amd.synth import make_input, make_ir

    nb = sum(sizes)
    x = make_input(nb * 256)
    irs = [make_ir(t, seed=5678 + 2 * j, norm=0.02) for j, t in enumerate(taps)]
    p0, p1 = dict(BASE, predelay=300, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)

    def run(no_ffa):
        monkeypatch.setenv("MCCONV_FFA_LEVELS", "0" if no_ffa else str(levels))
        monkeypatch.setenv("MCCONV_FFT2", "0")  # this test is about the fast-FIR MAC
        c = _conv(fftSize=n_ref, max_batch=max(sizes))
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        out = np.zeros((2, nb * 256), np.float32)
        o = 0
        for k, n in enumerate(sizes):
            if k == 2:
                c.cc[0].value.update(select=2, vsteps=100)  # cross-fade to a third IR during the last batch
            s = slice(o * 256, (o + n) * 256)
            out[:, s] = c.process(x[0, s], x[1, s])
            o += n
        c.enable_kernel_timing(True)
        s = slice(0, sizes[-1] * 256)
        c.process(x[0, s], x[1, s])
        ks = c.kernel_stats()
        c.close()
        return out, ks

    fast, ks_fast = run(False)
    direct, ks_direct = run(True)
    assert ks_fast["fast_levels"] == levels and ks_direct["fast_levels"] == 0
    assert rms(fast - direct) <= 2e-6, f"fast-FIR vs direct: {rms(fast - direct):.3e}"
    assert rms(fast - direct) > 0  # they really are different computations
    # oracle on the first two batches (float64 partitioned form, which models a constant select; the third batch,
    # with the IR switch, is covered by the comparison with the direct form above); the largest case: their start
    nchk = min(sizes[0] + sizes[1], 1000 if n_ref > 262144 else 1 << 30)
    o = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        o.prepare(i, ir)
    apply_params(o, p0, p1, True)
    want = o.process(x[0, : nchk * 256], x[1, : nchk * 256])
    err = rms(fast[:, : nchk * 256] - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("n_ref,taps,T,pd,sliced", [(8192, (5000, 4000), 40, 700, False), (4096, (3072, 3072), 24, 1024, False),
                                                     (131072, (88200, 80000), 4096, 0, False), (8192, (5000, 4000), 48, 300, True)],
                         ids=["small_batches", "taildrop", "fast_fir_batches", "block_slices"])
def test_pipelined_batches_equal_unpipelined(gpu_lib, n_ref, taps, T, pd, sliced):
    """mc_config.pipeline: the inverse transforms and the post stage of batch k run on a second stream under the MAC
    of batch k + 1; nothing is synchronised between the calls, one fence at the end.  Bit-for-bit the output of the
    unpipelined engine (same kernels, same order of arithmetic)."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    nbat = 7
    x = make_input(nbat * T * 256)
    irs = [make_ir(taps[0], seed=11, norm=0.05), make_ir(taps[1], seed=22, norm=0.05)]
    p0, p1 = dict(BASE, predelay=pd, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)
    st = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(st):
        dx = torch.from_numpy(x).cuda()
        for piped in (False, True):
            c = _conv(fftSize=n_ref, max_batch=T + 16, pipeline=piped)
            for i, ir in enumerate(irs):
                c.prepare(i, ir)
            apply_params(c, p0, p1, False)
            c.use_torch_stream(st)
            first, count = (T // 3, T // 3) if sliced else (0, T)
            out = torch.zeros(nbat, 2, count * 256, device="cuda")
            for k in range(nbat):
                if k == 4:
                    c.cc[1].value.wet = 0.3  # a parameter change between two batches in flight
                sl = slice(k * T * 256, (k + 1) * T * 256)
                i1, i2 = dx[0, sl], dx[1, sl]
                if sliced:
                    c.process_slice_device(i1.data_ptr(), i2.data_ptr(), out[k, 0].data_ptr(), out[k, 1].data_ptr(), T, first, count)
                else:
                    c.process_device(i1.data_ptr(), i2.data_ptr(), out[k, 0].data_ptr(), out[k, 1].data_ptr(), T)
            c.fence()
            st.synchronize()
            outs.append(out.cpu().numpy())
            c.close()
    assert rms(outs[0]) > 1e-3
    assert np.array_equal(outs[0], outs[1]), f"rms difference {rms(outs[0] - outs[1]):.3e}"


def test_overlap_add_in_the_inverse_kernel_is_bit_identical(gpu_lib):
    """Whole-batch path: k_inv_wet (inverse transform + overlap-add into the wet ring, tiles of 15 blocks + the block
    before them) for batch lengths around the tile size, with a predelay, single periods in between and a predelay
    change: two runs of the same events on fresh engines give the same bits (the tiles' hand-over through the segment
    ring depends on nothing but the batch)."""
    from cuda_audio_amd.synth import make_input, make_ir

    sizes = [1, 14, 15, 16, 1, 17, 29, 30, 31, 1, 1, 45, 46, 300, 7]
    nb = sum(sizes)
    x = make_input(nb * 256)
    irs = [make_ir(5000, seed=11, norm=0.05), make_ir(4000, seed=12, norm=0.05)]

    def run():
        c = _conv(fftSize=8192, max_batch=max(sizes))
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, dict(BASE, predelay=700, wet=0.8), dict(BASE, select=1, level=0.9), False)
        parts, o = [], 0
        for k, n in enumerate(sizes):
            if k == 9:
                c.cc[0].value.predelay = 300
            seg = x[:, o * 256:(o + n) * 256]
            parts.append(np.stack(c.onProcess(seg[0], seg[1])) if n == 1 else c.process(seg[0], seg[1]))
            o += n
        c.close()
        return np.concatenate(parts, axis=1)

    a, b = run(), run()
    assert rms(a) > 1e-3
    assert np.array_equal(a, b), f"max abs difference between the runs {np.abs(a - b).max():.3e}"


def test_preferred_batch_length(gpu_lib, monkeypatch):
    """mc_preferred_batch: whole chunks of the second-level transform for the longest loaded IR, minus one block,
    a multiple of 8, within at_most and max_batch; short limits come back as they are."""
    from cuda_audio_amd.synth import make_ir

    monkeypatch.setenv("MCCONV_FFT2", "1")  # (the suite is also run with the measurement switches set)
    monkeypatch.setenv("MCCONV_FFT2_FUSED", "1")
    # with the overlap-save form on (the default): whole segments of 16384 - P16 blocks once a batch can take the form
    monkeypatch.setenv("MCCONV_OS", "1")
    c = _conv(fftSize=524288, max_batch=40000)
    c.prepare(0, make_ir(441000, seed=1))   # 1723 partitions -> 1728: segments of 14656 blocks
    assert c.preferred_batch(32768) == 2 * 14656
    assert c.preferred_batch(20000) == 14656
    assert c.preferred_batch(14000) == 12928  # shorter than a segment: the second-level transform's chunks (two of 6465, minus one, to 8)
    assert c.preferred_batch(6000) == 6000
    c.close()
    monkeypatch.setenv("MCCONV_OS", "0")  # the rest of this test: the second-level transform's chunks

    c = _conv(fftSize=524288, max_batch=40000)
    assert c.preferred_batch(1000) == 1000  # nothing loaded: no preference
    c.prepare(0, make_ir(441000, seed=1))   # 1723 partitions -> 1728: chunks of 8192 - 1728 + 1 = 6465 blocks
    assert c.preferred_batch(32768) == 32320
    assert c.preferred_batch(20000) == 19392
    assert c.preferred_batch(6465) == 6464
    assert c.preferred_batch(6000) == 6000
    assert c.preferred_batch(10 ** 9) == (6 * 6465 - 1) // 8 * 8  # capped by max_batch = 40000
    c.close()
    c = _conv(fftSize=2097152, max_batch=40000)
    c.prepare(0, make_ir(1323000, seed=2))  # 5168 partitions: still the fused form, chunks of 8192 - 5168 + 1 = 3025
    assert c.preferred_batch(32768) == (10 * 3025 - 1) // 8 * 8
    c.close()
    monkeypatch.setenv("MCCONV_FFT2_FUSED", "0")  # the 16384-point form: chunks of 11217
    c = _conv(fftSize=2097152, max_batch=40000)
    c.prepare(0, make_ir(1323000, seed=2))
    assert c.preferred_batch(32768) == (2 * 11217 - 1) // 8 * 8
    c.close()


@pytest.mark.parametrize("fused", [False, True], ids=["split", "fused"])
@pytest.mark.parametrize("n_ref,taps", [(131072, (88200, 80000)), (524288, (441000, 400000))], ids=["P345", "P1723"])
def test_second_level_transform_of_long_batches(oracle_mod, gpu_lib, monkeypatch, n_ref, taps, fused):
    """Long batches skip the partition MAC: per bin the sum over partitions is a convolution along the block axis,
    done as one circular convolution with a 16384-point transform per chunk of blocks (k_f2_fwd, k_f2_prod) against
    the IRs' transformed partition sequences - of the two inputs when the window carries one set of gains, of
    gain(slot) x input per voice and path when it does not (cold-start ramp, a gain change).  Same output as the
    direct MAC and as the oracle; batches start at an odd block, one is not a multiple of anything, one is longer
    than a chunk."""
    from cuda_audio_amd.synth import make_input, make_ir

    # (the last one: bench.py's step for the 10 s IR, three full chunks of the fused form)
    sizes = [3, 1200, 4098, 15000 if n_ref == 131072 else 19392]
    if n_ref == 131072:
        sizes += [4096, 4096]  # a gain change before the first of these: its window carries two sets of gains
    nb = sum(sizes)
    x = make_input(nb * 256)
    irs = [make_ir(t, seed=5678 + 2 * j, norm=0.02) for j, t in enumerate(taps)] + [make_ir(taps[0] - 7000, seed=99, norm=0.02)]
    p0, p1 = dict(BASE, predelay=300, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)

    def run(direct):
        monkeypatch.setenv("MCCONV_FFT2", "0" if direct else "1")
        monkeypatch.setenv("MCCONV_FFT2_FUSED", "1" if fused else "0")
        monkeypatch.setenv("MCCONV_FFA_LEVELS", "0")
        monkeypatch.setenv("MCCONV_OS", "0")  # (the longest batches here would take the overlap-save form: tested on its own below)
        c = _conv(fftSize=n_ref, max_batch=max(sizes))
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        out = np.zeros((2, nb * 256), np.float32)
        o = 0
        c.enable_kernel_timing(True)
        levels = []
        for k, n in enumerate(sizes):
            if k == 4:
                c.cc[1].value.update(wet=0.3, panWet=-0.5)
                c.cc[0].value.level = 0.8
            if k == 5:
                c.cc[0].value.update(select=2, vsteps=100)  # two voices with per-slot gains in the last batch
            s = slice(o * 256, (o + n) * 256)
            out[:, s] = c.process(x[0, s], x[1, s])
            levels.append(c.kernel_stats()["fast_levels"])
            o += n
        ks = c.kernel_stats()
        c.close()
        if not direct:  # every batch of >= 768 blocks: cold-start ramp and gain change included (per-slot-gain sequences)
            assert all(lv in (254, 255) for lv, n in zip(levels, sizes) if n >= 768), levels
            assert (254 in levels) == fused  # the fused 8192-point form takes the uniform-gain batches
        return out, ks

    fast, ks_fast = run(False)
    direct, ks_direct = run(True)
    assert ks_fast["fast_levels"] in (254, 255) and ks_direct["fast_levels"] == 0
    assert rms(fast - direct) <= 2e-6, f"second-level transform vs direct MAC: {rms(fast - direct):.3e}"
    assert rms(fast - direct) > 0
    nchk = min(nb, 6000 if n_ref == 131072 else 1500)
    o = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        o.prepare(i, ir)
    apply_params(o, p0, p1, True)
    want = o.process(x[0, : nchk * 256], x[1, : nchk * 256])
    err = rms(fast[:, : nchk * 256] - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


@pytest.mark.parametrize("n_ref,taps,level,direct_cmp,at_most",
                         [(524288, 441000, 254, True, 32768), (2097152, 1323000, 255, False, 32768),
                          (2097152, 1323000, 254, False, 32768), (524288, 441000, 254, False, 131072),
                          (524288, 441000, 253, True, 32768), (2097152, 1323000, 253, False, 32768),
                          (524288, 441000, 253, False, 131072)],
                         ids=["P1723_fused", "P5168_split", "P5168_fused", "P1723_fused_bench_step",
                              "P1723_overlap_save", "P5168_overlap_save", "P1723_overlap_save_bench_step"])
def test_headline_launch_against_the_range_oracle(oracle_mod, gpu_lib, monkeypatch, n_ref, taps, level, direct_cmp, at_most):
    """The launch bench.py times (its step: mc_preferred_batch(131072) = 129296 blocks, twenty chunks - the last case),
    compared DIRECTLY with the oracle (conv.cu:392-401 restated as the partitioned sum,
    oracle.Upols.range): device-resident batches of mc_preferred_batch(32768) blocks - 32320 = five whole chunks of
    the fused 8192-point second-level transform for the 10 s IR, five items per persistent workgroup with window
    look-ahead; 22432 = two chunks of the split 16384-point form for the 30 s IR - in steady state (second and third
    batch of the stream; the 30 s IR also through the fused form, ten chunks of 3025 blocks, which it takes by
    default since round 2's kernel made it the faster one there).  Oracle blocks: inside chunk 0, across the first chunk boundary, the batch end and the
    first blocks of the next launch.  For the 10 s IR also the whole batch against the direct-form MAC.
    Level 253 (round 4, the default for these batches): the overlap-save form of csrc/ossave.hip.h - segments of
    16384 - P16 blocks through one 512 x 8192-point transform each; bench.py's step is then eight segments = 117248 blocks.
    Oracle blocks: inside segment 0, across the first segment boundary, the batch end and the next launch's first blocks."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    dev = torch.device("cuda:0")
    irs = [make_ir(taps, seed=5678), make_ir(taps, seed=5680)]  # bench.py's IRs and parameters
    p0, p1 = dict(BASE, select=0), dict(BASE, select=1)

    def run(direct, T=None):
        monkeypatch.setenv("MCCONV_FFT2", "0" if direct else "1")  # (the suite is also run with the measurement switches set)
        monkeypatch.setenv("MCCONV_FFT2_FUSED", "1" if level == 254 else "0")
        monkeypatch.setenv("MCCONV_FFA_LEVELS", "0")
        monkeypatch.setenv("MCCONV_OS", "1" if level == 253 and not direct else "0")
        c = _conv(fftSize=n_ref, max_batch=at_most)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        T = T or c.preferred_batch(at_most)
        x = make_input(3 * T * 256)
        d_in = torch.from_numpy(x).to(dev)
        d_out = torch.zeros(3, 2, T * 256, device=dev)
        c.enable_kernel_timing(True)
        levels = []
        for k in range(3):
            o = k * T * 256
            c.process_device(d_in[0, o:].data_ptr(), d_in[1, o:].data_ptr(), d_out[k, 0].data_ptr(), d_out[k, 1].data_ptr(), T)
            c.sync()
            levels.append(c.kernel_stats()["fast_levels"])
        out = d_out.cpu().numpy()
        c.close()
        return x, T, out, levels

    x, T, got, levels = run(False)
    p16 = -(-((taps + 255) // 256) // 16) * 16
    if level == 253:
        chunk = 16384 - p16  # blocks per segment
        assert T == at_most // chunk * chunk and T == ((117248 if at_most > 32768 else 29312) if taps == 441000 else 22432)
    else:
        assert T == ((129296 if at_most > 32768 else 32320) if taps == 441000 else (30248 if level == 254 else 22432))
        chunk = (8192 if level == 254 else 16384) - p16 + 1
        assert T == (-(-T // chunk) * chunk - 1) // 8 * 8  # whole chunks minus the halo block, rounded down to 8
    assert levels[1] == level and levels[2] == level, levels  # steady state: one set of gains over the window
    ranges = [(T + 100, 256), (T + chunk - 65, 130), (2 * T - 128, 128 + 64)]  # (first block, blocks) in the stream
    num = den = 0.0
    for b0, n in ranges:
        u = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            u.prepare(i, ir)
        apply_params(u, p0, p1, True)
        want = u.range(x[0], x[1], b0, n)
        u.close()
        flat = np.concatenate([got[1], got[2]], axis=1)  # batches 1 and 2 as one stream starting at block T
        mine = flat[:, (b0 - T) * 256:(b0 - T + n) * 256]
        err = rms(mine - want)
        assert rms(want) > 0.05
        assert err <= RMS_TOL, f"blocks [{b0}, {b0 + n}): rms {err:.3e} (signal {rms(want):.3e})"
        num += float(((mine - want) ** 2).sum())
        den += mine.size
    assert (num / den) ** 0.5 <= RMS_TOL
    if direct_cmp:
        _, _, ref, lv = run(True, T)
        assert lv[1] == 0
        d = rms(got[1] - ref[1])
        assert 0 < d <= 2e-6, f"second-level transform vs direct-form MAC over the whole {T}-block batch: {d:.3e}"


@pytest.mark.parametrize("n_ref,taps,case", [(131072, (88200, 80000), "aligned"), (131072, (88200, 80000), "odd_predelay"),
                                             (524288, (441000, 400000), "aligned")], ids=["P345", "P345_odd_predelay", "P1723"])
def test_overlap_save_batches_match_the_partitioned_passes(oracle_mod, gpu_lib, monkeypatch, n_ref, taps, case):
    """Round 4: whole batches of >= 12288 blocks whose window carries one set of gains run as overlap-save segments of
    16384 - P16 blocks (csrc/ossave.hip.h: one 512 x 8192-point transform per segment instead of zero-padded 512-point
    blocks and a second transform along the block axis).  The same stream through both forms (MCCONV_OS=0: the
    partitioned passes, which the other tests hold to the oracle): batches that are whole segments, ragged (a segment
    and a bit, a last segment nearly empty), right after a gain change (that batch's window carries two sets of gains:
    partitioned passes; the next one takes the form again with new spectra), after a select with a cross-fade (per-block
    gains, then two voices with one set of gains each folded into ONE pair of spectra), an unaligned predelay (the output
    stage frame by frame), and what follows a batch in this form - a short batch (resident MAC on the delay-line slots
    the form left) and single JACK periods (segment ring, wet ring, prefix ring).  Steady stretches also against the
    range oracle directly."""
    from cuda_audio_amd.synth import make_input, make_ir

    p16 = -(-((taps[0] + 255) // 256) // 16) * 16
    hop = 16384 - p16
    sizes = [p16 + 400, hop, hop + 1237, 2 * hop + 8, 12288, 13001, 13000, 12500, 12400, 600]  # (the first one: the cold-start ramp leaves the window)
    nper = 6
    nb = sum(sizes) + nper
    x = make_input(nb * 256)
    irs = [make_ir(t, seed=5678 + 2 * j, norm=0.02) for j, t in enumerate(taps)] + [make_ir(taps[0] - 7000, seed=99, norm=0.02)]
    pd = 1024 if case == "aligned" else 301
    p0, p1 = dict(BASE, predelay=pd, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9, predelay=pd)

    def run(os_on):
        import torch

        monkeypatch.setenv("MCCONV_OS", "1" if os_on else "0")
        monkeypatch.setenv("MCCONV_FFA_LEVELS", "0")
        c = _conv(fftSize=n_ref, max_batch=max(sizes))
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        dev = torch.device("cuda:0")
        d_in = torch.from_numpy(x).to(dev)
        d_out = torch.zeros(2, nb * 256, device=dev)
        c.enable_kernel_timing(True)
        levels, o = [], 0
        for k, n in enumerate(sizes):
            if k == 5:  # a gain change: this batch's window carries two sets of gains
                c.cc[1].value.update(wet=0.3, panWet=-0.5)
                c.cc[0].value.level = 0.8
            if k == 7:  # a select: the cross-fade ramps per block, afterwards two voices sound in the windows
                c.cc[0].value.update(select=2, vsteps=100)
            c.process_device(d_in[0, o * 256:].data_ptr(), d_in[1, o * 256:].data_ptr(), d_out[0, o * 256:].data_ptr(), d_out[1, o * 256:].data_ptr(), n)
            c.sync()
            levels.append(c.kernel_stats()["fast_levels"])
            o += n
        out = d_out.cpu().numpy()
        for j in range(nper):
            a = (o + j) * 256
            l, r = c.onProcess(x[0, a:a + 256], x[1, a:a + 256])
            out[0, a:a + 256], out[1, a:a + 256] = l, r
        st = c.os_stats()
        c.close()
        return out, levels, st

    ref, lv0, st0 = run(False)
    got, lv1, st1 = run(True)
    assert st0["batches"] == 0 and 253 not in lv0
    assert lv1[0] != 253 and lv1[5] != 253 and lv1[7] != 253, lv1  # cold-start ramp, gain change, cross-fade: per-slot gains
    # batches 1-4 and 6 (one set of gains), 8 and 9 after the cross-fade has settled within the window or not: at least these
    assert [lv1[k] for k in (1, 2, 3, 4, 6)] == [253] * 5, lv1
    assert st1["batches"] >= 5 and st1["spectra_builds"] >= 2
    o = 0
    for k, n in enumerate(sizes + [nper]):
        d = rms(got[:, o * 256:(o + n) * 256] - ref[:, o * 256:(o + n) * 256])
        assert d <= 1e-6, f"batch {k} ({n} blocks, form {lv1[k] if k < len(lv1) else 'periods'}): {d:.3e} from the partitioned passes"
        o += n
    assert rms(got - ref) > 0
    # steady stretches against the oracle itself: inside batch 2's second segment, the end of batch 3 and the start of batch 4
    s1, s3 = sum(sizes[:2]), sum(sizes[:4])
    for b0, n in [(s1 + hop - 40, 120), (s3 - 70, 140)]:
        u = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            u.prepare(i, ir)
        apply_params(u, p0, p1, True)
        want = u.range(x[0], x[1], b0, n)
        u.close()
        err = rms(got[:, b0 * 256:(b0 + n) * 256] - want)
        assert rms(want) > 0.01
        assert err <= RMS_TOL, f"blocks [{b0}, {b0 + n}): rms {err:.3e} (signal {rms(want):.3e})"


def test_overlap_save_form_in_the_q8_regime_and_around_retired_epochs(gpu_lib, monkeypatch):
    """The Q8 regime (taps + 255 + predelay > n_ref: the reference cuts what its shift pushes past n_ref) at the SHIPPED shape -
    settings.txt: fftSize 131072, predelay 1024, an IR of fftSize - 1024 frames on both halves - leaves every output block ONE cut
    term of ONE source block: the form takes such batches too, the forward transforms of all blocks summing the cut terms
    (k_fwd<true> with delay-line slots for the batch's tail only, k_drop_fft for the first 516 blocks) and the output pass
    subtracting them before the clamp.  Other Q8 shapes (here: predelay 2000, three partitions cut), the batch in which a predelay epoch is
    retired, and batches whose history reaches into the retired epoch run the partitioned passes (scripts/probes/os_q8_oracle.py holds
    the form in this regime to oracle.RefCompat directly: 1.1e-8 RMS at n_ref 16384).  Everything against MCCONV_OS=0,
    which the Q8 tests hold to oracle.RefCompat."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    n_ref, T = 131072, 13000
    nbat = 7
    x = make_input(nbat * T * 256)
    irs = [make_ir(130048, seed=7, norm=0.02), make_ir(100000, seed=8, norm=0.02)]

    def run(os_on):
        monkeypatch.setenv("MCCONV_OS", "1" if os_on else "0")
        c = _conv(fftSize=n_ref, max_batch=T)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, dict(BASE, predelay=1024), dict(BASE, select=0, predelay=1024), False)  # the shipped shape: Q8 regime
        dev = torch.device("cuda:0")
        d_in = torch.from_numpy(x).to(dev)
        d_out = torch.zeros(2, nbat * T * 256, device=dev)
        c.enable_kernel_timing(True)
        lv = []
        for k in range(nbat):
            if k == 3:  # a longer, unaligned predelay: several partitions' segments are cut - not the one-term shape
                c.cc[0].value.update(predelay=2000)
                c.cc[1].value.update(predelay=2000)
            if k == 5:  # the shorter IR on both halves, no predelay: out of the regime
                c.cc[0].value.update(select=1, predelay=0, vsteps=0)
                c.cc[1].value.update(select=1, predelay=0, vsteps=0)
            o = k * T * 256
            c.process_device(d_in[0, o:].data_ptr(), d_in[1, o:].data_ptr(), d_out[0, o:].data_ptr(), d_out[1, o:].data_ptr(), T)
            c.sync()
            lv.append(c.kernel_stats()["fast_levels"])
        out = d_out.cpu().numpy()
        st = c.drop_stats()
        c.close()
        return out, lv, st

    ref, lv0, st0 = run(False)
    got, lv1, st1 = run(True)
    assert 253 not in lv0
    assert lv1[0] != 253 and 253 not in lv1[3:6], lv1  # cold-start ramp; the predelay change and the three-partition Q8 shape; the change out of the regime
    if os.environ.get("MCCONV_TD_FFT") != "0":
        assert lv1[1] == 253 and lv1[2] == 253, lv1  # the shipped shape in the form
        assert st1["forward_transforms"] >= 2, st1
    assert lv1[6] == 253, lv1  # the window is settled again and the old epochs are out of reach
    for k in range(nbat):
        d = rms(got[:, k * T * 256:(k + 1) * T * 256] - ref[:, k * T * 256:(k + 1) * T * 256])
        assert d <= 1e-6, f"batch {k}: {d:.3e}"
    # the cut terms are there: the same stream as a plain linear convolution differs in the regime's batches
    assert rms(ref[:, T * 256:2 * T * 256]) > 0.01


@pytest.mark.parametrize("pd", [0, 1024, 301])
def test_overlap_save_form_of_block_slices(oracle_mod, gpu_lib, monkeypatch, pd):
    """Block-sliced engines (one per GPU, the same batch on all, no collective) take the overlap-save form for their slices too:
    the segments of a slice read their history from the batch's own buffers in front of the slice (rank 0: from the input-history
    ring, which the forward transforms of the previous batch's tail filled), the first segment also carries the blocks whose
    Q1/Q2 terms the slice's windows reach.  Two virtual ranks on one card against an unsliced engine running the partitioned
    passes (MCCONV_OS=0), and the second batch's middle against the range oracle."""
    import torch

    from cuda_audio_amd.sharded import slice_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    n_ref, taps, world = 131072, (88200, 80000), 2
    T = 2 * 13000
    nbat = 3
    x = make_input(nbat * T * 256)
    irs = [make_ir(t, seed=5678 + 2 * j, norm=0.02) for j, t in enumerate(taps)]
    p0, p1 = dict(BASE, predelay=pd, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9, predelay=pd)
    dx = torch.from_numpy(x).cuda()

    def mk(os_on, max_batch):
        monkeypatch.setenv("MCCONV_OS", "1" if os_on else "0")
        c = _conv(fftSize=n_ref, max_batch=max_batch)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        c.use_torch_stream()
        c.enable_kernel_timing(True)
        return c

    whole = mk(False, T)
    ranks = [mk(True, T) for _ in range(world)]
    ref = torch.zeros(2, nbat * T * 256, device="cuda")
    got = torch.zeros(2, nbat * T * 256, device="cuda")
    levels = []
    for k in range(nbat):
        sl = slice(k * T * 256, (k + 1) * T * 256)
        xin = dx[:, sl].contiguous()
        o = torch.zeros(2, T * 256, device="cuda")
        whole.process_device(xin[0].data_ptr(), xin[1].data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T)
        ref[:, sl] = o
        for r, c in enumerate(ranks):
            first, count = slice_bounds(T, world, r, 1)
            oo = torch.zeros(2, count * 256, device="cuda")
            c.process_slice_device(xin[0].data_ptr(), xin[1].data_ptr(), oo[0].data_ptr(), oo[1].data_ptr(), T, first, count)
            torch.cuda.synchronize()
            levels.append(c.kernel_stats()["fast_levels"])
            got[:, (k * T + first) * 256:(k * T + first + count) * 256] = oo
    torch.cuda.synchronize()
    st = [c.os_stats()["batches"] for c in ranks]
    for c in ranks + [whole]:
        c.close()
    ref, got = ref.cpu().numpy(), got.cpu().numpy()
    assert 253 not in levels[:2], levels  # (the first batch's window holds the cold-start ramp)
    assert levels[2:] == [253] * (2 * nbat - 2), levels
    assert st == [nbat - 1] * world, st
    for k in range(nbat):
        d = rms(got[:, k * T * 256:(k + 1) * T * 256] - ref[:, k * T * 256:(k + 1) * T * 256])
        assert d <= 1e-6, f"batch {k}: {d:.3e} from the unsliced partitioned passes"
    b0, n = T + T // 2 - 60, 120  # across the slice boundary of the second batch
    u = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
    apply_params(u, p0, p1, True)
    want = u.range(x[0], x[1], b0, n)
    u.close()
    err = rms(got[:, b0 * 256:(b0 + n) * 256] - want)
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want):.3e})"


_GROUP_DRIVER_ORACLE = {}


@pytest.mark.parametrize("ranks", [1, 2, 4, -1], ids=["one", "two_virtual", "four_virtual", "one_through_rccl"])
def test_native_group_driver(oracle_mod, gpu_lib, ranks):
    """include/mcconv_group.h (libmcconv_rccl.so): IR partitions sharded over the listed devices by a native driver - one host
    thread per device, the partial wet blocks summed by ncclReduceScatter on the engines' streams, every rank finishing its run of
    blocks.  On a one-GPU box: a group of ONE device runs RCCL-free and must equal the plain engine bit for bit; listing device 0
    two / four times makes virtual ranks on one card (RCCL refuses duplicate devices in a communicator: a sum kernel stands in
    for the collective, mc_group_exchange says so) - partition runs, per-rank threads, slice finishes and host copies are the
    real ones; and one device sent through partial -> ncclReduceScatter on a communicator of one -> slice finish runs the RCCL
    calls themselves (more than one rank of them has never run: no multi-GPU node has been available).  Batches that split evenly (reduce-scatter shape) and one that does not (reduce to rank 0), against the plain engine
    and the oracle, over the whole run and block by block (test_gpu_group_history.py has the small cases in which the batch after
    the ragged one is finished by ranks >= 1 inside its Q1/Q2 window; here that window lies in rank 0's run)."""
    from cuda_audio_amd.group import ConvolutionGroup
    from cuda_audio_amd.synth import make_input, make_ir

    n_ref, taps = 131072, (88200, 80000)
    sizes = [512, 2048, 1023, 2048]
    nb = sum(sizes)
    x = make_input(nb * 256)
    irs = [make_ir(t, seed=5678 + 2 * j, norm=0.02) for j, t in enumerate(taps)]
    p0, p1 = dict(BASE, predelay=300, wet=0.7, panWet=0.25), dict(BASE, select=1, level=0.9)
    solo = ranks < 0
    ranks = abs(ranks)
    c = _conv(fftSize=n_ref, max_batch=max(sizes))
    g = ConvolutionGroup(n_ref, [0] * ranks, max_batch=max(sizes), solo_exchange=solo)
    assert g.size() == ranks and g.exchange() == ("rccl" if solo else "none" if ranks == 1 else "device-sum")
    bounds = [g.shard(r) for r in range(ranks)]
    assert bounds[0][0] == 0 and all(bounds[r][1] == bounds[r + 1][0] for r in range(ranks - 1)) and bounds[-1][1] >= 345
    for i, ir in enumerate(irs):
        c.prepare(i, ir)
        g.prepare(i, ir)
    apply_params(c, p0, p1, False)
    for half, p in ((0, p0), (1, p1)):
        g.set_params(half, **p)
    ref = np.zeros((2, nb * 256), np.float32)
    got = np.zeros((2, nb * 256), np.float32)
    o = 0
    for n in sizes:
        s = slice(o * 256, (o + n) * 256)
        ref[:, s] = c.process(x[0, s], x[1, s])
        got[:, s] = g.process(x[0, s], x[1, s])
        o += n
    c.close()
    g.close()
    if ranks == 1 and not os.environ.get("MCCONV_LIB"):  # (one rank sums all partitions in the plain engine's order: the same bits, with or without the exchange)
        assert np.array_equal(got, ref)
    elif ranks == 1:  # (MCCONV_LIB swaps the library of the plain engine only: libmcconv_rccl.so links the default build)
        assert rms(got - ref) <= 1e-6
    else:
        assert 0 < rms(got - ref) <= 1e-6, rms(got - ref)
    # ... and block by block: one block finished from a wrong history vanishes in an RMS over 5631 of them
    from group_history_cases import block_rms

    apart = block_rms(got - ref)
    assert apart.max() <= 1e-6, f"block {int(np.argmax(apart))}: {apart.max():.3e} from the plain engine"
    if "want" not in _GROUP_DRIVER_ORACLE:  # the whole run, the ragged batch and the one after it included; once for all rank counts
        u = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            u.prepare(i, ir)
        apply_params(u, p0, p1, True)
        want = u.process(x[0], x[1])
        u.close()
        want.setflags(write=False)
        _GROUP_DRIVER_ORACLE["want"] = want
    want = _GROUP_DRIVER_ORACLE["want"]
    nchk = 1200
    err = rms(got[:, : nchk * 256] - want[:, : nchk * 256])
    assert err <= RMS_TOL, f"rms {err:.3e} (signal {rms(want[:, : nchk * 256]):.3e})"
    errs = block_rms(got - want)  # (every block within the bound: so is the RMS over the whole run)
    assert errs.max() <= RMS_TOL, f"block {int(np.argmax(errs))} of batches {sizes}: rms {errs.max():.3e}"


def test_fused_second_level_kernel_for_any_grid(gpu_lib, monkeypatch):
    """k_g2_mac, one workgroup per (bin, chunk) item: T is not a multiple of the chunk (6465 blocks) or of anything else,
    so the last chunk is ragged (bounds argument at the kernel).  The fused form takes the batch, and two runs
    on fresh engines give the same bits.  (The grid switch and the two alternative forms of the kernel that this test
    also compared are retired: docs/DESIGN_history.md.)"""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    dev = torch.device("cuda:0")
    irs = [make_ir(441000, seed=11, norm=0.05), make_ir(420000, seed=13, norm=0.05)]
    T0, T = 2000, 9001  # settle the cross-fade with a first batch, then 6465 + 2536 blocks = 512 items
    x = torch.from_numpy(make_input((T0 + T) * 256)).to(dev)

    def run():
        monkeypatch.setenv("MCCONV_FFT2", "1")  # (the suite is also run with the form switches set)
        monkeypatch.setenv("MCCONV_FFT2_FUSED", "1")
        c = _conv(fftSize=524288, max_batch=T)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, dict(BASE), dict(BASE, select=1), False)
        out = torch.zeros(2, (T0 + T) * 256, device=dev)
        c.enable_kernel_timing(True)
        o = 0
        for n in (T0, T):
            c.process_device(x[0, o:].data_ptr(), x[1, o:].data_ptr(), out[0, o:].data_ptr(), out[1, o:].data_ptr(), n)
            o += n * 256
        c.sync()
        assert c.kernel_stats()["fast_levels"] == 254
        c.close()
        return out[:, T0 * 256:].cpu().numpy()

    want = run()
    assert rms(want) > 0.01
    got = run()
    assert np.array_equal(got, want), f"rms difference between the runs {rms(got - want):.3e}"


def test_pinned_host_batches_overlap_copies_and_match(oracle_mod, gpu_lib):
    """mc_process_batch with pinned caller buffers (mc_host_alloc): chunks of the engine's preferred batch, copy-in /
    kernels / copy-out on three streams, two chunks in flight - same samples as the staged path for pageable buffers
    (chunks of 16384 blocks through the engine's pinned buffer) and as the oracle; run lengths that are not whole
    chunks, longer than max_batch and longer than the old 16384-block cap."""
    from cuda_audio_amd.synth import make_input, make_ir

    n_ref, nb = 32768, 40000
    irs = [make_ir(30000, seed=7, norm=0.05), make_ir(28000, seed=9, norm=0.05)]
    x = make_input(nb * 256)
    p0, p1 = dict(BASE, predelay=200, wet=0.6), dict(BASE, select=1, level=0.9)
    outs = []
    for pinned in (False, True):
        c = _conv(fftSize=n_ref, max_batch=6000)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        if pinned:
            xin, out = c.pinned_array((2, nb * 256)), c.pinned_array((2, nb * 256))
            xin[:] = x
        else:
            xin, out = x, np.zeros((2, nb * 256), np.float32)
        o = 0
        for n in (5, 17000, 6000, nb - 23005):  # 17000 > 16384; the last one: three chunks of <= 6000 and a rest
            s = slice(o * 256, (o + n) * 256)
            c.process(xin[0, s], xin[1, s], out[:, s])
            o += n
        outs.append(np.array(out))
        c.close()
    assert rms(outs[0] - outs[1]) <= 2e-6
    nchk = 700
    u = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
    apply_params(u, p0, p1, True)
    for b0 in (0, 16900, nb - nchk):
        uu = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            uu.prepare(i, ir)
        apply_params(uu, p0, p1, True)
        want = uu.range(x[0], x[1], b0, nchk)
        err = rms(outs[1][:, b0 * 256:(b0 + nchk) * 256] - want)
        assert err <= RMS_TOL, f"blocks from {b0}: rms {err:.3e}"


def test_config4_partition_shards_at_full_size(oracle_mod, gpu_lib, monkeypatch):
    """BASELINE config 4 at its stated shape, one stereo pair of the four (main.cu:31-39: one Convolution per pair):
    10 s IRs (441 000 taps, 1723 partitions) sharded over 8 engines - virtual ranks on one GPU, the sum of the partial
    wet blocks stands in for the RCCL reduce - in batches of the shard's preferred length.  A shard is a 224-tap
    convolution along the block axis whose window starts part_begin slots earlier, so its long batches take the
    second-level transform like an unsharded engine's.  Steady-state batch against the range oracle (conv.cu:392-401)."""
    import torch

    from cuda_audio_amd.sharded import shard_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    monkeypatch.setenv("MCCONV_FFT2", "1")  # (the suite is also run with the measurement switches set)
    monkeypatch.setenv("MCCONV_FFT2_FUSED", "1")
    dev = torch.device("cuda:0")
    n_ref, G = 524288, 8
    irs = [make_ir(441000, seed=5678), make_ir(441000, seed=5680)]
    p0, p1 = dict(BASE, select=0, predelay=300), dict(BASE, select=1, panWet=0.25)
    bounds = [shard_bounds(1723, G, g) for g in range(G)]
    assert bounds[0] == (0, 224) and bounds[-1][1] == 1728
    shards = [_conv(fftSize=n_ref, max_batch=16384, part_begin=a, part_end=b) for a, b in bounds]
    for s in shards:
        for i, ir in enumerate(irs):
            s.prepare(i, ir)
        apply_params(s, p0, p1, False)
    T = shards[0].preferred_batch(16384)
    assert T == (2 * (8192 - 224 + 1) - 1) // 8 * 8 and all(s.preferred_batch(16384) >= T for s in shards[:-1])
    x = make_input(2 * T * 256)
    xin = torch.from_numpy(x).to(dev)
    got = np.zeros((2, 2 * T * 256), np.float32)
    for s in shards:
        s.enable_kernel_timing(True)
    for k in range(2):
        sl = xin[:, k * T * 256:(k + 1) * T * 256]
        total = torch.zeros(2 * T * 256, device=dev)
        for s in shards:
            part = torch.zeros(2 * T * 256, device=dev)
            s.partial_device(sl[0].data_ptr(), sl[1].data_ptr(), part.data_ptr(), T)
            s.sync()
            total += part
        out = torch.zeros(2, T * 256, device=dev)
        torch.cuda.synchronize()
        shards[0].finish_device(sl[0].data_ptr(), sl[1].data_ptr(), total.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), T)
        shards[0].sync()
        for s in shards[1:]:
            s.finish_device(None, None, None, None, None, T)
        got[:, k * T * 256:(k + 1) * T * 256] = out.cpu().numpy()
    levels = [s.kernel_stats()["fast_levels"] for s in shards]
    for s in shards:
        s.close()
    assert all(lv == 254 for lv in levels), levels  # the steady-state batch: fused second-level form on every shard
    for b0, n in ((T + 50, 200), (2 * T - 100, 100)):
        u = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            u.prepare(i, ir)
        apply_params(u, p0, p1, True)
        want = u.range(x[0], x[1], b0, n)
        err = rms(got[:, b0 * 256:(b0 + n) * 256] - want)
        assert err <= RMS_TOL, f"blocks [{b0}, {b0 + n}): rms {err:.3e} (signal {rms(want):.3e})"


def test_partition_shards_finish_their_runs_after_a_reduce_scatter(oracle_mod, gpu_lib, monkeypatch):
    """The north-star layout with a reduce-scatter as its exchange (mc_finish_batch_slice_device): four virtual ranks on
    one GPU, 10 s IRs (1723 partitions, 432 per shard), batches of the shards' preferred length.  Every shard sums its
    partitions over the whole batch; the sum over shards stands in for the collective; shard g receives the sum for ITS
    quarter of the blocks only - [L | R] of that run - and finishes it: Q1/Q2 window sums from its own prefix ring (every
    shard keeps that history now), predelay already in the partials, clamp, dry mix.  The four runs together are, bit
    for bit, what one root finishing the whole sum gives (mc_finish_batch_device on a fifth set of shards), and the
    range oracle's samples (conv.cu:392-427) - also across the batch boundary, where the second batch's Q1/Q2 windows
    reach back into the first."""
    import torch

    from cuda_audio_amd.sharded import shard_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    monkeypatch.setenv("MCCONV_FFT2", "1")
    monkeypatch.setenv("MCCONV_FFT2_FUSED", "1")
    dev = torch.device("cuda:0")
    n_ref, G = 524288, 4
    irs = [make_ir(441000, seed=5678), make_ir(441000, seed=5680)]
    p0, p1 = dict(BASE, select=0, predelay=300, panDry=0.2), dict(BASE, select=1, panWet=0.25)
    bounds = [shard_bounds(1723, G, g) for g in range(G)]
    assert bounds[0] == (0, 432) and bounds[-1][1] == 1728

    def make_shards():
        out = [_conv(fftSize=n_ref, max_batch=16384, part_begin=a, part_end=b) for a, b in bounds]
        for s in out:
            for i, ir in enumerate(irs):
                s.prepare(i, ir)
            apply_params(s, p0, p1, False)
        return out

    scat, root = make_shards(), make_shards()
    T = scat[0].preferred_batch(16384)
    assert T % G == 0
    Ts = T // G
    x = make_input(2 * T * 256)
    x[0] += 0.05  # DC and an alternating component: the Q1/Q2 sums matter
    x[1, ::2] += 0.04
    xin = torch.from_numpy(x).to(dev)
    got = np.zeros((2, 2 * T * 256), np.float32)
    want_root = np.zeros_like(got)
    for k in range(2):
        sl = xin[:, k * T * 256:(k + 1) * T * 256]
        totals = []
        for group in (scat, root):
            total = torch.zeros(2 * T * 256, device=dev)
            for s in group:
                part = torch.zeros(2 * T * 256, device=dev)
                s.partial_device(sl[0].data_ptr(), sl[1].data_ptr(), part.data_ptr(), T)
                s.sync()
                total += part
            totals.append(total)
        assert torch.equal(totals[0], totals[1])
        t2 = totals[0].view(2, T * 256)
        for g, s in enumerate(scat):  # "reduce-scatter": rank g gets its run of both channel halves
            mine = t2[:, g * Ts * 256:(g + 1) * Ts * 256].contiguous()
            out = torch.full((2, Ts * 256), float("nan"), device=dev)
            s.finish_slice_device(sl[0].data_ptr(), sl[1].data_ptr(), mine.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), T, g * Ts, Ts)
            s.sync()
            got[:, (k * T + g * Ts) * 256:(k * T + (g + 1) * Ts) * 256] = out.cpu().numpy()
        out = torch.zeros(2, T * 256, device=dev)
        root[0].finish_device(sl[0].data_ptr(), sl[1].data_ptr(), totals[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), T)
        root[0].sync()
        for s in root[1:]:
            s.finish_device(None, None, None, None, None, T)
        want_root[:, k * T * 256:(k + 1) * T * 256] = out.cpu().numpy()
    # argument errors: a run outside the batch, and a finish with nothing pending
    e = scat[0]
    with pytest.raises(Exception):
        e.finish_slice_device(xin[0].data_ptr(), xin[1].data_ptr(), xin.data_ptr(), xin.data_ptr(), xin.data_ptr(), T, T - 1, 2)
    with pytest.raises(Exception):
        e.finish_slice_device(xin[0].data_ptr(), xin[1].data_ptr(), xin.data_ptr(), xin.data_ptr(), xin.data_ptr(), T, 0, Ts)
    for s in scat + root:
        s.close()
    assert np.isfinite(got).all()
    assert np.array_equal(got, want_root)
    for b0, n in ((Ts - 40, 80), (T - 60, 120), (T + 3 * Ts - 30, 60)):  # across runs, across the batch boundary
        u = oracle_mod.Upols(n_ref, True)
        for i, ir in enumerate(irs):
            u.prepare(i, ir)
        apply_params(u, p0, p1, True)
        want = u.range(x[0], x[1], b0, n)
        err = rms(got[:, b0 * 256:(b0 + n) * 256] - want)
        assert err <= RMS_TOL, f"blocks [{b0}, {b0 + n}): rms {err:.3e} (signal {rms(want):.3e})"


def test_q4_output_clamp_parts_from_the_reference_only_after_saturation(oracle_mod, gpu_lib):
    """Q4 (conv.cu:98), the one documented deviation: the engine clamps the finished wet sample, the reference its
    running accumulator.  With a loud IR the engine equals the partitioned oracle form (output clamp) everywhere and
    the single-FFT restatement of conv.cu up to sample 1298, the first one where a partial sum of the reference's
    accumulator saturated (tests/test_oracle.py::test_q4_running_accumulator_clamp_vs_output_clamp); INTEGRATION.md
    states the contract: keep the wet sum inside +-1 (the reference's own output is distorted beyond it)."""
    from test_oracle import q4_case

    n_ref, x, ir, p = q4_case()
    r, u = oracle_mod.RefCompat(n_ref, True), oracle_mod.Upols(n_ref, True)
    for e in (r, u):
        e.prepare(0, ir)
        apply_params(e, p, p, True)
    ref, out_clamp = r.process(x[0], x[1]), u.process(x[0], x[1])
    for mb in (8, 1):
        c = _conv(fftSize=n_ref, max_batch=mb)
        c.prepare(0, ir)
        apply_params(c, p, p, False)
        if mb == 1:
            got = np.concatenate([np.stack(c.onProcess(x[0, b * 256:(b + 1) * 256], x[1, b * 256:(b + 1) * 256]))
                                  for b in range(x.shape[1] // 256)], axis=1)
        else:
            got = c.process(x[0], x[1])
        c.close()
        assert rms(got - out_clamp) <= RMS_TOL
        assert np.abs(got[:, :1298] - ref[:, :1298]).max() < 1e-5
        assert np.abs(got - ref).max() > 0.3  # and differs where the reference's partial sums saturated


@pytest.mark.parametrize("period", [256, 512, 1024])
def test_parked_periods_survive_pauses_and_interleaved_calls(oracle_mod, gpu_lib, monkeypatch, period):
    """JACK path with periods launched one call ahead (process_one / process_period_fused): a period is parked only once
    the cross-fade has converged EXACTLY (params_steady: coefficient == wet; the recurrence coef += (wet - coef) / 5 needs
    ~160 calls from a cold start or a controller change), so the stream first settles for 180 calls and the test asserts
    that periods WERE parked (mc_debug_read item 6).  Then: a host that pauses longer than the park time (here 20 ms)
    finds that the parked tail gave up on its own and launches the period again - the kernel queued behind it has
    meanwhile swept into this period's partial sums, which are summed again (round-2 advice: process_one did not);
    a controller change, a batch call and an IR reload tell the parked period to give up; the samples are the oracle's
    throughout.  MCCONV_NO_PARK=1 (every period launched on arrival) gives the same samples to rounding: since round 4 a
    256-frame period that has to be waited for takes partition 0 in the time domain, one that is already there in the frequency
    domain (csrc/jack_tail.hip.h, tail1_body); the 512-frame path has one form and gives the same bits."""
    import time

    from cuda_audio_amd.synth import make_input, make_ir

    n_ref = 8192
    settle = 180
    batch = 8 * 256  # frames of the batch call in between
    plan = (settle, 10, 10, settle, 5, 12, 10)
    ncalls = sum(plan)
    total = ncalls * period + batch
    x = make_input(total, seed=31)
    irs = [make_ir(6000, seed=61, norm=0.05), make_ir(5000, seed=63, norm=0.05)]
    p0, p1 = dict(BASE, select=0, wet=0.6), dict(BASE, select=1, level=0.9)
    ref = oracle_mod.RefCompat(n_ref, True)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    want = np.zeros((2, total))
    stats = {}

    def stream(c, with_pauses):
        got = np.zeros((2, total), np.float32)
        pos = 0

        def periods(n):
            nonlocal pos
            for _ in range(n):
                s = slice(pos, pos + period)
                got[:, s] = np.stack(c.onProcess(x[0, s], x[1, s]))
                pos += period

        periods(plan[0])                 # the cold-start ramp converges exactly: periods are parked from ~call 160 on
        stats["settled"] = c.park_stats()
        if with_pauses:
            time.sleep(0.06)             # longer than the park time: the parked tail gives up on its own
        periods(plan[1])                 # (the first of them finds the exited tail and launches the period again)
        stats["paused"] = c.park_stats()
        c.cc[0].value.wet = 0.3          # a controller moves: the parked period was staged with the old value
        periods(plan[2])
        s = slice(pos, pos + batch)
        got[:, s] = c.process(x[0, s], x[1, s])  # a batch call in between (max_batch 8)
        pos += batch
        periods(plan[3])                 # the cross-fade towards wet = 0.3 converges: parked again
        stats["resettled"] = c.park_stats()
        if with_pauses:
            time.sleep(0.06)
        periods(plan[4])
        c.prepare(1, irs[1])             # an IR reload (same taps): the parked tail had its spectra loaded already
        periods(plan[5])
        if with_pauses:
            time.sleep(0.06)
        periods(plan[6])
        stats["end"] = c.park_stats()
        assert pos == total
        return got

    # the oracle sees the same events at the same periods
    o = 0
    first = (plan[0] + plan[1]) * period
    for n, ev in ((first, None), (total - first, "wet")):
        if ev == "wet":
            ref.set(0, wet=0.3)
        s = slice(o, o + n)
        want[:, s] = ref.process(x[0, s], x[1, s], block=period)
        o += n
    outs = []
    for park in (True, False):
        monkeypatch.setenv("MCCONV_PARK_MS", "20")
        if park:
            monkeypatch.delenv("MCCONV_NO_PARK", raising=False)
        else:
            monkeypatch.setenv("MCCONV_NO_PARK", "1")
        c = _conv(fftSize=n_ref, max_batch=8, period=period)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        outs.append(stream(c, with_pauses=park))
        forms = c.tail_forms()
        c.close()
        if period == 256 and not os.environ.get("MCCONV_LIB") and not os.environ.get("MCCONV_TAIL_FORM"):
            # both forms of the 256-frame tail ran: a parked tail that had to wait takes partition 0 in the time domain, a period
            # launched on arrival (every one of them with MCCONV_NO_PARK=1) in the frequency domain
            if park and not any(os.environ.get(k) for k in ("MCCONV_NO_SPIN", "MCCONV_NO_PARK")):
                assert forms["time_domain"] >= 30 and forms["frequency_domain"] >= 20, forms
            else:
                assert forms["time_domain"] == 0 and forms["frequency_domain"] == ncalls, forms
        if park and not os.environ.get("MCCONV_NO_SPIN"):  # (that switch leaves nothing parked)
            # the paths under test really ran: parked periods were used before the first pause, a pause made one time out,
            # the controller / batch / reload told parked periods to give up, and parking resumed after the second settling
            assert stats["settled"]["used"] >= 5, stats
            assert stats["paused"]["timed_out"] >= 1, stats
            assert stats["resettled"]["used"] > stats["paused"]["used"] + 5, stats
            assert stats["resettled"]["cancelled"] >= 1, stats
            assert stats["end"]["timed_out"] >= 3, stats
        else:
            assert stats["end"] == dict(used=0, timed_out=0, cancelled=0), stats
        err = rms(outs[-1] - want)
        assert err <= RMS_TOL, f"park={park}: rms {err:.3e}"
    if period == 256 and not os.environ.get("MCCONV_TAIL_FORM"):  # (MCCONV_TAIL_FORM: one form forced)
        assert np.abs(outs[0] - outs[1]).max() <= 5e-7, np.abs(outs[0] - outs[1]).max()
    else:
        assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("predelay", [0, 64, 300, 301, 2047, 8192])
def test_output_finished_by_the_inverse_transforms(oracle_mod, gpu_lib, monkeypatch, predelay):
    """Whole batches on one engine with no Q8 pass and no retired predelay epoch: the inverse-transform launches
    (k_inv_wet<true>) finish the output themselves - Q1/Q2 window sums, clamp, dry mix, shifted by the predelay - and
    k_post only fills the head the predelay reaches back for; the Q1/Q2 prefix sums ride along with k_g2_mac in one pass.
    The oracle's samples, and the same samples from two runs on fresh engines, for predelays that are and are not multiples
    of four frames, batches shorter than the predelay, a device-buffer and a host-buffer call, and a parameter change
    between batches (conv.cu:89-100, 126-140, 411-427)."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    dev = torch.device("cuda:0")
    n_ref = 131072
    irs = [make_ir(88200, seed=11, norm=0.08), make_ir(70000, seed=13, norm=0.08)]
    runs = (1200, 3, 1500, 40, 1024, 1233)  # 3 and 40 blocks: shorter than the longest predelay's reach
    nb = sum(runs)
    x = make_input(nb * 256)
    x[0] += 0.05  # DC and an alternating component: the Q1/Q2 sums matter
    x[1, ::2] += 0.04
    p0, p1 = dict(BASE, predelay=predelay, wet=0.6, panDry=0.3), dict(BASE, select=1, level=0.9, panWet=-0.4)
    outs = []
    for _ in range(2):
        monkeypatch.setenv("MCCONV_FFT2", "1")
        monkeypatch.setenv("MCCONV_FFT2_FUSED", "1")
        c = _conv(fftSize=n_ref, max_batch=2048)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        out = np.zeros((2, nb * 256), np.float32)
        o = 0
        for k, n in enumerate(runs):
            s = slice(o * 256, (o + n) * 256)
            if k == 2:  # dry gains change between batches (the wet path keeps its gains: no cross-fade restarts)
                c.cc[0].value.update(dry=0.25, panDry=-0.5)
            if k % 2 == 0:  # device buffers
                d_in = torch.from_numpy(x[:, s].copy()).to(dev)
                d_out = torch.full((2, n * 256), float("nan"), device=dev)
                c.process_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), n)
                c.sync()
                out[:, s] = d_out.cpu().numpy()
            else:
                c.process(x[0, s], x[1, s], out[:, s])
            o += n
        outs.append(out)
        c.close()
    assert np.isfinite(outs[0]).all()
    assert rms(outs[0] - outs[1]) <= 1e-7, f"rms difference between the runs {rms(outs[0] - outs[1]):.3e}"
    u = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
    apply_params(u, p0, p1, True)
    nchk, nchg = 1300, runs[0] + runs[1]  # the first two batches and the start of the third (the oracle steps block by block)
    want = np.zeros((2, nchk * 256))
    want[:, :nchg * 256] = u.process(x[0, :nchg * 256], x[1, :nchg * 256])
    u.set(0, dry=0.25, panDry=-0.5)
    want[:, nchg * 256:] = u.process(x[0, nchg * 256:nchk * 256], x[1, nchg * 256:nchk * 256])
    err = rms(outs[0][:, :nchk * 256] - want)
    assert err <= RMS_TOL, f"rms {err:.3e}"


def test_batch_longer_than_the_riding_prefix_chain(oracle_mod, gpu_lib):
    """Batches of more than 160 x 256 blocks: the Q1/Q2 prefix sums do not ride along with the MAC launch (every riding
    workgroup would look at the totals of all chunks before it) but run as their own two launches ahead of the inverse
    transforms that finish the output.  The same samples from two runs on fresh engines, the oracle's samples at the
    batch end."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    dev = torch.device("cuda:0")
    n_ref, T = 8192, 41216
    irs = [make_ir(6000, seed=3, norm=0.1), make_ir(5000, seed=4, norm=0.1)]
    x = make_input(T * 256, seed=8)
    x[0] += 0.04
    p0, p1 = dict(BASE, predelay=128, wet=0.7), dict(BASE, select=1, panWet=0.4)
    outs = []
    for _ in range(2):
        c = _conv(fftSize=n_ref, max_batch=T)
        for i, ir in enumerate(irs):
            c.prepare(i, ir)
        apply_params(c, p0, p1, False)
        d_in = torch.from_numpy(x).to(dev)
        d_out = torch.full((2, T * 256), float("nan"), device=dev)
        c.process_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), T)
        c.sync()
        outs.append(d_out.cpu().numpy())
        c.close()
    assert np.isfinite(outs[0]).all()
    assert rms(outs[0] - outs[1]) <= 1e-7, f"rms difference between the runs {rms(outs[0] - outs[1]):.3e}"
    u = oracle_mod.Upols(n_ref, True)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
    apply_params(u, p0, p1, True)
    n = 96
    want = u.range(x[0], x[1], T - n, n)
    err = rms(outs[0][:, (T - n) * 256:] - want)
    assert err <= RMS_TOL, f"rms {err:.3e}"


@pytest.mark.parametrize("seed,moving_predelay", [(1, False), (2, False), (3, False), (4, True), (5, True)])
def test_random_mix_of_batch_lengths_and_single_periods(oracle_mod, gpu_lib, seed, moving_predelay):
    """One stream through every path in random order: single periods (parked tails), batches below the streaming
    threshold, resident-MAC batches, batches long enough for the fused second-level transform (output finished by the
    inverse transforms), host and device buffers - with controller changes (dry / wet / pans / level) between calls.  Each path leaves the rings the next one reads (wet ring written only where it
    can still be read, segment ring, prefix sums, delay line).  Fixed predelay (a multiple of four or not): against the
    partitioned oracle, 26 000 blocks.  With IR selects (short cross-fades: per-slot gains, the split form) and predelay
    changes as well (blocks already played keep their offset: retired epochs ring out under batches that then go through
    k_post): against the single-transform restatement of conv.cu, which is slower, 13 000 blocks."""
    import torch

    from cuda_audio_amd.synth import make_input, make_ir

    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0")
    if moving_predelay:
        n_ref, total, long_lo, long_hi = 8192, 13000, 9400, 9900          # P = 28 -> 32: fused from 9375 blocks
        irs = [make_ir(7000, seed=70, norm=0.05), make_ir(6500, seed=71, norm=0.05), make_ir(4000, seed=72, norm=0.05)]
    else:
        n_ref, total, long_lo, long_hi = 16384, 26000, 4700, 9000          # P = 59 -> 64: fused from 4688 blocks
        irs = [make_ir(15000, seed=70, norm=0.05), make_ir(14000, seed=71, norm=0.05), make_ir(9000, seed=72, norm=0.05)]
    sizes = []
    while sum(sizes) < total:
        kind = int(rng.integers(0, 5))
        sizes.append([1, 1, int(rng.integers(2, 47)), int(rng.integers(48, 400)), int(rng.integers(long_lo, long_hi))][kind])
        if kind < 2:
            sizes += [1] * int(rng.integers(3, 12))  # runs of single periods: they park once nothing moves
    nb = sum(sizes)
    x = make_input(nb * 256, seed=100 + seed)
    x[0] += 0.03
    u = oracle_mod.RefCompat(n_ref, True) if moving_predelay else oracle_mod.Upols(n_ref, True)
    c = _conv(fftSize=n_ref, max_batch=10000)
    for i, ir in enumerate(irs):
        u.prepare(i, ir)
        c.prepare(i, ir)
    pd0 = int(rng.choice([0, 64, 301, 1024]))
    p0, p1 = dict(BASE, select=0, wet=0.6, predelay=pd0), dict(BASE, select=1, level=0.9)
    apply_params(u, p0, p1, True)
    apply_params(c, p0, p1, False)
    got = np.zeros((2, nb * 256), np.float32)
    want = np.zeros((2, nb * 256))
    o = 0
    for k, n in enumerate(sizes):
        if k and rng.random() < 0.3:
            half = int(rng.integers(0, 2))
            what = int(rng.integers(0, 5 if moving_predelay else 3))  # (the partitioned oracle blends no IRs: no selects there)
            if what == 0:
                p = dict(dry=float(rng.uniform(0.1, 0.6)), panDry=float(rng.uniform(-1, 1)))
            elif what == 1:
                p = dict(wet=float(rng.uniform(0.2, 0.7)), panWet=float(rng.uniform(-1, 1)))
            elif what == 2:
                p = dict(level=float(rng.uniform(0.5, 1.0)))
            elif what == 3:
                sp = int(rng.integers(2, 30))
                p = dict(select=int(rng.integers(0, 3)), speed=sp, vsteps=sp)
            else:
                half, p = 0, dict(predelay=int(rng.choice([0, 64, 300, 301, 1024, 4097])))
            u.set(half, **p)
            c.cc[half].value.update(**p)
        s = slice(o * 256, (o + n) * 256)
        want[:, s] = u.process(x[0, s], x[1, s])
        if n == 1:
            got[0, s], got[1, s] = c.onProcess(x[0, s], x[1, s])
        elif rng.random() < 0.5:
            got[:, s] = c.process(x[0, s], x[1, s])
        else:
            d_in = torch.from_numpy(x[:, s].copy()).to(dev)
            d_out = torch.full((2, n * 256), float("nan"), device=dev)
            c.process_device(d_in[0].data_ptr(), d_in[1].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), n)
            c.sync()
            got[:, s] = d_out.cpu().numpy()
        o += n
    c.close()
    assert np.isfinite(got).all()
    assert np.abs(want).max() < 1.0  # (the wet sum stays inside the clamp: Q4)
    err = rms(got - want)
    assert err <= RMS_TOL, f"seed {seed}: rms {err:.3e} (signal {rms(want):.3e}), calls {len(sizes)}"


@pytest.mark.parametrize("case", ["plain", "predelay_inside_the_block", "predelay_of_two_blocks", "q8_regime", "two_irs"])
def test_spaced_jack_periods_take_the_time_domain_tail_and_match_the_oracle(oracle_mod, gpu_lib, case):
    """256-frame periods with the host away between calls (1 ms here; jackd: 5.8 ms): once the cross-fade has settled every period is
    parked a call ahead, the parked tail finds no period at its first look, finishes the older partitions' inverse transform, makes its
    dry run and waits - partition 0 is then the direct convolution on eight wavefronts (csrc/jack_tail.hip.h, tail1_body / tail1_helper).
    The device-side count (Convolution.tail_forms) says that this form ran for the spaced calls; the samples are the oracle's: with a
    predelay inside the block (the delayed sample is another thread's), of two blocks, in the Q8 regime (cut terms carried by the launch
    before), and with a different IR on each input."""
    import time

    from cuda_audio_amd.synth import make_input, make_ir

    if any(os.environ.get(k) for k in ("MCCONV_NO_PARK", "MCCONV_NO_SPIN")) or os.environ.get("MCCONV_TAIL_FORM") == "fd":
        pytest.skip("nothing is parked / one form is forced under this switch")
    n_ref, settle, spaced = 4096, 200, 120
    compat = True
    taps = n_ref - 1024 if case == "q8_regime" else 2500
    irs = [make_ir(taps, seed=71, norm=0.05), make_ir(taps - 300, seed=73, norm=0.05)]
    pd = {"plain": 0, "predelay_inside_the_block": 100, "predelay_of_two_blocks": 512, "q8_regime": 1024, "two_irs": 64}[case]
    p0 = dict(BASE, select=0, predelay=pd, wet=0.6)
    p1 = dict(BASE, select=1 if case == "two_irs" else 0, predelay=pd, level=0.9)
    total = (settle + spaced) * 256
    x = make_input(total, seed=77)
    ref = oracle_mod.RefCompat(n_ref, compat)
    c = _conv(fftSize=n_ref, max_batch=8, compat=compat)
    for i, ir in enumerate(irs):
        ref.prepare(i, ir)
        c.prepare(i, ir)
    apply_params(ref, p0, p1, True)
    apply_params(c, p0, p1, False)
    want = ref.process(x[0], x[1], block=256)
    got = np.zeros((2, total), np.float32)
    for b in range(settle + spaced):
        if b >= settle:
            time.sleep(0.001)
        s = slice(b * 256, (b + 1) * 256)
        got[:, s] = np.stack(c.onProcess(x[0, s], x[1, s]))
    forms, parked = c.tail_forms(), c.park_stats()
    c.close()
    assert rms(got - want) <= RMS_TOL, rms(got - want)
    assert rms(got[:, settle * 256:] - want[:, settle * 256:]) <= RMS_TOL
    if os.environ.get("MCCONV_TAIL_FORM") != "td":
        assert parked["used"] >= spaced - 2 and forms["time_domain"] >= spaced - 2, (forms, parked)
    assert forms["time_domain"] + forms["frequency_domain"] == settle + spaced, forms
