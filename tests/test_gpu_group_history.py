"""The Q1/Q2 history of a multi-device group across batches that only rank 0 finishes (group_history_cases.py has the cases and
why they are sensitive; test_group_history_cases_cpu.py proves that they are).  Every bound here is per 256-frame block: one
block finished from a stale history is wrong by a hundred tolerances and still vanishes in an RMS over the whole run."""
import numpy as np
import pytest

import group_history_cases as ghc
from helpers import RMS_TOL, apply_params

pytestmark = pytest.mark.gpu

MC_ERR_ARG = -1


def _conv(**kw):
    from cuda_audio_amd.engine import Convolution

    kw.setdefault("stream_threshold", 8)  # (as test_gpu_parity.py: batches of >= 8 blocks take the resident kernel)
    return Convolution("test", **kw)


def _where(case, ranks, block, win):
    i, q = ghc.finisher(case, ranks, block)
    return f"block {block} (batch {i} of {list(case.sizes)}, finished by rank {q}{', a window block' if block in win else ''})"


@pytest.mark.parametrize("name,ranks", ghc.CASE_RANKS, ids=[f"{n}-{r}" for n, r in ghc.CASE_RANKS])
def test_group_keeps_history_across_ragged_batches(oracle_mod, gpu_lib, name, ranks):
    """Virtual ranks on one device through the native driver: even batches are finished run by run on every rank, ragged ones on
    rank 0 - and the blocks that ranks >= 1 finish afterwards, whose Q1/Q2 windows reach back into the ragged batch, are the
    oracle's.  The plain engine, fed the same batches, gives the same blocks to 1e-6."""
    from cuda_audio_amd.group import ConvolutionGroup

    case = ghc.CASES[name]
    x, want, _ = ghc.build(oracle_mod, name)
    win = set(ghc.window_blocks(case, ranks))
    p0, p1 = ghc.params(case)
    c = _conv(fftSize=ghc.N_REF, max_batch=ghc.MAX_BATCH, period=case.period)
    g = ConvolutionGroup(ghc.N_REF, [0] * ranks, max_batch=ghc.MAX_BATCH, period=case.period)
    assert g.size() == ranks and g.exchange() == "device-sum"
    assert [g.shard(q) for q in range(ranks)] == [(q * 64 // ranks, (q + 1) * 64 // ranks) for q in range(ranks)]
    for i, ir in enumerate(ghc.impulse_responses()):
        c.prepare(i, ir)
        g.prepare(i, ir)
    apply_params(c, p0, p1, False)
    g.set_params(0, **p0)
    g.set_params(1, **p1)
    got = np.zeros(x.shape, np.float32)
    plain = np.zeros(x.shape, np.float32)
    for o, n, i in ghc.batches(case):
        if i in case.changes:
            c.cc[0].value.predelay = case.changes[i]
            g.set_params(0, **dict(p0, predelay=case.changes[i]))
        s = slice(o * 256, (o + n) * 256)
        plain[:, s] = c.process(x[0, s], x[1, s])
        got[:, s] = g.process(x[0, s], x[1, s])
    c.close()
    g.close()
    err = ghc.block_rms(got - want)
    worst = int(np.argmax(err))
    apart = ghc.block_rms(got - plain)
    worst_p = int(np.argmax(apart))
    wl = sorted(win)
    print(f"{name}-{ranks}: worst block against the oracle {err[worst]:.3e} at {_where(case, ranks, worst, win)}; over the window blocks "
          f"{err[wl].max():.3e}, over the others {np.delete(err, wl).max():.3e}; against the plain engine {apart[worst_p]:.3e} at block {worst_p}; "
          f"plain engine against the oracle {ghc.block_rms(plain - want).max():.3e}")
    assert err[worst] <= RMS_TOL, f"rms {err[worst]:.3e} in {_where(case, ranks, worst, win)}"
    assert apart[worst_p] <= 1e-6, f"{apart[worst_p]:.3e} from the plain engine in {_where(case, ranks, worst_p, win)}"


def test_shard_that_retired_a_batch_without_output_still_has_its_history(oracle_mod, gpu_lib):
    """The engine's side of it, without the driver (mcconv.h, mc_finish_batch_device): four partition shards; the first batch
    (37 blocks) is finished by shard 0 alone, the others retire it without output; the second (64 blocks) is finished run
    by run, 16 blocks per shard, from the sum of the partials - every Q1/Q2 window of it reaches back into the first."""
    import torch

    case = ghc.CASES["ragged_first"]
    assert case.sizes == (37, 64) and case.period == 256
    x, want, _ = ghc.build(oracle_mod, case.name)
    p0, p1 = ghc.params(case)
    G = 4
    shards = [_conv(fftSize=ghc.N_REF, max_batch=ghc.MAX_BATCH, part_begin=16 * q, part_end=16 * (q + 1)) for q in range(G)]
    for s in shards:
        s.use_torch_stream()
        for i, ir in enumerate(ghc.impulse_responses()):
            s.prepare(i, ir)
        apply_params(s, p0, p1, False)
    xin = torch.from_numpy(np.array(x)).cuda()
    out = torch.full(xin.shape, float("nan"), device="cuda")

    def partial_sum(sl, T):
        total = torch.zeros(2 * T * 256, device="cuda")
        for s in shards:
            part = torch.zeros(2 * T * 256, device="cuda")
            s.partial_device(sl[0].data_ptr(), sl[1].data_ptr(), part.data_ptr(), T)
            total += part
        return total

    T = 37
    sl = xin[:, : T * 256].contiguous()
    total = partial_sum(sl, T)
    o = torch.zeros(2, T * 256, device="cuda")
    shards[0].finish_device(sl[0].data_ptr(), sl[1].data_ptr(), total.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T)
    for s in shards[1:]:
        s.finish_device(None, None, None, None, None, T)
    out[:, : T * 256] = o
    T, Ts = 64, 16
    sl = xin[:, 37 * 256:].contiguous()
    t2 = partial_sum(sl, T).view(2, T * 256)
    for q, s in enumerate(shards):  # "reduce-scatter": shard q gets its run of both channel halves
        mine = t2[:, q * Ts * 256:(q + 1) * Ts * 256].contiguous()
        o = torch.full((2, Ts * 256), float("nan"), device="cuda")
        s.finish_slice_device(sl[0].data_ptr(), sl[1].data_ptr(), mine.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), T, q * Ts, Ts)
        out[:, (37 + q * Ts) * 256:(37 + (q + 1) * Ts) * 256] = o
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s in shards:
        s.close()
    assert np.isfinite(got).all()
    err = ghc.block_rms(got - want)
    worst = int(np.argmax(err))
    print(f"shards: worst block against the oracle {err[worst]:.3e} at block {worst}; per shard of the second batch "
          + ", ".join(f"{err[37 + q * Ts:37 + (q + 1) * Ts].max():.3e}" for q in range(G)))
    assert err[worst] <= RMS_TOL, f"rms {err[worst]:.3e} in block {worst}" + (f" (shard {(worst - 37) // Ts} of the second batch)" if worst >= 37 else "")


@pytest.mark.parametrize("devices", [[0, 0, 1], [0, 1, 1], [0, 0, 99]], ids=["0_0_1", "0_1_1", "0_0_99"])
def test_group_rejects_mixed_device_lists(gpu_lib, devices):
    """A device list is all distinct (RCCL) or all equal (virtual ranks, a sum kernel on that device); a mixture would have the sum
    kernel of one device read partials that live on another.  Refused as a bad argument that names the list, before any engine
    is created: the last list names a device no box has, and is still refused for its shape, not for that device.  Nothing
    is processed.  (n_ref = 32768: 124 partitions, of which three ranks would own 48, 48 and 32 - nothing else is wrong with
    the request.)"""
    from cuda_audio_amd.group import ConvolutionGroup, GroupError

    with pytest.raises(GroupError) as ei:
        ConvolutionGroup(32768, devices, max_batch=ghc.MAX_BATCH)
    msg = str(ei.value)
    assert msg.startswith(f"mc_group status {MC_ERR_ARG}:"), msg
    assert "device list" in msg and "{" + ", ".join(str(d) for d in devices) + "}" in msg, msg
    assert "rank" not in msg, msg  # (an engine's own failure is reported as "rank q (device d): ...")
