#!/usr/bin/env python3
"""Headline benchmark: real-time factor of the convolution hot path.

Workload (BASELINE.json configs[2], the one the metric is quoted on): stereo
44.1 kHz, 256-frame blocks, 10 s / 441 000-tap IR (P = 1723 partitions,
N_ref = 524288), reference routing (2 inputs x 2 outputs = 4 convolution
paths), fp32.  One "step" = one batch of --blocks (default: the engine's
preferred length up to --max-blocks, 129296) consecutive blocks pushed through forward FFT ->
sum over partitions -> inverse FFT -> overlap-add -> predelay / Q1-Q2 terms /
clamp / dry mix, inputs and outputs resident in HBM.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus N --steps K --warmup W          (starts its N ranks itself, as child processes)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

N = 1: the line also carries `roofline` (compulsory bytes of the dominant kernel /
its event-bracketed duration, inside the timed steps); with --full also `parity`
(the last timed step's output against the CPU oracle, same run), `host_io` (the
same path with pinned host buffers in and out, PCIe-inclusive), `latency_mode`
(one JACK period per call), `literal_mac` and `cpu_baseline`.  Without --full a
run sets up, warms up, times the steps and prints the line, nothing else.

    python bench.py --full                                  (every leg named here, as the records under profiles/ were taken)
    python bench.py --steps 20 --warmup 5 --dump-outputs D  (the last timed step's output as D/<name>.npy)

N > 1 with --full measures BOTH multi-GPU layouts in the same run (each with an
untimed check against an unsharded engine; without --full only the first):
  * output blocks sliced over the GPUs, no data-path collective (weak scaling:
    every GPU finishes --blocks blocks per step) -> `value`;
  * IR partitions sharded over the GPUs + RCCL sum-reduce of the partial wet
    blocks (BASELINE.json's north-star layout; strong scaling: the step stays
    --blocks blocks) -> `north_star_layout`.
--channels 8 runs BASELINE config 4: four stereo `Convolution` pairs
(main.cu:31-39 makes one object per pair) per rank.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FS = 44100
BLOCK = 256
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: 8.0 TB/s spec
FP32_PEAK_TFLOPS = 157.3  # vector = f32-MFMA rate
RMS_TOL = 1e-5            # BASELINE.json north star: <= 1e-5 RMS vs the float64 oracle


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=0,
                    help="blocks per step (batch length T). 0 (default): what the engine prefers up to --max-blocks "
                         "(mc_preferred_batch: whole chunks of the second-level transform minus one halo block) - 129296 = 750 s "
                         "of audio = twenty chunks of 8192 - 1728 + 1 blocks for the 1723-partition IR")
    ap.add_argument("--max-blocks", type=int, default=131072,
                    help="upper limit of the preferred batch length (per GPU; eight block-sliced ranks then share a global batch "
                         "of 8 x 129296 blocks, inside mc_config.max_batch <= 1048576). Longer batches amortise the launches' "
                         "ramps and tails: 892 k x at 32320 blocks, 970 k x at 64640, 1.0 M x at 129296")
    ap.add_argument("--taps", type=int, default=441000)
    ap.add_argument("--fft-size", type=int, default=524288, help="reference fftSize (N_ref)")
    ap.add_argument("--predelay", type=int, default=0, help="predelay of both halves in frames (conv.h:26-28: 0..8192; SURVEY 8(d): 0 for perf)")
    ap.add_argument("--same-ir", action="store_true", help="both halves select IR 0 (settings.txt:38,63 select one IR for both)")
    ap.add_argument("--shipped-defaults", action="store_true",
                    help="the operating point the reference ships (settings.txt:19,38-45): fftSize 131072, both halves on one IR, "
                         "predelay 1024, an IR longer than fftSize - 1024 (14 of the shipped files): --fft-size 131072 --taps 130048 "
                         "--predelay 1024 --same-ir. taps + 255 + predelay > fftSize: the Q8 tail-drop regime (k_post<true>, no fused output)")
    ap.add_argument("--channels", type=int, default=2, choices=[2, 4, 6, 8],
                    help="2 per `Convolution` object (main.cu:31-39): 8 = BASELINE config 4, four pairs with their own IRs")
    ap.add_argument("--mode", choices=["resident", "stream"], default="resident",
                    help="resident: IR held on chip across the batch; stream: every block re-reads IR+delay line")
    ap.add_argument("--precision", choices=["fp32", "fp16"], default="fp32",
                    help="fp16: IR spectra and delay line stored as half for the streaming sweep (implies --mode stream)")
    ap.add_argument("--form", choices=["partitioned", "single"], default="partitioned",
                    help="single: the path in the reference's own shape (mc_config.form = 1; BASELINE config 2: one "
                         "fft-size-point transform per 256-frame call). Use with --taps 88200 --fft-size 131072")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-latency", action="store_true", help="skip the 1-block-per-call (JACK) measurement")
    ap.add_argument("--no-host-io", action="store_true", help="skip the pinned-host-buffer (PCIe-inclusive) leg")
    ap.add_argument("--no-parity", action="store_true", help="skip the same-run comparison with the CPU oracle")
    ap.add_argument("--layouts", choices=["both", "blocks", "partitions"], default="both",
                    help="N > 1: which multi-GPU layouts to measure (default both; `value` is the block-sliced one)")
    ap.add_argument("--exchange", choices=["gather", "none"], default="none",
                    help="block slices: leave every rank's finished slice on the GPU that computed it (default: like the "
                         "inputs, the outputs of the batch path live in HBM) or gather the slices on rank 0 over RCCL")
    ap.add_argument("--collective", choices=["reduce_scatter", "reduce", "allreduce"], default="reduce_scatter",
                    help="partition shards: how the partial wet blocks are summed. reduce_scatter (default): every rank receives "
                         "and finishes the sum for its 1/N of the batch's blocks (mc_finish_batch_slice_device); reduce: the whole "
                         "sum to rank 0, which finishes the batch (the round-2 form: N - 1 ranks' partials funnel into one GPU); "
                         "allreduce: the whole sum to every rank")
    ap.add_argument("--no-overlap", action="store_true", help="N > 1: finish each batch before starting the next")
    ap.add_argument("--pipeline", action="store_true",
                    help="mc_config.pipeline: post stage of batch k on a second stream under the MAC of batch k + 1")
    ap.add_argument("--no-literal-mac", action="store_true", help="skip the literal partition x bin MAC record (streaming kernel, 2048-block launches)")
    ap.add_argument("--no-direct-mac", action="store_true", help="N > 1: skip the third curve (partition shards with the literal resident MAC)")
    ap.add_argument("--no-check", action="store_true",
                    help="N > 1: skip the untimed comparison of the sharded pipeline with an unsharded engine on rank 0")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="with --force-sharded on one GPU: be rank 0 of this many ranks (its slice / its partition shard)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="N > 1 collective backend. gloo is a rehearsal of the launch path on a box with fewer GPUs than "
                         "ranks (ranks share cards, the sum goes through host memory): never a headline number")
    ap.add_argument("--force-sharded", action="store_true",
                    help="use the multi-GPU code paths even with one rank (rehearsal on one GPU)")
    ap.add_argument("--prewarm-ms", type=float, default=300.0,
                    help="untimed: run the step back to back for this long before the --warmup steps so that the timed region "
                         "does not start on idle clocks (the driver's 20-step region is 6 ms long); reported in the line")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: the same-run parity with the CPU oracle, host_io, "
                         "latency_mode, literal_mac, cpu_baseline, the multi-pair kernel pass and, for N > 1, the north-star layouts, "
                         "the kernels-only / collective-only times and sharded_check (the --no-* options still switch legs off). "
                         "Without it a run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (float32; "
                         "a fixed, seeded sample of the blocks where the output exceeds the size limit, with the block indices "
                         "in DIR/<name>_blocks.npy)")
    a = ap.parse_args()
    if not a.full:
        a.no_parity = a.no_host_io = a.no_latency = a.no_literal_mac = a.no_cpu_baseline = True
        a.no_check = a.no_direct_mac = True
        if a.layouts == "both":
            a.layouts = "blocks"
    return a


DUMP_LIMIT_BYTES = 48 << 20  # (under the 64 MB a dump may take in all)
DUMP_EDGE_BLOCKS = 64
DUMP_SEED = 20240611


def dump_outputs(dirname, outputs):
    """Write {name: device tensor [2, n * 256]} as DIR/<name>.npy, float32 [2, blocks, 256].  Outputs too large for the
    limit are sampled: the first and last DUMP_EDGE_BLOCKS blocks and a seeded choice of the rest, the same for the same
    batch length; the block indices go to DIR/<name>_blocks.npy (float64)."""
    import torch

    os.makedirs(dirname, exist_ok=True)
    per = DUMP_LIMIT_BYTES // max(len(outputs), 1) // (2 * BLOCK * 4)
    for name, t in outputs.items():
        nblk = t.shape[1] // BLOCK
        v = t.reshape(2, nblk, BLOCK)
        if nblk > per:
            rest = np.arange(DUMP_EDGE_BLOCKS, nblk - DUMP_EDGE_BLOCKS)
            pick = np.random.default_rng(DUMP_SEED).choice(rest, per - 2 * DUMP_EDGE_BLOCKS, replace=False)
            idx = np.sort(np.concatenate([np.arange(DUMP_EDGE_BLOCKS), pick, np.arange(nblk - DUMP_EDGE_BLOCKS, nblk)]))
            v = v.index_select(1, torch.from_numpy(idx).to(t.device))
            np.save(os.path.join(dirname, name + "_blocks.npy"), idx.astype(np.float64))
        np.save(os.path.join(dirname, name + ".npy"), v.float().cpu().numpy())


def git_head():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def cpu_threads():
    """Threads for the CPU baseline: the cgroup CPU quota of this box when there is one (a GPU box shows all
    host CPUs but is throttled to its share), else what OpenMP reports."""
    import oracle

    n = oracle.max_threads()
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except Exception:
        pass
    return n


def fftw_probe():
    """FFTW is not installed in the image; if a GPU box happens to carry libfftw3f, say so (it is only
    reported: the baseline's transforms are the oracle's own, so that the number means the same thing on every box)."""
    import ctypes
    import ctypes.util

    for name in (ctypes.util.find_library("fftw3f"), "libfftw3f.so.3", "libfftw3f.so"):
        if not name:
            continue
        try:
            ctypes.CDLL(name)
            return f"found ({name}); not used: the baseline keeps the oracle's own radix-2 FFT"
        except OSError:
            continue
    return "not found (dlopen of libfftw3f failed): the baseline uses the oracle's own radix-2 FFT"


def cpu_baseline(ir, ir_b, x, seconds):
    """SURVEY 8(d)'s CPU baseline, timed in this run on the box's host cores, on a bounded sample of the same workload:
    oracle Cpu32 (float32 OpenMP partitioned overlap-save, own FFT) with all the cores this box may use - `value` - and
    with one thread; the reference's own single-transform algorithm at config 2 (oracle RefCompat: one 131072-point
    transform per call, float64, one thread); and whether FFTW could have been loaded."""
    import oracle
    from cuda_audio_amd.synth import make_ir

    threads = cpu_threads()
    eng = oracle.Cpu32(ir, ir_b)
    g = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    chunk, avail = 128, x.shape[1] // BLOCK

    def run(nthreads, secs):
        eng.process(x[0, : chunk * BLOCK], x[1, : chunk * BLOCK], g, g, nthreads)  # warm-up, untimed
        t0 = time.perf_counter()
        done = 0
        while time.perf_counter() - t0 < secs:
            o = (done % max(avail - chunk, 1))
            eng.process(x[0, o * BLOCK: (o + chunk) * BLOCK], x[1, o * BLOCK: (o + chunk) * BLOCK], g, g, nthreads)
            done += chunk
        return done, time.perf_counter() - t0

    done, dt = run(threads, 0.6 * seconds)
    done1, dt1 = run(1, 0.25 * seconds)
    eng.close()
    # config 2 in the reference's own shape on the CPU (what run_single_form's parity leg times, here beside the headline)
    r = oracle.RefCompat(131072, True)
    r.prepare(0, make_ir(88200, seed=5678))
    r.prepare(1, make_ir(88200, seed=5680))
    r.set(1, select=1)
    ncall = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.15 * seconds or ncall < 4:
        r.process(x[0, ncall * BLOCK:(ncall + 1) * BLOCK], x[1, ncall * BLOCK:(ncall + 1) * BLOCK])
        ncall += 1
    dtr = time.perf_counter() - t0
    r.close()
    return {
        "value": round(done * BLOCK / FS / dt, 3),
        "unit": "x realtime",
        "cores": threads,
        "kind": "port",
        "sample": f"{done} blocks ({done * BLOCK / FS:.1f} s of audio) of the same stereo/{ir.shape[0]}-tap workload, "
                  f"oracle/oracle.c orc_cpu32 (own radix-2 FFT, OpenMP over bins), {dt:.1f} s wall",
        "single_thread": {"value": round(done1 * BLOCK / FS / dt1, 3), "unit": "x realtime", "cores": 1,
                          "sample": f"{done1} blocks of the same workload, one thread, {dt1:.1f} s wall"},
        "refcompat_config2": {"value": round(ncall * BLOCK / FS / dtr, 3), "unit": "x realtime", "cores": 1,
                              "sample": f"{ncall} calls of oracle/oracle.c orc_ref_process at BASELINE config 2 (88200-tap IRs, one 131072-point "
                                        f"transform per 256-frame call, float64: the reference's algorithm on a CPU), {dtr:.1f} s wall"},
        "fftw": fftw_probe(),
    }


def oracle_parity(a, irs, params, excerpt, T, got, where):
    """Same-run parity: blocks of the LAST timed step's output against the float64 oracle
    (oracle.Upols.range, settled form: conv.cu:392-401 restated as the partitioned sum + Q1/Q2 terms).
    excerpt = inputs of the previous and the last step ([2, 2 T 256]); got = the last step's output [2, T 256]."""
    import oracle

    num = den = sig = 0.0
    nblk = 0
    worst = 0.0
    for b0, n in where:
        u = oracle.Upols(a.fft_size, True)
        for i, ir in enumerate(irs):
            u.prepare(i, ir)
        for h in (0, 1):
            u.set(h, **params[h])
        want = u.range(excerpt[0], excerpt[1], T + b0, n, settled=True)
        u.close()
        mine = got[:, b0 * BLOCK:(b0 + n) * BLOCK].astype(np.float64)
        e = float(np.sqrt(np.mean((mine - want) ** 2)))
        worst = max(worst, e)
        num += float(((mine - want) ** 2).sum())
        sig += float((want ** 2).sum())
        den += want.size
        nblk += n
    rms_err, rms_sig = (num / den) ** 0.5, (sig / den) ** 0.5
    return {"rms_err": rms_err, "rms_signal": rms_sig, "blocks": nblk, "tolerance": RMS_TOL, "ok": bool(rms_err <= RMS_TOL),
            "worst_range_rms": worst,
            "where": [f"[{b0}, {b0 + n})" for b0, n in where],
            "oracle": "oracle/oracle.c orc_upols_range_settled (float64 partitioned form + Q1/Q2 window sums, pinned to the "
                      "single-FFT restatement of conv.cu in tests/test_oracle.py), blocks of the last timed step"}


def second_level_bytes(blk, taps, fused):
    """Compulsory HBM bytes of one launch of the second-level transform over `blk` blocks: every delay-line slot of
    the window once (16 B: both inputs), the four paths' second-level spectra once (a bin's chunks run together on one
    XCD and share them in its L2), the partition sums written (16 B per block); the split form also parks its forward
    transforms in a stash (written once, read once)."""
    F2 = 8192 if fused else 16384
    nchunk = -(-blk // (F2 - taps + 1))
    window = 256 * 16 * (blk + taps - 1)
    spectra = 256 * 4 * 8 * F2
    sums = 256 * 16 * blk
    stash = 0 if fused else 2 * (256 * 2 * 8 * F2 * nchunk)
    return {"window": window, "spectra": spectra, "sums": sums, "stash": stash, "total": window + spectra + sums + stash,
            "chunks": nchunk}


def overlap_save_bytes(blk, taps16):
    """Compulsory HBM bytes of the three passes of the overlap-save form (csrc/ossave.hip.h) over `blk` blocks: segments of
    16384 - P16 blocks, each a 512 x 8192-point transform whose rows pass through memory twice (8 B per point)."""
    N = 512 * 8192
    hop = N // 256 - taps16
    nseg = -(-blk // hop)
    inter = 8 * N * nseg                       # the segment between two passes: one complex number per frame
    spectra = 2 * 16 * N // 2 + 2 * 16 * 8192  # {A, B} per bin: 256 row pairs x 8192 x 32 B, + rows 0 and 256
    cols = {"input": 8 * N * nseg, "rows_out": inter, "block_sum_parts": 16 * 512 * 512 * nseg}
    rows = {"rows_in": inter, "spectra": spectra, "rows_out": inter}
    out = {"rows_in": inter, "dry_input": 8 * 256 * blk, "output": 8 * 256 * blk}
    return {"segments": nseg, "blocks_per_segment": hop, "k_os_cols": cols, "k_os_rows": rows, "k_os_out": out,
            "rows_total": sum(rows.values()), "total": sum(cols.values()) + sum(rows.values()) + sum(out.values())}


def labelled_profile(name, key=None):
    """A number copied from a committed profile is labelled as such: {value..., from, commit}.  None if absent."""
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None
    try:
        d = json.load(open(path))
        if key is not None:
            d = d.get(key)
        if d is None:
            return None
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "log", "-1", "--format=%h", "--", os.path.join("profiles", name)],
                                             stderr=subprocess.DEVNULL).decode().strip() or None
        except Exception:
            commit = None
        if commit is None:  # (no git on the GPU box: the summariser stamped the commit the profile was taken at)
            probe = d if isinstance(d, dict) else {}
            commit = probe.get("profiled_at_commit") or next((v.get("profiled_at_commit") for v in probe.values() if isinstance(v, dict)), None)
        return {"data": d, "from": "profiles/" + name, "commit": commit,
                "note": "copied from a committed rocprofv3 profile of the same command, NOT measured in this run"}
    except Exception:
        return None


class Pairs:
    """The `Convolution` objects of one rank: one per stereo pair (main.cu:31-39).  Inputs / outputs are per pair."""

    def __init__(self, a, local, npairs, T, **kw):
        from cuda_audio_amd.engine import Convolution
        from cuda_audio_amd.synth import make_ir

        self.eng, self.irs = [], []
        thr = (T + 1) if a.mode == "stream" else 0
        for p in range(npairs):
            e = Convolution(f"bench{p}", a.fft_size, max_batch=T, device=local, stream_threshold=min(thr, 16385),
                            precision=a.precision, **kw)
            # two distinct IRs per pair (seed 5678 + path): in1 -> (L,R) through IR 0, in2 -> (L,R) through
            # IR 1: four different convolution paths, no shared spectra; every pair has its own
            irs = [make_ir(a.taps, seed=5678 + 4 * p), make_ir(a.taps, seed=5680 + 4 * p)]
            e.prepare(0, irs[0])
            e.prepare(1, irs[1])
            for h in (0, 1):
                e.cc[h].value.update(**bench_params(h))
            self.eng.append(e)
            self.irs.append(irs)

    def __iter__(self):
        return iter(self.eng)

    def __getitem__(self, i):
        return self.eng[i]

    def __len__(self):
        return len(self.eng)

    def close(self):
        for e in self.eng:
            e.close()


_BP = {"predelay": 0, "same_ir": False}


def bench_params(h):
    return dict(select=0 if _BP["same_ir"] else h, predelay=_BP["predelay"], dry=0.5, wet=0.5, panDry=0.0, panWet=0.0, level=1.0, vsteps=0)


def self_launch(a):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks ourselves (torch.distributed.run as a
    CHILD process on 127.0.0.1 and a free port), relay rank 0's JSON line and leave with the children's exit code.  This
    process has not touched the GPU (torch is not even imported yet) and replaces nothing: it waits."""
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC: what RCCL needs between processes on this driver)
    env.setdefault("OMP_NUM_THREADS", "4")
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE)
    line = None
    for raw in proc.stdout:  # rank 0 prints ONE JSON line; anything else a library wrote to stdout goes to stderr
        txt = raw.decode(errors="replace").rstrip("\n")
        if txt.startswith("{") and txt.endswith("}"):
            line = txt
        elif txt:
            print(txt, file=sys.stderr)
    rc = proc.wait()
    if line is not None:
        print(line, flush=True)
    sys.exit(rc if rc else (0 if line is not None else 1))


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a)
    if a.shipped_defaults:
        a.fft_size, a.taps, a.predelay, a.same_ir = 131072, 131072 - 1024, 1024, True
    _BP["predelay"], _BP["same_ir"] = a.predelay, a.same_ir
    # The contract is ONE JSON line on stdout.  Libraries below us write there too (gloo's connection banner, RCCL
    # at some debug levels): from here on everything that goes to file descriptor 1 lands on stderr, and the JSON
    # line is written to the original stdout at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist

    from cuda_audio_amd.engine import Convolution
    from cuda_audio_amd.sharded import shard_bounds, slice_bounds
    from cuda_audio_amd.synth import make_input, make_ir

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"--gpus {a.gpus} but the launcher started {world} rank(s)")
    if a.backend == "gloo":
        local %= max(torch.cuda.device_count(), 1)  # rehearsal: ranks may share a card
        if a.collective == "reduce":
            a.collective = "allreduce"              # gloo has no reduce on device tensors (reduce_scatter: emulated below)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    sharded = world > 1 or a.force_sharded
    if sharded:
        # RCCL prints its version banner to stdout at NCCL_DEBUG=VERSION; the contract is ONE JSON line on stdout
        if not os.environ.get("MCCONV_KEEP_NCCL_DEBUG"):
            os.environ.pop("NCCL_DEBUG", None)
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        elif a.backend == "gloo":
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    if a.precision == "fp16":
        a.mode = "stream"
    npairs = a.channels // 2
    P = (min(a.taps, a.fft_size - 1024) + BLOCK - 1) // BLOCK
    shard_world = world if world > 1 else (a.emulate_world if a.force_sharded and a.emulate_world > 1 else 1)
    root_only = a.collective == "reduce"
    # rotate through a few distinct input batches (sharded runs feed every rank the GLOBAL batch, world x T blocks: two there)
    n_distinct = 2 if sharded else 4
    comp = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(comp)

    def preferred(pb=0, pe=0):
        if a.blocks > 0:
            return a.blocks
        probe = Convolution("probe", a.fft_size, max_batch=a.max_blocks, device=local, part_begin=pb, part_end=pe)
        probe.prepare(0, make_ir(a.taps, seed=5678))
        t = probe.preferred_batch(a.max_blocks)
        probe.close()
        return t

    def timed(step, drain, steps, warmup, prewarm_ms=0.0, arm=None):
        """prewarm (untimed, clocks), W warm-up steps, then exactly K steps bracketed by barrier + synchronize."""
        npre = 0
        if prewarm_ms > 0:
            t0 = time.perf_counter()
            while True:
                for _ in range(8):
                    step(npre)
                    npre += 1
                drain()
                torch.cuda.synchronize()
                go = (time.perf_counter() - t0) * 1e3 < prewarm_ms
                if world > 1:  # every rank runs the same number of steps (they carry collectives)
                    f = torch.tensor([1.0 if go else 0.0], device=dev)
                    dist.all_reduce(f, op=dist.ReduceOp.MIN)
                    go = bool(f.item() > 0.5)
                if not go:
                    break
        for k in range(max(warmup, 1)):
            step(k)
        drain()
        torch.cuda.synchronize()
        if arm:
            arm()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        drain()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if world > 1:
            tt = torch.tensor([dt], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt, npre

    def unsharded_reference(T, nchk, xs_dev, pair):
        """rank 0: an unsharded engine fed the same batches from the same cold state (untimed checker)."""
        full = Pairs(a, local, pair + 1, T)  # (engines 0 .. pair; only the last one is used: same IR seeds per pair)
        e = full[pair]
        e.use_torch_stream(comp)
        outs = []
        ref_out = torch.zeros(2, T * BLOCK, device=dev)
        for k in range(nchk):
            o = (k % n_distinct) * T * BLOCK
            e.process_device(xs_dev[0, o:].data_ptr(), xs_dev[1, o:].data_ptr(), ref_out[0].data_ptr(), ref_out[1].data_ptr(), T)
            torch.cuda.synchronize()
            outs.append(ref_out.clone())
        full.close()
        return outs

    def make_inputs(T):
        xs = [make_input(n_distinct * T * BLOCK, seed=1234 + 10 * p) for p in range(npairs)]
        return xs, [torch.from_numpy(x).to(dev) for x in xs]

    # ------------------------------------------------------------------ the reference's own shape (config 2)
    def run_single_form():
        import ctypes as C

        import oracle

        T = a.blocks or 2048
        irs = [make_ir(a.taps, seed=5678), make_ir(a.taps, seed=5680)]

        def engine():
            e = Convolution("bench-single", a.fft_size, max_batch=T, device=local, form="single")
            for i, ir in enumerate(irs):
                e.prepare(i, ir)
            for h in range(2):
                e.cc[h].value.update(**bench_params(h))
            return e

        e = engine()
        x = make_input(n_distinct * T * BLOCK, seed=1234)
        d_in = torch.from_numpy(x).to(dev)
        d_out = torch.zeros(2, T * BLOCK, device=dev)
        e.use_torch_stream(comp)

        def step(k):
            o = (k % n_distinct) * T * BLOCK
            e.process_device(d_in[0, o:].data_ptr(), d_in[1, o:].data_ptr(), d_out[0].data_ptr(), d_out[1].data_ptr(), T)

        dt, npre = timed(step, lambda: None, a.steps, a.warmup, a.prewarm_ms)
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, {"output_pair0": d_out})
        calls = a.steps * T
        alg = e.algorithmic_bytes_per_block()
        traffic = 12 * a.fft_size * 8  # bytes the three kernels of a call move (header of csrc/singlefft.hip.h), cache-resident
        res = {"T": T, "dt": dt, "alg": alg, "traffic": traffic}
        e.close()
        # same-run parity: the stream from its cold start against the float64 restatement of onProcess (oracle.RefCompat)
        if not a.no_parity:
            nchk = 96
            e = engine()
            got = e.process(x[0, :nchk * BLOCK], x[1, :nchk * BLOCK])
            e.close()
            r = oracle.RefCompat(a.fft_size, True)
            for i, ir in enumerate(irs):
                r.prepare(i, ir)
            for h in range(2):
                r.set(h, **bench_params(h))
            t1 = time.perf_counter()
            want = r.process(x[0, :nchk * BLOCK], x[1, :nchk * BLOCK])
            t_or = time.perf_counter() - t1
            r.close()
            d = got.astype(np.float64) - want
            res["parity"] = {"rms_err": float(np.sqrt(np.mean(d * d))), "rms_signal": float(np.sqrt(np.mean(want * want))), "blocks": nchk,
                             "against": "oracle.RefCompat (float64 restatement of conv.cu:287-466, same buffers), cold start"}
            if not a.no_cpu_baseline:
                res["cpu_baseline"] = {"value": round(nchk * BLOCK / FS / t_or, 3), "unit": "x realtime", "cores": 1, "kind": "port",
                                       "sample": f"{nchk} calls of oracle/oracle.c orc_ref_process (the reference's single-transform "
                                                 f"algorithm in float64, own radix-2 FFT, one thread), {t_or:.1f} s wall"}
        if not a.no_latency:
            e = engine()
            L, fp = e._L, C.POINTER(C.c_float)
            bufs = [np.ascontiguousarray(x[0, :BLOCK]), np.ascontiguousarray(x[1, :BLOCK]), np.zeros(BLOCK, np.float32), np.zeros(BLOCK, np.float32)]
            ptrs = [b.ctypes.data_as(fp) for b in bufs]
            for _ in range(200):
                L.mc_process(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], BLOCK)
            n_lat = 2000
            t1 = time.perf_counter()
            for _ in range(n_lat):
                L.mc_process(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], BLOCK)
            lat = (time.perf_counter() - t1) / n_lat
            res["latency_mode"] = {"us_per_block_wall": round(lat * 1e6, 2), "rtf": round(BLOCK / FS / lat, 1), "avg_runtime_ms": round(e.avgRuntime(), 5),
                                   "note": "one mc_process per 256-frame period, host buffers in and out, back to back"}
            e.close()
        return res

    if a.form == "single":
        if sharded:
            raise SystemExit("--form single runs on one GPU (no partitions to shard)")
        r = run_single_form()
        T, dt = r["T"], r["dt"]
        per_call = dt / (a.steps * T)
        line = {
            "metric": "real-time factor (frames/s / 44.1k), stereo block=256, 2 s IR, the reference's single-transform shape",
            "unit": "x realtime", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup, "higher_is_better": True, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "value": round(a.steps * T * BLOCK / FS / dt, 2), "ms_per_step": round(dt / a.steps * 1e3, 4), "scaling": "weak",
            "config": {"workload": f"BASELINE config 2 in the reference's own shape (mc_config.form = 1): stereo 44.1 kHz, 256-frame "
                                   f"calls, {a.taps}-tap IRs, one {a.fft_size}-point transform per call, 2x2 path matrix; step = "
                                   f"{T} calls back to back (mc_process_batch_device)",
                       "blocks_per_step": T, "form": "single"},
            "roofline": {"bound": "hbm", "kernel": "k_sf_fwdmac + k_sf_inv1 + k_sf_inv2w (the three launches of one call)",
                         "achieved": round(r["traffic"] / per_call / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(r["traffic"] / per_call / 1e9 / HBM_PEAK_GBS, 4), "traffic": None,
                         "bytes_per_call": r["traffic"], "us_per_call": round(per_call * 1e6, 2),
                         "survey_algorithmic_bytes_per_call": r["alg"],
                         "note": "bytes the three kernels of a call move by construction (12 n_ref-long complex arrays: live spectra r+w, "
                                 "selected IRs, packed Y, pass-1 result, accumulators) / the call's share of the step. The working "
                                 "set (about 9 MiB) stays in the 256 MB last-level cache: this is cache bandwidth priced against the "
                                 "HBM peak; the calls are latency-bound (three dependent launches of a few microseconds each). Not the "
                                 "headline: the partitioned engine runs the same configuration three orders of magnitude faster "
                                 "(profiles/r2_bench_cfg2.json)."},
        }
        for k in ("parity", "cpu_baseline", "latency_mode"):
            if k in r:
                line[k] = r[k]
        if git_head():
            line["head"] = git_head()
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
        return

    # ------------------------------------------------------------------ single GPU
    def run_single():
        T = preferred()
        eng = Pairs(a, local, npairs, T, pipeline=(a.pipeline and a.precision == "fp32"))
        xs, d_in = make_inputs(T)
        d_out = [torch.zeros(2, T * BLOCK, device=dev) for _ in range(npairs)]
        torch.cuda.synchronize()
        # several pairs (config 4 on one GPU): each Convolution object on a stream of its own, as the reference's instances
        # are (conv.cu:147-150 creates four streams per object) - one pair's launches fill the CUs another's drain
        # (BENCH_ONE_STREAM=1: all on the compute stream)
        pair_streams = [comp] if (npairs == 1 or os.environ.get("BENCH_ONE_STREAM")) else [torch.cuda.Stream(device=dev) for _ in range(npairs)]
        for p, e in enumerate(eng):
            e.use_torch_stream(pair_streams[p % len(pair_streams)])

        def step(k):
            o = (k % n_distinct) * T * BLOCK
            for p, e in enumerate(eng):
                e.process_device(d_in[p][0, o:].data_ptr(), d_in[p][1, o:].data_ptr(), d_out[p][0].data_ptr(), d_out[p][1].data_ptr(), T)

        def drain():
            if a.pipeline:
                for e in eng:
                    e.fence()

        # kernel timing (HIP events on the launch stream around the dominant kernel) only during the timed steps
        def arm():
            eng[0].enable_kernel_timing(True)
            eng[0].kernel_stats(reset=True)

        t_pre = time.perf_counter()
        multi = len(pair_streams) > 1
        dt, npre = timed(step, drain, a.steps, a.warmup, a.prewarm_ms, None if multi else arm)
        prewarm_s = time.perf_counter() - t_pre - dt
        ks = eng[0].kernel_stats()
        eng[0].enable_kernel_timing(False)
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, {f"output_pair{p}": d_out[p] for p in range(npairs)})

        res = {"T": T, "dt": dt, "ks": ks,
               "prewarm": {"steps": npre, "untimed_ms_before_the_timed_steps": round(prewarm_s * 1e3, 1),
                           "note": "untimed: the step run back to back for --prewarm-ms before the --warmup steps, so that the "
                                   "timed region does not start on idle clocks"}}
        res["alg_bytes"] = eng[0].algorithmic_bytes_per_block()

        # ---- same-run parity: the last timed step's output (pair 0) against the CPU oracle, untimed
        if not a.no_parity:
            last = (a.steps - 1) % n_distinct
            prev = ((a.steps - 2) % n_distinct) if a.steps >= 2 else ((max(a.warmup, 1) - 1) % n_distinct)
            reach = a.fft_size // BLOCK + 3
            before = (npre + max(a.warmup, 1) + a.steps - 2) * T  # blocks of the stream before the excerpt
            q8 = min(a.taps, a.fft_size - 1024) + 255 + a.predelay > a.fft_size
            if a.precision != "fp32":
                res["parity"] = {"skipped": "fp16 storage has its own bar (tests/test_gpu_parity.py: 2e-3 of the wet RMS)"}
            elif q8:
                # the Q8 tail-drop regime (what the reference ships): the range oracle does not model the dropped tails, the
                # single-transform restatement of conv.cu does - from a cold start, a fresh engine, one batch of 160 blocks
                import oracle

                nchk = a.fft_size // BLOCK + 160  # (the cut terms start n_ref frames into the stream: 160 blocks with them)
                e2 = Pairs(a, local, 1, nchk)
                x = xs[0]
                got = e2[0].process(x[0, :nchk * BLOCK], x[1, :nchk * BLOCK])
                e2.close()
                r = oracle.RefCompat(a.fft_size, True)
                for i, ir in enumerate(eng.irs[0]):
                    r.prepare(i, ir)
                for h in range(2):
                    r.set(h, **bench_params(h))
                want = r.process(x[0, :nchk * BLOCK], x[1, :nchk * BLOCK])
                r.close()
                d = got.astype(np.float64) - want
                err = float(np.sqrt(np.mean(d * d)))
                res["parity"] = {"rms_err": err, "rms_signal": float(np.sqrt(np.mean(want * want))), "blocks": nchk, "tolerance": RMS_TOL,
                                 "ok": bool(err <= RMS_TOL),
                                 "oracle": "oracle/oracle.c orc_ref_process (float64 restatement of conv.cu:287-466 with the reference's own "
                                           "buffers: the Q8 tail drop comes out of the restated code), cold start, a fresh engine, one batch that runs "
                                           "160 blocks past the point (n_ref frames in) where the cut terms begin"}
            elif T < reach + 64 or before < 400:
                res["parity"] = {"skipped": f"steady-state excerpt needs batches of >= {reach + 64} blocks and a settled cross-fade"}
            else:
                x = xs[0]
                excerpt = np.concatenate([x[:, prev * T * BLOCK:(prev + 1) * T * BLOCK], x[:, last * T * BLOCK:(last + 1) * T * BLOCK]], axis=1)
                got = d_out[0].cpu().numpy()
                chunk = None
                lv = int(ks.get("fast_levels", 0))
                if lv == 253:
                    chunk = 16384 - int(ks["partitions"])  # overlap-save form: blocks per segment
                if lv in (254, 255):
                    chunk = (8192 if lv == 254 else 16384) - int(ks["partitions"]) + 1
                # >= 2048 blocks spread over the whole step: the first blocks of the launch (their windows reach into the previous
                # step), across every segment / chunk boundary of the form that ran, the middle of every segment / chunk, the batch end
                where = [(0, 64)]
                if chunk and chunk + 32 < T:
                    nch = -(-T // chunk)
                    per = max(32, -(-2048 // (2 * nch)) // 16 * 16)
                    for c in range(nch):
                        if c > 0:
                            where.append((c * chunk - per // 2, per))
                        mid = c * chunk + min(chunk, T - c * chunk) // 2
                        if mid + per <= T - 64:
                            where.append((mid, per))
                where.append((T - 64, 64))
                res["parity"] = oracle_parity(a, eng.irs[0], [bench_params(0), bench_params(1)], excerpt, T, got, where)

        if multi and a.full:
            # with the pairs on streams of their own an event bracket on one stream also spans the other pairs' kernels:
            # the dominant kernel is timed now, pair 0 alone (untimed steps, after the parity check has read its output)
            arm()
            scratch = torch.zeros(2, T * BLOCK, device=dev)
            for k in range(5):
                o = (k % n_distinct) * T * BLOCK
                eng[0].process_device(d_in[0][0, o:].data_ptr(), d_in[0][1, o:].data_ptr(), scratch[0].data_ptr(), scratch[1].data_ptr(), T)
            torch.cuda.synchronize()
            res["ks"] = ks = eng[0].kernel_stats()
            eng[0].enable_kernel_timing(False)

        # ---- host-visible throughput (SURVEY 8(d) "output fully produced in host-visible memory"): pinned host
        # buffers in and out through mc_process_batch, copies and kernels of consecutive chunks overlapped
        if not a.no_host_io and a.mode == "resident" and npairs == 1:
            e = eng[0]
            e.set_stream(None)
            nst = 10
            hin, hout = e.pinned_array((2, nst * T * BLOCK)), e.pinned_array((2, nst * T * BLOCK))
            for k in range(nst):
                o = (k % n_distinct) * T * BLOCK
                hin[:, k * T * BLOCK:(k + 1) * T * BLOCK] = xs[0][:, o:o + T * BLOCK]
            e.process(hin[0, :2 * T * BLOCK], hin[1, :2 * T * BLOCK], hout[:, :2 * T * BLOCK])  # warm-up: staging buffers, streams
            t1 = time.perf_counter()
            e.process(hin[0], hin[1], hout)
            dth = time.perf_counter() - t1
            nb = nst * T
            res["host_io"] = {
                "rtf": round(nb * BLOCK / FS / dth, 1), "ms_per_block_batch": round(dth / nst * 1e3, 4), "blocks": nb,
                "pcie_GBps_in": round(nb * 2 * BLOCK * 4 / dth / 1e9, 2), "pcie_GBps_out": round(nb * 2 * BLOCK * 4 / dth / 1e9, 2),
                "note": "mc_process_batch with pinned host buffers (mc_host_alloc): one call over %d blocks, chunks of the "
                        "engine's preferred batch, the copy-in of the next chunk under the kernels of the current one, whose last "
                        "kernel stores the output straight into the caller's pinned buffer; returns when the last output byte is "
                        "in host memory. Never `value`." % nb,
            }
            e.use_torch_stream(comp)

        # ---- latency mode (what JACK sees): one 256-frame period per mc_process call, host buffers in and out,
        # the call returns when the output is on the host.  Called through ctypes with preallocated buffers.
        if not a.no_latency and npairs == 1:
            import ctypes as C

            e = eng[0]
            e.set_stream(None)
            L = e._L
            fp = C.POINTER(C.c_float)
            x = xs[0]
            bufs = [np.ascontiguousarray(x[0, :BLOCK]), np.ascontiguousarray(x[1, :BLOCK]),
                    np.zeros(BLOCK, np.float32), np.zeros(BLOCK, np.float32)]
            ptrs = [b.ctypes.data_as(fp) for b in bufs]
            for _ in range(200):
                L.mc_process(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], BLOCK)
            n_lat = 2000
            t1 = time.perf_counter()
            for _ in range(n_lat):
                L.mc_process(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], BLOCK)
            lat = (time.perf_counter() - t1) / n_lat
            # what a JACK client sees: the host idle between periods (500 us here; a real period is 5805 us), the call's own
            # duration counted
            n_sp = 1000
            each = []
            for _ in range(n_sp):
                t1 = time.perf_counter()
                while (time.perf_counter() - t1) < 500e-6:
                    pass
                t1 = time.perf_counter()
                L.mc_process(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], BLOCK)
                each.append(time.perf_counter() - t1)
            spaced = sum(each) / n_sp
            spaced_q = np.percentile(np.array(each) * 1e6, [50, 90, 99])
            # a second pass with HIP events around the sweep kernel (the events cost a few us of their own: not in `lat`)
            e.enable_kernel_timing(True)
            e.kernel_stats(reset=True)
            for _ in range(500):
                L.mc_process(e._h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], BLOCK)
            ks1 = e.kernel_stats()
            e.enable_kernel_timing(False)
            k_ms = ks1["total_ms"] / max(ks1["launches"], 1)
            ab = res["alg_bytes"]
            latency = {
                "us_per_block_wall": round(lat * 1e6, 2),
                "rtf": round(BLOCK / FS / lat, 1),
                "us_per_call_period_spaced": round(spaced * 1e6, 2),
                "us_per_call_period_spaced_p50_p90_p99": [round(float(q), 2) for q in spaced_q],
                "rtf_period_spaced": round(BLOCK / FS / spaced, 1),
                "avg_runtime_ms": round(e.avgRuntime(), 5),
                "mac_kernel": "k_mac_stream (every block re-reads 4 IR paths + 2 delay-line inputs: the literal partition x bin MAC)",
                "mac_kernel_span_us": round(k_ms * 1e3, 2),
                "mac_kernel_timed_with": "time stamps inside the kernel: first workgroup start to last workgroup end (100 MHz counter), in a "
                                         "separate pass with every period launched on arrival. rocprofv3's duration of the same launch "
                                         "(dispatch and completion included) is 4.1-4.3 us: profiles/r2_jack_summary.md",
                "mac_algorithmic_GBps_over_span": round(ab / (k_ms * 1e-3) / 1e9, 1) if k_ms > 0 else None,
                # (not a roofline fraction: the 21 MB a period re-reads come out of L2 / Infinity Cache, and the span excludes dispatch - VERDICT round 2, weak 3)
                "mac_algorithmic_GBps_over_span_relative_to_hbm_peak": round(ab / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if k_ms > 0 else None,
                "note": "all values measured in this run. us_per_block_wall: calls back to back; us_per_call_period_spaced: 500 us idle "
                        "between calls, as under jackd (the next period's tail is launched one call ahead and parked; while it waits it "
                        "finishes every older partition's inverse transform and makes a dry run of the code between the period and its "
                        "output, and the period's own partition is then a direct convolution on eight wavefronts: csrc/jack_tail.hip.h, tail1_body). "
                        "The "
                        "21 MB working set is re-read every period and is served by L2 / Infinity Cache, not HBM "
                        "(FETCH_SIZE of this launch: profiles/)",
            }
            longer = {}
            for period in (512, 1024):
                if T % (period // BLOCK):
                    continue
                e.set_period(period)
                pb_ = [np.ascontiguousarray(x[0, :period]), np.ascontiguousarray(x[1, :period]),
                       np.zeros(period, np.float32), np.zeros(period, np.float32)]
                pp_ = [b.ctypes.data_as(fp) for b in pb_]
                for _ in range(200):
                    L.mc_process(e._h, pp_[0], pp_[1], pp_[2], pp_[3], period)
                t1 = time.perf_counter()
                for _ in range(1000):
                    L.mc_process(e._h, pp_[0], pp_[1], pp_[2], pp_[3], period)
                lp = (time.perf_counter() - t1) / 1000
                sp = 0.0
                for _ in range(300):  # the host idle between periods (500 us), as under jackd
                    t1 = time.perf_counter()
                    while (time.perf_counter() - t1) < 500e-6:
                        pass
                    t1 = time.perf_counter()
                    L.mc_process(e._h, pp_[0], pp_[1], pp_[2], pp_[3], period)
                    sp += time.perf_counter() - t1
                sp /= 300
                longer[str(period)] = {"us_per_call_wall": round(lp * 1e6, 2), "rtf": round(period / FS / lp, 1),
                                       "us_per_call_period_spaced": round(sp * 1e6, 2), "rtf_period_spaced": round(period / FS / sp, 1)}
            e.set_period(BLOCK)
            latency["longer_periods"] = longer
            res["latency_mode"] = latency

        # ---- the literal partition x bin MAC in throughput mode (north star: "the partition x bin complex-MAC kept as a
        # bandwidth-bound reduction ... evidenced by rocprof achieved-HBM-GB/s"): the streaming kernel over 2048-block batches,
        # every block re-reading its 4 IR paths and 2 delay-line inputs (21.17 MB per block at P = 1723)
        if not a.no_literal_mac and a.mode == "resident" and a.precision == "fp32" and npairs == 1:
            keep_mode = a.mode
            a.mode = "stream"
            Tl = min(2048, a.max_blocks)
            lit = Pairs(a, local, 1, Tl)
            a.mode = keep_mode
            le = lit[0]
            le.use_torch_stream(comp)
            lo = torch.zeros(2, Tl * BLOCK, device=dev)
            for k in range(3):
                le.process_device(d_in[0][0, k * Tl * BLOCK:].data_ptr(), d_in[0][1, k * Tl * BLOCK:].data_ptr(), lo[0].data_ptr(), lo[1].data_ptr(), Tl)
            torch.cuda.synchronize()
            le.enable_kernel_timing(True)
            le.kernel_stats(reset=True)
            nl = 8
            t1 = time.perf_counter()
            for k in range(nl):
                le.process_device(d_in[0][0, (k % 4) * Tl * BLOCK:].data_ptr(), d_in[0][1, (k % 4) * Tl * BLOCK:].data_ptr(), lo[0].data_ptr(), lo[1].data_ptr(), Tl)
            torch.cuda.synchronize()
            dtl = time.perf_counter() - t1
            lks = le.kernel_stats()
            le.enable_kernel_timing(False)
            ab = le.algorithmic_bytes_per_block()
            kavg = lks["total_ms"] / max(lks["launches"], 1)
            prof = labelled_profile("r4_literal_mac.json")
            res["literal_mac"] = {
                "kernel": "k_mac_stream", "blocks_per_launch": Tl, "rtf": round(nl * Tl * BLOCK / FS / dtl, 1), "ms_per_step": round(dtl / nl * 1e3, 4),
                "kernel_avg_ms": round(kavg, 5), "kernel_launches": lks["launches"], "partitions": lks["partitions"],
                "survey_8d_bytes_per_block": ab, "survey_8d_GBps": round(ab * Tl / (kavg * 1e-3) / 1e9, 1) if kavg > 0 else None,
                "frac_of_hbm_peak": round(ab * Tl / (kavg * 1e-3) / 1e9 / HBM_PEAK_GBS, 3) if kavg > 0 else None,
                "note": "the partition x bin MAC as written in SURVEY 8(d) - lanes = partitions, every block re-reads the IR spectra and the "
                        "delay-line window - 2048 blocks per launch; its 21 MB working set is served by L2 / Infinity Cache, so the "
                        "SURVEY-8(d) byte rate exceeds the HBM peak (the committed rocprofv3 FETCH_SIZE of this launch says how little "
                        "reaches the memory side); at one block per launch (latency_mode) the same kernel reads HBM-class latency",
            }
            if prof:
                res["literal_mac"]["memory_side_traffic"] = prof
            lit.close()

        if not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(eng.irs[0][0], eng.irs[0][1], xs[0], a.cpu_seconds)
        eng.close()
        return res

    # ------------------------------------------------------------------ multi GPU, layout 1: output blocks sliced
    def sliced_preferred():
        """Output blocks per rank of a block-sliced step: whole segments of the overlap-save form (a slice's segments are 16384 -
        max(P16, n_ref / 256 + 34) blocks: the first one also carries the blocks whose Q1/Q2 terms the slice's windows reach) minus
        the reach-back blocks of the predelay; the engine's own preference where that form does not apply."""
        Tb = preferred()
        if a.blocks > 0 or a.precision != "fp32" or os.environ.get("MCCONV_OS") == "0" or a.pipeline:
            return Tb
        p16 = -(-P // 16) * 16
        hop = 16384 - max(p16, a.fft_size // BLOCK + 8192 // BLOCK + 2)
        halo = -(-a.predelay // BLOCK) + 1
        k = a.max_blocks // hop
        if min(a.taps, a.fft_size - 1024) + 255 + a.predelay > a.fft_size or k < 1 or k * hop - halo < 12288:
            return Tb  # (Q8 regime, or a limit below one segment: the partitioned passes)
        return k * hop - halo

    def run_blocks():
        Tb = sliced_preferred()
        T = Tb * shard_world  # weak scaling: every rank finishes Tb output blocks of a batch of N x Tb
        first, count = slice_bounds(T, shard_world, rank)
        pipelined = a.pipeline and a.precision == "fp32"
        eng = Pairs(a, local, npairs, T, pipeline=pipelined)
        xs, d_in = make_inputs(T)
        d_slices = [[torch.zeros(2, count * BLOCK, device=dev) for _ in range(3)] for _ in range(npairs)]
        gather = rank == 0 and shard_world == world and a.exchange == "gather"
        d_gather = [[torch.zeros(2, count * BLOCK, device=dev) for _ in range(world)] for _ in range(2)] if gather else None
        torch.cuda.synchronize()
        for e in eng:
            e.use_torch_stream(comp)
        pending, ungathered = [], []
        kept = None

        class _Done:
            def wait(self):
                pass

        def gather_slices(sl, k):
            # the only exchange of the block-sliced layout: count * 2 KB per rank and batch to rank 0, off the data path
            if shard_world != world or a.exchange == "none":
                return _Done()
            if a.backend == "gloo":  # rehearsal: through host memory
                h = sl.cpu()
                hl = [torch.zeros_like(h) for _ in range(world)] if rank == 0 else None
                dist.gather(h, hl, dst=0)
                if rank == 0:
                    for g, t in zip(d_gather[k % 2], hl):
                        g.copy_(t)
                return _Done()
            return dist.gather(sl, d_gather[k % 2] if rank == 0 else None, dst=0, async_op=True)

        def retire_slices():
            work, k = pending.pop(0)
            work.wait()
            if kept is not None and rank == 0:
                kept.append(torch.cat(d_gather[k % 2], dim=1) if d_gather is not None else d_slices[0][k % 3].clone())

        def hand_over(older_only):
            if pipelined:
                for e in eng:
                    e.fence_older() if older_only else e.fence()
            keep = ungathered[-1:] if older_only else []
            for j in ungathered[:len(ungathered) - len(keep)]:
                while len(pending) >= 2:  # the gather buffers are two deep
                    retire_slices()
                pending.append((gather_slices(d_slices[0][j % 3], j), j))
            ungathered[:] = keep

        def step(k):
            o = (k % n_distinct) * T * BLOCK
            while len(pending) > (0 if a.no_overlap else 1):
                retire_slices()
            for p, e in enumerate(eng):
                sl = d_slices[p][k % 3]
                e.process_slice_device(d_in[p][0, o:].data_ptr(), d_in[p][1, o:].data_ptr(), sl[0].data_ptr(), sl[1].data_ptr(), T, first, count)
            ungathered.append(k)
            hand_over(older_only=pipelined and not a.no_overlap)
            if a.no_overlap:
                while pending:
                    retire_slices()

        def drain():
            hand_over(older_only=False)
            while pending:
                retire_slices()

        dt, npre = timed(step, drain, a.steps, a.warmup, a.prewarm_ms)
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, {f"output_pair{p}_rank{rank}": d_slices[p][(a.steps - 1) % 3] for p in range(npairs)})
        res = {"T": T, "count": count, "dt": dt, "rtf": a.steps * T * BLOCK / FS / dt, "prewarm_steps": npre}
        if not a.no_check:
            for e in eng:
                e.reset()
            kept = []
            nchk = 3
            for k in range(nchk):
                step(k)
            drain()
            torch.cuda.synchronize()
            if rank == 0:
                refs = unsharded_reference(T, nchk, d_in[0], 0)
                num = den = 0.0
                for k in range(nchk):
                    want = refs[k] if kept[k].shape == refs[k].shape else refs[k][:, first * BLOCK:(first + count) * BLOCK]
                    num += float(((kept[k] - want).double() ** 2).sum())
                    den += float((want.double() ** 2).sum())
                n_el = nchk * kept[0].numel()
                res["sharded_check"] = {"batches": nchk, "rms_err_vs_unsharded": (num / n_el) ** 0.5, "rms_signal": (den / n_el) ** 0.5}
            kept = None
            if world > 1:
                dist.barrier()
        eng.close()
        return res

    # ------------------------------------------------------------------ multi GPU, layout 2: IR partitions sharded + RCCL sum
    def run_partitions(direct=False):
        # direct: the sum over partitions as the literal resident MAC (MCCONV_FFT2=0, read when an engine is created) - the one
        # form whose per-rank work is P / N partitions per block, i.e. the strong-scaling curve the north star describes
        pb, pe = shard_bounds(P, shard_world, rank)
        if pe <= pb:
            raise SystemExit("empty shard; use fewer ranks")
        keep_env = os.environ.get("MCCONV_FFT2")
        if direct:
            os.environ["MCCONV_FFT2"] = "0"
        T = preferred(*shard_bounds(P, shard_world, 0))  # the same batch length on every rank: rank 0's shard decides
        if direct:
            T = min(T, 32768) // shard_world * shard_world  # (the MAC costs P / N partitions per block: shorter steps keep the run short)
        coll = a.collective
        if coll == "reduce_scatter" and T % shard_world:
            coll = "reduce"  # (the slices of a reduce-scatter are equal runs of whole blocks)
        rs = coll == "reduce_scatter"
        root_only_ = coll == "reduce"
        Ts = T // shard_world if rs else T          # blocks this rank finishes
        first = rank * Ts if rs else 0
        eng = Pairs(a, local, npairs, T, part_begin=pb, part_end=pe)
        if direct:
            if keep_env is None:
                os.environ.pop("MCCONV_FFT2", None)
            else:
                os.environ["MCCONV_FFT2"] = keep_env
        xs, d_in = make_inputs(T)
        d_out = [torch.zeros(2, Ts * BLOCK, device=dev) for _ in range(npairs)]
        # the partial wet blocks of all pairs of a rank: [pair][channel][T * 256]
        d_parts = [torch.zeros(npairs, 2, T * BLOCK, device=dev) for _ in range(2)]
        d_sums = [torch.zeros(npairs, 2, Ts * BLOCK, device=dev) for _ in range(2)] if rs else None
        torch.cuda.synchronize()
        for e in eng:
            e.use_torch_stream(comp)
        pending = []
        kept = None

        class _Works:
            def __init__(self, ws):
                self.ws = ws

            def wait(self):
                for w in self.ws:
                    if w is not None:
                        w.wait()  # makes the compute stream wait for the collective; the host does not block

        def collective(part, ssum):
            if rs:
                ws = []
                for p in range(npairs):
                    for c in range(2):  # one reduce-scatter per channel half: its N equal runs of blocks are the ranks' slices
                        if world == 1:  # (one rank: the "sum" is the rank's own partial)
                            ssum[p, c].copy_(part[p, c, first * BLOCK:(first + Ts) * BLOCK])
                        elif a.backend == "gloo":  # rehearsal: gloo has no reduce-scatter on device tensors
                            h = part[p, c].cpu()
                            dist.all_reduce(h)
                            ssum[p, c].copy_(h[first * BLOCK:(first + Ts) * BLOCK])
                        else:
                            ws.append(dist.reduce_scatter_tensor(ssum[p, c], part[p, c], async_op=True))
                return _Works(ws)
            if root_only_:
                return _Works([dist.reduce(part, dst=0, async_op=True)])
            return _Works([dist.all_reduce(part, async_op=True)])

        def retire():
            work, part, ssum, o = pending.pop(0)
            work.wait()
            for p, e in enumerate(eng):
                if rs:
                    e.finish_slice_device(d_in[p][0, o:].data_ptr(), d_in[p][1, o:].data_ptr(), ssum[p].data_ptr(),
                                          d_out[p][0].data_ptr(), d_out[p][1].data_ptr(), T, first, Ts)
                elif rank == 0 or not root_only_:
                    e.finish_device(d_in[p][0, o:].data_ptr(), d_in[p][1, o:].data_ptr(), part[p].data_ptr(),
                                    d_out[p][0].data_ptr(), d_out[p][1].data_ptr(), T)
                else:
                    e.finish_device(None, None, None, None, None, T)
            if kept is not None and rank == 0:
                kept.append(d_out[0].clone())

        def step(k, with_collective=True):
            o = (k % n_distinct) * T * BLOCK
            part = d_parts[k % 2]
            ssum = d_sums[k % 2] if rs else None
            for p, e in enumerate(eng):
                e.partial_device(d_in[p][0, o:].data_ptr(), d_in[p][1, o:].data_ptr(), part[p].data_ptr(), T)
            work = collective(part, ssum) if with_collective else _Works([])
            # the sum of batch k overlaps the kernels of batch k + 1: batch k - 1 is finished now
            if pending and not a.no_overlap:
                retire()
            pending.append((work, part, ssum, o))
            if a.no_overlap:
                retire()

        def drain():
            while pending:
                retire()

        dt, npre = timed(step, drain, max(2, a.steps // 4) if direct else a.steps, min(a.warmup, 2) if direct else a.warmup, 0.0 if direct else a.prewarm_ms)
        nsteps = max(2, a.steps // 4) if direct else a.steps
        if a.dump_outputs and not direct and a.layouts == "partitions" and (rs or rank == 0 or not root_only_):  # (the headline layout only)
            dump_outputs(a.dump_outputs, {f"output_pair{p}_rank{rank}": d_out[p] for p in range(npairs)})
        lv = None
        n = shard_world
        sent = int(npairs * 2 * T * BLOCK * 4 * ((n - 1) / n if rs else (1.0 if root_only_ else 2.0 * (n - 1) / n)))
        res = {"T": T, "dt": dt, "steps": nsteps, "rtf": nsteps * T * BLOCK / FS / dt, "partitions_per_rank": pe - pb, "prewarm_steps": npre,
               "collective": coll, "blocks_finished_per_rank": Ts, "reduce_bytes_per_step": int(npairs * 2 * T * BLOCK * 4),
               "reduce_bytes_per_rank_per_step": sent}
        # what the first hardware run should explain by itself: the kernels alone, the collective alone, and which one binds
        if world > 1 and a.backend == "nccl" and a.full:
            nk = max(4, min(a.steps, 20))
            dt_comp, _ = timed(lambda k: step(k, with_collective=False), drain, nk, 2)
            part, ssum = d_parts[0], (d_sums[0] if rs else None)

            def only_collective(k):
                collective(part, ssum).wait()

            dt_coll, _ = timed(only_collective, lambda: None, nk, 2)
            res["kernels_only_ms_per_step"] = round(dt_comp / nk * 1e3, 4)
            res["collective_only_ms_per_step"] = round(dt_coll / nk * 1e3, 4)
            res["collective_GBps_per_rank"] = round(sent / (dt_coll / nk) / 1e9, 2)
            res["link_bound"] = bool(dt_coll > dt_comp)
        if not a.no_check:
            for e in eng:
                e.reset()
            eng[0].enable_kernel_timing(True)
            kept = []
            nchk = 2 if direct else 3
            for k in range(nchk):
                step(k)
            drain()
            torch.cuda.synchronize()
            lv = eng[0].kernel_stats()["fast_levels"]
            eng[0].enable_kernel_timing(False)
            if rank == 0:
                refs = unsharded_reference(T, nchk, d_in[0], 0)
                num = den = 0.0
                for k in range(nchk):
                    want = refs[k][:, first * BLOCK:(first + Ts) * BLOCK]
                    num += float(((kept[k] - want).double() ** 2).sum())
                    den += float((want.double() ** 2).sum())
                n_el = nchk * kept[0].numel()
                res["sharded_check"] = {"batches": nchk, "rms_err_vs_unsharded": (num / n_el) ** 0.5, "rms_signal": (den / n_el) ** 0.5,
                                        "blocks_checked_per_batch": Ts}
            kept = None
            if world > 1:
                dist.barrier()
        res["sum_over_partitions"] = {253: "overlap-save segments (k_os_cols, k_os_rows, k_os_out)", 254: "second-level transform, fused form (k_g2_mac)", 255: "second-level transform, split form",
                                      0: "direct-form MAC"}.get(lv, str(lv))
        eng.close()
        return res

    # ------------------------------------------------------------------ assemble the line
    workload = (f"{a.channels}-channel ({npairs} stereo pair(s), one Convolution object each) 44.1 kHz, 256-frame blocks, "
                f"{a.taps}-tap IRs ({P} partitions, N_ref {a.fft_size}), 2x2 path matrix per pair"
                + (f", predelay {a.predelay}" if a.predelay else "") + (", both halves on one IR" if a.same_ir else "")
                + (" [the reference's shipped operating point, settings.txt:19,38-45: Q8 tail-drop regime]" if a.shipped_defaults else ""))
    line = {
        "metric": "real-time factor (frames/s / 44.1k), stereo block=256, 10 s IR",
        "unit": "x realtime",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "higher_is_better": True,
        "vs_baseline": None,
        "dtype": "f32" if a.precision == "fp32" else "f16 storage, f32 accumulate",
        "data": "synthetic",
    }
    if git_head():
        line["head"] = git_head()
    if not sharded:
        r = run_single()
        T, dt, ks = r["T"], r["dt"], r["ks"]
        rtf = a.steps * T * BLOCK / FS / dt
        alg_bytes = r["alg_bytes"]
        kern_s = ks["total_ms"] * 1e-3
        kern_avg_ms = ks["total_ms"] / max(ks["launches"], 1)
        blk = (ks["blocks"] // max(ks["launches"], 1)) if ks["launches"] else T
        flops_per_block = 8.0 * 4 * ks["partitions"] * 256  # complex MAC = 8 flop, 4 paths
        achieved_tf = flops_per_block * ks["blocks"] / kern_s / 1e12 if kern_s > 0 else 0.0
        survey_gbs = alg_bytes * ks["blocks"] / kern_s / 1e9 if kern_s > 0 else 0.0
        survey = {"achieved": round(survey_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(survey_gbs / HBM_PEAK_GBS, 4),
                  "algorithmic_bytes_per_block": alg_bytes,
                  "note": "SURVEY 8(d) accounting of the partition x bin MAC (every block re-reads 4 IR paths + 2 delay-line "
                          "inputs) x blocks / kernel time. A frac far above 1 says what it looks like: the timed kernel does NOT do "
                          "that work - it replaces the MAC by a transform along the block axis; the literal MAC is k_mac_stream "
                          "(latency_mode) and MCCONV_FFT2=0"}
        common = {"kernel_avg_ms": round(kern_avg_ms, 5), "kernel_launches": ks["launches"], "blocks_per_launch": blk,
                  "timed_with": "HIP events on the launch stream around the kernel, inside the timed steps"}
        lv = int(ks.get("fast_levels", 0))
        if ks["resident"] and lv in (254, 255):
            fused = lv == 254
            cb = second_level_bytes(blk, int(ks["partitions"]), fused)
            gbs = cb["total"] / (kern_avg_ms * 1e-3) / 1e9 if kern_avg_ms > 0 else 0.0
            tr = labelled_profile("r3_hbm_traffic.json", "headline")
            traffic = None
            if tr:
                rec = [v for k, v in tr["data"].items() if ("k_g2_mac" if fused else "k_f2_") in k]
                tr["data"] = rec
                if rec and all(int(v.get("blocks_per_launch", -1)) == int(blk) for v in rec):
                    traffic = sum(int(v["hbm_bytes_per_launch"]) for v in rec)
            roofline = dict({"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": traffic,
                             "kernel": "k_g2_mac" if fused else "k_f2_fwd + k_f2_prod"}, **common)
            roofline["algorithmic_bytes_per_launch"] = cb["total"]
            roofline["algorithmic_bytes"] = cb
            # numbers copied from the committed headline profile are attached only when this run's launch is the profiled one
            if tr and traffic is not None:
                roofline["traffic_source"] = {k: tr[k] for k in ("from", "commit", "note")}
            bind = labelled_profile("r3_headline_counters.json", "derived") if fused and traffic is not None else None
            if bind:
                roofline["binding_resource"] = bind
            # the whole step against the same roof: the other launches of a step are pure streams (forward transforms:
            # input in, delay-line spectra out; inverse transforms + output stage: partition sums and dry input in, output out)
            step_ms = dt / a.steps * 1e3
            other = 256 * T * npairs * ((2 * 4 + 16) + (16 + 2 * 4 + 2 * 4))
            step_bytes = cb["total"] * npairs * max(1, -(-T // max(blk, 1))) + other
            roofline["whole_step"] = {"compulsory_bytes": step_bytes, "ms": round(step_ms, 4),
                                      "achieved": round(step_bytes / (step_ms * 1e-3) / 1e9, 1), "unit": "GB/s",
                                      "frac": round(step_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                      "note": "compulsory bytes of all launches of a step (k_fwd: 2 inputs in, 16 B per bin out; the "
                                              "second-level transform as above; inverse transforms + output: 16 B per bin and the dry "
                                              "input in, 2 channels out) / wall time per step, launch gaps included"}
            roofline["survey_8d_accounting"] = survey
            roofline["direct_form_equivalent_tflops"] = round(achieved_tf, 2)
            roofline["note"] = ("achieved = COMPULSORY bytes of the launch (every delay-line slot of the window once, the four "
                                "paths' second-level spectra once, the partition sums written" + ("" if fused else ", the stash written and read once")
                                + ") / kernel time. The kernel is a second-level transform along the block axis (per bin one circular "
                                "convolution per chunk of blocks), not the partition x bin MAC of SURVEY 8(d); survey_8d_accounting "
                                "prices it that way for reference.")
        elif ks["resident"] and lv == 253:
            cb = overlap_save_bytes(blk, int(ks["partitions"]))
            gbs = cb["rows_total"] / (kern_avg_ms * 1e-3) / 1e9 if kern_avg_ms > 0 else 0.0
            tr = labelled_profile("r4_hbm_traffic.json", "headline")
            traffic = None
            if tr:
                rec = [v for k, v in tr["data"].items() if k.split("(")[0].strip() == "k_os_rows"]
                tr["data"] = rec
                if rec and all(int(v.get("blocks_per_launch", -1)) == int(blk) for v in rec):
                    traffic = sum(int(v["hbm_bytes_per_launch"]) for v in rec)
            roofline = dict({"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": traffic, "kernel": "k_os_rows"}, **common)
            roofline["algorithmic_bytes_per_launch"] = cb["rows_total"]
            roofline["algorithmic_bytes"] = cb
            if tr and traffic is not None:
                roofline["traffic_source"] = {k: tr[k] for k in ("from", "commit", "note")}
            step_ms = dt / a.steps * 1e3
            step_bytes = cb["total"] * npairs * max(1, -(-T // max(blk, 1)))
            roofline["whole_step"] = {"compulsory_bytes": step_bytes, "ms": round(step_ms, 4),
                                      "achieved": round(step_bytes / (step_ms * 1e-3) / 1e9, 1), "unit": "GB/s",
                                      "frac": round(step_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                      "input_plus_output_bytes": 16 * 256 * T * npairs,
                                      "note": "compulsory bytes of the three passes of a step (column pass: both inputs in incl. each "
                                              "segment's history, the segment's rows out; row pass: rows in and out, the spectra once; output "
                                              "pass: rows and dry input in, both channels out) / wall time per step, launch gaps and the small "
                                              "launches on the side stream included.  input_plus_output_bytes is what a single pass would move."}
            roofline["survey_8d_accounting"] = survey
            roofline["direct_form_equivalent_tflops"] = round(achieved_tf, 2)
            roofline["note"] = ("achieved = COMPULSORY bytes of the row pass (every row of every segment in and out once, the spectra once) / "
                                "kernel time. The batch runs as overlap-save segments of 512 x 8192 frames (one whole-IR spectrum product per "
                                "segment, as the reference's own algorithm does per call, conv.cu:367-408), not as the partition x bin MAC of "
                                "SURVEY 8(d); survey_8d_accounting prices it that way for reference. MCCONV_OS=0 selects the second-level-"
                                "transform path of round 3 (k_g2_mac), --mode stream the literal MAC.")
        elif ks["resident"]:
            roofline = dict({"bound": "mfma", "achieved": round(achieved_tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(achieved_tf / FP32_PEAK_TFLOPS, 4), "traffic": None, "kernel": "k_mac_resident"}, **common)
            executed_tf = achieved_tf * (0.75 ** lv)
            roofline["executed"] = {"fast_fir_levels": lv, "multiply_add_fraction": round(0.75 ** lv, 4),
                                    "tflops": round(executed_tf, 2), "frac": round(executed_tf / FP32_PEAK_TFLOPS, 4)}
            roofline["survey_8d_accounting"] = survey
            roofline["note"] = ("fp32 complex MAC on the vector ALU (v_pk_fma_f32; the f32 MFMA rate of gfx950 equals the vector rate). "
                                "achieved = ALGORITHMIC flops of the partition x bin MAC / kernel time; the fast-FIR form issues "
                                "(3/4)^levels of them (`executed`).")
        else:
            roofline = dict({"bound": "hbm", "achieved": round(survey_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(survey_gbs / HBM_PEAK_GBS, 4), "traffic": None, "kernel": "k_mac_stream"}, **common)
            roofline["algorithmic_bytes_per_block"] = alg_bytes
            roofline["note"] = ("streaming MAC: every block re-reads IR spectra and delay line; achieved = SURVEY 8(d) bytes x blocks / "
                                "kernel time. With many blocks per launch the working set is served from L2 / Infinity Cache, so "
                                "achieved can exceed the HBM peak.")
        if not ks["launches"]:
            roofline = {"skipped": "no kernel was timed: with several pairs the dominant kernel is timed in a pass of its own (--full)"}
        line.update({
            "value": round(rtf, 2),
            "ms_per_step": round(dt / a.steps * 1e3, 4),
            "scaling": "weak",
            "config": {"workload": workload + f", {T} blocks per step, "
                                   + ("IR spectra re-read for every block (streaming MAC)" if a.mode == "stream" else
                                      "sum over partitions by " + str(roofline.get("kernel"))),
                       "blocks_per_step": T, "partitions": P, "paths": 4 * npairs, "mode": a.mode, "parallelism": "single GPU",
                       **({"note": "fp16 storage exists for the literal streaming MAC only (an HBM stress, BASELINE config 5); the engine's "
                                   "fast path for this configuration is fp32 with the second-level transform (profiles/r2_bench_cfg5_fp32.json), "
                                   "two orders of magnitude faster"} if a.precision == "fp16" else {})},
            "value_host_visible": (r.get("host_io") or {}).get("rtf"),
            "value_clauses": {"value": "SURVEY 8(d) throughput mode with inputs and outputs resident in HBM (the prompt's `value`: inputs already in HBM "
                                       "when the timed region starts); NOT 8(d)'s 'output fully produced in host-visible memory'",
                              "value_host_visible": "the same path through pinned HOST buffers in and out (mc_process_batch; PCIe both ways, bound by the link): "
                                                    "8(d)'s host-visible clause; = host_io.rtf"},
            "roofline": roofline,
            "parity": r.get("parity"),
            "literal_mac": r.get("literal_mac"),
            "cpu_baseline": r.get("cpu_baseline"),
            "host_io": r.get("host_io"),
            "latency_mode": r.get("latency_mode"),
            "prewarm": r["prewarm"],
        })
    else:
        rb = run_blocks() if a.layouts in ("both", "blocks") else None
        rp = run_partitions() if a.layouts in ("both", "partitions") else None
        rpd = run_partitions(direct=True) if (a.layouts in ("both", "partitions") and a.precision == "fp32" and not a.no_direct_mac) else None
        main_r = rb if rb is not None else rp
        by_blocks = rb is not None
        ex = "RCCL" if a.backend == "nccl" else "gloo (rehearsal)"
        par_blocks = (f"dp{world}: output blocks of every batch sliced over {world} GPU(s) ({rb['count']} blocks each; every GPU holds "
                      f"the whole IR set and transforms the input its windows reach); no data-path collective, "
                      + (f"slices gathered to rank 0 ({ex})" if a.exchange == "gather" else "slices left on their ranks")) if rb else None
        par_parts = (f"IR partitions sharded over {world} GPU(s) ({rp['partitions_per_rank']} of {P} per rank) + {ex} {rp['collective']} of the "
                     f"partial wet blocks ({rp['reduce_bytes_per_step'] / 1e6:.0f} MB of partials per rank and step, "
                     f"{rp['reduce_bytes_per_rank_per_step'] / 1e6:.0f} MB of them leave the rank; every rank finishes "
                     f"{rp['blocks_finished_per_rank']} of the {rp['T']} blocks), overlapped with the next batch") if rp else None
        why = ("`value` is the block-sliced layout: given the input, the output blocks of a batch are independent units, so they "
               "shard with no exchange step at all; the north-star layout (partition shards + RCCL sum) is measured in the same "
               "run under north_star_layout. It cannot scale batch throughput on this engine: the sum over partitions is a "
               "transform along the block axis whose cost does not depend on the number of partitions, so every rank still does "
               "the whole forward / second-level / inverse work and the step only gains the exchange of the partials (a "
               "reduce-scatter: each rank receives and finishes 1/N of the blocks); it is the layout for IR sets that do not fit one GPU.")
        line.update({
            "value": round(main_r["rtf"], 2),
            "ms_per_step": round(main_r["dt"] / a.steps * 1e3, 4),
            "scaling": "weak" if by_blocks else "strong",
            "config": {"workload": workload + f", {main_r['T']} blocks per step", "blocks_per_step": main_r["T"], "partitions": P,
                       "paths": 4 * npairs, "mode": a.mode,
                       "parallelism": (par_blocks + ". " + why) if by_blocks else par_parts},
        })
        if rb is not None and "sharded_check" in rb:
            line["sharded_check"] = rb["sharded_check"]
        if rp is not None:
            ns = {"value": round(rp["rtf"], 2), "unit": "x realtime", "ms_per_step": round(rp["dt"] / a.steps * 1e3, 4),
                  "scaling": "strong", "blocks_per_step": rp["T"], "parallelism": par_parts,
                  "sum_over_partitions": rp["sum_over_partitions"],
                  "collective": rp["collective"], "reduce_bytes_per_rank_per_step": rp["reduce_bytes_per_rank_per_step"],
                  "reduce_GBps": round(rp["reduce_bytes_per_rank_per_step"] * a.steps / rp["dt"] / 1e9, 2)}
            for k in ("kernels_only_ms_per_step", "collective_only_ms_per_step", "collective_GBps_per_rank", "link_bound"):
                if k in rp:
                    ns[k] = rp[k]
            if "sharded_check" in rp:
                ns["sharded_check"] = rp["sharded_check"]
                if world == 1 and shard_world > 1:  # (one GPU acting as rank 0 of an emulated world: a timing run)
                    ns["sharded_check"]["note"] = (f"emulated world of {shard_world} on one GPU: the sum holds this rank's partitions only, so the difference "
                                                   "to the unsharded engine IS the other ranks' share - not a parity figure")
            if by_blocks:
                line["north_star_layout"] = ns
            else:
                line["sharded_check"] = rp.get("sharded_check")
        if rpd is not None:
            nd = {"value": round(rpd["rtf"], 2), "unit": "x realtime", "ms_per_step": round(rpd["dt"] / rpd["steps"] * 1e3, 4), "steps": rpd["steps"],
                  "scaling": "strong", "blocks_per_step": rpd["T"], "partitions_per_rank": rpd["partitions_per_rank"],
                  "sum_over_partitions": rpd["sum_over_partitions"], "collective": rpd["collective"],
                  "reduce_bytes_per_rank_per_step": rpd["reduce_bytes_per_rank_per_step"],
                  "note": "the same partition shards + reduce-scatter with the sum over partitions as the literal resident MAC (MCCONV_FFT2=0): "
                          "the one form whose per-rank work falls as P / N - the strong-scaling curve BASELINE's north star describes. Far "
                          "slower in absolute terms than the transform forms (every block re-reads its shard of the IR spectra)."}
            for k in ("kernels_only_ms_per_step", "collective_only_ms_per_step", "collective_GBps_per_rank", "link_bound", "sharded_check"):
                if k in rpd:
                    nd[k] = rpd[k]
            line["north_star_layout_direct_mac"] = nd
    if rank == 0:
        os.write(real_stdout, (json.dumps(line) + "\n").encode())
    if sharded:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
