#!/usr/bin/env python
"""bench.py — utterances/sec of a full SpatialNet-small bf16-mixed TRAINING step on MI355X.

Workload (BASELINE.json configs[1]): synthetic 4-s, 6-channel, 8-kHz mixtures
(x[B,6,32000], 2 speakers), n_fft 256 / hop 128 -> F=129, T=251; one step = STFT + per-bin norm ->
SpatialNet-small (8 layers, H=96) forward -> inorm + iSTFT -> uPIT neg-SI-SDR -> full backward ->
[gradient all-reduce over RCCL] -> clip(5) + Adam(1e-3) -> re-pack of the MFMA weight fragments.
Inputs are resident in HBM before the timed region.  One process per GPU (torchrun sets RANK / LOCAL_RANK /
WORLD_SIZE), weak scaling: the per-GPU batch is fixed.

Prints ONE JSON line (rank 0) with the contract keys (ms_per_step: wall time of one timed step).  A plain run sets up, warms up,
times --steps steps and nothing else; --full adds
  roofline     : dominant kernel (largest share of GPU time), algorithmic HBM bytes per launch / its average
                 duration measured with HIP events on the launch stream during the timed steps, vs 8 TB/s
  cpu_baseline : the oracle (a CPU restatement of the reference's fp32 training step) timed on this host
and the batch sweep, SpatialNet-large, the narrow-band archs and the per-kernel milliseconds of the profiled warm-up steps.
--dump-outputs DIR writes what the last timed step computed (loss, updated parameters, Adam moments) as DIR/<name>.npy.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

S_BYTES_BF16 = 129 * 251 * 96 * 2  # one utterance's residual stream (S)
HBM_PEAK = 8.0e12    # B/s   (/opt/skills/guides/MI355X_MICROARCH.md)
MFMA_PEAK = 2.5e15   # FLOP/s dense bf16 (same guide; the 2:1-sparsity headline figure is not used)
# algorithmic forward FLOPs per utterance of one sub-block launch (backward = 2x):
# f-conv 373 M; full 49.7 + 66.8 + 49.7 M; attention 1 790 + 3 120 + 597 M; T-ConvFFN 5 072 M
FWD_FLOPS = {"fconv": 373e6, "full": 166.2e6, "mhsa": 5507e6, "tconvffn": 5072e6}
STEP_FLOPS = 277.0e9  # per utterance-train-step


def synth_batch(B, C, S, N, seed, device):
    """two random 'speech-like' sources (low-passed noise bursts) mixed into C channels with random gains/delays + noise"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, S, N, generator=g)
    k = torch.hann_window(33)[None, None]
    src = torch.nn.functional.conv1d(src.reshape(B * S, 1, N), k / k.sum(), padding=16).reshape(B, S, N)
    env = (torch.rand(B, S, N // 800 + 1, generator=g) > 0.3).float().repeat_interleave(800, -1)[..., :N]
    src = src * env * 3.0
    gains = 0.5 + torch.rand(B, C, S, generator=g)
    mix = torch.einsum("bcs,bsn->bcn", gains, src) + 0.01 * torch.randn(B, C, N, generator=g)
    yr = src * gains[:, 0, :, None]  # targets at the reference channel
    return mix.to(device), yr.contiguous().to(device)


def profile_read(lib):
    n = lib.nbss_profile_kernels()
    ms = (C.c_double * n)()
    cnt = (C.c_int64 * n)()
    lib.nbss_profile_read(ms, cnt)
    return {lib.nbss_profile_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}


def algorithmic_bytes(name, B):
    """per-launch algorithmic HBM bytes (each residual sub-block reads + writes the stream once in
    forward (2S) and reads x, dy, writes dx in backward (3S); S = 6.2 MB per utterance in bf16)"""
    S = S_BYTES_BF16 * B
    if name.endswith("_fwd") and name.split("_")[0] in ("fconv", "full", "mhsa", "tconvffn"):
        return 2 * S
    if name.endswith("_bwd") and name.split("_")[0] in ("fconv", "full", "mhsa", "tconvffn"):
        return 3 * S
    return None


def algorithmic_flops(name, B):
    """per-launch algorithmic FLOPs of a sub-block kernel (forward table above; backward = 2 x forward)"""
    blk, _, d = name.rpartition("_")
    if blk in FWD_FLOPS and d in ("fwd", "bwd"):
        return FWD_FLOPS[blk] * B * (2 if d == "bwd" else 1)
    return None


def csrc_hash():
    """identifies the kernel sources a PMC file was measured on (.git does not travel to the GPU box)"""
    import hashlib
    h = hashlib.sha1()
    for f in sorted((ROOT / "nbss_amd" / "csrc").glob("*")):
        if f.suffix in (".hip", ".h"):
            h.update(f.name.encode())
            h.update(f.read_bytes())
    return h.hexdigest()[:12]


def roofline_entry(name, B, ms, cnt, share):
    """both lower bounds of one sub-block kernel: algorithmic bytes at 8 TB/s and algorithmic FLOPs at 2.5 PFLOP/s (dense bf16 MFMA);
    `bound` names the larger one — the kernel's own roofline — and `frac` is that bound's time over the measured launch duration"""
    t = ms / cnt * 1e-3
    by, fl = algorithmic_bytes(name, B), algorithmic_flops(name, B)
    t_hbm, t_mfma = by / HBM_PEAK, fl / MFMA_PEAK
    bound = "mfma" if t_mfma > t_hbm else "hbm"
    e = {"kernel": name, "bound": bound, "avg_launch_us": t * 1e6, "launches": cnt,
         "frac_hbm": t_hbm / t, "frac_mfma": t_mfma / t, "frac": max(t_hbm, t_mfma) / t,
         "algorithmic_bytes_per_launch": by, "algorithmic_flops_per_launch": fl, "share_of_gpu_time": share}
    if bound == "mfma":
        e.update(achieved=fl / t / 1e12, peak=MFMA_PEAK / 1e12, unit="TFLOP/s")
    else:
        e.update(achieved=by / t / 1e9, peak=HBM_PEAK / 1e9, unit="GB/s")
    return e


def _cpu_train_step_fn(B, use_reference):
    """one fp32 SpatialNet-small training step on the host (STFT .. clip + Adam), reference semantics.  use_reference: the network,
    STFT and Norm are the reference's OWN modules imported from /root/reference (present in the build container only); the uPIT
    neg-SI-SDR loss is the oracle's restatement either way (the reference takes it from torchmetrics, which is not installed)."""
    from oracle import io_ref
    from oracle import spatialnet_ref as ref
    torch.manual_seed(2)
    x, yr = synth_batch(B, 6, 2, 32000, 99, "cpu")
    if use_reference:
        import importlib
        saved = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]}
        sys.path.insert(0, "/root/reference")
        try:
            RefNet = importlib.import_module("models.arch.SpatialNet").SpatialNet
            RefSTFT = importlib.import_module("models.io.stft").STFT
            RefNorm = importlib.import_module("models.io.norm").Norm
        finally:
            sys.path.remove("/root/reference")
            for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
                del sys.modules[k]
            sys.modules.update(saved)
        net = RefNet(dim_input=12, dim_output=4, num_layers=8, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192, num_heads=4, dropout=(0, 0, 0),
                     kernel_size=(5, 3), conv_groups=(8, 8), norms=("LN", "LN", "GN", "LN", "LN", "LN"), dim_squeeze=8, num_freqs=129, full_share=0)
        stft, norm = RefSTFT(n_fft=256, n_hop=128), RefNorm(mode="frequency")
        leaves = list(net.parameters())
        opt = torch.optim.Adam(leaves, lr=1e-3)

        def step():
            opt.zero_grad(set_to_none=True)
            X, n = stft.stft(x)
            Bq, C, F, T = X.shape
            X, (Xr, XrMM) = norm.norm(X, ref_channel=0)
            out = net(torch.view_as_real(X.permute(0, 2, 3, 1)).reshape(Bq, F, T, -1))
            out = torch.view_as_complex(out.float().reshape(Bq, F, T, -1, 2)).permute(0, 3, 1, 2)
            yr_hat = stft.istft(norm.inorm(out, (Xr, XrMM)), n)
            loss, _, _ = io_ref.pit_neg_si_sdr(yr_hat, yr)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(leaves, 5.0)
            opt.step()
        return step
    p = ref.init_params(num_layers=8)
    leaves, seen = [], {}
    for k, v in p.items():
        if id(v) not in seen:
            seen[id(v)] = v.clone().requires_grad_(True)
            leaves.append(seen[id(v)])
        p[k] = seen[id(v)]
    opt = torch.optim.Adam(leaves, lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss, _, _ = io_ref.train_forward(x, yr, p, 8)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(leaves, 5.0)
        opt.step()
    return step


def cpu_baseline(seconds_budget=20.0):
    """the reference's CPU training step timed on THIS host: fp32, batch 2.  The thread count is the best of a short sweep over
    {2 (the reference's own setting, models/utils/base_cli.py:7), 8, 32, all}: on a 128-thread host the all-threads run was SLOWER than two threads
    (0.112 vs 0.311 utt/s, round 5: oversubscription of a step made of small ops).  A reported baseline only; bounded sample."""
    use_ref = Path("/root/reference/models/arch/SpatialNet.py").exists()
    threads = torch.get_num_threads()
    sweep = {}
    step1 = _cpu_train_step_fn(1, use_ref)
    for n in sorted({2, 8, 32, threads}):
        if n > threads:
            continue
        torch.set_num_threads(n)
        step1()  # warm-up at this thread count
        t1 = time.perf_counter()
        step1()
        sweep[n] = 1.0 / (time.perf_counter() - t1)
    best = max(sweep, key=sweep.get)
    torch.set_num_threads(best)
    B = 2
    step = _cpu_train_step_fn(B, use_ref)
    step()  # warm-up
    t0 = time.perf_counter()
    n = 0
    while n < 1 or (time.perf_counter() - t0 < seconds_budget and n < 3):
        step()
        n += 1
    dt = time.perf_counter() - t0
    torch.set_num_threads(threads)
    what = "the reference's own SpatialNet / STFT / Norm modules (/root/reference) + restated uPIT loss" if use_ref else \
           "the oracle (CPU restatement of the reference's training step; /root/reference is not on this box)"
    return {"value": B * n / dt, "unit": "utterances/s", "cores": best, "kind": "reference" if use_ref else "port",
            "value_2_threads": sweep.get(2), "utt_per_s_by_threads": {str(k): round(v, 4) for k, v in sweep.items()},
            "sample": f"{n} fp32 training steps (STFT..clip+Adam) of {what} at batch {B}, 4-s 6-ch utterances, torch CPU {best} threads = the best of a "
                      f"one-step sweep at batch 1 over {sorted(sweep)} threads (os.cpu_count() = {os.cpu_count()}); value_2_threads: base_cli.py:7's setting"}


def nb_arch_rates(dev, batch=4, steps=3):
    """the three narrow-band archs behind NBSS.forward, native training step (forward + backward of every parameter, fp32
    stream) at batch x 129 x 251, with a FLOP statement: forward FLOPs counted from the torch.nn modules' own shapes (every Linear / Conv1d /
    ConvTranspose1d / LSTM call of one torch.nn forward, plus the attention contractions 4 T H per token and layer — 6 T H with NBC's relative-position
    term), training = 3 x forward, against the exact-f32 MFMA peak these paths compute on (157.3 TFLOP/s)."""
    import warnings
    import torch.nn as nn
    out = {}
    F_, T_ = 129, 251

    def fwd_flops(net, x, attn_layers, attn_h, attn_mult):
        tot = [0.0]

        def hook(m, inp, res):
            if isinstance(m, nn.Linear):
                tot[0] += 2.0 * res.numel() * m.in_features
            elif isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                tot[0] += 2.0 * res.numel() * m.kernel_size[0] * (m.in_channels // m.groups)
            elif isinstance(m, nn.LSTM):
                y = res[0]
                nd = 2 if m.bidirectional else 1
                isz = m.input_size
                for _ in range(m.num_layers):
                    tot[0] += 2.0 * (y.numel() / (nd * m.hidden_size)) * nd * 4 * m.hidden_size * (isz + m.hidden_size)
                    isz = nd * m.hidden_size
        hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, (nn.Linear, nn.Conv1d, nn.ConvTranspose1d, nn.LSTM))]
        with torch.no_grad():
            net(x)
        for h in hs:
            h.remove()
        return tot[0] + attn_layers * attn_mult * T_ * attn_h * (x.shape[0] * F_ * T_)

    def one(name, make, env, attn):
        try:
            torch.manual_seed(0)
            net, cin = make()
            net = net.to(dev).train()
            x = torch.randn(batch, F_, T_, cin, device=dev)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                os.environ[env] = "0"
                net.eval()
                fl = fwd_flops(net, x, *attn)
                net.train()
                os.environ[env] = "1"

                def step():
                    net.zero_grad(set_to_none=True)
                    net(x).square().mean().backward()
                step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / steps
            os.environ.pop(env, None)
            out[name] = {"train_ms": round(dt * 1e3, 2), "batch": batch, "fwd_gflop": round(fl / 1e9, 1), "train_tflops": round(3 * fl / dt / 1e12, 2),
                         "frac_of_f32_mfma_peak": round(3 * fl / dt / 157.3e12, 4)}
        except Exception as e:  # reported, never fatal for the headline line
            out[name] = {"error": str(e)[:200]}

    def nbc2():
        from models.arch.NBC2 import NBC2
        return NBC2(dim_input=16, dim_output=6, n_layers=8, dim_hidden=96, dim_ffn=192, num_freqs=F_), 16

    def nbc():
        from models.arch.NBC import NBC
        return NBC(dim_input=16, dim_output=4, n_layers=4, encoder_kernel_size=4, n_heads=8, hidden_size=192, ffn_size=384), 16

    def blstm():
        from models.arch.blstm2_fc1 import BLSTM2_FC1
        return BLSTM2_FC1(dim_input=12, dim_output=4, hidden_size=(256, 128)), 12
    one("NBC2", nbc2, "NBSS_NBC2_NATIVE", (8, 96, 4))
    one("NBC", nbc, "NBSS_NBC_NATIVE", (4, 192, 6))
    one("NB-BLSTM", blstm, "NBSS_BLSTM_NATIVE", (0, 0, 0))
    return out


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU on this node"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), "--gpus", str(args.gpus), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--batch", str(args.batch)] + (["--no-cpu-baseline"] if args.no_cpu_baseline else []) + (["--dry-run"] if args.dry_run else []) + \
          (["--full"] if args.full else []) + (["--dump-outputs", args.dump_outputs] if args.dump_outputs else [])
    # HSA_ENABLE_IPC_MODE_LEGACY=0: the images this runs on export it (the host driver supports dmabuf IPC only; without it RCCL's
    # hipIpcGetMemHandle fails between processes) — inherited when set, defaulted for shells that lost it; nothing else is altered
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def dry_run(args, rank, world):
    """the launch / rendezvous / exchange skeleton of a multi-GPU run WITHOUT a GPU (tests, CPU containers): gloo instead of RCCL, the
    real gradient-bucket table of the benchmark model, one all-reduce per bucket per step on host tensors, the same barrier + max-over-
    ranks timing, the same JSON contract keys (value is meaningless and says so: "dry_run": true)"""
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("gloo")
    from nbss_amd.build import build_emu
    from nbss_amd._lib import Lib, make_cfg
    from nbss_amd.params import param_table
    lib = Lib(build_emu())  # (parameter table only: arithmetic on the configuration, no kernel runs)
    cfg = make_cfg(1, 129, 16, 12, 4, L=8)
    n = max(off + int(torch.tensor(shape).prod()) for _, (off, shape) in param_table(lib, cfg).items())
    grads = torch.full((n,), float(rank + 1))
    bounds = [(i * n // 8, (i + 1) * n // 8) for i in range(8)]
    for _ in range(args.warmup):
        pass
    if world > 1:
        torch.distributed.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if world > 1:
            hs = [torch.distributed.all_reduce(grads[lo:hi], async_op=True) for lo, hi in reversed(bounds)]
            for h in hs:
                h.wait()
            grads.mul_(1.0 / world)
    if world > 1:
        torch.distributed.barrier()
    dt = time.perf_counter() - t0
    worlds = [world]
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt)
        worlds = [None] * world
        torch.distributed.all_gather_object(worlds, torch.distributed.get_world_size())
    if rank == 0:
        print(json.dumps({"metric": "utterances/sec (4 s, 6ch, 129 freqs) SpatialNet bf16 train at 1/2/4/8 MI355X", "value": 0.0, "unit": "utterances/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / max(args.steps, 1) * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic", "dry_run": True,
                          "rccl_world": worlds, "backend": "gloo", "grad_elements": n,
                          "config": {"workload": "launch / rendezvous / bucketed all-reduce skeleton only (no GPU)", "batch_per_gpu": args.batch,
                                     "global_batch": args.batch * world, "parallelism": f"dp{world}"}}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def large_train_rate(lib, dev, batch=4, steps=2):
    """SpatialNet-large (12 layers, 192 / 384 / squeeze 16: the "for large" comments of configs/SpatialNet.yaml), same 4-s 6-ch input, full bf16
    train step through the geometry-generic path (csrc/gbwd.hip sequencing gemm_g.hip's tile GEMM, tchain.hip's conv chain, fconv_g.hip's F-conv
    backward, the generic attention and wgrad.hip)"""
    from models.arch.SpatialNet import SpatialNet
    from nbss_amd._lib import NBSS_BF16
    from nbss_amd.engine import SpatialNetEngine, TrainStep
    try:
        torch.manual_seed(3)
        net = SpatialNet(dim_input=12, dim_output=4, num_layers=12, encoder_kernel_size=5, dim_hidden=192, dim_ffn=384, num_heads=4, dropout=(0, 0, 0),
                         kernel_size=(5, 3), conv_groups=(8, 8), norms=("LN", "LN", "GN", "LN", "LN", "LN"), dim_squeeze=16, num_freqs=129, full_share=0)
        eng = SpatialNetEngine(lib, dev, dtype=NBSS_BF16, **net.hp)
        eng.load_params({k: v for k, v in net.named_parameters(remove_duplicate=False)})
        ts = TrainStep(eng, n_fft=256, ref_channel=0, lr=1e-3, clip=5.0)
        x, yr = synth_batch(batch, 6, 2, 32000, 99, dev)
        loss0 = float(ts.step(x, yr))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            loss = ts.step(x, yr)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t1
        return {"value": round(batch * steps / dt, 2), "unit": "utterances/s", "batch": batch, "layers": 12, "ms_per_step": round(dt / steps * 1e3, 1),
                "loss_first": round(loss0, 4), "loss_last": round(float(loss), 4)}
    except Exception as e:  # reported, never fatal for the headline line
        return {"error": str(e)[:200]}


def dump_outputs(out_dir, ts, loss):
    """what a caller of the timed path holds after its last step: the loss it returned, the parameters it updated and the Adam moments
    (flat fp32, the engine's parameter order; 3 x 4.8 MB at SpatialNet-small).  The gradient itself is not among them: the optimizer
    kernel re-zeroes it for the next step, and the moments carry it."""
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    for name, t in (("loss", loss), ("params", ts.e.params), ("exp_avg", ts.m), ("exp_avg_sq", ts.v)):
        np.save(out / f"{name}.npy", t.detach().float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    # headline batch 32 (SURVEY.md §8(d) names B/GPU in {2, 8, 32}); with --full the line also carries a short sweep over the other two
    ap.add_argument("--batch", type=int, default=32, help="utterances per GPU per step")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: the roofline line only (no in-order child run, sweep, "
                    "SpatialNet-large, narrow-band archs or CPU baseline)")
    ap.add_argument("--full", action="store_true", help="also the roofline / per-kernel figures, the batch sweep, SpatialNet-large, the "
                    "narrow-band archs and the CPU baseline (a plain run measures the headline steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy (float32)")
    ap.add_argument("--dry-run", action="store_true", help="CPU-only rehearsal of the multi-process launch + gradient exchange (gloo); no measurement")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        if "WORLD_SIZE" not in os.environ and args.gpus > 1:
            self_launch(args)
        raise SystemExit(f"--gpus {args.gpus} != WORLD_SIZE {world}")
    if args.dry_run:
        return dry_run(args, rank, world)
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl")  # RCCL on ROCm

    from models.arch.SpatialNet import SpatialNet
    from nbss_amd._lib import NBSS_BF16, hip
    from nbss_amd.engine import SpatialNetEngine, TrainStep

    lib = hip()
    torch.manual_seed(2)  # seed_everything: 2 (configs/SpatialNet.yaml:1); identical init on every rank
    net = SpatialNet(dim_input=12, dim_output=4, num_layers=8, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192, num_heads=4, dropout=(0, 0, 0),
                     kernel_size=(5, 3), conv_groups=(8, 8), norms=("LN", "LN", "GN", "LN", "LN", "LN"), dim_squeeze=8, num_freqs=129, full_share=0)
    eng = SpatialNetEngine(lib, dev, dtype=NBSS_BF16, **net.hp)
    eng.load_params({k: v for k, v in net.named_parameters(remove_duplicate=False)})
    ts = TrainStep(eng, n_fft=256, ref_channel=0, lr=1e-3, clip=5.0)
    ts.sync_replicas()  # rank 0's parameters / Adam state on every rank (what DDP's init broadcast does); no-op on one GPU
    B = args.batch
    x, yr = synth_batch(B, 6, 2, 32000, 1234 + rank, dev)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    # ---- warm-up (untimed); with --full the steps from the second on are fully profiled to find the dominant kernel -------
    nk = lib.nbss_profile_kernels()
    losses, prof, nprof = [], {}, 0
    dominant = dom_id = None
    for i in range(max(args.warmup, 2) if args.full else args.warmup):
        if args.full and i == 1:  # step 0 pays the one-time code-object loads: profile from step 1 on
            torch.cuda.synchronize()
            lib.nbss_profile_enable((1 << nk) - 1)
        losses.append(ts.step(x, yr))
        if i >= 1:
            nprof += 1
    torch.cuda.synchronize()
    if args.full:
        prof = profile_read(lib)
        lib.nbss_profile_enable(0)
        cand = {k: v for k, v in prof.items() if algorithmic_bytes(k, B) and v[1] > 0}
        dominant = max(cand, key=lambda k: cand[k][0]) if cand else None
        dom_id = [i for i in range(nk) if lib.nbss_profile_name(i).decode() == dominant][0] if dominant else None

    # ---- timed region: EXACTLY --steps steps, events only around the dominant kernel ------------------
    if dom_id is not None:
        lib.nbss_profile_enable(1 << dom_id)
    if world > 1:
        ts.comm_wait_ms = 0.0  # accumulate the host-visible wait for the gradient buckets behind backward
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = ts.step(x, yr)
    sync()
    dt = time.perf_counter() - t0
    if dom_id is not None:
        lib.nbss_profile_enable(0)
    if args.dump_outputs and rank == 0:  # (before --full's sweep below takes more steps on the same parameters)
        dump_outputs(args.dump_outputs, ts, loss)
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt)
    timed_prof = profile_read(lib) if args.full else {}
    final_loss = float(loss)
    comm_ms, worlds = None, [1]
    if world > 1:
        comm_ms = ts.comm_wait_read() / args.steps
        ts.check_replicas()  # raises when the replicas' parameters / optimizer state differ after the timed steps
        worlds = [None] * world
        torch.distributed.all_gather_object(worlds, torch.distributed.get_world_size())  # what RCCL's group says on every rank

    if rank == 0:
        roof = None
        if dominant and timed_prof[dominant][1] > 0:
            ms, cnt = timed_prof[dominant]
            total_gpu_ms = sum(v[0] for v in prof.values())
            roof = roofline_entry(dominant, B, ms, cnt, prof[dominant][0] / total_gpu_ms if total_gpu_ms > 0 else None)
            # HBM traffic and MFMA utilisation of the dominant kernel come from separate rocprofv3 --pmc passes (tools/round_artefacts.sh writes
            # them with the commit and a hash of nbss_amd/csrc they were measured on); a bench run cannot collect counters itself, so it
            # says whether the committed figures belong to THIS build of the kernels
            traffic = traffic_commit = mfma_util = None
            stale = None
            here = csrc_hash()
            tfile = ROOT / "profiles" / "pmc_traffic.json"
            if tfile.exists():
                tj = json.loads(tfile.read_text())
                if tj.get("batch") == B and dominant in tj.get("kernels", {}):
                    k = tj["kernels"][dominant]
                    traffic, traffic_commit = k["hbm_bytes"], k.get("commit", tj.get("commit"))
                    stale = k.get("csrc_hash", tj.get("csrc_hash")) != here
            mfile = ROOT / "profiles" / "pmc_mfma.json"
            if mfile.exists():
                mj = json.loads(mfile.read_text())
                if dominant in mj.get("kernels", {}):
                    mfma_util = mj["kernels"][dominant].get("mfma_busy_frac")
            roof.update(traffic=traffic, traffic_commit=traffic_commit, traffic_stale=stale, csrc_hash=here, mfma_util=mfma_util)
            # the other sub-block kernels, same two bounds (from the profiled warm-up steps)
            roof["all_kernels"] = {k: {kk: (round(vv, 4) if isinstance(vv, float) else vv) for kk, vv in roofline_entry(k, B, v[0], v[1], None).items()
                                       if kk in ("bound", "frac", "frac_hbm", "frac_mfma", "avg_launch_us")}
                                   for k, v in prof.items() if algorithmic_bytes(k, B) and v[1] > 0}
            ups = B * args.steps / dt  # per GPU
            roof["step"] = {"bytes_per_utt": 204 * S_BYTES_BF16, "flops_per_utt": STEP_FLOPS, "frac_hbm": ups * 204 * S_BYTES_BF16 / HBM_PEAK,
                            "frac_mfma": ups * STEP_FLOPS / MFMA_PEAK, "bound": "hbm" if 204 * S_BYTES_BF16 / HBM_PEAK > STEP_FLOPS / MFMA_PEAK else "mfma"}
        base = None
        sweep = None
        large = None
        nb = None
        if world == 1 and not args.no_cpu_baseline and roof is not None:
            # the same kernels with the walks IN ORDER (NBSS_SIDE_STREAM=0 is read once per process: a short child run): the live figures above
            # include whatever the gradient stream's launches cost the dominant kernel while they overlap it
            try:
                env = dict(os.environ, NBSS_SIDE_STREAM="0")
                r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "4", "--warmup", "3", "--batch", str(B), "--full", "--no-cpu-baseline"],
                                   env=env, capture_output=True, text=True, timeout=240)
                child = json.loads(r.stdout.strip().splitlines()[-1])
                io = child["roofline"]["all_kernels"][dominant]
                roof["frac_in_order"] = io["frac"]
                roof["avg_launch_us_in_order"] = io["avg_launch_us"]
                roof["utt_per_s_in_order"] = round(child["value"], 1)
                roof["kernel_ms_per_step_in_order"] = child["kernel_ms_per_step"]
            except Exception as e:  # reported, never fatal
                roof["frac_in_order"] = None
                roof["in_order_error"] = str(e)[:200]
        if world == 1 and args.full and not args.no_cpu_baseline:
            # utterances/s at the other per-GPU batches of SURVEY.md §8(d) (short runs: 3 warm-up + 8 timed steps each — with 1 + 3 the first steps
            # at a new shape (workspace re-sizing, allocator) weighed on the figure: batch 8 read 562 here against 585 in a run of its own)
            sweep = {str(B): round(B * args.steps / dt, 1)}
            for b2 in (2, 8, 32):
                if b2 == B:
                    continue
                x2, y2 = synth_batch(b2, 6, 2, 32000, 77, dev)
                for _ in range(3):
                    ts.step(x2, y2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(8):
                    ts.step(x2, y2)
                torch.cuda.synchronize()
                sweep[str(b2)] = round(b2 * 8 / (time.perf_counter() - t1), 1)
            large = large_train_rate(lib, dev)
            if large and "value" in large:  # ... and at twice the batch (one more ~0.3 s of steps)
                l8 = large_train_rate(lib, dev, batch=8, steps=2)
                large["batch8"] = {k: l8.get(k) for k in ("value", "ms_per_step", "error") if k in l8}
            nb = nb_arch_rates(dev)
            base = cpu_baseline()
        line = {
            "metric": "utterances/sec (4 s, 6ch, 129 freqs) SpatialNet bf16 train at 1/2/4/8 MI355X",
            "value": world * B * args.steps / dt, "unit": "utterances/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic",
            "config": {"workload": "SpatialNet-small 6ch->2spk, 4-s 8-kHz utterances (32000 samples), n_fft 256/hop 128 (F=129, T=251), 8 layers, "
                                   f"full train step (STFT..Adam), bf16 stream + fp32 master/stats, {B} utterances per GPU per step", "batch_per_gpu": B, "global_batch": B * world,
                       "parallelism": f"dp{world}", "final_loss": final_loss},
            "rccl_world": worlds, "comm_ms_per_step": comm_ms,
        }
        if args.full:
            line.update({"roofline": roof, "cpu_baseline": base, "utt_per_s_by_batch": sweep, "utt_per_s_large": large, "nb_archs": nb,
                         "kernel_ms_per_step": {k: round(v[0] / max(nprof, 1), 4) for k, v in prof.items() if v[1] > 0}})
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
