"""RIR convolution of the on-device simulator (profiles/README.md, "Room simulation"): the shipped torch.fft path (convolve='fft': rocFFT at the padded
power of two, the full convolution, a gather) beside the HIP kernels of csrc/conv1d.hip (convolve='native': nbss_rir_delay + nbss_fir_convolve, only
the N samples from the direct-path delay onward), in the same run on the same device.

  conv points   convolve_aligned / convolve_aligned_native at B in {32, 2}, S = 2, M = 6, N = 32 000, L in {3 200, 6 400}, with and without rir_target:
                --warmup untimed calls, then --reps calls each between a pair of HIP events (median, min, max in ms), the peak of
                torch.cuda.max_memory_allocated over the calls above what the inputs hold (MB), and the rel-L2 distance of the two results.
                FLOP/s of the native kernel: 2 N L MACs per output row (the useful work, not the zero blocks), over its time.
  dm points     utterances/s of SimulatedRoomDataModule.batches (batch 32, 4 s, 6 channels, 2 speakers) with each switch, for rir = synthetic and ism
                (host clock around batches that end in a synchronise, after two warm-up batches).

The driver starts every point as a child process of its own under a time limit (--limit seconds) and stops at the first one that fails, so a fault
in one point starts nothing more on the device.  One JSON line per point, then markdown tables.
usage: python tools/convolve_bench.py [--reps 10] [--warmup 2] [--batches 10] [--limit 120] [--json out.json]"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
S, M, N = 2, 6, 32000


def conv_point(a):
    import torch
    from data_loaders.gpu_simulation import convolve_aligned, convolve_aligned_native
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    wav = torch.randn(a.B, S, N, generator=g, device=dev)
    t = torch.arange(a.L, device=dev) / 8000.0
    rir = torch.randn(a.B, S, M, a.L, generator=g, device=dev) * torch.exp(-6.9 * t / 0.4) * 0.3
    rir[..., 40] = 1.0  # the direct path
    tgt = torch.zeros_like(rir) if a.target else None
    if a.target:
        tgt[..., 40] = 1.0
    torch.cuda.synchronize()
    row = {"point": "conv", "B": a.B, "S": S, "M": M, "N": N, "L": a.L, "rir_target": bool(a.target)}
    outs = {}
    for side, fn in (("fft", convolve_aligned), ("native", convolve_aligned_native)):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        for _ in range(a.warmup):
            fn(wav, rir, tgt)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(wav, rir, tgt)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        outs[side] = [o.clone() for o in out]
        del out
        row.update({f"{side}_median_ms": round(statistics.median(ms), 3), f"{side}_min_ms": round(min(ms), 3), f"{side}_max_ms": round(max(ms), 3),
                    f"{side}_peak_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20)})
    convs = 2 if a.target else 1
    row["native_useful_tflops"] = round(convs * 2.0 * a.B * S * M * N * a.L / (row["native_median_ms"] * 1e-3) / 1e12, 2)
    row["fft_over_native"] = round(row["fft_median_ms"] / row["native_median_ms"], 3)
    row["rel_l2_native_vs_fft"] = [float((n_ - f_).double().norm() / f_.double().norm()) for n_, f_ in zip(outs["native"], outs["fft"])]
    print(json.dumps(row), flush=True)


def dm_point(a):
    import torch
    from data_loaders.gpu_simulation import SimulatedRoomDataModule
    B = 32
    dm = SimulatedRoomDataModule(batch_size=[B, B], num_samples=[B * (a.batches + 2), B, B], audio_time_len=[4.0, 4.0, 4.0], device="cuda:0", rir=a.rir,
                                 convolve=a.convolve)
    it = dm.batches(0)
    for _ in range(2):  # warm-up: rocFFT plans, code objects, allocator
        next(it)
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    for x, ys, _ in it:
        n += x.shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"point": "dm", "rir": a.rir, "convolve": a.convolve, "batch": B, "utterances": n, "utt_per_s": round(n / dt, 1),
                      "finite": bool(torch.isfinite(x).all() and torch.isfinite(ys).all())}), flush=True)


def driver(a):
    points = [["--point", "conv", "--B", str(B), "--L", str(L), "--target", str(t)] for B in (32, 2) for L in (3200, 6400) for t in (0, 1)]
    points += [["--point", "dm", "--rir", r, "--convolve", c] for r in ("synthetic", "ism") for c in ("fft", "native")]
    rows = []
    for p in points:
        cmd = [sys.executable, str(Path(__file__).resolve()), *p, "--reps", str(a.reps), "--warmup", str(a.warmup), "--batches", str(a.batches)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"stopped: {' '.join(p)} ran into its limit of {a.limit} s", flush=True)
            return 1
        if r.returncode != 0:
            print(f"stopped: {' '.join(p)} exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    print("\n| B | L | rir_target | fft ms (min - max) / peak MB | native ms (min - max) / peak MB | fft / native | native useful TFLOP/s |\n|---|---|---|---|---|---|---|")
    for w in (w for w in rows if w["point"] == "conv"):
        cell = lambda s: f"{w[s + '_median_ms']} ({w[s + '_min_ms']} - {w[s + '_max_ms']}) / {w[s + '_peak_mb']}"  # noqa: E731
        print(f"| {w['B']} | {w['L']} | {'yes' if w['rir_target'] else 'no'} | {cell('fft')} | {cell('native')} | {w['fft_over_native']} | {w['native_useful_tflops']} |")
    print("\n| rir | convolve | utt/s |\n|---|---|---|")
    for w in (w for w in rows if w["point"] == "dm"):
        print(f"| {w['rir']} | {w['convolve']} | {w['utt_per_s']} |")
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps({"S": S, "M": M, "N": N, "reps": a.reps, "warmup": a.warmup, "rows": rows}, indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", default=None, choices=["conv", "dm"])
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--L", type=int, default=3200)
    ap.add_argument("--target", type=int, default=0)
    ap.add_argument("--rir", default="synthetic")
    ap.add_argument("--convolve", default="fft")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.point == "conv":
        conv_point(a)
    elif a.point == "dm":
        dm_point(a)
    else:
        sys.exit(driver(a))


if __name__ == "__main__":
    main()
